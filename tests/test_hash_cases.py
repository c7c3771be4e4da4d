"""The case lists of tests/hash_cases.py against the CPU oracle (oracle/pwg.c, oracle/hashes.c): status, error kind, failing opcode, the aux words, the
text and the whole witness map of every row must equal the expectation of the Python model (tests/hash_ref.py); the model is pinned to hashlib and to
Keccak's known answers; the lists must cover what they are built to cover -- the launcher's kernel modes among it, from the item and word counts --; and
each list must notice the mistake it is meant to catch. No GPU: tests/test_gpu_hash_edges.py runs the same lists on the device."""
import collections
import hashlib

import pytest

import hash_cases as hc
import hash_ref as hr
from acvm_amd.acir import P, BlackBoxFuncCall as BB, Circuit, FunctionInput as FI
from acvm_amd.synth import values_from_rows
from keccak_ref import keccak256

EVERY_CASE = hc.all_cases() + list(hc.big_cases())


def oracle_got(oracle, case):
    return oracle.solve_batch(oracle.Circuit(case.circuit.to_bytes()), case.ids, values_from_rows(case.rows), len(case.rows))


def same(a, b):
    return a[:7] == b[:7]


# ---- the models
def test_codes_are_the_oracles(oracle):
    assert (hr.E_BLACKBOX_FAILED, hr.E_PANIC, hr.E_UNSATISFIED, hr.E_MISSING_ASSIGNMENT) == (oracle.E_BLACKBOX_FAILED, oracle.E_PANIC, oracle.E_UNSATISFIED, oracle.E_MISSING_ASSIGNMENT)


def test_keccak_known_answers():
    """known answers of Keccak-256 (rate 1088, the original padding): the empty message and "abc"; SHA-3's answers are others"""
    assert keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert keccak256(b"abc") != hashlib.sha3_256(b"abc").digest() and keccak256(b"\xa3" * 200) != hashlib.sha3_256(b"\xa3" * 200).digest()


def test_model_on_a_message_known_by_hand():
    """widths 8, 16 and 9 over the values 0x1FF, 0x010203 and 0x1FF: the bytes FF | 03 02 | FF 01"""
    circ = Circuit(40, [BB("SHA256", {"inputs": [FI(1, 8), FI(2, 16), FI(3, 9)], "outputs": list(range(4, 36))}),
                        BB("HashToField128Security", {"inputs": [FI(1, 8), FI(2, 16), FI(3, 9)], "output": 36})])
    x, messages = hr.run_traced(circ, {1: 0x1FF, 2: 0x010203, 3: 0x1FF})
    assert [m for _, _, m in messages] == [b"\xff\x03\x02\xff\x01"] * 2
    assert [x.witnesses[w] for w in range(4, 36)] == list(hashlib.sha256(b"\xff\x03\x02\xff\x01").digest())
    assert x.witnesses[36] == int.from_bytes(hashlib.blake2s(b"\xff\x03\x02\xff\x01").digest(), "big") % P
    assert hr.msg_slice(33) == b"range end index 33 out of range for slice of length 32"


@pytest.mark.parametrize("case", EVERY_CASE, ids=lambda c: c.name)
def test_oracle_agrees_with_the_model(oracle, case):
    hc.compare(case, oracle_got(oracle, case), "oracle")


def test_oracle_agrees_on_the_initial_sets(oracle):
    circ, maps, expect, notes = hc.initial_set_case()
    case = hc.Case("G", circ, [], list(maps), list(expect), list(notes), None, {})
    got = []
    for m in maps:
        a = oracle.ACVM(oracle.Circuit(circ.to_bytes()), m)
        a.solve()
        got.append((a.result().as_tuple(), a.result().message, a.witness_map()))
    hc.compare_maps(case, got, "oracle")
    assert collections.Counter(n.split(",")[0] for n in notes) == {"the plain set": 7, "knows an output": 7, "lacks an input": 7}


def test_second_rows_differ_everywhere():
    for case in (hc.chain_case("two buffers"), hc.chain_case("one buffer")):
        second = hc.second_rows(case)
        for a, b in zip(case.expect, second.expect):
            outs = [w for w in a.witnesses if w not in case.ids]
            assert len(outs) == 128 and sum(a.witnesses[w] != b.witnesses[w] for w in outs) > 100


# ---- what the lists cover
def test_sizes():
    for case in hc.all_cases():
        assert 0 < len(case.rows) <= 200 and len(case.rows) % 64, case.name
    for case in hc.big_cases():
        assert len(case.rows) == 963, case.name


def test_every_branch_outcome_and_text_at_least_twice():
    expects = [x for c in EVERY_CASE for x in {id(x): x for x in c.expect}.values()] + list(hc.initial_set_case()[2])
    branches = collections.Counter(l for x in expects for l in x.branches)
    assert not [l for l in hr.LABELS if branches[l] < 2], [l for l in hr.LABELS if branches[l] < 2]
    kinds = collections.Counter((x.status, x.err) for x in expects)
    want = {(hr.ST_SOLVED, hr.E_NONE)} | {(hr.ST_FAILURE, e) for e in (hr.E_MISSING_ASSIGNMENT, hr.E_UNSATISFIED, hr.E_BLACKBOX_FAILED, hr.E_PANIC)}
    assert set(kinds) == want and min(kinds.values()) >= 2, kinds
    texts = collections.Counter(x.message for x in expects if x.message is not None)
    for width in hc.PANIC_WIDTHS:
        assert texts[hr.msg_slice((width + 7) // 8)] >= 2, hex(width)
    for n in hc.OUTPUT_COUNTS:
        assert texts[hr.msg_outputs(n)] >= 2, n
    assert sum(1 for t in texts if t.startswith(b"the number of bytes to take")) >= 10
    assert all(x.message is not None for x in expects if x.err in (hr.E_PANIC, hr.E_BLACKBOX_FAILED))


def coop_records(circ):
    """the byte-message records as plan.cpp admits them to the cooperative kernel: 32 distinct outputs, 1 .. 1 024 inputs of 1 .. 8 bits"""
    return [op for op in circ.opcodes if isinstance(op, BB) and op.name in hc.COOP and len(op.args["outputs"]) == 32 == len(set(op.args["outputs"]))
            and 1 <= len(op.args["inputs"]) <= 1024 and all(1 <= f.num_bits <= 8 for f in op.args["inputs"])]


def test_the_launcher_modes_the_lists_promise():
    """from the item and word counts, with the launcher's rule (hash_cases.launch_mode restates it): which instantiation a case's launch takes and how many
    message buffers; and from the planner (host only) how many records run behind their predecessor"""
    import acvm_amd
    modes = {}
    for case in EVERY_CASE:
        if not case.meta:
            continue
        coop = coop_records(case.circuit)
        assert len(coop) - case.meta["chained"] == case.meta["coop_heads"], case.name
        assert max((len(op.args["inputs"]) + 3) // 4 for op in coop) == case.meta["max_words"], case.name
        st = acvm_amd.Circuit(case.circuit.to_bytes()).plan_stats(case.ids)
        assert st["n_hash_chained"] == case.meta["chained"], (case.name, st["n_hash_chained"])
        modes[case.name] = hc.launch_mode(len(case.rows), case.meta["coop_heads"], case.meta["max_words"])
        for n in (65, 130):  # the padded batches stay in the same mode
            assert len(case.rows) > n or hc.launch_mode(n, case.meta["coop_heads"], case.meta["max_words"]) == modes[case.name], case.name
    for f in hc.COOP:
        assert modes[f"A, {f}, four waves"] == (4, 2) and modes[f"A, {f}, one wave"] == (1, 1)
    for r in ("", ", RANGE checks"):
        assert modes["B, chain, two buffers" + r] == (4, 2) and modes["B, chain, one buffer" + r] == (4, 1) and modes["B, chain, one wave" + r] == (1, 1)
    assert [modes[f"B, head of {n} bytes"] for n in hc.THRESHOLDS] == [(4, 2)] * 5 + [(4, 1)]
    assert [hc.threshold_case(n).meta["max_words"] for n in hc.THRESHOLDS] == [32, 33, 64, 65, 88, 89]
    # a record with one witness twice among its outputs takes the lane kernel whatever its shape (its second occurrence compares with the first)
    assert modes["F, one witness twice among the outputs, one wave"] == (1, 1)
    for m in hc.TWICE_MODES:
        ops = hc.twice_case(m).circuit.opcodes
        assert not [op for op in coop_records(hc.twice_case(m).circuit) if op in ops[:3]] and all(len(set(op.args["outputs"])) == 31 for op in ops[:3])
    with acvm_amd.tuning(hash_chain=0):
        case = hc.chain_case("two buffers")
        assert acvm_amd.Circuit(case.circuit.to_bytes()).plan_stats(case.ids)["n_hash_chained"] == 0


def test_list_a_covers_every_length():
    for f in hc.COOP + ("HashToField128Security",):
        assert sorted(len(op.args["inputs"]) for op in hc.length_case(f, "four waves").circuit.opcodes) == list(range(1, 141))
    for f in hc.COOP:
        lens = [len(op.args["inputs"]) for op in hc.length_case(f, "one wave").circuit.opcodes]
        assert len(lens) == 140 and set(lens) == set(range(1, 129))
        assert [len(op.args["inputs"]) for op in hc.long_case(f).circuit.opcodes] == list(hc.LONG_LENGTHS)
        notes = set(hc.length_case(f, "four waves").notes)
        assert {"all 0x00", "all 0xff", "all 0x80", "all 0x01", "random bytes"} <= notes
        assert all(f"{v:#x} in every position" in notes and f"{v:#x} in the last position" in notes for v in hc.NOT_BYTES)
    assert set(hc.LONG_LENGTHS) >= {0, 255, 256, 257, 258, 271, 272, 273, 274, 1023, 1024, 1025} | set(range(351, 359))


def test_list_b_chains_are_what_they_say():
    for mode in hc.CHAIN_MODES:
        case = hc.chain_case(mode)
        ops = [op for op in case.circuit.opcodes if isinstance(op, BB)][:4]
        lens = [len(op.args["inputs"]) for op in ops]
        assert [a - b for a, b in zip(lens, lens[1:])] == list(hc.CHAIN_SHORTER_BY) and lens[0] == hc.CHAIN_MODES[mode]
        assert [op.name for op in ops] == list(hc.CHAIN_FUNCS)
        for prev, op in zip(ops, ops[1:]):
            src = [prev.args["outputs"].index(f.witness) if f.witness in prev.args["outputs"] else None for f in op.args["inputs"]]
            taken = [s for s in src if s is not None]
            assert sorted(taken) == list(range(32)) and taken != sorted(taken) and None in src[:src.index(taken[-1])]   # out of order, interleaved
            assert all(f.witness in case.ids for f, s in zip(op.args["inputs"], src) if s is None)
    assert 353 <= hc.CHAIN_MODES["one buffer"] <= 400
    ranged = hc.chain_case("two buffers", True)
    fails = collections.Counter(x.opcode_index for x in ranged.expect if x.status == hr.ST_FAILURE)
    assert len(fails) >= 2 and all(ranged.circuit.opcodes[oi].name == "RANGE" for oi in fails), fails   # a head input and a digest byte
    assert any(x.status == hr.ST_SOLVED for x in ranged.expect)


def test_list_c_widths_and_panics():
    for f in hc.ALL:
        case = hc.width_case(f)
        hashes = [op for op in case.circuit.opcodes if isinstance(op, BB)]
        assert [op.args["inputs"][1].num_bits for op in hashes[:len(hc.WIDTHS)]] == list(hc.WIDTHS)
        runs, run = [], 0
        for fi in hashes[len(hc.WIDTHS)].args["inputs"]:
            if fi.num_bits == 8:
                run += 1
            else:
                runs.append(run)
                run = 0
        runs.append(run)
        assert runs == [5] + list(range(1, 10)) + [7]
        assert sum(1 for row in case.rows if row[3] + row[4] >= P) >= 5 and sum(1 for row in case.rows if row[3] + row[4] < P) >= 5
        assert {0, 1, P - 1, (1 << 248) - 1} <= {row[1] for row in case.rows}
        where = collections.Counter(c.name.split(" bits ")[1] for c in hc.panic_cases(f)[:6])
        assert where == {"first": 2, "middle": 2, "last": 2}
    assert set(hc.WIDTHS) | set(hc.PANIC_WIDTHS) == {0, 1, 7, 8, 9, 16, 17, 24, 25, 32, 248, 249, 255, 256, 257, 300, 1 << 31, 0xFFFFFFF8, 0xFFFFFFF9, 0xFFFFFFFF}
    assert hc.WRAPPING_WIDTHS == (0xFFFFFFF9, 0xFFFFFFFF)


def test_list_d_sizes():
    for n in hc.VAR_LENGTHS:
        sizes = {row[-1] for row in hc.var_case(n).rows}
        assert {0, max(n - 1, 0), n, n + 1, 135, 136, 137, (1 << 32) - 1, 1 << 32, (1 << 64) + 5, (1 << 128) + 5, P - 1} <= sizes
    mixed = hc.var_mixed_case()[0]
    assert all(x.status == hr.ST_SOLVED for x in mixed.expect[:-3]) and all(x.err == hr.E_BLACKBOX_FAILED for x in mixed.expect[-3:])


def test_list_e_every_quotient():
    case = hc.to_field_case()
    q = collections.Counter()
    for row in case.rows:
        msg = b"".join(v.to_bytes(w // 8, "little") for v, w in zip(row, (8, 16, 8, 32)))
        q[int.from_bytes(hashlib.blake2s(msg).digest(), "big") // P] += 1
    assert q == {k: 3 for k in range(6)}
    assert 0.05 < ((1 << 256) - 5 * P) / (1 << 256) < 0.06   # the share of digests in the top class
    assert sum(1 for x in case.expect if x.err == hr.E_UNSATISFIED and x.opcode_index == 1) == 6
    assert len(case.circuit.opcodes[2].args["inputs"]) == 0


def test_list_f_outputs():
    for f in hc.WITH_OUTPUTS:
        assert [len(c.circuit.opcodes[0].args["outputs"]) for c in hc.count_cases(f)] == list(hc.OUTPUT_COUNTS)
    assert all(x.aux0 == 11 for c in hc.count_cases("Keccak256VariableLength") for x in c.expect)   # function 12 fails as Keccak256
    for case in (hc.preassigned_case("SHA256", 8), hc.preassigned_case("SHA256", 16), hc.preassigned_case("Keccak256", 8)):
        for x in case.expect:
            if x.status == hr.ST_FAILURE and x.opcode_index < 4:   # the outputs in front of the wrong one stay in the map, the ones behind it do not
                outs = case.circuit.opcodes[x.opcode_index].args["outputs"]
                pos = hc.POSITIONS[x.opcode_index]
                assert all(w in x.witnesses for w in outs[:pos + 1]) and not any(w in x.witnesses for w in outs[pos + 1:])
    for mode in hc.TWICE_MODES:
        case = hc.twice_case(mode)
        pairs = [tuple(k for k, w in enumerate(op.args["outputs"]) if op.args["outputs"].count(w) == 2) for op in case.circuit.opcodes[:3]]
        assert pairs == [tuple(sorted(p)) for p in hc.TWICE]
        distinct = {id(x): x for x in case.expect}.values()
        assert sum(1 for x in distinct if x.status == hr.ST_SOLVED) == 3 and sum(1 for x in distinct if x.err == hr.E_UNSATISFIED) == 6


# ---- each list bites
BITES = [("width_rounded_down", "C"), ("bytes_big_endian", "C"), ("var_size_geq", "D"), ("sha3_domain_byte", "A"), ("digest_not_reduced", "E"), ("outputs_past_conflict", "F")]


@pytest.mark.parametrize("variant,letter", BITES, ids=[f"{v} on {l}" for v, l in BITES])
def test_each_list_bites(variant, letter):
    """a model that is wrong in one way expects something else of at least one row of the list meant to catch it"""
    changed = 0
    for case in hc.lists()[letter]:
        if letter == "A" and "Keccak256, long" not in case.name:
            continue   # (one Keccak case is enough, and the quickest)
        for row, want in list(zip(case.rows, case.expect))[:23]:
            changed += not same(hr.run(case.circuit, dict(zip(case.ids, row)), variant=variant), want)
    assert changed >= 2, (variant, letter)
