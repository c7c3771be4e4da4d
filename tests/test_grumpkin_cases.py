"""The integer model of tests/grumpkin_ref.py against the reference's own vectors, and the case lists of tests/grumpkin_cases.py against the CPU oracle
(oracle/grumpkin.c): status, error kind, failing opcode and the whole witness map of every row must equal the Python expectation, the lists must cover
what they are built to cover (the minima below are conditions on the inputs, which the builders meet by construction), and each list must bite: one
perturbed expectation per list fails the comparison. No GPU: tests/test_gpu_grumpkin_edges.py runs the same lists on the device.

What the model is pinned to: the five vectors the reference holds for these functions (scalar_mul.rs:72-97 twice, pedersen.rs:38-54, acvm_js/test/shared/
pedersen.ts, schnorr_verify.ts). Everything else -- hash_index != 0, the empty commitment, the point at infinity as (0, 0), every rejecting signature but
by its digest -- is UNPINNED: three restatements of SURVEY Appendix A (HIP, C, Python) agreeing with one another."""
import collections

import numpy as np
import pytest

import grumpkin_cases as gc
import grumpkin_ref as gr
from grumpkin_ref import LAMBDA, P, Q

GY = 0x0000000000000002CF135E7506A45D632D270D45F1181294833FC48D823F272C


def oracle_rows(oracle, case):
    """[(status, err, opcode_index, {witness: value})] of the oracle, one per row"""
    B = len(case.rows)
    values = b"".join(v.to_bytes(32, "big") for row in case.rows for v in row)
    res, asg, vals = oracle.solve_batch(oracle.Circuit(case.circuit.to_bytes()), case.ids, values, B)
    out = []
    for j in range(B):
        wm = {int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])}
        out.append((res[j].status, res[j].err, res[j].opcode_index, wm))
    return out


def test_error_codes_are_the_oracles(oracle):
    assert (gc.ST_SOLVED, gc.ST_FAILURE, gc.E_NONE, gc.E_UNSATISFIED, gc.E_BLACKBOX_FAILED, gc.E_PANIC) == (
        oracle.ST_SOLVED, oracle.ST_FAILURE, oracle.E_NONE, oracle.E_UNSATISFIED, oracle.E_BLACKBOX_FAILED, oracle.E_PANIC)


# ---------------------------------------------------------------------------------------------- the model against the reference's vectors
def test_model_reproduces_the_reference_vectors(golden):
    R = gr.ref()
    # scalar_mul.rs:72-97 and pedersen.rs:38-54 (tests/test_gpu_grumpkin.py test_rust_unit_vectors)
    assert R.fixed_base(1, 0) == (gr.FB_OK, (1, GY))
    assert R.fixed_base(1, 2) == (gr.FB_OK, (0x0702AB9C7038EEECC179B4F209991BCB68C7CB05BF4C532D804CCAC36199C9A9, 0x23F10E9E43A3AE8D75D24154E796AAE12AE7AF546716E8F81A2564F1B5814130))
    assert R.pedersen([0, 1], 0) == (0x0C5E1DDECD49DE44ED5E5798D3F6FB7C71FE3D37F5BEE8664CF88A445B5BA0AF, 0x230294A041E26FE80B827C2EF5CB8784642BBAA83842DA2714D62B1F3C4F9752)
    # the acvm_js fixtures: the circuit's inputs through the model, every expected witness
    for name, run in (("fixed_base_scalar_mul", lambda w: R.fixed_base(w[1], w[2])[1]), ("pedersen", lambda w: R.pedersen([w[1]], 0))):
        fx = golden["acvm_js"][name]
        iw = {int(k): int(v, 16) for k, v in fx["initialWitnessMap"].items()}
        want = {int(k): int(v, 16) for k, v in fx["expectedWitnessMap"].items()}
        outs = sorted(set(want) - set(iw))
        assert len(outs) == 2 and run(iw) == (want[outs[0]], want[outs[1]]), name
    fx = golden["acvm_js"]["schnorr_verify"]
    iw = {int(k): int(v, 16) for k, v in fx["initialWitnessMap"].items()}
    want = {int(k): int(v, 16) for k, v in fx["expectedWitnessMap"].items()}
    pk, sig, msg = (iw[1], iw[2]), bytes(iw[i] & 255 for i in range(3, 67)), bytes(iw[i] & 255 for i in range(67, 77))
    out = sorted(set(want) - set(iw))
    assert len(out) == 1 and want[out[0]] == 1 and R.schnorr_verify(pk, sig, msg)
    assert not R.schnorr_verify(pk, sig, b"\x01" + msg[1:])
    # SURVEY A.3's intermediates of that vector
    s, e = int.from_bytes(sig[:32], "big") % Q, int.from_bytes(sig[32:], "big") % Q
    assert R.schnorr_point(pk, s, e) == (0x2EC2A0154DCF06E1D6EB7048636869C789FFFE3F3CB8B93226A6EF7B4AAF05E9, 0x18C1ECB6A8718257EE0988BDAE7AF1B39E02E177076A2113B7C0E33904D97348)
    assert R.compress((1, 2, 3)) == 0x1953091855EF296FB51DB6232AD7B20CC1563001B9CED4FBF0571B6BA04E676D
    assert gr.reduce_count(int.from_bytes(sig[32:], "big")) >= 1   # (the vector's e exceeds q)


def test_model_failure_classes_and_the_empty_commitment():
    R = gr.ref()
    assert R.fixed_base(1 << 128, 1 << 128)[0] == gr.FB_LIMB_LOW and R.fixed_base(0, 1 << 128)[0] == gr.FB_LIMB_HIGH
    assert R.fixed_base(Q & gc.M128, Q >> 128)[0] == gr.FB_SCALAR and R.fixed_base((Q - 1) & gc.M128, (Q - 1) >> 128) == (gr.FB_OK, (1, P - GY))
    assert R.fixed_base(0, 0) == (gr.FB_OK, (0, 0)) and R.pedersen([], 7) == (0, 0)
    assert R.pedersen([5], 0) != R.pedersen([5], 1) != R.pedersen([5], (1 << 32) - 1)


# ---------------------------------------------------------------------------------------------- the lists against the oracle
@pytest.mark.parametrize("name", list(gc.CASE_BUILDERS))
def test_oracle_agrees_with_integers(oracle, name):
    case = gc.case(name)
    gc.compare(case, oracle_rows(oracle, case), "oracle")


@pytest.mark.parametrize("name,what", gc.PERTURBATIONS)
def test_each_list_bites(oracle, name, what):
    """one expected value per list moved (a coordinate, a status, a verdict, a failing opcode): the comparison with the oracle must fail, and must name that row"""
    j, bad = gc.perturbed(name, what)
    got = oracle_rows(oracle, bad)
    gc.compare(gc.case(name), got, "oracle")
    with pytest.raises(AssertionError, match=f"row {j} "):
        gc.compare(bad, got, "oracle")


# ---------------------------------------------------------------------------------------------- what the lists cover
def test_pedersen_values_cover_every_slice_pair_and_window():
    values = [v for v, _ in gc.pedersen_values()]
    assert {0, 1, P - 1, P - 2, 1 << 253, gc.ALL} <= set(values)
    for kind, (width, n) in gc.FIELDS.items():
        assert width * n >= 254 > width * (n - 1)
        for i in range(n):
            full = gc.ones_below_p(width * i, width) >> (width * i)
            # all ones: the whole field, or at the top of the value as many ones as a value below P can carry there
            assert full == (1 << width) - 1 or (i == n - 1 and full == (1 << (full.bit_length())) - 1 and (2 * full + 1) << (width * i) >= P), (kind, i)
            assert any(gc.field_of(v, kind, i) == full and v == full << (width * i) for v in values), (kind, i)            # alone
            near = [j for j in (i - 1, i + 1) if 0 <= j < n]
            assert any(gc.field_of(v, kind, i) == 0 and all(gc.field_of(v, kind, j) == gc.field_of(gc.ALL, kind, j) for j in near) for v in values), (kind, i)
    for width, n in ((18, 15), (24, 11)):
        for i in range(1, n):
            assert {(1 << (width * i)) - 1, (1 << (width * i)) + 1} <= set(values)


def test_pedersen_cases_cover_counts_indices_batches_and_compared_outputs():
    one, six, cmp_ = gc.pedersen_single_case(), gc.pedersen_records_case(), gc.pedersen_compared_case()
    assert sorted(len(c.rows) for c in (one, six, cmp_)) == list(gc.BATCH_SIZES)
    assert len(one.circuit.opcodes) == 1 and len(six.circuit.opcodes) >= 5
    counts = [len(op.args["inputs"]) for op in six.circuit.opcodes]
    assert counts == [1, 2, 4, 5, 8, 20] and sum(1 for n in counts if n >= 4) >= 4      # the quad kernel's tail rotation: n >= 4, several records, several blocks
    indices = {op.args["domain_separator"] for c in (one, six, cmp_) for op in c.circuit.opcodes}
    assert indices == set(gc.HASH_INDICES)
    values = {v for v, _ in gc.pedersen_values()}
    assert values <= {row[0] for row in one.rows}
    assert values <= {v for row in six.rows for v in row}
    assert all(x.status == gc.ST_SOLVED for c in (one, six) for x in c.expect)
    kinds = collections.Counter((x.status, x.err, x.opcode_index) for x in cmp_.expect)
    assert kinds[(gc.ST_SOLVED, gc.E_NONE, 0)] >= 20 and kinds[(gc.ST_FAILURE, gc.E_UNSATISFIED, 0)] >= 20 and kinds[(gc.ST_FAILURE, gc.E_UNSATISFIED, 1)] >= 20


def test_fixed_base_scalars_cover_both_window_widths_and_the_refusals():
    R = gr.ref()
    rows = gc.fixed_base_scalars()
    ks = {hi << 128 | lo for lo, hi, _ in rows if lo <= gc.M128 and hi <= gc.M128}
    for bits, n in ((16, 16), (8, 32)):
        top = (1 << bits) - 1
        for w in range(n):
            largest = min(top, (Q - 1) >> (bits * w))   # (the top window ends at q)
            assert 1 << (bits * w) in ks and largest << (bits * w) in ks, (bits, w)
    assert all((1 << (16 * w)) - 1 in ks for w in range(1, 16))
    assert {Q - 1, Q - 2, (Q - 1) // 2, 0} <= ks
    assert any(lo == gc.M128 and ((hi + 1) << 128 | lo) >= Q > (hi << 128 | lo) for lo, hi, _ in rows)
    classes = collections.Counter(R.fixed_base(lo, hi)[0] for lo, hi, _ in rows)
    assert classes[gr.FB_LIMB_LOW] >= 3 and classes[gr.FB_LIMB_HIGH] >= 1 and classes[gr.FB_SCALAR] >= 4 and classes[gr.FB_OK] >= 100
    assert {(1 << 128, 0), (P - 1, 0), (0, 1 << 128), (Q & gc.M128, Q >> 128), ((Q + 1) & gc.M128, (Q + 1) >> 128), (0, 1 << 126)} <= {(lo, hi) for lo, hi, _ in rows}
    case = gc.fixed_base_case()
    assert [tuple(r) for r in case.rows[:len(rows)]] == [(lo, hi) for lo, hi, _ in rows]
    assert sum(1 for x in case.expect if x.err == gc.E_BLACKBOX_FAILED) == classes[gr.FB_LIMB_LOW] + classes[gr.FB_LIMB_HIGH] + classes[gr.FB_SCALAR]


def test_accepting_signatures_cover_keys_lengths_and_every_reduction_count():
    counts, halves16, halves0 = collections.Counter(), set(), set()
    for n in gc.MSG_LENGTHS:
        signed = gc.signed_messages(n)
        assert {s.sk for s in signed} >= {1, 2, Q - 1, LAMBDA, Q - LAMBDA} and len({s.sk for s in signed}) >= 6 and all(len(s.msg) == n for s in signed)
        case = gc.schnorr_accepting_case(n)
        assert all(x.witnesses[max(x.witnesses)] == 1 for x in case.expect)
        assert sum(1 for note in case.notes if " q" in note) >= 3 * len(signed)   # s + m q: 2^256 / q > 5, so four or five variants each
        for s in signed:
            e = int.from_bytes(s.sig[32:], "big")
            counts[gr.reduce_count(e)] += 1
            _, a16, b16, a0, b0 = gc.split_class(e)
            halves16 |= {h for h, f in ((1, a16), (2, b16)) if f}
            halves0 |= {h for h, f in ((1, a0), (2, b0)) if f}
    assert {s.k for n in gc.MSG_LENGTHS for s in gc.signed_messages(n)} >= {1, 2, Q - 1}
    assert all(counts[c] >= 2 for c in range(6)), counts
    assert halves16 == {1, 2} and halves0 == {1, 2}
    assert {32 + n for n in gc.MSG_LENGTHS} >= {63, 64, 65, 127, 128, 129} and max(gc.MSG_LENGTHS) + 128 == 1023


def test_rejecting_and_cell_rows_cover_every_reason():
    rej = gc.schnorr_rejecting_case()
    for reason in ("bit of s", "bit of e", "bit of the message", "pk_y negated", "off the curve", "pk = (0, 0)", "s = 0", "s = q", "e = 0", "e = q", "doubles", "infinity", "e sk + q"):
        assert sum(1 for n in rej.notes if reason in n) >= 6, reason
    R = gr.ref()
    for row, note in zip(rej.rows, rej.notes):   # the two exceptional groups are what their notes say
        if "doubles" in note or "infinity" in note:
            pk, s, e = (row[0], row[1]), int.from_bytes(bytes(row[2:34]), "big") % Q, int.from_bytes(bytes(row[34:66]), "big") % Q
            a, b = gr.ec_mul(gr.GRUMPKIN, e, pk), R.mul_g(s)
            assert (a == b) if "doubles" in note else (a == gr.neg(b) and R.schnorr_point(pk, s, e) is None), note
    cells = gc.schnorr_cells_case()
    sig_msg = [v for row in cells.rows for v in row[2:-1]]
    assert sum(1 for v in sig_msg if 256 <= v < P - 256) >= 500 and sum(1 for v in sig_msg if v >= P - 256) >= 500 and sum(1 for v in sig_msg if v < 256) >= 500
    kinds = collections.Counter((x.status, x.err, x.witnesses[max(x.witnesses)]) for x in cells.expect)
    assert all(kinds[k] >= 5 for k in ((gc.ST_SOLVED, gc.E_NONE, 0), (gc.ST_SOLVED, gc.E_NONE, 1), (gc.ST_FAILURE, gc.E_UNSATISFIED, 0), (gc.ST_FAILURE, gc.E_UNSATISFIED, 1))), kinds
    short, long_ = gc.schnorr_panic_cases()
    assert len(short.circuit.opcodes[0].args["signature"]) == 63 and len(long_.circuit.opcodes[0].args["message"]) == 896


def test_split_scalars_cover_the_sign_classes_that_exist():
    """k1 >= 0 always (the argument stands at grumpkin_ref.glv_split, which asserts it for every scalar it is given); k2 < 0 for a random scalar"""
    classes, sixteen, top_zero = collections.Counter(), set(), set()
    scalars = [k for k, _ in gc.split_scalars()]
    for n in gc.MSG_LENGTHS:
        scalars += [int.from_bytes(s.sig[32:], "big") % Q for s in gc.signed_messages(n)]
    scalars += [t.e for t in gc.r_triples()]
    for k in scalars:
        k1, k2 = gr.glv_split(k)
        assert k1 >= 0, hex(k)                               # no scalar of the lists has k1 < 0
        d1, d2 = gr.signed_windows5(k1), gr.signed_windows5(abs(k2))
        sixteen |= {h for h, d in ((1, d1), (2, d2)) if 16 in d or -16 in d}
        top_zero |= {h for h, d in ((1, d1), (2, d2)) if d[25] == 0}
    for k, _ in gc.split_scalars():
        k2 = gr.glv_split(k)[1]
        classes[(k2 > 0) - (k2 < 0)] += 1
    assert classes[-1] >= 8 and classes[1] >= 8 and classes[0] >= 8, classes
    assert sixteen == {1, 2} and top_zero == {1, 2}
    assert sum(1 for k, _ in gc.split_scalars() if all(d in (0, 16) for d in gr.signed_windows5(gr.glv_split(k)[0])) and k > 16) >= 2   # whole runs of digit 16
    # and over the scalar range at large: a seeded sample never leaves the class (k1 >= 0, k2 < 0)
    import random
    rng = random.Random(gc.SEED)
    assert all(gr.glv_split(rng.randrange(Q))[1] < 0 for _ in range(2000))


def test_probe_lists_hold_the_exceptional_items():
    for which, n in (("dbl", 3), ("add_aff29", 5), ("add", 6)):
        items = gc.formula_items(which)
        assert len(items) % 64 and all(len(it.coords) == n == len(it.reps) for it in items)
        notes = collections.Counter(it.note.split(",")[0].split(":")[0] for it in items)
        if which == "dbl":
            assert notes["Y = 0 (mod p)"] >= 24 and notes["Z = 0 (mod p)"] >= 24 and notes["ordinary"] >= 18
            assert {it.reps[1] for it in items if it.note.startswith("Y = 0")} == {0, 1} and {it.reps[2] for it in items if it.note.startswith("Z = 0")} == {0, 1}
        else:
            assert notes["doubling"] >= 2 ** n and notes["opposite points"] >= 2 ** n and notes["ordinary"] >= 30 and notes["P at infinity"] >= 2 ** n
            for kind in ("doubling", "opposite points", "P at infinity"):    # every coordinate in both representatives
                assert {it.reps for it in items if it.note.startswith(kind)} >= set(gc._reps(n, None, True)), (which, kind)
            assert all((it.want is None) == it.note.startswith(("opposite", "both")) for it in items)
        if which == "add":
            assert notes["Q at infinity"] >= 64 and notes["both at infinity"] >= 64
            assert {it.note for it in items} >= {"doubling, equal Z", "doubling, different Z", "opposite points, equal Z", "opposite points, different Z"}
    triples = gc.r_triples()
    assert sum(1 for t in triples if t.want is None) >= 30 and sum(1 for t in triples if "e sk +0" in t.note and "-e sk" not in t.note) >= 30
    assert sum(1 for t in triples if "window end" in t.note) >= 30
