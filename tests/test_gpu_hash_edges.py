"""The hash black boxes on the device (acvm_amd/csrc/ops_hash.hpp op_hash, hash_device.hpp, kernels_hash.hip: hash_coop_level_kernel<4> with two message
buffers and with one, hash_coop_level_kernel<1>, the lane-per-instance kernel, the exact path), on the case lists of tests/hash_cases.py: every message length
up to 140 bytes and around 256, 272, 352 and 1 024 in both instantiations; chains whose successors are shorter than their predecessor by 1, 2 and 3 bytes in
each kernel mode, with fused RANGE checks, and heads at the launcher's thresholds; input widths from 0 bits to the ones whose byte count wraps in 32 bits;
the variable length of Keccak; HashToField128Security with every quotient of digest / p; wrong output counts, pre-assigned outputs and one witness twice
among the outputs. Every row is compared with the Python model of the reference first (tests/hash_ref.py -- hashlib and tests/keccak_ref.py: status, error
kind, failing opcode, aux words, text, the whole witness map) and with the CPU oracle second, through the level kernels and through the exact in-order
kernels. tests/test_hash_cases.py (no GPU) proves what the lists cover, which kernel mode each case's launch takes, and that the oracle agrees with the model."""
import numpy as np
import pytest

import hash_cases as hc
import hash_ref as hr
from acvm_amd.synth import values_from_rows

pytestmark = pytest.mark.gpu

LETTERS = sorted(hc.lists())


def device_got(case, force_slow=False, batch=None):
    """((results, assigned, values) of one solve, the statistics)"""
    import acvm_amd
    own = batch is None
    if own:
        batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids)
        batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(values_from_rows(case.rows))
    n_left = batch.solve()
    assert n_left == sum(1 for x in case.expect if x.status != hr.ST_SOLVED), (case.name, n_left)
    asg, vals = batch.witness_map()
    got, stats = (batch.results(), asg, vals), batch.stats()
    if own:
        batch.free()
    return got, stats


def against_the_oracle(oracle, case, got, who):
    """the oracle second: heads, texts, assigned sets and every value, array against array"""
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(case.circuit.to_bytes()), case.ids, values_from_rows(case.rows), len(case.rows))
    res, asg, vals = got
    for j in range(len(case.rows)):
        assert res[j].as_tuple() == ores[j].as_tuple() and res[j].message == ores[j].message, f"{hc.describe(case, j)}: {who} {res[j].as_tuple()} {res[j].message!r}, oracle {ores[j].as_tuple()} {ores[j].message!r}"
    nw = min(oasg.shape[1], asg.shape[1])
    assert np.array_equal(oasg[:, :nw] != 0, asg[:, :nw] != 0), f"{case.name}: {who}: the assigned sets are not the oracle's"
    assert np.array_equal(ovals[:, :nw] * (oasg[:, :nw, None] != 0), vals[:, :nw] * (asg[:, :nw, None] != 0)), f"{case.name}: {who}: the values are not the oracle's"


def check_stats(case, stats):
    if case.meta:
        assert stats["n_hash_chained"] == case.meta["chained"], (case.name, stats["n_hash_chained"])
    # the rows that fail, and nobody else, went through the exact path
    n_failed = sum(1 for x in case.expect if x.status != hr.ST_SOLVED)
    assert stats["n_slow_instances"] == n_failed, (case.name, stats["n_slow_instances"], n_failed)


def on_the_device(oracle, case, exact=True):
    """the model first, on both paths; then the oracle"""
    got, stats = device_got(case)
    hc.compare(case, got, "device, level kernels")
    against_the_oracle(oracle, case, got, "device, level kernels")
    if stats["truncated_at"] == 0xFFFFFFFF:
        check_stats(case, stats)
    if exact:
        got, _ = device_got(case, True)
        hc.compare(case, got, "device, exact kernels")
        against_the_oracle(oracle, case, got, "device, exact kernels")
    return stats


@pytest.mark.parametrize("letter", LETTERS)
def test_every_list_on_both_paths(oracle, letter):
    for case in hc.lists()[letter]:
        on_the_device(oracle, case)


@pytest.mark.parametrize("k", range(len(hc.big_cases())), ids=[c.name for c in hc.big_cases()])
def test_the_one_wave_instantiation(oracle, k):
    """963 rows x 140 and more records on one level: more than 2 048 items of at most 32 message words, which hash_coop_level_kernel<1> takes
    (tests/test_hash_cases.py works the mode out from the counts). The level kernels' run; the rows that fail re-run on the exact path."""
    case = hc.big_cases()[k]
    assert hc.launch_mode(len(case.rows), case.meta["coop_heads"], case.meta["max_words"]) == (1, 1)
    on_the_device(oracle, case, exact=False)


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("letter", LETTERS)
def test_special_rows_in_a_partial_last_wave(letter, n):
    """passing rows in front up to 65 and 130 rows: the rows a list is about are the last wave's, beside dead lanes. A case that lets no row pass (its rows
    fail alike in every lane) stays as it is and is not run again."""
    for case in hc.lists()[letter]:
        if len(case.rows) < n and case.filler is not None:
            p = hc.padded(case, n)
            for force_slow in (False, True):
                got, _ = device_got(p, force_slow)
                hc.compare(p, got, f"device, {n} rows (exact kernels: {force_slow})")


# which lists a planner or driver key can affect: a key that cannot change a list's plan or launches is not run on it
MODES = {
    # a hash of a digest runs behind its predecessor, or gets a launch of its own on the next level: the chains of B
    "hash_chain": "B",
    # an initial witness a byte-message record reads has a 4-byte copy beside its row, or the record reads the row: A (every length; the values that are no
    # bytes), B (the chains' inputs that are no digest bytes) and F (the records whose outputs meet)
    "byte_plane": "ABF",
    # RANGE checks of at most 8 bits ride in the hash record that reads the witness, or are records of their own, eight to a record or one: only B has them
    "range_fuse": "B",
    "range_merge": "B",
    # the gates that feed hash inputs and sizes ride with light records in one launch or not: C and D have gates
    "light_fuse": "CD",
    # the hash launches (a heavy class) go to streams of their own beside the gate levels, or stay on the main stream: the lists whose circuits have levels
    # behind or beside a hash -- B (chains and the RANGE records), C and D (gates)
    "overlap": "BCD",
    "heavy_streams": "BCD",
    "heavy_only_streams": "BCD",
    # a gate output may be stored scaled / relaxed, and a hash that reads it as input or size must get the reduced value: C (sums that wrap past p) and D
    "scale": "CD",
    "relax": "CD",
}


@pytest.mark.parametrize("key", sorted(MODES))
def test_planner_and_driver_modes_switched_off(key):
    """each key off in turn, on every case of the lists whose plan or launches it can change (MODES above says which and why)"""
    import acvm_amd
    with acvm_amd.tuning(**{key: 0}):
        for letter in MODES[key]:
            for case in hc.lists()[letter]:
                got, stats = device_got(case)
                hc.compare(case, got, f"device, level kernels, {key} = 0")
                if key == "hash_chain":
                    assert stats["n_hash_chained"] == 0
                if key == "byte_plane":
                    assert stats["n_byte_planes"] == 0


def test_inputs_on_byte_planes_by_default():
    """the chains and the every-length circuits read their initial witnesses from byte planes unless the key is off"""
    import acvm_amd
    for case in (hc.chain_case("two buffers"), hc.chain_case("one buffer"), hc.length_case("Keccak256", "four waves")):
        st = acvm_amd.Circuit(case.circuit.to_bytes()).plan_stats(case.ids)
        assert st["n_byte_planes"] >= 48 and st["n_byte_plane_reads"] > st["n_byte_planes"], (case.name, st["n_byte_planes"])


def test_every_plan_checks_what_it_promises():
    """plan_validate = 1: every pass of the planner checks its own invariants while the handles of every list are built"""
    import acvm_amd
    with acvm_amd.tuning(plan_validate=1):
        for letter in LETTERS:
            for case in hc.lists()[letter]:
                got, _ = device_got(case)
                hc.compare(case, got, "device, level kernels, plan_validate")


@pytest.mark.parametrize("which", ["chain", "widths"])
def test_recycled_slots_and_a_folded_digest(oracle, which):
    """reuse_slots with fold_digest: the rows of the table are recycled, so the map leaves as its digest and the kept witnesses; both are the model's"""
    import acvm_amd
    case = hc.chain_case("two buffers", True) if which == "chain" else hc.width_case("SHA256")
    keep = [op for op in case.circuit.opcodes if hasattr(op, "args") and "outputs" in op.args][-1].args["outputs"][-3:]
    nw = case.circuit.current_witness_index + 1
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids, fold_digest=True, reuse_slots=True, keep=keep)
    batch.set_initial_witness(values_from_rows(case.rows))
    batch.solve()
    res, dig = batch.results(), batch.digest()
    solved = [j for j, x in enumerate(case.expect) if x.status == hr.ST_SOLVED]
    kept = {j: batch.extract(keep, j, 1) for j in solved if res[j].status == hr.ST_SOLVED}
    batch.free()
    assert len(solved) >= 10
    for j, x in enumerate(case.expect):
        assert res[j].as_tuple() == tuple(x[:5]), f"{hc.describe(case, j)}: device {res[j].as_tuple()}, want {tuple(x[:5])}"
    for j in solved:
        assert [int.from_bytes(kept[j][0, k].tobytes(), "big") for k in range(3)] == [case.expect[j].witnesses[w] for w in keep], hc.describe(case, j)
    for j, x in enumerate(case.expect):  # the digest is of the map as it stands: a failed row's is that of the model's partial map
        asg = [1 if w in x.witnesses else 0 for w in range(nw)]
        vals = b"".join(x.witnesses.get(w, 0).to_bytes(32, "big") for w in range(nw))
        assert bytes(dig[j]) == oracle.witness_map_digest(asg, vals), f"{hc.describe(case, j)}: the digest is not the digest of the model's map"


def test_partial_maps_while_stepping():
    """acvm_batch_solve_opcode on the chain with RANGE checks: the partial map after every step is the model's after the same number of opcodes"""
    import acvm_amd
    case = hc.chain_case("two buffers", True)
    B, n_ops = len(case.rows), len(case.circuit.opcodes)
    runs = [hr.run_stepped(case.circuit, dict(zip(case.ids, row))) for row in case.rows]
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), B, case.ids)
    batch.set_initial_witness(values_from_rows(case.rows))
    want_asg = np.zeros((B, batch.nw), dtype=np.uint8)
    want_vals = np.zeros((B, batch.nw, 32), dtype=np.uint8)

    def put(j, items):
        for w, v in items:
            want_asg[j, w] = 1
            want_vals[j, w] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)

    for j, row in enumerate(case.rows):
        put(j, zip(case.ids, row))
    for step in range(1, n_ops + 1):
        left = batch.solve_opcode()
        res = batch.results()
        for j, (final, added) in enumerate(runs):
            if step <= len(added):
                put(j, added[step - 1])
                want = (hr.ST_SOLVED, 0, 0, 0, 0) if step == n_ops else (hr.ST_IN_PROGRESS, 0, step, 0, 0)
            else:
                if step == len(added) + 1:
                    put(j, final.witnesses.items())
                want = tuple(final[:5])
            assert res[j].as_tuple()[:3] == want[:3] and (want[0] != hr.ST_FAILURE or res[j].as_tuple() == want), (step, hc.describe(case, j), res[j].as_tuple(), want)
        asg, vals = batch.witness_map()
        assert np.array_equal(asg != 0, want_asg != 0) and np.array_equal(vals * (want_asg[:, :, None] != 0), want_vals), f"after {step} steps the maps differ"
        assert left == sum(1 for final, _ in runs if not (step == n_ops and final.status == hr.ST_SOLVED))
    batch.free()


@pytest.mark.parametrize("mode", ["two buffers", "one buffer"])
def test_one_handle_solved_three_times(mode):
    """one handle: the chain's rows, then rows whose every message differs, then the first rows again. No byte of an earlier solve's messages or digests --
    in LDS behind a shorter successor, in the table -- shows in a later one."""
    import acvm_amd
    case = hc.chain_case(mode)
    second = hc.second_rows(case)
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids)
    for k, c in enumerate((case, second, case)):
        got, stats = device_got(c, batch=batch)
        hc.compare(c, got, f"device, solve {k + 1} on one handle")
        assert stats["n_hash_chained"] == 3
    batch.free()


@pytest.mark.parametrize("mode", ["two buffers", "one buffer", "lane"])
def test_one_witness_twice_among_the_outputs_on_a_used_handle(mode):
    """The second solve's rows are ground so that the byte the record COMPARES with the shared output (position 1) is what the first solve left in that
    output's row, while the byte it STORES there (position 0) is another: the reference answers UnsatisfiedConstrain at opcode 0 in every row. (In the
    cooperative kernel two waves would handle the two positions side by side, and these rows passed opcode 0 there: plan.cpp sends such records to the lane kernel.)"""
    import acvm_amd
    first, second = hc.stale_rows(mode)
    batch = acvm_amd.Batch(acvm_amd.Circuit(first.circuit.to_bytes()), len(first.rows), first.ids)
    for k, c in enumerate((first, second, first)):
        got, _ = device_got(c, batch=batch)
        hc.compare(c, got, f"device, solve {k + 1} on one handle")
    batch.free()


def test_initial_sets_that_differ_by_row(oracle):
    import acvm_amd
    circ, maps, expect, notes = hc.initial_set_case()
    multi = acvm_amd.MultiBatch(acvm_amd.Circuit(circ.to_bytes()), list(maps))
    assert multi.n_groups == 3
    multi.solve()
    res = multi.results()
    got = []
    for j in range(len(maps)):
        asg, vals = multi.witness_map(j)
        got.append((res[j].as_tuple(), res[j].message, {int(w): int.from_bytes(vals[w].tobytes(), "big") for w in np.flatnonzero(asg)}))
    case = hc.Case("G", circ, [], list(maps), list(expect), list(notes), None, {})
    hc.compare_maps(case, got, "device, MultiBatch")
    for j, m in enumerate(maps):  # and the oracle
        a = oracle.ACVM(oracle.Circuit(circ.to_bytes()), m)
        a.solve()
        assert a.result().as_tuple() == got[j][0] and a.witness_map() == got[j][2], hc.describe(case, j)
