"""MemoryInit / MemoryOp on the device (acvm_amd/csrc/ops_light.hpp op_mem_init / op_mem_op, the block passes of plan.cpp, the replay of memory side effects
in exact_run_kernel, run_exact_segments in batch_exact.cpp), on the case lists of tests/mem_cases.py: indices at and past the block's end, at 2^32, 2^64 and
p - 1, in every form an index takes; operations that are witnesses or expressions; read targets that only become a witness after evaluation; written values
with unknown witnesses; blocks re-initialised shorter, longer and empty, or never initialised; seeded programs whose rows take their event in mid-program;
memory state across a foreign call, a step-limit retry, stepping and handle reuse. Every row is compared with the Python model of the reference first
(tests/mem_ref.py: status, error kind, failing opcode, aux words, panic text, the whole witness map) and with the CPU oracle second, through the level
kernels and through the exact in-order kernels. tests/test_mem_cases.py (no GPU) proves what the lists cover and that the oracle agrees with the model."""
import numpy as np
import pytest

import mem_cases as mc
import mem_ref as mr
from acvm_amd.synth import values_from_rows
from test_gpu_foreign_call import drive
from test_gpu_opcodes import both_paths

pytestmark = pytest.mark.gpu

LETTERS = sorted(mc.lists())


def rows_of(batch, res):
    """the rows of a solve as mc.compare takes them"""
    asg, vals = batch.witness_map()
    return [(r.as_tuple(), r.message, {int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])}) for j, r in enumerate(res)]


def device_rows(case, force_slow, respond=None, sites=None):
    """(the rows of one solve, the statistics); respond: the host's answers to rows that wait; sites: a list that takes the sites at which rows wait"""
    import acvm_amd
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids)
    batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(values_from_rows(case.rows))
    if respond:
        _, res = drive(batch, len(case.rows), respond)
    else:
        batch.solve()
        res = batch.results()
    if sites is not None:
        sites += batch.foreign_call_sites()
    got, stats = rows_of(batch, res), batch.stats()
    batch.free()
    return got, stats


def device_against_the_model(case, expect=None):
    """both paths; the statistics of the level kernels' run"""
    got, stats = device_rows(case, False)
    mc.compare(case, got, "device, level kernels", expect)
    got, _ = device_rows(case, True)
    mc.compare(case, got, "device, exact kernels", expect)
    return stats


def on_the_device(oracle, case):
    """the model first, on both paths; then the oracle (test_gpu_opcodes.run_both, both paths)"""
    stats = device_against_the_model(case)
    both_paths(oracle, case.circuit, case.ids, case.rows)
    return stats


@pytest.mark.parametrize("letter", LETTERS)
def test_every_list_on_both_paths(oracle, letter):
    for case in mc.lists()[letter]:
        stats = on_the_device(oracle, case)
        if letter == "F":  # the failing rows, and nobody else, went through the exact path and its replay
            assert stats["n_slow_instances"] == sum(1 for x in case.expect if x.status == mr.ST_FAILURE) == 5, (case.name, stats["n_slow_instances"])
            assert stats["n_levels"] * 3 < stats["n_opcodes"] and stats["truncated_at"] == 0xFFFFFFFF
        if letter == "G" and stats["truncated_at"] == 0xFFFFFFFF:  # the straight-line Brillig opcode is a light record of the level schedule
            assert stats["n_brillig_inlined"] == 1, (case.name, stats["n_brillig_inlined"])


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("letter", LETTERS)
def test_special_rows_in_a_partial_last_wave(letter, n):
    """passing rows in front up to 65 and 130 rows: the rows a list is about are the last wave's, beside dead lanes. A case that has that many rows
    already (A: 135, which is two waves and seven rows) or lets no row pass (its rows fail alike in every lane) stays as it is and is not run again."""
    for case in mc.lists()[letter]:
        if len(case.rows) < n and case.filler is not None:
            device_against_the_model(mc.padded(case, n))


# which lists a planner or driver key can affect: a key that cannot change a list's plan or launches is not run on it
MODES = {
    # the light records (every MemoryInit / MemoryOp is one) ride in the gate launch of their level, or get launches of their own: every list has a gate
    # somewhere, so every list runs
    "light_fuse": "ABCDEFG",
    # the heavy lanes (the Brillig opcodes of G) and the inversion batches of the gates run on streams of their own, or on the main stream between the
    # memory levels: F (gates between memory ops) and G
    "overlap": "FG",
    # a gate output may be stored scaled / relaxed, and a MemoryOp that reads it as index, value or predicate must get the reduced value: A (the index
    # that is the sum of two gate outputs and wraps past p) and F (gate outputs as indices)
    "scale": "AF",
    "relax": "AF",
    # only G has Brillig opcodes: the straight-line one between its writes and its reads is inlined by default (test_every_list_on_both_paths asserts that)
    # and runs in the VM kernel with the key off (in the circuits with a witness operation the plan ends in front of it: nothing is inlined either way)
    "brillig_inline": "G",
}


@pytest.mark.parametrize("key", sorted(MODES))
def test_planner_and_driver_modes_switched_off(key):
    """each key off in turn, on every case of the lists whose plan or launches it can change (MODES above says which and why): light_fuse on every list;
    overlap on F and G; scale and relax on A and F, the lists whose gate outputs a MemoryOp reads; brillig_inline on G, the only list with Brillig opcodes."""
    import acvm_amd
    with acvm_amd.tuning(**{key: 0}):
        for letter in MODES[key]:
            for case in mc.lists()[letter]:
                stats = device_against_the_model(case)
                if key == "brillig_inline":
                    assert stats["n_brillig_inlined"] == 0


def test_every_plan_checks_what_it_promises():
    """plan_validate = 1: every pass of the planner checks its own invariants while the handles of every list are built"""
    import acvm_amd
    with acvm_amd.tuning(plan_validate=1):
        for letter in LETTERS:
            for case in mc.lists()[letter]:
                got, _ = device_rows(case, False)
                mc.compare(case, got, "device, level kernels, plan_validate")


def kept_witnesses(case):
    """the targets of the circuit's last three reads"""
    reads = [op.value.linear_combinations[0][1] for op in case.circuit.opcodes if hasattr(op, "block_id") and hasattr(op, "operation") and mr.is_constant(op.operation)
             and op.operation.q_c == 0]
    return reads[-3:]


@pytest.mark.parametrize("letter", ["A", "F"])
def test_recycled_slots_and_a_folded_digest(oracle, letter):
    """reuse_slots with fold_digest: the rows of the table are recycled, so the map leaves as its digest and the kept witnesses; both are the model's. The
    kept witnesses of a row that failed are not handed out (extract refuses an unassigned witness); its digest is compared like every other row's."""
    import acvm_amd
    for case in mc.lists()[letter]:
        keep = kept_witnesses(case)
        nw = case.circuit.current_witness_index + 1
        batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids, fold_digest=True, reuse_slots=True, keep=keep)
        batch.set_initial_witness(values_from_rows(case.rows))
        batch.solve()
        res, dig = batch.results(), batch.digest()
        solved = [j for j, x in enumerate(case.expect) if x.status == mr.ST_SOLVED]
        kept = {j: batch.extract(keep, j, 1) for j in solved if res[j].status == mr.ST_SOLVED}
        batch.free()
        assert len(solved) >= 20
        for j, x in enumerate(case.expect):
            assert res[j].as_tuple() == tuple(x[:5]), f"{mc.describe(case, j)}: device {res[j].as_tuple()}, want {tuple(x[:5])}"
            if x.message is not None:
                assert res[j].message == x.message, mc.describe(case, j)
        for j in solved:
            x = case.expect[j]
            assert [int.from_bytes(kept[j][0, k].tobytes(), "big") for k in range(len(keep))] == [x.witnesses[w] for w in keep], mc.describe(case, j)
        for j, x in enumerate(case.expect):  # the digest is of the map as it stands: a failed row's is that of the model's partial map
            asg = [1 if w in x.witnesses else 0 for w in range(nw)]
            vals = b"".join(x.witnesses.get(w, 0).to_bytes(32, "big") for w in range(nw))
            assert bytes(dig[j]) == oracle.witness_map_digest(asg, vals), f"{mc.describe(case, j)}: the digest is not the digest of the model's map"


# ---- G: re-entries
@pytest.mark.parametrize("relevel", [0, 1])
@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_memory_across_a_foreign_call_answered_per_instance(dynamic, relevel):
    """every row waits at the Brillig opcode behind the writes; the host answers; the reads behind the call see the cells as the writes left them"""
    import acvm_amd
    case = mc.reentry_case("call", dynamic)
    expect = mc.answered_expect(case)
    with acvm_amd.tuning(fc_relevel=relevel):
        for force_slow in (False, True):
            sites = []
            got, _ = device_rows(case, force_slow, sites=sites)
            mc.compare(case, got, "device, waiting")
            assert [(s["opcode_index"], s["n_waiting"]) for s in sites] == [(case.expect[0].opcode_index, len(case.rows))]  # where every row stands
            asked = {}

            def respond(j, fn, inputs):
                asked[j] = (fn, inputs)
                return mc.answer_of(case.rows[j])

            got, _ = device_rows(case, force_slow, respond)
            assert asked == {j: x.pending for j, x in enumerate(case.expect)}
            mc.compare(case, got, f"device, answered (exact kernels: {force_slow})", expect)


@pytest.mark.parametrize("relevel", [0, 1])
@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_memory_across_a_foreign_call_answered_as_a_device_column(dynamic, relevel):
    """the same round trip through acvm_batch_resolve_foreign_calls_device: one column of answers for the whole waiting list"""
    import acvm_amd
    case = mc.reentry_case("call", dynamic)
    expect = mc.answered_expect(case)
    B = len(case.rows)
    with acvm_amd.tuning(fc_relevel=relevel):
        batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), B, case.ids)
        batch.set_initial_witness(values_from_rows(case.rows))
        assert batch.solve() == B
        sites = batch.foreign_call_sites()
        assert len(sites) == 1 and sites[0]["n_waiting"] == B and sites[0]["opcode_index"] == case.expect[0].opcode_index
        answers = acvm_amd.DeviceBuffer(b"".join(mc.answer_of(row)[0].to_bytes(32, "big") for row in case.rows))  # the waiting list ascends by instance
        batch.resolve_foreign_calls_device(sites[0]["opcode_index"], sites[0]["brillig_index"], [None], answers.ptr)
        assert batch.solve() == 0
        got = rows_of(batch, batch.results())
        batch.free()
        answers.free()
    mc.compare(case, got, "device, answered by a column", expect)


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_memory_across_a_step_limit_retry(oracle, dynamic):
    """with the level kernels' step limit at 2^8 the loops of 63 iterations and more reach it and are run again with the limit raised (batch.cpp
    retry_device_limits): the exact path re-enters behind the writes and in front of the reads"""
    import acvm_amd
    case = mc.reentry_case("loop", dynamic)
    assert {row[7] for row in case.rows} == set(mc.LOOP_COUNTS) and min(n for n in mc.LOOP_COUNTS if 4 * n + 5 > 1 << mc.LOOP_STEPS_LOG2) == 63
    with acvm_amd.tuning(brillig_steps_log2=mc.LOOP_STEPS_LOG2):
        stats = on_the_device(oracle, case)
    assert all(x.status == mr.ST_SOLVED for x in case.expect)
    assert stats["n_brillig_retries"] >= 1, stats["n_brillig_retries"]


# ---- F: stepping and handle reuse
def test_partial_maps_while_stepping():
    """acvm_batch_solve_opcode on every row of a program of list F: the partial map after every step is the model's after the same number of opcodes --
    rows that pass, rows that end at each tripwire and at the out-of-bounds index. The model's maps are kept as the arrays witness_map returns and grow
    by what each step adds."""
    import acvm_amd
    case = mc.order_case(mc.ORDER_SEEDS[0])[0]
    B, n_ops = len(case.rows), len(case.circuit.opcodes)
    runs = [mr.run_stepped(case.circuit, dict(zip(case.ids, row))) for row in case.rows]
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
            if step <= len(added):  # the row got through this opcode
                put(j, added[step - 1])
                want = (mr.ST_SOLVED, 0, 0, 0, 0) if step == n_ops else (mr.ST_IN_PROGRESS, 0, step, 0, 0)
            else:
                if step == len(added) + 1:  # it ends here: whatever the failing opcode still put into the map
                    put(j, final.witnesses.items())
                want = tuple(final[:5])
            assert res[j].as_tuple()[:3] == want[:3] and (want[0] != mr.ST_FAILURE or res[j].as_tuple() == want), (step, mc.describe(case, j), res[j].as_tuple(), want)
        asg, vals = batch.witness_map()
        if not (np.array_equal(asg != 0, want_asg != 0) and np.array_equal(vals * (want_asg[:, :, None] != 0), want_vals)):
            bad = np.argwhere(((asg != 0) != (want_asg != 0)) | (vals * (want_asg[:, :, None] != 0) != want_vals).any(axis=2))
            raise AssertionError(f"after {step} steps the maps differ at (row, witness) {bad[:8].tolist()}")
        assert left == sum(1 for final, _ in runs if not (step == n_ops and final.status == mr.ST_SOLVED))
    assert {len(added) for final, added in runs if final.status == mr.ST_FAILURE} == {final.opcode_index for final, _ in runs if final.status == mr.ST_FAILURE}
    batch.free()


def test_one_handle_solved_again_and_again():
    """one handle: rows that fail, then rows that all pass, then the failures at other instances and tripwires, then one instance alone (failing, then passing).
    No cell, witness or event of an earlier solve shows in a later one."""
    import acvm_amd
    case, failing, _ = mc.order_case(mc.ORDER_SEEDS[1])
    B = len(case.rows)
    passing = [j for j in range(B) if j not in failing]
    first = list(range(B))
    second = [j if j not in failing else passing[k] for k, j in enumerate(range(B))]
    third = first[-9:] + first[:-9]
    third[third.index(failing[0])], third[third.index(failing[2])] = failing[2], failing[0]
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), B, case.ids)
    for order in (first, second, third, [failing[4]], [passing[3]], [failing[1]]):
        if len(order) == 1 and batch.B != 1:
            batch.set_instances(1)
        sub = case._replace(rows=[case.rows[j] for j in order], expect=[case.expect[j] for j in order], notes=[case.notes[j] for j in order])
        batch.set_initial_witness(values_from_rows(sub.rows))
        n_bad = sum(1 for x in sub.expect if x.status != mr.ST_SOLVED)
        assert batch.solve() == n_bad
        mc.compare(sub, rows_of(batch, batch.results()), f"device, solve of {len(order)} rows on the reused handle")
        assert batch.stats()["n_slow_instances"] == n_bad
    batch.free()


# ---- H
def test_initial_sets_that_differ_by_row(oracle):
    import acvm_amd
    circ, maps, expect, notes = mc.initial_set_case()
    multi = acvm_amd.MultiBatch(acvm_amd.Circuit(circ.to_bytes()), list(maps))
    assert multi.n_groups == 3
    multi.solve()
    res = multi.results()
    got = []
    for j in range(len(maps)):
        asg, vals = multi.witness_map(j)
        got.append((res[j].as_tuple(), res[j].message, {int(w): int.from_bytes(vals[w].tobytes(), "big") for w in np.flatnonzero(asg)}))
    case = mc.Case("H", circ, [], list(maps), list(expect), list(notes), None, None)
    mc.compare(case, got, "device, MultiBatch")
    for j, m in enumerate(maps):  # and the oracle
        a = oracle.ACVM(oracle.Circuit(circ.to_bytes()), m)
        a.solve()
        assert a.result().as_tuple() == got[j][0] and a.witness_map() == got[j][2], mc.describe(case, j)
