"""Opcode::Arithmetic on the device (acvm_amd/csrc/plan.cpp level_gate, gate_eval.hpp, the inversion batches, the hand-over of a flagged row to
exact_run_kernel), on the case lists of tests/arith_cases.py: the shapes as written (zero coefficients, duplicate terms, x x, residual products), the rows
that leave the generic path (zero partners of SOLVE_DYN gates and what follows them, failing asserts, the first failure in program order), the values and
counts of the folded gate (forced outputs at the limb boundaries, sums that are k p, the side-sum budget, the periodic reduction, the 8-bit count fields,
the grid of record shapes) and initial sets that differ by row. Every row is compared with the Python model of the reference first (tests/arith_ref.py:
status, error kind, failing opcode, aux words, panic text, the whole witness map, the expression of a TooManyUnknowns row) and with the CPU oracle second,
through the level kernels and through the exact in-order kernels. tests/test_arith_cases.py (no GPU) proves what the lists cover, which record shapes the
plans of list C hold, and that the oracle agrees with the model."""
import numpy as np
import pytest

import arith_cases as ac
import arith_ref as ar
from acvm_amd.acir import BlackBoxFuncCall
from acvm_amd.synth import values_from_rows
from test_gpu_opcodes import both_paths

pytestmark = pytest.mark.gpu

LETTERS = sorted(ac.lists())
TOO_MANY = "Cannot solve opcode: expression has too many unknowns "


def rows_of(batch, res):
    """the rows of a solve as ac.compare takes them"""
    asg, vals = batch.witness_map()
    return [(r.as_tuple(), r.message, {int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])}) for j, r in enumerate(res)]


def check_expressions(case, batch, who, expect=None):
    """Batch.error_expression / error_string of every row: the evaluated expression of a TooManyUnknowns row, as data and in the reference's Display; no
    expression anywhere else"""
    for j, x in enumerate(expect or case.expect):
        got = batch.error_expression(j)
        if x.expression is None:
            assert got is None, f"{ac.describe(case, j)}: {who} reports the expression {got} of a row that has none"
            continue
        mul, lin, qc = x.expression
        assert got == {"opcode_index": x.opcode_index, "mul": mul, "lin": lin, "q_c": qc}, f"{ac.describe(case, j)}: {who} expression {got}, want {x.expression}"
        assert batch.error_string(j) == TOO_MANY + ar.expr_display(mul, lin, qc), f"{ac.describe(case, j)}: {who} error string {batch.error_string(j)!r}"


def device_rows(case, force_slow, who="device", **handle):
    """(the rows of one solve, the statistics), the expressions checked on the way"""
    import acvm_amd
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids, **handle)
    batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(values_from_rows(case.rows))
    n_left = batch.solve()
    assert n_left == sum(1 for x in case.expect if x.status != ar.ST_SOLVED), (case.name, n_left)
    got, stats = rows_of(batch, batch.results()), batch.stats()
    check_expressions(case, batch, who)
    batch.free()
    return got, stats


def device_against_the_model(case, who=""):
    """both paths; the statistics of the level kernels' run"""
    got, stats = device_rows(case, False)
    ac.compare(case, got, "device, level kernels" + who)
    assert stats["truncated_at"] == ac.expected_truncation(case), (case.name, stats["truncated_at"])
    got, _ = device_rows(case, True)
    ac.compare(case, got, "device, exact kernels" + who)
    return stats


def has_range(case):
    return any(isinstance(op, BlackBoxFuncCall) for op in case.circuit.opcodes)


@pytest.mark.parametrize("letter", LETTERS)
def test_every_list_on_both_paths(oracle, letter):
    """the model first, on both paths; then the oracle (test_gpu_opcodes.both_paths). On list B exactly the rows that deviate for the model took the exact
    path; on A and C the plan ends where tests/test_arith_cases.py found it to end (device_against_the_model)."""
    for case in ac.lists()[letter]:
        stats = device_against_the_model(case)
        both_paths(oracle, case.circuit, case.ids, case.rows)
        if letter == "B":
            assert stats["n_slow_instances"] == sum(1 for x in case.expect if ac.deviates(x)), (case.name, stats["n_slow_instances"])


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("letter", LETTERS)
def test_special_rows_in_a_partial_last_wave(letter, n):
    """passing rows in front up to 65 and 130 rows: the rows a case is about are the last wave's, beside dead lanes. A case that has that many rows already
    (list B's own placements) or lets no row pass (its rows end alike in every lane) stays as it is and is not run again."""
    for case in ac.lists()[letter]:
        if len(case.rows) < n and case.filler is not None:
            padded = ac.padded(case, n)
            stats = device_against_the_model(padded, f", padded to {n}")
            if letter == "B":
                assert stats["n_slow_instances"] == sum(1 for x in padded.expect if ac.deviates(x)), (case.name, n)


# which lists a planner or driver key can affect, and the value that switches it off: a key that cannot change a list's plan or launches is not run on it
MODES = {
    # the projective scales move every coefficient of every gate that has a general one, and every stored output behind it: all three lists. With the key
    # off list C's records are the circuit's terms as written (tests/test_arith_cases.py test_list_c_as_written_without_projective_scales)
    "scale": (0, "ABC"),
    # relaxed rows: every output that only gates read is stored as it comes -- A's and B's few, and the bounds list C is built around
    "relax": (0, "ABC"),
    # wave programs need a gate that reads the output of the gate before it: A's circuits of three to six dependent gates, B's chain, C
    "pairs": (0, "ABC"),
    # a tail behind a tail, and more than zero tails: only where a third dependent gate follows -- B's chain of twenty products and list C
    "chains": (0, "BC"),
    "max_tails": (0, "BC"),
    # only records of general linear terms without a product carry tables: A's have none that list C does not have in every count
    "lin_table": (0, "C"),
    # the light records here are the RANGE readers: the cases that have one (has_range) of every list
    "light_fuse": (0, "ABC"),
    # the inversion batches run on a stream of their own, or on the main stream between the gate levels: the lists with SOLVE_DYN gates in numbers
    "overlap": (0, "BC"),
}


@pytest.mark.parametrize("key", sorted(MODES))
def test_planner_and_driver_modes_switched_off(key):
    """each key off in turn on the cases whose plan or launches it can change (MODES above says which and why), through the level kernels: the exact
    kernels read no record of the plan, and the rows the level kernels flag reach them here as well"""
    import acvm_amd
    value, letters = MODES[key]
    with acvm_amd.tuning(**{key: value}):
        for letter in letters:
            for case in ac.lists()[letter]:
                if key != "light_fuse" or has_range(case):
                    got, stats = device_rows(case, False)
                    ac.compare(case, got, f"device, level kernels, {key} = {value}")
                    assert stats["truncated_at"] == ac.expected_truncation(case), (case.name, stats["truncated_at"])


@pytest.mark.parametrize("key,value", [("inv_share", 1), ("inv_share", 2), ("inv_share", 8), ("inv_chunk", 1), ("inv_chunk", 3)])
def test_inversion_batches_cut_otherwise(key, value):
    """list B under one, two and eight waves to a field inversion and under chunks of one and of three denominators: a zero partner in a chunk of its own, at
    a chunk's first and last place, beside live denominators that must get their inverses all the same"""
    import acvm_amd
    with acvm_amd.tuning(**{key: value}):
        for case in ac.lists()["B"]:
            got, stats = device_rows(case, False)
            ac.compare(case, got, f"device, level kernels, {key} = {value}")
            assert stats["n_slow_instances"] == sum(1 for x in case.expect if ac.deviates(x)), (case.name, stats["n_slow_instances"])


def test_every_plan_checks_what_it_promises():
    """plan_validate = 1: every pass of the planner checks its own invariants while the handles of every list are built"""
    import acvm_amd
    with acvm_amd.tuning(plan_validate=1):
        for case in ac.all_cases():
            got, _ = device_rows(case, False)
            ac.compare(case, got, "device, level kernels, plan_validate")


def kept_witnesses(case):
    """the three highest witnesses that are no inputs: the outputs of the circuit's last gates"""
    return [w for w in range(case.circuit.current_witness_index, 0, -1) if w not in case.ids][:3][::-1]


@pytest.mark.parametrize("letter", ["B", "C"])
def test_recycled_slots_and_a_folded_digest(oracle, letter):
    """reuse_slots with fold_digest: the rows of the table are recycled, so the map leaves as its digest and the kept witnesses; both are the model's. A kept
    witness the model leaves unassigned is not handed out (extract refuses it); the digest of such a row is compared like every other row's. The two
    circuits of list C whose plan ends at the gate of 256 general terms cannot recycle rows: their handles must say so."""
    import acvm_amd
    for case in ac.lists()[letter]:
        keep = kept_witnesses(case)
        nw = case.circuit.current_witness_index + 1
        if ac.expected_truncation(case) != ac.NOT_TRUNCATED:  # (a plan that ends in mid-circuit cannot recycle rows: the handle says so)
            with pytest.raises(acvm_amd.AcvmError, match="slot reuse needs a circuit the level kernels cover entirely"):
                acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids, fold_digest=True, reuse_slots=True, keep=keep)
            continue
        batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids, fold_digest=True, reuse_slots=True, keep=keep)
        batch.set_initial_witness(values_from_rows(case.rows))
        batch.solve()
        res, dig = batch.results(), batch.digest()
        whole = [j for j, x in enumerate(case.expect) if all(w in x.witnesses for w in keep)]
        kept = {j: batch.extract(keep, j, 1) for j in whole}
        check_expressions(case, batch, "device, recycled slots")
        batch.free()
        for j, x in enumerate(case.expect):
            assert res[j].as_tuple() == tuple(x[:5]), f"{ac.describe(case, j)}: device {res[j].as_tuple()}, want {tuple(x[:5])}"
            if x.message is not None:
                assert res[j].message == x.message, ac.describe(case, j)
        for j in whole:
            x = case.expect[j]
            assert [int.from_bytes(kept[j][0, k].tobytes(), "big") for k in range(len(keep))] == [x.witnesses[w] for w in keep], ac.describe(case, j)
        for j, x in enumerate(case.expect):  # the digest is of the map as it stands: a failed row's is that of the model's partial map
            asg = [1 if w in x.witnesses else 0 for w in range(nw)]
            vals = b"".join(x.witnesses.get(w, 0).to_bytes(32, "big") for w in range(nw))
            assert bytes(dig[j]) == oracle.witness_map_digest(asg, vals), f"{ac.describe(case, j)}: the digest is not the digest of the model's map"


@pytest.mark.parametrize("letter", ["A", "B"])
def test_partial_maps_while_stepping(letter):
    """acvm_batch_solve_opcode on every row of lists A and B: the head and the partial map after every step are the model's after the same number of opcodes
    (the model's maps grow by what each step of its one run added)"""
    import acvm_amd
    for case in ac.lists()[letter]:
        B, n_ops = len(case.rows), len(case.circuit.opcodes)
        runs = []
        for row in case.rows:
            added = []
            runs.append((ar.run(case.circuit, dict(zip(case.ids, row)), snapshots=added), added))
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
                    want = (ar.ST_SOLVED, 0, 0, 0, 0) if step == n_ops else (ar.ST_IN_PROGRESS, 0, step, 0, 0)
                else:
                    want = tuple(final[:5])
                assert res[j].as_tuple()[:3] == want[:3] and (want[0] != ar.ST_FAILURE or res[j].as_tuple() == want), (step, ac.describe(case, j), res[j].as_tuple(), want)
            asg, vals = batch.witness_map()
            if not (np.array_equal(asg != 0, want_asg != 0) and np.array_equal(vals * (want_asg[:, :, None] != 0), want_vals)):
                bad = np.argwhere(((asg != 0) != (want_asg != 0)) | (vals * (want_asg[:, :, None] != 0) != want_vals).any(axis=2))
                raise AssertionError(f"{case.name}: after {step} steps the maps differ at (row, witness) {bad[:8].tolist()}")
            assert left == sum(1 for final, _ in runs if not (step == n_ops and final.status == ar.ST_SOLVED)), (case.name, step)
        check_expressions(case, batch, "device, stepped")
        assert {len(added) for final, added in runs if final.status == ar.ST_FAILURE} == {final.opcode_index for final, _ in runs if final.status == ar.ST_FAILURE}
        batch.free()


def test_one_handle_solved_again_and_again():
    """one handle per case: list B's rows, then rows that all pass, then B's rows again (in another order): no inverse row, event word or expression of an
    earlier solve shows in a later one"""
    import acvm_amd
    cases = [ac.dyn_cases(f)[6] for f in ac.FOLLOW_UPS] + [ac.dyn_cases("too many unknowns")[5], ac.wide_dyn_case()] + list(ac.order_cases())
    for case in cases:
        B = len(case.rows)
        first = list(range(B))
        second = [case.filler] * B
        third = first[-7:] + first[:-7]
        batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), B, case.ids)
        for order in (first, second, third):
            sub = case._replace(rows=[case.rows[j] for j in order], expect=[case.expect[j] for j in order], notes=[case.notes[j] for j in order])
            batch.set_initial_witness(values_from_rows(sub.rows))
            assert batch.solve() == sum(1 for x in sub.expect if x.status != ar.ST_SOLVED)
            ac.compare(sub, rows_of(batch, batch.results()), f"device, solve of {'passing rows' if order is second else 'the rows'} on the reused handle")
            check_expressions(sub, batch, "device, reused handle")
            assert batch.stats()["n_slow_instances"] == sum(1 for x in sub.expect if ac.deviates(x)), case.name
        batch.free()


# ---- D
def test_initial_sets_that_differ_by_row(oracle):
    import acvm_amd
    circ, maps, expect, notes = ac.initial_set_case()
    multi = acvm_amd.MultiBatch(acvm_amd.Circuit(circ.to_bytes()), list(maps))
    assert multi.n_groups == 3
    multi.solve()
    res = multi.results()
    got = []
    for j in range(len(maps)):
        asg, vals = multi.witness_map(j)
        got.append((res[j].as_tuple(), res[j].message, {int(w): int.from_bytes(vals[w].tobytes(), "big") for w in np.flatnonzero(asg)}))
    case = ac.Case("D", circ, [], list(maps), list(expect), None, list(notes))
    ac.compare(case, got, "device, MultiBatch")
    for j, m in enumerate(maps):  # and the oracle
        a = oracle.ACVM(oracle.Circuit(circ.to_bytes()), m)
        a.solve()
        assert a.result().as_tuple() == got[j][0] and a.witness_map() == got[j][2], ac.describe(case, j)
