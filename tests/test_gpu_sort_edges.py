"""Directive::PermutationSort on the device (acvm_amd/csrc/ops_sort.hpp op_perm_sort in the scratch-carrying kernel of kernels_hash.hip, the reservation of
plan.cpp), on the case lists of tests/sort_cases.py: every permutation of up to six elements and the structured ones around every power of two up to 257;
keys that differ in one limb, that wrap past p, that are constants; every shape of sort_by, and a column past the tuple that the comparator reaches in some
rows of a batch and not in others; fewer and more bit witnesses than switches, bits the row already knows, one witness twice; unassigned inputs; two sorts
whose scratch lies beside a hash's and a variable-length Keccak's. Every row is compared with the Python model of the reference first (tests/sort_ref.py:
status, error kind, failing opcode, aux words, panic text, the whole witness map) and with the CPU oracle second, through the level kernels and through the
exact in-order kernels. tests/test_sort_cases.py (no GPU) proves what the lists cover and that the oracle agrees with the model."""
import numpy as np
import pytest

import sort_cases as sc
import sort_ref as sr
from acvm_amd.synth import values_from_rows

pytestmark = pytest.mark.gpu

LETTERS = sorted(sc.lists())


def device_got(case, force_slow=False, batch=None):
    import acvm_amd
    own = batch is None
    if own:
        batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids)
        batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(values_from_rows(case.rows))
    n_left = batch.solve()
    assert n_left == sum(1 for x in case.expect if x.status != sr.ST_SOLVED), (case.name, n_left)
    asg, vals = batch.witness_map()
    got, stats = (batch.results(), asg, vals), batch.stats()
    if own:
        batch.free()
    return got, stats


def against_the_oracle(oracle, case, got, who):
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(case.circuit.to_bytes()), case.ids, values_from_rows(case.rows), len(case.rows))
    res, asg, vals = got
    for j in range(len(case.rows)):
        assert res[j].as_tuple() == ores[j].as_tuple() and res[j].message == ores[j].message, f"{sc.describe(case, j)}: {who} {res[j].as_tuple()} {res[j].message!r}, oracle {ores[j].as_tuple()} {ores[j].message!r}"
    nw = min(oasg.shape[1], asg.shape[1])
    assert np.array_equal(oasg[:, :nw] != 0, asg[:, :nw] != 0), f"{case.name}: {who}: the assigned sets are not the oracle's"
    assert np.array_equal(ovals[:, :nw] * (oasg[:, :nw, None] != 0), vals[:, :nw] * (asg[:, :nw, None] != 0)), f"{case.name}: {who}: the values are not the oracle's"


def on_the_device(oracle, case):
    """the model first, on both paths; then the oracle"""
    for force_slow in (False, True):
        who = "device, exact kernels" if force_slow else "device, level kernels"
        got, stats = device_got(case, force_slow)
        sc.compare(case, got, who)
        against_the_oracle(oracle, case, got, who)
        if not force_slow and stats["truncated_at"] == 0xFFFFFFFF:   # the rows that end in an error, and nobody else, went through the exact path
            assert stats["n_slow_instances"] == sum(1 for x in case.expect if x.status != sr.ST_SOLVED), (case.name, stats["n_slow_instances"])


@pytest.mark.parametrize("letter", LETTERS)
def test_every_list_on_both_paths(oracle, letter):
    for case in sc.lists()[letter]:
        on_the_device(oracle, case)


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("letter", [l for l in LETTERS if l != "E"])
def test_special_rows_in_a_partial_last_wave(letter, n):
    """passing rows in front up to 65 and 130 rows: the rows a list is about are the last wave's, beside dead lanes (list E has 65 and 130 rows of its own). A
    case that has that many rows already or lets no row pass stays as it is and is not run again."""
    for case in sc.lists()[letter]:
        if len(case.rows) < n and case.filler is not None:
            p = sc.padded(case, n)
            for force_slow in (False, True):
                got, _ = device_got(p, force_slow)
                sc.compare(p, got, f"device, {n} rows (exact kernels: {force_slow})")


# which lists a planner or driver key can affect: a key that cannot change a list's plan or launches is not run on it
MODES = {
    # the scratch-carrying launch (a heavy class) goes to a stream of its own or stays on the main stream: every list has one
    "overlap": "ABCDE",
    "heavy_streams": "BE",
    "heavy_only_streams": "BE",
    # the circuits are one level of heavy records; with no gate there is nothing for light_fuse, scale or relax to change but the expressions of list
    # B's keys, which the sort evaluates itself: B
    "light_fuse": "B",
    "scale": "B",
    "relax": "B",
}


@pytest.mark.parametrize("key", sorted(MODES))
def test_planner_and_driver_modes_switched_off(key):
    """each key off in turn, on every case of the lists whose plan or launches it can change (MODES above says which and why)"""
    import acvm_amd
    with acvm_amd.tuning(**{key: 0}):
        for letter in MODES[key]:
            for case in sc.lists()[letter]:
                got, _ = device_got(case)
                sc.compare(case, got, f"device, level kernels, {key} = 0")


def test_every_plan_checks_what_it_promises():
    import acvm_amd
    with acvm_amd.tuning(plan_validate=1):
        for letter in LETTERS:
            for case in sc.lists()[letter]:
                got, _ = device_got(case)
                sc.compare(case, got, "device, level kernels, plan_validate")


def test_recycled_slots_and_a_folded_digest(oracle):
    """reuse_slots with fold_digest on the neighbours: the kept witnesses and the digest are the model's"""
    import acvm_amd
    case = sc.neighbours_case(65)
    keep = case.circuit.opcodes[0].bits[:2] + case.circuit.opcodes[2].bits[-2:]
    nw = case.circuit.current_witness_index + 1
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids, fold_digest=True, reuse_slots=True, keep=keep)
    batch.set_initial_witness(values_from_rows(case.rows))
    assert batch.solve() == 0
    dig = batch.digest()
    kept = batch.extract(keep)
    batch.free()
    for j, x in enumerate(case.expect):
        assert [int.from_bytes(kept[j, k].tobytes(), "big") for k in range(len(keep))] == [x.witnesses[w] for w in keep], sc.describe(case, j)
        asg = [1 if w in x.witnesses else 0 for w in range(nw)]
        vals = b"".join(x.witnesses.get(w, 0).to_bytes(32, "big") for w in range(nw))
        assert bytes(dig[j]) == oracle.witness_map_digest(asg, vals), f"{sc.describe(case, j)}: the digest is not the digest of the model's map"


def test_partial_maps_while_stepping():
    """acvm_batch_solve_opcode on the neighbours: after each of the four opcodes the map is the model's"""
    import acvm_amd
    case = sc.neighbours_case(65)
    B, n_ops = len(case.rows), len(case.circuit.opcodes)
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), B, case.ids)
    batch.set_initial_witness(values_from_rows(case.rows))
    for step in range(1, n_ops + 1):
        batch.solve_opcode()
        expect = [sr.run(case.circuit, dict(zip(case.ids, row)), n_opcodes=step if step < n_ops else None) for row in case.rows]
        asg, vals = batch.witness_map()
        sc.compare(case, (batch.results(), asg, vals), f"device, after {step} steps", expect)
    batch.free()


def test_one_handle_solved_three_times():
    """one handle: the past-the-tuple rows (half of them panic), the same rows in another order, then rows that all pass: no key, order or switch of an
    earlier solve shows in a later one"""
    import acvm_amd
    case = sc.past_tuple_case(2)
    turned = case._replace(rows=case.rows[::-1], expect=case.expect[::-1], notes=case.notes[::-1])
    passing = case._replace(rows=[case.rows[j] for j in (0, 2, 4, 6, 8)] * 2, expect=[case.expect[j] for j in (0, 2, 4, 6, 8)] * 2, notes=[case.notes[j] for j in (0, 2, 4, 6, 8)] * 2)
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids)
    for k, c in enumerate((case, turned, passing, case)):
        got, _ = device_got(c, batch=batch)
        sc.compare(c, got, f"device, solve {k + 1} on one handle")
    batch.free()


def test_initial_sets_that_differ_by_row(oracle):
    """MultiBatch: maps that know a control bit (right or wrong) or lack a key, beside plain ones"""
    import acvm_amd
    case = sc.bits_cases()[2]
    circ, bits = case.circuit, case.circuit.opcodes[0].bits
    maps = []
    for j, (row, x) in enumerate(zip(case.rows * 3, case.expect * 3)):
        m = dict(zip(case.ids, row))
        if j % 3 == 1:
            m[bits[3]] = x.witnesses[bits[3]] if j % 2 else 1 - x.witnesses[bits[3]]
        elif j % 3 == 2:
            del m[case.ids[2]]
        maps.append(m)
    expect = [sr.run(circ, m) for m in maps]
    assert {x.err for x in expect} == {sr.E_NONE, sr.E_UNSATISFIED, sr.E_MISSING_ASSIGNMENT}
    multi = acvm_amd.MultiBatch(acvm_amd.Circuit(circ.to_bytes()), maps)
    assert multi.n_groups == 3
    multi.solve()
    res = multi.results()
    for j, (m, x) in enumerate(zip(maps, expect)):
        asg, vals = multi.witness_map(j)
        got = {int(w): int.from_bytes(vals[w].tobytes(), "big") for w in np.flatnonzero(asg)}
        assert res[j].as_tuple() == tuple(x[:5]) and got == x.witnesses, (j, res[j].as_tuple(), tuple(x[:5]))
        a = oracle.ACVM(oracle.Circuit(circ.to_bytes()), m)
        a.solve()
        assert a.result().as_tuple() == res[j].as_tuple() and a.witness_map() == got, j
