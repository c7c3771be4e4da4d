"""The Brillig VM (acvm_amd/csrc/ops_brillig.hpp) and the straight-line inliner (plan.cpp emit_straight_line, ops_light.hpp op_brillig_sl) on the device,
on the case lists of tests/brillig_cases.py: memory at and past its end, the last register, jumps and calls to and past the end of the bytecode, call
stacks around the 16 entries a result keeps, every shape of a foreign-call result, black-box operands at the memory's edges, empty arrays among inputs
and outputs. Every row is compared with the Python model of the reference first (tests/brillig_ref.py: status, error kind, failing opcode, failure
text, call stack, pending foreign call, the whole witness map) and with the CPU oracle second, through the level kernels and through the exact
in-order kernels; the programs the planner inlines run once more in the VM. tests/test_brillig_cases.py (no GPU) proves what the lists cover and that
the oracle agrees with the model."""
import numpy as np
import pytest

import brillig_cases as bc
import brillig_ref as br
from acvm_amd.synth import values_from_rows
from test_gpu_foreign_call import drive
from test_gpu_opcodes import both_paths

pytestmark = pytest.mark.gpu

INLINED = [n for n in bc.NAMES if bc.n_inlinable(bc.case(n))]


def device_rows(case, force_slow, respond=None):
    """the rows of one solve as bc.compare takes them, and the batch's stats; respond(j, function, inputs): the host's answer to a row that waits"""
    import acvm_amd
    B = len(case.rows)
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), B, case.ids)
    batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(values_from_rows(case.rows))
    if respond:
        _, res = drive(batch, B, respond)
    else:
        batch.solve()
        res = batch.results()
    asg, vals = batch.witness_map()
    got = []
    for j, r in enumerate(res):
        wm = {int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])}
        pending = batch.get_pending_foreign_call(j) if r.status == bc.ST_REQUIRES_FOREIGN_CALL else None
        got.append((r.status, r.err, r.opcode_index, r.message, wm, list(r.call_stack[:r.n_call_stack]) if r.err == bc.E_BRILLIG_FAILED else None, pending))
    stats = batch.stats()
    batch.free()
    return got, stats


def device_against_the_model(case, force_slow, expect=None):
    got, stats = device_rows(case, force_slow)
    assert all(p is not None for x, (*_, p) in zip(expect or case.expect, got) if x.pending is not None), f"{case.name}: a waiting row has no pending call"
    bc.compare(case, got, "device, exact kernels" if force_slow else "device, level kernels", expect)
    return stats


def on_the_device(oracle, case):
    """the model first, on both paths; then the oracle (test_gpu_opcodes.run_both, both paths)"""
    stats = device_against_the_model(case, False)
    device_against_the_model(case, True)
    both_paths(oracle, case.circuit, case.ids, case.rows)
    return stats


@pytest.mark.parametrize("name", bc.NAMES)
def test_every_list_on_both_paths(oracle, name):
    case = bc.case(name)
    stats = on_the_device(oracle, case)
    assert stats["n_brillig_inlined"] == bc.n_inlinable(case), stats["n_brillig_inlined"]


@pytest.mark.parametrize("name", INLINED)
def test_inlined_programs_in_the_vm(oracle, name):
    """what the planner inlines by default (op_brillig_sl) runs in the VM kernel with the inliner switched off: the same expectations for both engines"""
    import acvm_amd
    with acvm_amd.tuning(brillig_inline=0):
        stats = on_the_device(oracle, bc.case(name))
    assert stats["n_brillig_inlined"] == 0


@pytest.mark.parametrize("force_slow", [False, True], ids=["level", "exact"])
def test_answers_from_the_host(oracle, force_slow):
    """every row of the vector program waits once; the host answers an empty array, one element or five (the pointer below, at and past the memory's end), and
    the continued run is the model's with that result appended. The inputs the device hands out are the model's."""
    case = bc.case("foreign call, answered by the host")
    asked = {}

    def respond(j, fn, inputs):
        asked[j] = (fn, inputs)
        return bc.answer_of(j)

    got, _ = device_rows(case, force_slow, respond)
    assert asked == {j: x.pending for j, x in enumerate(case.expect)}
    bc.compare(case, got, "device, answered", bc.answered_expect(case))
    # the oracle behind the same answers
    for j in range(len(case.rows)):
        a = oracle.ACVM(oracle.Circuit(case.circuit.to_bytes()), dict(zip(case.ids, case.rows[j])))
        assert a.solve() == oracle.ST_REQUIRES_FOREIGN_CALL
        a.resolve_pending_foreign_call(bc.answer_of(j))
        a.solve()
        r = a.result()
        assert (r.status, r.err, r.opcode_index) == got[j][:3] and a.witness_map() == got[j][4], bc.describe(case, j)


@pytest.mark.parametrize("force_slow", [False, True], ids=["level", "exact"])
def test_a_single_answered_by_the_host(force_slow):
    """a single into a register; in every third row the host answers an array where the single is due: the reference panics"""
    case = bc.case("foreign call, a single answered by the host")
    answer = lambda j: [[5]] if j % 3 == 2 else [case.rows[j][0] * 3 % bc.P]  # noqa: E731
    got, _ = device_rows(case, force_slow, lambda j, fn, inputs: answer(j))
    expect = [bc.model(case.circuit, case.ids, row, answers=[answer(j)]) for j, row in enumerate(case.rows)]
    assert [x.kind for x in expect] == [br.SOLVED, br.SOLVED, br.PANIC, br.SOLVED, br.SOLVED]
    bc.compare(case, got, "device, answered", expect)


@pytest.mark.parametrize("name,what", bc.DEVICE_PERTURBATIONS, ids=[w for _, w in bc.DEVICE_PERTURBATIONS])
def test_each_list_bites_on_the_device(name, what):
    """one expectation of a list moved (a zero-filled cell, a call-stack entry, a failure text, a pending input): the comparison of the device's run with the
    model fails and names that row, on the level kernels and on the exact kernels"""
    case, expect, j = bc.perturbed(name, what)
    for force_slow in (False, True):
        with pytest.raises(AssertionError, match=f"row {j} "):
            device_against_the_model(case, force_slow, expect)
