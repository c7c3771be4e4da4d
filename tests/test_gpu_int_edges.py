"""The integer opcodes of acvm_amd/csrc/ops_light.hpp (canon_divrem, op_to_le_radix, op_range / op_range_multi, op_logic, int_op_core) on the
device, on the case lists of tests/int_cases.py: inputs built to reach every branch -- every pre-shift of the restoring division, the first
divisors past the 64-by-32 path, digits that straddle two limbs, every RANGE and AND / XOR width, the sign classes of SignedDiv -- compared
bit for bit with the Python-integer expectation first (status, error kind, failing opcode, panic text, the whole witness map) and with the CPU
oracle second, through the level kernels and through the exact in-order kernels, and again with the planner features switched off that decide how
these opcodes are scheduled (merged RANGE records, relaxed / scaled gate rows in front of a directive, inlined straight-line Brillig).
tests/test_int_cases.py (no GPU) proves what the lists cover and that the oracle agrees with the integers."""
import functools

import numpy as np
import pytest

import int_cases as ic
from acvm_amd.synth import values_from_rows
from test_gpu_opcodes import both_paths

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in ic.all_cases()}
BRILLIG = [c.name for c in ic.brillig_cases()]


@functools.lru_cache(maxsize=None)
def expected_arrays(name, nw):
    """the expectation of a case as the arrays Batch.witness_map returns: (assigned [B, nw], values [B, nw, 32])"""
    case = BY_NAME[name]
    asg = np.zeros((len(case.rows), nw), dtype=np.uint8)
    vals = np.zeros((len(case.rows), nw, 32), dtype=np.uint8)
    for j, x in enumerate(case.expect):
        for w, v in x.witnesses.items():
            asg[j, w] = 1
            vals[j, w] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    return asg, vals


def device_against_integers(case, force_slow):
    import acvm_amd
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids)
    batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(values_from_rows(case.rows))
    batch.solve()
    res = batch.results()
    asg, vals = batch.witness_map()
    batch.free()
    who = "device, exact kernels" if force_slow else "device, level kernels"
    nw = asg.shape[1]
    assert nw > max(max(x.witnesses) for x in case.expect)
    want_asg, want_vals = expected_arrays(case.name, nw)
    heads_agree = all((r.status, r.err) == (x.status, x.err) and (x.status != ic.ST_FAILURE or r.opcode_index == x.opcode_index) and
                      (x.message is None or r.message == x.message) for r, x in zip(res, case.expect))
    if heads_agree and np.array_equal(asg != 0, want_asg != 0) and np.array_equal(vals * (want_asg[:, :, None] != 0), want_vals):
        return
    got = []  # something differs: row by row, so that the message names the operands, the witness, got and want
    for j, r in enumerate(res):
        wm = {int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])}
        got.append((r.status, r.err, r.opcode_index, r.message, wm))
    ic.compare(case, got, who)
    raise AssertionError(f"{case.name}: {who} differs from the expectation outside what compare() looks at")


def on_the_device(oracle, case):
    """integers first, on both paths; then the oracle (test_gpu_opcodes.run_both, both paths)"""
    device_against_integers(case, False)
    device_against_integers(case, True)
    return both_paths(oracle, case.circuit, case.ids, case.rows)


@pytest.mark.parametrize("name", [n for n in BY_NAME if n not in BRILLIG])
def test_directives_range_and_logic(oracle, name):
    on_the_device(oracle, BY_NAME[name])


@pytest.mark.parametrize("name", ["range, one witness", "range, own witnesses"])
def test_range_one_record_per_opcode(oracle, name):
    """the same checks as K_RANGE records (op_range) where the default plan merges eight into one K_RANGE_MULTI"""
    import acvm_amd
    with acvm_amd.tuning(range_merge=0):
        on_the_device(oracle, BY_NAME[name])


@pytest.mark.parametrize("mode", [{"relax": 0}, {"scale": 0}], ids=["relax=0", "scale=0"])
@pytest.mark.parametrize("name", ["quotient", "radix A", "radix B"])
def test_directives_behind_canonical_gate_rows(oracle, name, mode):
    """By default a gate output may be stored relaxed or scaled, and a directive that reads it must be handed the reduced value: the gates in
    front of the quotient of gate outputs, and in front of circuit A's second group of radices, whose sums wrap past P in half of the rows. The
    directives must read the same values with either feature switched off. Circuit B has no gates: its plan is the same in every mode, and
    it runs here only because the radix circuits are asked for as a pair."""
    import acvm_amd
    with acvm_amd.tuning(**mode):
        on_the_device(oracle, BY_NAME[name])


@pytest.mark.parametrize("name", BRILLIG)
def test_brillig_divisions(oracle, name):
    """opcode 0 inlined (op_brillig_sl), opcode 1 in the VM kernel; then both in the VM"""
    import acvm_amd
    _, st = on_the_device(oracle, BY_NAME[name])
    assert st["n_brillig_inlined"] == 1, st["n_brillig_inlined"]
    with acvm_amd.tuning(brillig_inline=0):
        _, st0 = on_the_device(oracle, BY_NAME[name])
    assert st0["n_brillig_inlined"] == 0
