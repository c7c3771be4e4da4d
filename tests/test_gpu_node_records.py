"""acvm_node_solve_records: the node driver fed host records. One device listed three times, tiles of 64, 200 instances of the mixed-struct
circuit (fn main(msg: [u8; 8], a: Field, b: Field, root: Field) as one packed 108-byte record, tests/records_ref.py) with instances planted to
fail, so that the exact path of a tile runs beside the next tile: results, kept witnesses, assigned bytes and digests equal those of
acvm_node_solve on the same values as 32-byte big-endian rows."""
import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import BlackBoxFuncCall as BB, Circuit, Expression as E, FunctionInput as FI
import records_ref as rr
from records_ref import P, U8, U16, BE32

pytestmark = pytest.mark.gpu
B, TILE, DEVICES = 200, 64, [0, 0, 0]


def _mixed_struct_circuit():
    """tests/test_gpu_typed_io.py _mixed_input_circuit: SHA256 over the bytes (RANGE on each), w44 = a b + root, w45 = w44^2 + 7 w12"""
    ids = list(range(1, 12))
    ops = [BB("RANGE", {"input": FI(w, 8)}) for w in ids[:8]]
    ops.append(BB("SHA256", {"inputs": [FI(w, 8) for w in ids[:8]], "outputs": list(range(12, 44))}))
    ops.append(E([(1, 9, 10)], [(1, 11), (P - 1, 44)], 0))
    ops.append(E([(1, 44, 44)], [(7, 12), (P - 1, 45)], 0))
    return Circuit(current_witness_index=45, opcodes=ops, private_parameters=ids, return_values=[45]).to_bytes(), ids


def _rows(seed):
    rng = np.random.default_rng(seed)
    rows = [[int(b) for b in rng.integers(0, 256, 8)] + [int.from_bytes(rng.bytes(32), "big") % P for _ in range(3)] for _ in range(B)]
    rows[5][7] = 256      # tile 0 of lane 0: its exact path runs beside tile 1
    rows[130][7] = 40000  # tile 0 of lane 1, beside the partial last tile
    return rows


@pytest.fixture(scope="module")
def node():
    data, ids = _mixed_struct_circuit()
    gc = acvm_amd.Circuit(data)
    n = acvm_amd.Node(gc, ids, keep=[45, 12, 9, 50], devices=DEVICES, tile=TILE)
    yield n
    n.free()


def _assert_equal_calls(got, want, what):
    assert got[0] == want[0] == 2, what
    assert [r.as_tuple() for r in got[1]] == [r.as_tuple() for r in want[1]], what
    for k, name in ((2, "kept witnesses"), (3, "assigned bytes"), (4, "digests")):
        assert np.array_equal(got[k], want[k]), (what, name)


def test_records_equal_be32_rows(node):
    rows = _rows(0xAC1D0730)
    want = node.solve(synth.values_from_rows(rows), B)
    assert [j for j, r in enumerate(want[1]) if r.status != acvm_amd.STATUS_SOLVED] == [5, 130]
    records = rr.build_records(B, rr.MIXED_STRUCT_PITCH, rr.MIXED_STRUCT_FIELDS, rr.mixed_struct_raws(rows))
    got = node.solve_records(records, B, rr.MIXED_STRUCT_PITCH, rr.MIXED_STRUCT_FIELDS)
    _assert_equal_calls(got, want, "records against BE32 rows")
    st = node.stats()
    assert sum(st["tiles"]) == 4 and sum(st["exact_instances"]) == 2


def test_refused_descriptors_leave_the_node_usable(node):
    rows = _rows(0xAC1D0731)
    want = node.solve(synth.values_from_rows(rows), B)
    records = rr.build_records(B, rr.MIXED_STRUCT_PITCH, rr.MIXED_STRUCT_FIELDS, rr.mixed_struct_raws(rows))
    wide = 32 * 11 + 1
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*pitch 353 is above 32 \\* n_initial"):
        node.solve_records(b"\0" * (B * wide), B, wide, rr.MIXED_STRUCT_FIELDS)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*position 10 .*no field"):
        node.solve_records(records, B, rr.MIXED_STRUCT_PITCH, rr.MIXED_STRUCT_FIELDS[:-1])
    got = node.solve_records(records, B, rr.MIXED_STRUCT_PITCH, rr.MIXED_STRUCT_FIELDS)
    _assert_equal_calls(got, want, "after the refusals")


def test_a_second_descriptor_on_the_same_node(node):
    """every input as a 32-byte big-endian field at an odd offset, in descending order, behind the call with the mixed record"""
    rows = _rows(0xAC1D0732)
    want = node.solve(synth.values_from_rows(rows), B)
    records = rr.build_records(B, rr.MIXED_STRUCT_PITCH, rr.MIXED_STRUCT_FIELDS, rr.mixed_struct_raws(rows))
    _assert_equal_calls(node.solve_records(records, B, rr.MIXED_STRUCT_PITCH, rr.MIXED_STRUCT_FIELDS), want, "the mixed record")
    pitch = 32 * 11  # (the widest record the node takes)
    fields = [(k, U8, 3 + k) for k in range(7)] + [(7, U16, 1)] + [(10 - k, BE32, 11 + 33 * k) for k in range(3)]
    fields = fields[::-1]
    enc = {p_: e for p_, e, _ in fields}
    raws = [[rr.element(v, enc[k]) for k, v in enumerate(r)] for r in rows]
    got = node.solve_records(rr.build_records(B, pitch, fields, raws), B, pitch, fields)
    _assert_equal_calls(got, want, "the second descriptor")
