"""The record import (acvm_batch_import_device_records, acvm_batch_set_initial_witness_records): one packed record of mixed-width fields per
instance, at any pitch, field offset and base alignment, on the device. Imports are judged by Python integers through the read-back circuit of
tests/test_gpu_import.py (w[n_in + k] = 3 w[k] + 1), loaded the way tests/test_gpu_typed_io.py loads it; the hash circuit by the CPU oracle and
by the same bytes through ACVM_ENC_U8 and ACVM_ENC_BE32. Buffers hold 0xA5 wherever no field lies and are exactly lead + B * pitch bytes."""
import importlib.util
import os

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
import records_ref as rr
from records_ref import BE32, LE32, MONT, P, U8, U16, U32, U64, U128

pytestmark = pytest.mark.gpu
IM = acvm_amd.LAYOUT_INSTANCE_MAJOR


def _gpu_import_module():
    spec = importlib.util.spec_from_file_location("_gpu_import_for_records", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_import.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GI = _gpu_import_module()
EDGE = _GI.EDGE
_readback_circuit = _GI._readback_circuit


# ---- values: the strings a field holds
def _narrow_edges(encoding):
    bits = 8 * rr.size_of(encoding)
    vals = [0, 1, 255, 256, 257, (1 << 29) - 1, 1 << 29, (1 << 29) + 7, 1 << (bits - 1), (1 << bits) - 1]
    out = []
    for v in [v for v in vals if v < (1 << bits)] + [e % (1 << bits) for e in EDGE]:
        if v not in out:
            out.append(v)
    return out


def _raw(j, position, encoding, rot):
    """the element's bytes of instance j: the value edges of the width, every 256-bit edge string for the 32-byte encodings (as the encoding reads it)"""
    if rr.size_of(encoding) == 32:
        return EDGE[(j + position + rot) % len(EDGE)].to_bytes(32, "big")
    ed = _narrow_edges(encoding)
    return ed[(j + 3 * position + rot) % len(ed)].to_bytes(rr.size_of(encoding), "little")


def _edge_raws(B, fields, rot=0):
    return [{position: _raw(j, position, encoding, rot) for position, encoding, _ in fields} for j in range(B)]


def _byte_raws(B, fields, odd_one=None):
    """every element a byte, so that whole waves take the closed form of the row; odd_one = (instance, position): one lane that is no byte"""
    raws = [{position: rr.element((7 * j + position) % 256, encoding) for position, encoding, _ in fields} for j in range(B)]
    if odd_one is not None:
        j, position = odd_one
        encoding = {p_: e for p_, e, _ in fields}[position]
        raws[j][position] = rr.element(256 + j, encoding)
    return raws


# ---- the record shapes of the sweep: name -> (pitch, fields)
MIXED108 = (108, [(0, U8, 0), (1, U16, 1), (2, U32, 3), (3, U64, 7), (4, U128, 15), (5, BE32, 31), (6, LE32, 64), (7, U8, 107), (8, U32, 100)])
SHAPES = {
    "pitch1": (1, [(0, U8, 0)]),
    "pitch3": (3, [(0, U8, 0), (1, U16, 1)]),
    "pitch7": (7, [(0, U32, 3), (1, U8, 0), (2, U16, 1)]),
    "pitch33_be32": (33, [(0, BE32, 1)]),
    "pitch33_le32": (33, [(0, LE32, 1)]),
    "pitch33_mont": (33, [(0, MONT, 1)]),
    "mixed108": MIXED108,
    "pitch128": (128, [(0, U64, 8), (1, BE32, 64), (2, U8, 127), (3, U128, 100), (4, U16, 33)]),
    "pitch256": (256, [(0, MONT, 3), (1, U8, 255), (2, U32, 130), (3, LE32, 200), (4, U64, 249 - 8)]),
    "two_windows1500": (1500, [(0, BE32, 2), (1, U8, 0), (2, LE32, 1468), (3, U16, 1465)]),
}


def _be_rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for r in vals for v in r), dtype=np.uint8).reshape(len(vals), -1, 32)


def _assert_read_back(batch, vals, what=""):
    """vals[j][k]: the value input k of instance j holds. Every initial witness reads back as it, every gate output as 3 x + 1."""
    n_in = len(vals[0])
    assert all(r.status == acvm_amd.STATUS_SOLVED for r in batch.results()), what
    asg, got = batch.witness_map()
    want = np.concatenate([_be_rows(vals), _be_rows([[(3 * x + 1) % P for x in r] for r in vals])], axis=1)
    assert asg[:, 1:2 * n_in + 1].all(), what
    bad = np.argwhere((got[:, 1:2 * n_in + 1] != want).any(axis=2))
    assert bad.size == 0, (f"{what}: witness {1 + bad[0][1]} of instance {bad[0][0]} is {got[bad[0][0], 1 + bad[0][1]].tobytes().hex()}, expected "
                           f"{want[bad[0][0], bad[0][1]].tobytes().hex()} ({len(bad)} differ)")


def _import(batch, B, pitch, fields, raws, lead=0, pattern=rr.PATTERN):
    """imports the records through a device buffer of exactly lead + B * pitch bytes; returns the values the inputs then hold"""
    data = rr.build_records(B, pitch, fields, raws, lead, pattern)
    assert len(data) == lead + B * pitch
    buf = acvm_amd.DeviceBuffer(data)
    try:
        batch.import_device_records(buf.ptr + lead, pitch, fields)
    finally:
        buf.free()
    return rr.values_of(raws, fields, len(fields))


def _whole_state(batch):
    asg, vals = batch.witness_map()
    return [r.as_tuple() for r in batch.results()], asg, vals


def _assert_same_state(got, want, what=""):
    assert got[0] == want[0], what
    nw = min(got[1].shape[1], want[1].shape[1])
    assert np.array_equal(got[1][:, :nw], want[1][:, :nw]), what
    bad = np.argwhere((got[2][:, :nw] != want[2][:, :nw]).any(axis=2))
    assert bad.size == 0, f"{what}: witness {bad[0][1]} of instance {bad[0][0]} differs ({len(bad)} differ)"


# ---- 1. the sweep: B x record shape x base pointer
# B: one instance, below / on / above the block of 64 instances, five blocks with a last one of one instance
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_sizes_and_base_alignments(shape, B):
    pitch, fields = SHAPES[shape]
    n_in = len(fields)
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    for lead in range(4):
        vals = _import(batch, B, pitch, fields, _edge_raws(B, fields, rot=5 * lead), lead)
        assert batch.solve() == 0
        _assert_read_back(batch, vals, f"{shape} B={B} base+{lead}")
    batch.free()


@pytest.mark.parametrize("odd_one", [None, (70, 2), (3, 5)])
def test_waves_of_bytes_and_one_lane_that_is_none(odd_one):
    """every field of the mixed record holds a byte: whole waves take the closed form of the row (the ballot of every width and of the 32-byte
    encodings); with one value that is no byte its wave takes the product"""
    pitch, fields = MIXED108
    B, n_in = 130, len(fields)
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    vals = _import(batch, B, pitch, fields, _byte_raws(B, fields, odd_one), lead=1)
    assert batch.solve() == 0
    _assert_read_back(batch, vals, f"bytes, odd one {odd_one}")
    batch.free()


# ---- 2. one case each
def test_buffer_ends_inside_a_dword():
    """lead + B * pitch is no multiple of 4: the last record ends inside an aligned dword, the buffer with it"""
    pitch, fields = SHAPES["pitch7"]
    B, lead = 65, 3
    assert (lead + B * pitch) % 4 == 2
    batch = acvm_amd.Batch(_readback_circuit(3), B, [1, 2, 3])
    vals = _import(batch, B, pitch, fields, _edge_raws(B, fields), lead)
    assert batch.solve() == 0
    _assert_read_back(batch, vals)
    batch.free()


def test_fields_in_descending_position_order():
    pitch, fields = MIXED108
    B, n_in = 65, len(fields)
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    down = sorted(fields, key=lambda f: -f[0])
    assert [f[0] for f in down] == list(range(n_in - 1, -1, -1))
    vals = _import(batch, B, pitch, down, _edge_raws(B, fields), lead=2)
    assert batch.solve() == 0
    _assert_read_back(batch, vals)
    batch.free()


def test_two_positions_on_the_same_and_on_overlapping_bytes():
    B, pitch = 65, 9
    fields = [(0, U32, 1), (1, U32, 1), (2, U16, 2), (3, U64, 1)]
    words = [_narrow_edges(U64)[(j + 4) % len(_narrow_edges(U64))].to_bytes(8, "little") for j in range(B)]
    raws = [{0: w[:4], 1: w[:4], 2: w[1:3], 3: w} for w in words]
    buf = np.full((B, pitch), rr.PATTERN, dtype=np.uint8)
    buf[:, 1:9] = np.frombuffer(b"".join(words), dtype=np.uint8).reshape(B, 8)
    batch = acvm_amd.Batch(_readback_circuit(4), B, [1, 2, 3, 4])
    d = acvm_amd.DeviceBuffer(buf.tobytes())
    batch.import_device_records(d.ptr, pitch, fields)
    assert batch.solve() == 0
    _assert_read_back(batch, rr.values_of(raws, fields, 4))
    d.free()
    batch.free()


def test_padding_bytes_influence_nothing():
    pitch, fields = MIXED108
    B, n_in = 65, len(fields)
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    raws = _edge_raws(B, fields, rot=9)
    states = []
    for pattern in (0xA5, 0x00, 0xFF):
        _import(batch, B, pitch, fields, raws, lead=1, pattern=pattern)
        assert batch.solve() == 0
        states.append(_whole_state(batch))
    _assert_same_state(states[1], states[0], "padding 0x00 against 0xA5")
    _assert_same_state(states[2], states[0], "padding 0xFF against 0xA5")
    batch.free()


def test_slot_reuse_rows():
    """ACVM_BATCH_REUSE_SLOTS: the rows of the initial witnesses are the plan's slots, not the ids"""
    pitch, fields = MIXED108
    B, n_in = 96, len(fields)
    ids = list(range(1, n_in + 1))
    keep = [n_in + 2, n_in + 6, 3]
    raws = _edge_raws(B, fields, rot=2)
    vals = rr.values_of(raws, fields, n_in)
    ref = acvm_amd.Batch(_readback_circuit(n_in), B, ids, reuse_slots=True, keep=keep)
    ref.set_initial_witness(synth.values_from_rows(vals))
    assert ref.solve() == 0
    want = ([r.as_tuple() for r in ref.results()], ref.digest(), ref.extract(keep))
    ref.free()
    new = acvm_amd.Batch(_readback_circuit(n_in), B, ids, reuse_slots=True, keep=keep)
    _import(new, B, pitch, fields, raws, lead=3)
    assert new.solve() == 0
    assert [r.as_tuple() for r in new.results()] == want[0]
    assert np.array_equal(new.digest(), want[1]) and np.array_equal(new.extract(keep), want[2])
    got = new.extract(keep)
    assert np.array_equal(got[:, 0], _be_rows([[(3 * r[1] + 1) % P] for r in vals])[:, 0]) and np.array_equal(got[:, 2], _be_rows([[r[2]] for r in vals])[:, 0])
    new.free()


def test_live_count_below_capacity():
    pitch, fields = SHAPES["pitch128"]
    n_in, cap, n = len(fields), 130, 70
    batch = acvm_amd.Batch(_readback_circuit(n_in), cap, list(range(1, n_in + 1)))
    vals = _import(batch, cap, pitch, fields, _edge_raws(cap, fields), lead=1)
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "capacity")
    batch.set_instances(n)
    vals = _import(batch, n, pitch, fields, _edge_raws(n, fields, rot=11), lead=2)  # (a buffer of exactly n records)
    assert batch.solve() == 0
    _assert_read_back(batch, vals, f"{n} live instances")
    batch.set_instances(cap)
    vals = _import(batch, cap, pitch, fields, _edge_raws(cap, fields, rot=4))
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "capacity again")
    batch.free()


def test_refusals_leave_the_previous_import_in_place():
    pitch, fields = SHAPES["pitch7"]
    B = 65
    batch = acvm_amd.Batch(_readback_circuit(3), B, [1, 2, 3])
    vals = _import(batch, B, pitch, fields, _edge_raws(B, fields))
    ptr = 1 << 20  # (never read: every call below is refused by the host checks)
    refused = [
        (pitch, fields[:2], "position 2 .*no field"),
        (pitch, fields + [(1, U8, 6)], "position 1 is supplied twice"),
        (pitch, [(3, U8, 0)] + fields, "field 0 .*position 3 is not below n_initial 3"),
        (pitch, [(0, 3, 0)] + fields[1:], "field 0 .*unknown encoding 3"),
        (pitch, [(0, U32, 4)] + fields[1:], "field 0 .*beyond the pitch"),
        (pitch, [(0, U32, (1 << 64) - 2)] + fields[1:], "field 0 .*beyond the pitch"),
        (0, fields, "field 0 .*beyond the pitch"),
    ]
    for pt, fl, message in refused:
        copies = batch.import_list_copies()
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            batch.import_device_records(ptr, pt, fl)
        assert batch.import_list_copies() == copies  # nothing was copied or enqueued
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*null records"):
        batch.import_device_records(None, pitch, fields)
    L = acvm_amd.lib()
    assert L.acvm_batch_import_device_records(batch._h, None, ptr) == -1 and b"null argument" in L.acvm_last_error()
    d = acvm_amd.RecordDesc(pitch=pitch, fields=None, n_fields=3)
    assert L.acvm_batch_import_device_records(batch._h, d, ptr) == -1 and b"null fields" in L.acvm_last_error()
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "after the refusals")
    batch.free()


def test_the_field_table_is_copied_once():
    pitch, fields = MIXED108
    B, n_in = 65, len(fields)
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    assert batch.import_list_copies() == 0
    for rot in range(3):
        vals = _import(batch, B, pitch, fields, _edge_raws(B, fields, rot), lead=rot)
        assert batch.import_list_copies() == 1
    assert batch.solve() == 0
    _assert_read_back(batch, vals)
    # another table: one more copy
    other = [(p_, e, o) for p_, e, o in fields if p_ != 7] + [(7, U8, 99)]
    vals = _import(batch, B, pitch, other, _edge_raws(B, other))
    assert batch.import_list_copies() == 2
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "another table")
    batch.free()


def test_a_circuit_without_initial_witnesses_reads_nothing():
    from acvm_amd.acir import Circuit, Expression as E
    gc = acvm_amd.Circuit(Circuit(1, [E([], [(1, 1)], P - 5)]).to_bytes())
    batch = acvm_amd.Batch(gc, 65, [])
    batch.import_device_records(None, 0, [])
    assert batch.solve() == 0
    assert batch.import_list_copies() == 0
    batch.free()


def test_hash_circuit_bytes_as_records_equal_u8_be32_and_the_oracle(oracle):
    """SHA256 -> Keccak256 + RANGE read the plane words and rows the record import wrote: the whole state equals that of the same bytes through
    ACVM_ENC_U8 instance-major and through BE32 on fresh handles, and the oracle's"""
    B = 65
    circ, ids = synth.hash_circuit(n_msg=8)
    n_in, data = len(ids), circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    rows = [[int(v) for v in r] for r in np.frombuffer(synth.byte_batch(B, n_in, seed=0xAC1D0720), dtype=np.uint8).reshape(B, n_in, 32)[:, :, 31]]
    rows[0][:2], rows[B - 1][-2:] = [0, 255], [255, 0]
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, synth.values_from_rows(rows), B)
    want = ([r.as_tuple() for r in ores], oasg, ovals)
    assert all(r[0] == 0 for r in want[0])
    dense = np.array(rows, dtype=np.uint8).tobytes()
    states = {}
    for name in ("be32", "u8", "records"):
        h = acvm_amd.Batch(gc, B, ids)
        assert h.stats()["n_byte_planes"] == n_in
        buf = acvm_amd.DeviceBuffer(synth.values_from_rows(rows) if name == "be32" else dense)
        if name == "be32":
            h.import_device(buf.ptr, encoding=BE32, layout=IM)
        elif name == "u8":
            h.import_device(buf.ptr, encoding=U8, layout=IM)
        else:
            h.import_device_records(buf.ptr, n_in, [(k, U8, k) for k in range(n_in)])
        assert h.solve() == 0
        states[name] = _whole_state(h)
        buf.free()
        h.free()
    for name in ("be32", "u8", "records"):
        _assert_same_state(states[name], want, f"{name} against the oracle")
    _assert_same_state(states["records"], states["u8"], "records against U8")
    _assert_same_state(states["records"], states["be32"], "records against BE32")


def test_host_form_equals_the_device_form():
    pitch, fields = MIXED108
    B, n_in = 65, len(fields)
    ids = list(range(1, n_in + 1))
    raws = _edge_raws(B, fields, rot=1)
    dev = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    vals = _import(dev, B, pitch, fields, raws)
    assert dev.solve() == 0
    host = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    host.set_initial_witness_records(rr.build_records(B, pitch, fields, raws), pitch, fields)
    assert host.solve() == 0
    _assert_read_back(host, vals, "host form")
    _assert_same_state(_whole_state(host), _whole_state(dev), "host form against device form")
    # a numpy structured array through the dtype helper
    dt = np.dtype([("a", "u1"), ("b", "<u2"), ("c", "<u4"), ("d", "<u8"), ("e", "V16"), ("f", "V32"), ("pad", "u1"), ("g", "V32"), ("h", "V4"), ("i", "<u4"), ("j", "V3"), ("k", "u1")])
    dpitch, dfields = acvm_amd.record_fields_from_dtype(dt, {"a": 0, "b": 1, "c": 2, "d": 3, "e": 4, "f": 5, "g": (6, LE32), "k": 7, "i": 8})
    assert dpitch == pitch and sorted(dfields) == sorted(fields)
    arr = np.frombuffer(rr.build_records(B, pitch, fields, raws), dtype=dt)
    host.set_initial_witness_records(arr, dpitch, dfields)
    assert host.solve() == 0
    _assert_read_back(host, vals, "structured array")
    with pytest.raises(ValueError):
        host.set_initial_witness_records(b"\0" * (B * pitch - 1), pitch, fields)
    for x in (dev, host):
        x.free()
