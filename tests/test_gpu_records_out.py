"""The record export (acvm_batch_export_device_records, acvm_batch_witness_records): the witness map as one packed record of mixed-width fields
per output row, at any pitch, field offset and base alignment, on the device. Expected bytes are built in Python (tests/records_out_ref.py) from
Batch.witness_map and its assigned set, which the other suites pin to the oracle. Every buffer is lead + n * pitch + 64 bytes of 0xA5 and is
compared WHOLE: every byte that no field and no mask byte covers -- padding, the lead, the tail -- must still be 0xA5 afterwards."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import Circuit, Expression as E
import records_ref as rr
import records_out_ref as ro
from records_ref import BE32, LE32, MONT, P, U8, U16, U32, U64, U128

pytestmark = pytest.mark.gpu
PATTERN = rr.PATTERN


def _load(name):
    spec = importlib.util.spec_from_file_location("_%s_for_records_out" % name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GR = _load("test_gpu_records")
EDGE = _GR.EDGE
_readback_circuit = _GR._readback_circuit
# which fields of the import's shapes get a mask byte, and where: half of them wherever the record has room (pitch 1, 3 and 7 are covered whole).
# two_windows1500: the mask byte of the element at byte 2 lies at byte 1467, in the OTHER window; that of the element at 1465 at byte 1.
MASKS = {
    "pitch1": {}, "pitch3": {}, "pitch7": {},
    "pitch33_be32": {0: 0}, "pitch33_le32": {0: 0}, "pitch33_mont": {0: 0},
    "mixed108": {0: 96, 2: 97, 5: 104, 8: 106},
    "pitch128": {0: 7, 1: 63, 3: 99},
    "pitch256": {0: 2, 2: 129, 4: 254},
    "two_windows1500": {0: 1467, 3: 1},
}


def _out_fields(shape):
    """the import's shape as out fields: position k is input k + 1 where k is even and the gate output n_in + k + 1 where it is odd"""
    pitch, fields = _GR.SHAPES[shape]
    n_in = len(fields)
    return pitch, n_in, [((k + 1) if k % 2 == 0 else (n_in + k + 1), e, o, MASKS[shape].get(k)) for k, e, o in fields]


def _rows(B, n_in, rot=0):
    """inputs: the 256-bit edge strings mod p, and small values every third cell so that narrow fields both fit and do not fit"""
    return [[(7 * j + 3 * k + rot) % 70000 if (j + k) % 3 == 0 else EDGE[(j + k + rot) % len(EDGE)] % P for k in range(n_in)] for j in range(B)]


@functools.lru_cache(maxsize=None)
def _solved(n_in, B):
    """a solved handle of the read-back circuit and its whole map: shared, read only"""
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    batch.set_initial_witness(synth.values_from_rows(_rows(B, n_in)))
    assert batch.solve() == 0
    asg, vals = batch.witness_map()
    return batch, asg, vals


def _export(batch, pitch, fields, n, lead, first=0, instances=None):
    """exports into lead + n * pitch + 64 bytes of 0xA5 at an address that is `lead` past an aligned one; the whole buffer afterwards"""
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (lead + n * pitch + ro.TAIL))
    d_l = acvm_amd.DeviceBuffer(np.array(instances, dtype=np.uint32).tobytes()) if instances is not None else None
    try:
        batch.export_device_records(buf.ptr + lead, pitch, fields, first=first, n=n, d_instances=d_l.ptr if d_l else None)
        return np.frombuffer(buf.download(), dtype=np.uint8)
    finally:
        buf.free()
        if d_l:
            d_l.free()


def _assert_equal(got, want, lead, pitch, what=""):
    bad = np.flatnonzero(got != want)
    if bad.size:
        at = int(bad[0])
        where = "the lead" if at < lead else "row %d byte %d" % ((at - lead) // pitch, (at - lead) % pitch)
        raise AssertionError("%s: byte %d (%s) is %#x, expected %#x (%d bytes differ)" % (what, at, where, got[at], want[at], bad.size))


def _check(batch, asg, vals, pitch, fields, rows, lead, first=0, instances=None, what=""):
    got = _export(batch, pitch, fields, len(rows), lead, first, instances)
    want = ro.expected_buffer(lead, pitch, fields, rows, asg, vals)
    _assert_equal(got, want, lead, pitch, what)


# ---- 1. the sweep: B x record shape x base pointer
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("shape", list(_GR.SHAPES))
def test_shapes_sizes_and_base_alignments(shape, B):
    pitch, n_in, fields = _out_fields(shape)
    batch, asg, vals = _solved(n_in, B)
    for lead in range(4):
        _check(batch, asg, vals, pitch, fields, list(range(B)), lead, what=f"{shape} B={B} base+{lead}")


def test_the_sweep_has_masks_fits_and_misfits():
    """what the sweep relies on: narrow fields of the mixed record see values that fit and values that do not"""
    pitch, n_in, fields = _out_fields("mixed108")
    _, asg, vals = _solved(n_in, 130)
    masks = {ro.element_and_mask(int.from_bytes(vals[j, w].tobytes(), "big"), True, e)[1] for j in range(130) for w, e, o, m in fields if rr.size_of(e) < 32}
    assert masks == {1, 2} and sum(m is not None for _, _, _, m in fields) == 4


# ---- 2. joints: whoever stores a whole dword where it owns only some bytes is seen here
@pytest.mark.parametrize("pitch,fields", [(3, [(2, U16, 1, None)]), (7, [(1, U32, 3, None)]), (7, [(1, U32, 3, None), (2, U8, 1, None)]), (3, [(1, U8, 2, 0)])])
def test_joint_bytes_of_records_blocks_and_the_buffer(pitch, fields):
    """pitch 3 and 7 at B = 130: every field ends on the last byte of its record, the bytes in front of it are padding -- the dword at the joint of
    two records (and of two blocks, rows 63 | 64 and 127 | 128) holds covered bytes of one record and padding of the next"""
    B = 130
    batch, asg, vals = _solved(3, B)
    for lead in range(4):
        _check(batch, asg, vals, pitch, fields, list(range(B)), lead, what=f"pitch {pitch} base+{lead}")


def test_buffer_ends_inside_a_dword():
    """lead + n * pitch is no multiple of 4: the last field lies in the last dword of the last record, whose other bytes are the tail's"""
    pitch, n_in, fields = _out_fields("pitch7")
    B, lead = 65, 3
    assert (lead + B * pitch) % 4 == 2 and max(o + rr.size_of(e) for _, e, o, _ in fields) == pitch
    batch, asg, vals = _solved(n_in, B)
    _check(batch, asg, vals, pitch, fields, list(range(B)), lead)


# ---- 3. the exact path
@functools.lru_cache(maxsize=None)
def _asserting(B, force_slow=False):
    """w4 = 3 w1 + 1; assert w2 == 11; w5 = 3 w2 + 1; w6 = 3 w3 + 1. Every fourth instance holds 11 and solves; the others fail at the assert on
    the exact path and never assign w5, w6."""
    gc = acvm_amd.Circuit(Circuit(6, [E([], [(3, 1), (P - 1, 4)], 1), E([], [(1, 2)], P - 11), E([], [(3, 2), (P - 1, 5)], 1), E([], [(3, 3), (P - 1, 6)], 1)]).to_bytes())
    batch = acvm_amd.Batch(gc, B, [1, 2, 3])
    batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(synth.values_from_rows([[EDGE[j % len(EDGE)] % P, 11 if j % 4 == 0 else 300 + j, 5 + j] for j in range(B)]))
    batch.solve()
    asg, vals = batch.witness_map()
    return batch, asg, vals


EXACT_FIELDS = (44, [(5, U8, 0, 1), (6, BE32, 2, 34), (2, U16, 35, 37), (1, U32, 38, 43)])


@pytest.mark.parametrize("force_slow", [False, True])
def test_instances_of_the_exact_path(force_slow):
    B = 70
    batch, asg, vals = _asserting(B, force_slow)
    n_slow = batch.stats()["n_slow_instances"]
    assert n_slow == B if force_slow else 1 <= n_slow < B
    assert not asg[1, 5] and not asg[1, 6] and asg[0, 5] and asg[1, 4]  # a failed instance's later witnesses are unassigned: zero bytes, mask 0
    pitch, fields = EXACT_FIELDS
    for lead in (0, 3):
        _check(batch, asg, vals, pitch, fields, list(range(B)), lead, what=f"force_slow={force_slow} base+{lead}")
    got = _export(batch, pitch, fields, B, 0).reshape(-1)[:B * pitch].reshape(B, pitch)
    assert not got[1, 0:2].any() and not got[1, 2:35].any() and got[1, 37] == 1 and got[0, 1] == 1  # (instance 1 failed at the assert; its w2 = 301 is there)


def test_a_narrow_value_that_does_not_fit_is_mask_2_with_its_low_bytes():
    B = 70
    batch, asg, vals = _asserting(B)
    # w2 = 300 + j as U8: 300 + j >= 256, low byte written; w3 = 5 + j as U8 fits; w1 (an edge string) as U64 and U128
    pitch, fields = 40, [(2, U8, 0, 1), (3, U8, 2, 3), (1, U64, 5, 4), (1, U128, 14, 13)]
    got = _export(batch, pitch, fields, B, 1)[1:1 + B * pitch].reshape(B, pitch)
    for j in range(B):
        w1, w2 = EDGE[j % len(EDGE)] % P, 11 if j % 4 == 0 else 300 + j
        assert (got[j, 0], got[j, 1]) == (w2 % 256, 2 if w2 >= 256 else 1) and (got[j, 2], got[j, 3]) == (5 + j, 1)
        assert got[j, 5:13].tobytes() == (w1 % (1 << 64)).to_bytes(8, "little") and got[j, 4] == (2 if w1 >> 64 else 1)
        assert got[j, 14:30].tobytes() == (w1 % (1 << 128)).to_bytes(16, "little") and got[j, 13] == (2 if w1 >> 128 else 1)
    _check(batch, asg, vals, pitch, fields, list(range(B)), 1)


def test_a_witness_beyond_the_circuit_and_a_witness_in_two_encodings():
    B = 65
    batch, asg, vals = _solved(3, B)
    pitch, fields = 80, [(2, U8, 0, 1), (2, BE32, 3, 2), (batch.nw, LE32, 36, 35), (0xFFFFFFFF, U16, 70, 72)]
    got = _export(batch, pitch, fields, B, 2)
    _assert_equal(got, ro.expected_buffer(2, pitch, fields, list(range(B)), asg, vals), 2, pitch)
    rows = got[2:2 + B * pitch].reshape(B, pitch)
    assert not rows[:, 35:68].any() and not rows[:, 70:73].any()  # zero bytes, mask 0
    assert (rows[:, 0] == rows[:, 34]).all() and (rows[:, 2] == 1).all()  # the U8 is the BE32's last byte


# ---- 4. lists, ranges, live counts
def test_list_form_reversed_with_repeats_and_entries_beyond_the_batch():
    B = 70
    batch, asg, vals = _asserting(B)
    pitch, fields = EXACT_FIELDS
    lst = list(range(B - 1, -1, -1)) + [3, 3, 1, B, 0xFFFFFFFF, 0, B + 5, 68]
    rows = [j if j < B else None for j in lst]
    for lead in (0, 1):
        _check(batch, asg, vals, pitch, fields, rows, lead, instances=lst, what=f"list base+{lead}")
    # the same list on a handle nobody left the generic path of, and a long record
    pitch, n_in, fields = _out_fields("two_windows1500")
    batch, asg, vals = _solved(n_in, 65)
    lst = [64, 0, 0, 70, 33] + list(range(64, -1, -1))
    _check(batch, asg, vals, pitch, fields, [j if j < 65 else None for j in lst], 3, instances=lst)


def test_first_above_zero():
    pitch, n_in, fields = _out_fields("mixed108")
    batch, asg, vals = _solved(n_in, 130)
    for first, n in ((1, 129), (63, 66), (129, 1), (64, 64)):
        _check(batch, asg, vals, pitch, fields, list(range(first, first + n)), 1, first=first, what=f"first={first} n={n}")
    batch, asg, vals = _asserting(70)
    _check(batch, asg, vals, *EXACT_FIELDS, list(range(5, 70)), 2, first=5, what="exact lanes, first=5")


def test_live_count_below_capacity():
    pitch, n_in, fields = _out_fields("pitch128")
    cap, n = 130, 70
    batch = acvm_amd.Batch(_readback_circuit(n_in), cap, list(range(1, n_in + 1)))
    batch.set_instances(n)
    batch.set_initial_witness(synth.values_from_rows(_rows(n, n_in, rot=11)))
    assert batch.solve() == 0
    asg, vals = batch.witness_map()
    _check(batch, asg, vals, pitch, fields, list(range(n)), 1)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*beyond the 70 live instances"):
        _export(batch, pitch, fields, n + 1, 0)
    lst = [69, 70, 129, 0]  # a list entry at or beyond the LIVE count assigned nothing
    _check(batch, asg, vals, pitch, fields, [69, None, None, 0], 0, instances=lst)
    batch.free()


def test_slot_reuse_kept_ids_and_the_state_refusal():
    pitch, n_in, _ = _out_fields("mixed108")
    B = 96
    ids = list(range(1, n_in + 1))
    keep = [n_in + 2, n_in + 6, 3]
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, ids, reuse_slots=True, keep=keep)
    batch.set_initial_witness(synth.values_from_rows(_rows(B, n_in, rot=2)))
    assert batch.solve() == 0
    ws = keep + [1, n_in]
    kept = batch.extract(ws)
    asg = np.zeros((B, 2 * n_in + 1), dtype=np.uint8)
    vals = np.zeros((B, 2 * n_in + 1, 32), dtype=np.uint8)
    asg[:, ws], vals[:, ws] = 1, kept
    fields = [(keep[0], BE32, 1, 0), (keep[1], U16, 33, 35), (3, MONT, 36, None), (1, U8, 68, 69), (n_in, U64, 71, 70), (keep[0], U32, 80, None)]
    for lead in (0, 3):
        _check(batch, asg, vals, 84, fields, list(range(B)), lead, what=f"reuse base+{lead}")
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (B * 84))
    with pytest.raises(acvm_amd.AcvmError, match="error -5: .*witness %d was not kept" % (n_in + 3)):
        batch.export_device_records(buf.ptr, 84, fields + [(n_in + 3, U8, 79, None)])
    assert set(buf.download()) == {PATTERN}
    buf.free()
    batch.free()


# ---- 5. refusals, the table copy
def test_refusals_write_nothing():
    pitch, n_in, fields = _out_fields("pitch128")
    B = 65
    batch, asg, vals = _solved(n_in, B)
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (B * pitch + ro.TAIL))
    d_l = acvm_amd.DeviceBuffer(np.arange(4, dtype=np.uint32).tobytes())
    w, e, o, m = fields[1]
    refused = [
        (dict(pitch=pitch, fields=[(w, 3, o, m)] + fields[2:]), "field 0 .*unknown encoding 3"),
        (dict(pitch=pitch, fields=fields[:1] + [(w, e, pitch - 31, None)]), "field 1 .*beyond the pitch"),
        (dict(pitch=pitch, fields=fields[:1] + [(w, e, (1 << 64) - 2, None)]), "field 1 .*beyond the pitch"),
        (dict(pitch=pitch, fields=fields[:1] + [(w, e, o, pitch)]), "field 1 .*mask offset 128 is beyond the pitch"),
        (dict(pitch=pitch, fields=fields + [(1, U8, o + 5, None)]), "field 5 .*overlaps the element of field 1"),
        (dict(pitch=pitch, fields=fields + [(1, U8, 0, m)]), "the mask byte of field 5 .*overlaps the mask byte of field 1"),
        (dict(pitch=pitch, fields=fields, first=1, n=B), "beyond the 65 live instances"),
        (dict(pitch=pitch, fields=fields, first=1, n=3, d_instances=d_l.ptr), "first must be 0 for a list export"),
    ]
    h2d = batch.export_h2d_bytes()
    for kw, message in refused:
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            batch.export_device_records(buf.ptr, **kw)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*null records"):
        batch.export_device_records(None, pitch, fields)
    L = acvm_amd.lib()
    assert L.acvm_batch_export_device_records(batch._h, None, None, buf.ptr) == -1 and b"null argument" in L.acvm_last_error()
    d = acvm_amd.RecordOutDesc(pitch=pitch, fields=None, n_fields=3, first=0, n=B)
    assert L.acvm_batch_export_device_records(batch._h, d, None, buf.ptr) == -1 and b"null fields" in L.acvm_last_error()
    # not solved: ACVM_E_STATE as acvm_batch_export_device
    fresh = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    fresh.set_initial_witness(synth.values_from_rows(_rows(B, n_in)))
    with pytest.raises(acvm_amd.AcvmError, match="error -5"):
        fresh.export_device_records(buf.ptr, pitch, fields)
    fresh.free()
    # nothing to write succeeds, with any pointer
    batch.export_device_records(None, pitch, [])
    batch.export_device_records(None, pitch, fields, n=0)
    assert batch.export_h2d_bytes() == h2d and set(buf.download()) == {PATTERN}
    buf.free()
    d_l.free()


def test_after_solve_then_import_the_initial_witnesses_are_refused():
    """ACVM_E_STATE where acvm_batch_export_device returns it: the rows of the initial witnesses hold the next tile's inputs"""
    B, n_in = 65, 3
    rows = _rows(B, n_in, rot=4)
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, [1, 2, 3])
    d_in, d_next = acvm_amd.DeviceBuffer(synth.values_from_rows(rows)), acvm_amd.DeviceBuffer(synth.values_from_rows(_rows(B, n_in, rot=9)))
    batch.set_initial_witness_device(d_in.ptr)
    assert batch.solve(then_import=d_next.ptr) == 0
    asg = np.zeros((B, 2 * n_in + 1), dtype=np.uint8)
    vals = np.zeros((B, 2 * n_in + 1, 32), dtype=np.uint8)
    asg[:, 4:] = 1
    vals[:, 4:] = _GR._be_rows([[(3 * x + 1) % P for x in r] for r in rows])
    fields = [(4, BE32, 1, 0), (6, U16, 33, 35), (5, LE32, 36, None)]
    _check(batch, asg, vals, 68, fields, list(range(B)), 1)  # the gate outputs are still there
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (B * 68))
    with pytest.raises(acvm_amd.AcvmError, match="error -5: .*initial witnesses"):
        batch.export_device_records(buf.ptr, 68, fields[:2] + [(2, LE32, 36, None)])
    assert set(buf.download()) == {PATTERN}
    for x in (buf, d_in, d_next):
        x.free()
    batch.free()


def test_the_tables_are_copied_once_for_a_repeated_descriptor():
    pitch, n_in, fields = _out_fields("two_windows1500")
    B = 65
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    batch.set_initial_witness(synth.values_from_rows(_rows(B, n_in)))
    assert batch.solve() == 0
    asg, vals = batch.witness_map()
    before = batch.export_h2d_bytes()
    _check(batch, asg, vals, pitch, fields, list(range(B)), 0)
    first_call = batch.export_h2d_bytes() - before
    # two windows of 5 + 8 words, six entries of 4 words (two of the four fields have their mask byte in the other window: two entries each)
    assert first_call == 4 * (2 * 13 + 6 * 4)
    for lead in (1, 2):
        _check(batch, asg, vals, pitch, fields, list(range(B)), lead)
        _check(batch, asg, vals, pitch, fields, [3, 2, 1], lead, instances=[3, 2, 1])
    assert batch.export_h2d_bytes() - before == first_call
    _check(batch, asg, vals, pitch, fields[:3], list(range(B)), 0)  # another table: one more copy
    assert batch.export_h2d_bytes() - before == first_call + 4 * (2 * 13 + 4 * 4)
    batch.free()


# ---- 6. record to record, and the host form
def test_round_trip_through_the_record_import():
    """batch A's initial witnesses leave as records, batch B reads the same buffer with the same offsets: both solve to the same whole state"""
    pitch, in_fields = _GR.MIXED108
    B, n_in, lead = 130, len(in_fields), 3
    ids = list(range(1, n_in + 1))
    raws = _GR._edge_raws(B, in_fields, rot=3)
    a = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    a.set_initial_witness(synth.values_from_rows(rr.values_of(raws, in_fields, n_in)))  # (every narrow value fits its field)
    assert a.solve() == 0
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (lead + B * pitch + ro.TAIL))
    a.export_device_records(buf.ptr + lead, pitch, [(k + 1, e, o, None) for k, e, o in in_fields])
    b = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    b.import_device_records(buf.ptr + lead, pitch, in_fields)
    assert b.solve() == 0
    _GR._assert_same_state(_GR._whole_state(b), _GR._whole_state(a), "record to record")
    _GR._assert_read_back(b, rr.values_of(raws, in_fields, n_in), "record to record")
    buf.free()
    for x in (a, b):
        x.free()


def test_host_form_equals_the_device_form_with_zero_padding():
    for shape, B, first in (("mixed108", 65, 0), ("two_windows1500", 65, 7), ("pitch7", 130, 0)):
        pitch, n_in, fields = _out_fields(shape)
        batch, asg, vals = _solved(n_in, B)
        n = B - first
        host = batch.witness_records(pitch, fields, first=first, n=n)
        assert host.shape == (n, pitch)
        want = ro.expected_buffer(0, pitch, fields, list(range(first, B)), asg, vals, padding=0, tail=0).reshape(n, pitch)
        assert np.array_equal(host, want), shape
        dev = _export(batch, pitch, fields, n, 0, first=first)[:n * pitch].reshape(n, pitch)
        c = ro.covered(pitch, fields)
        assert np.array_equal(host[:, c], dev[:, c]) and not host[:, ~c].any() and (dev[:, ~c] == PATTERN).all()
