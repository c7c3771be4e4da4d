"""The deflating container of the batch-wide WitnessMap wire format (ACVM_WIRE_GZIP_DEFLATE of acvm_batch_witness_maps_wire_device,
acvm_batch_witness_maps_wire, acvm_batch_wire_bound) on the device: every output row's map as one gzip member of one dynamic-Huffman block.
Expected buffers are built in Python (tests/wire_deflate_ref.py, pinned by tests/test_wire_deflate_ref.py against zlib's inflater) from
Batch.witness_map. With tests/test_gpu_wire.py's discipline every buffer is 16 + n * pitch + 64 bytes of 0xA5 and is compared WHOLE -- the lead,
the bytes behind each row's length, between slots and the tail must still be 0xA5 -- and so is the lengths column around its n words."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import P
import wire_deflate_cases as cases
import wire_deflate_ref as ref
from wire_deflate_ref import GZIP_DEFLATE

pytestmark = pytest.mark.gpu
BINCODE = 0


def _load(name):
    spec = importlib.util.spec_from_file_location("_%s_for_wire_deflate" % name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GW = _load("test_gpu_wire")
PATTERN, LEAD, TAIL, PATTERN64 = _GW.PATTERN, _GW.LEAD, _GW.TAIL, _GW.PATTERN64
EDGE, _readback_circuit, _maps_of, _export, _assert_equal, _rows = _GW.EDGE, _GW._readback_circuit, _GW._maps_of, _GW._export, _GW._assert_equal, _GW._rows


def _check(batch, maps, rows, pitch_extra=0, witnesses=None, first=0, instances=None, what=""):
    """rows: per output row the instance whose map it holds, or None = an instance that assigned nothing. Returns the slots and the lengths."""
    n = len(rows)
    pitch = batch.wire_bound(GZIP_DEFLATE, witnesses) + pitch_extra
    n_positions = batch.nw if witnesses is None else len(witnesses)
    assert pitch - pitch_extra == ref.bound(GZIP_DEFLATE, n_positions), what
    want_maps = [({} if j is None else maps[j]) if witnesses is None else ref.restrict({} if j is None else maps[j], witnesses) for j in rows]
    want, want_lengths = ref.slots(want_maps, GZIP_DEFLATE, pitch, tail=TAIL)
    got, lengths, _ = _export(batch, GZIP_DEFLATE, n, pitch, witnesses, first, instances)
    _assert_equal(got, bytes([PATTERN]) * LEAD + want, pitch, what)
    assert list(lengths[1:n + 1]) == want_lengths and lengths[0] == PATTERN64 and lengths[n + 1] == PATTERN64, what
    for i in range(n):  # every row read by acvm_witness_map_decode gives the map
        assert _decoded(got[LEAD + i * pitch:LEAD + i * pitch + want_lengths[i]]) == want_maps[i], (what, i)
    return (got[LEAD:LEAD + n * pitch].reshape(n, pitch) if n else got[:0]), want_lengths


def _decoded(row_bytes):
    """the map acvm_witness_map_decode reads"""
    return acvm_amd.decompress_witness(bytes(row_bytes))


# ---- 1. sizes
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_sizes_and_pitches(B):
    batch, maps = _GW._solved(3, B)
    for extra in (0, 48):
        slots, lengths = _check(batch, maps, list(range(B)), extra, what=f"B={B} pitch=bound+{extra}")
    for j in {0, B - 1}:
        assert _decoded(slots[j, :lengths[j]]) == maps[j] and ref.inflate(slots[j, :lengths[j]].tobytes()) == ref.body(maps[j])


# ---- 2. the case rows through a solved handle
@functools.lru_cache(maxsize=None)
def _case_handle():
    """instance j's inputs are case row j: 2 x 64 + 2 instances, so the rows come round more than once and the last wave is partial"""
    B, n_in = 130, cases.ROW_VALUES
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    batch.set_initial_witness(synth.values_from_rows([cases.row_values(j) for j in range(B)]))
    assert batch.solve() == 0
    return batch, _maps_of(batch)


def test_case_rows_whole_map_and_witness_lists():
    batch, maps = _case_handle()
    B, n_in = batch.B, cases.ROW_VALUES
    assert B >= cases.N_ROWS and all(maps[j][1 + k] == v for j in range(B) for k, v in enumerate(cases.row_values(j)))
    slots, lengths = _check(batch, maps, list(range(B)), what="case rows, whole map")
    for j in range(0, B, 7):
        assert _decoded(slots[j, :lengths[j]]) == maps[j]
    inputs = list(range(1, n_in + 1))
    _check(batch, maps, list(range(B)), 48, witnesses=inputs, what="case rows, the inputs")  # exactly the case rows' pairs
    _check(batch, maps, list(range(B)), witnesses=inputs[1:] + [2 * n_in + 1, 1 << 24, 0xFFFFFFFF], what="pairs the other way round, witnesses beyond the circuit")
    for witnesses in ([], [0], [1], inputs[::2], [3, 2 * n_in]):
        _check(batch, maps, list(range(B)), witnesses=witnesses, what=f"list {witnesses}")


@functools.lru_cache(maxsize=None)
def _wide_handle():
    """300 inputs: keys 256 apart, 600 entries a row, bytes and field elements mixed"""
    B, n_in = 65, 300
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    rows = [[(cases.CHAIN[(j + 3 * k) % len(cases.CHAIN)] if (k + j) % 3 else (37 * k + j) % 256) for k in range(n_in)] for j in range(B)]
    batch.set_initial_witness(synth.values_from_rows(rows))
    assert batch.solve() == 0
    return batch, _maps_of(batch)


def test_keys_256_apart_and_a_row_of_600_entries():
    batch, maps = _wide_handle()
    B = batch.B
    assert all(len(m) == 600 for m in maps)
    slots, lengths = _check(batch, maps, list(range(B)), what="600 entries")
    assert len(set(lengths)) > 1 and _decoded(slots[64, :lengths[64]]) == maps[64]
    for witnesses in ([5, 6], [255, 256], [5, 261], [5, 6, 262, 263], [44, 300, 556]):
        _check(batch, maps, list(range(B)), witnesses=witnesses, what=f"keys {witnesses}")


@pytest.mark.parametrize("count", ["0", "1", "W-1", "W", "W+1", "2W+1"])
def test_entry_counts_around_the_window(count):
    w = cases.window()
    n = {"0": 0, "1": 1, "W-1": w - 1, "W": w, "W+1": w + 1, "2W+1": 2 * w + 1}[count]
    batch, maps = _case_handle()
    witnesses = list(range(1, n + 1))  # the inputs, then gate outputs
    slots, lengths = _check(batch, maps, list(range(batch.B)), witnesses=witnesses, what=f"{n} entries")
    assert all(len(ref.restrict(maps[j], witnesses)) == n for j in (0, 129))
    if n == 0:
        assert set(lengths) == {len(ref.encode({}))}


# ---- 3. the list form
def test_list_form_repeats_any_order_and_entries_beyond_the_live_count():
    batch, maps = _case_handle()
    B = batch.B
    lst = list(range(B - 1, -1, -1)) + [3, 3, 1, B, 0xFFFFFFFF, 0, B + 5, 68]
    slots, lengths = _check(batch, maps, [j if j < B else None for j in lst], instances=lst, what="list")
    for i, j in enumerate(lst):
        if j >= B:
            assert lengths[i] == len(ref.encode({}))
    _check(batch, maps, [7, 0, 129, None, 3], 48, witnesses=[1, 2, 3, 9], instances=[7, 0, 129, 200, 3])
    _check(batch, maps, list(range(60, 130)), witnesses=[2, 3, 4], first=60)


# ---- 4. rows of one block that end at different windows: partial maps of the exact path among generic rows, in the last partial wave too
SPECIAL_WIDE = (0, 63, 64, 129)  # (129: the last row of the block of two rows; 128 beside it is generic)


def _partial_wide(kind):
    """circuits of more than 2 W + 1 witnesses whose special instances stop early: (the handle, its maps)"""
    from acvm_amd.acir import Circuit, Expression as E
    B, w = 130, cases.window()
    if kind == "assert":  # w21 = 3 w1 + 1; assert w2 == 11; w(20 + k) = 3 w(k) + 1 for k = 2 .. 20: a failing instance stops at witness 21
        n_in = 20
        ops = [E([], [(3, 1), (P - 1, n_in + 1)], 1), E([], [(1, 2)], P - 11)] + [E([], [(3, k), (P - 1, n_in + k)], 1) for k in range(2, n_in + 1)]
        batch = acvm_amd.Batch(acvm_amd.Circuit(Circuit(2 * n_in, ops).to_bytes()), B, list(range(1, n_in + 1)))
        rows = [[v if k != 1 else (300 + j if j in SPECIAL_WIDE else 11) for k, v in enumerate(cases.row_values(j))] for j in range(B)]
        batch.set_initial_witness(synth.values_from_rows(rows))
        batch.solve()
    else:  # the read-back circuit of 24 inputs; the special instances lack inputs W .. 2 W - 1, the whole second window of the whole map
        n_in = 3 * w
        assert n_in > cases.ROW_VALUES
        batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
        mask = np.ones((B, n_in), dtype=np.uint8)
        for j in SPECIAL_WIDE:
            mask[j, w - 1:2 * w - 1] = 0  # (input k is witness k + 1)
        rows = [(cases.row_values(j) + cases.row_values(j + 1))[:n_in] for j in range(B)]
        d_v, d_m = acvm_amd.DeviceBuffer(synth.values_from_rows(rows)), acvm_amd.DeviceBuffer(mask.tobytes())
        batch.import_device_masked(d_v.ptr, d_m.ptr)
        batch.solve()
        d_v.free()
        d_m.free()
    return batch, _maps_of(batch)


@pytest.mark.parametrize("kind", ["assert", "hole"])
def test_rows_that_end_at_different_windows(kind):
    """exact-path lanes whose maps end windows before their neighbours' (they idle, cursor and partial dword carried) and, for `hole`, have a
    whole window without an entry in front of later entries (the predecessor kept across it)"""
    batch, maps = _partial_wide(kind)
    w, nw = cases.window(), batch.nw
    assert nw >= 2 * w + 1 and batch.stats()["n_slow_instances"] >= len(SPECIAL_WIDE)
    last_window = [max(m) // w for m in maps]  # the whole map: list position = witness
    generic = [j for j in range(batch.B) if j not in SPECIAL_WIDE]
    top = (nw - 1) // w  # (witness 0 is nobody's: nw - 1 is the last witness)
    assert {last_window[j] for j in generic} == {top} and all(last_window[j] < top - 1 for j in SPECIAL_WIDE)
    assert all(len(maps[j]) == nw - 1 for j in generic) and 128 in generic and 129 in SPECIAL_WIDE
    if kind == "hole":
        for j in SPECIAL_WIDE:
            windows = {k // w for k in maps[j]}
            assert 1 not in windows and 0 in windows and 2 in windows and max(windows) > 2
    slots, lengths = _check(batch, maps, list(range(batch.B)), 48, what=kind)
    for j in SPECIAL_WIDE:
        assert (slots[j, lengths[j]:] == PATTERN).all()
    # a list that puts special rows between generic ones, in blocks of their own mix; a witness list that moves the windows
    lst = [129, 5, 64, 128, 0, 500, 63, 7] + list(range(60, 130))
    _check(batch, maps, [j if j < batch.B else None for j in lst], instances=lst, what=kind + ", list")
    _check(batch, maps, list(range(batch.B)), witnesses=list(range(3, nw + 1, 2)) + [nw + 4], what=kind + ", every other witness")
    batch.free()


@pytest.mark.parametrize("kind", ["assert", "masked", "waiting"])
def test_partial_maps_of_the_exact_path_in_one_window(kind):
    batch, maps = _GW._partial(kind)
    full = len(maps[1])
    special = _GW.SPECIAL
    assert all(len(maps[j]) < full for j in special) and 64 in special and batch.B == 130
    slots, lengths = _check(batch, maps, list(range(batch.B)), 48, what=kind)
    isize = [int.from_bytes(slots[j, lengths[j] - 4:lengths[j]].tobytes(), "little") for j in range(batch.B)]
    assert isize == [8 + 76 * len(m) for m in maps] and all(isize[j] < isize[1] for j in special)  # (a shorter map need not deflate to fewer bytes)
    for j in special:
        assert (slots[j, lengths[j]:] == PATTERN).all() and _decoded(slots[j, :lengths[j]]) == maps[j]
    _check(batch, maps, [129, 64, 128, 0, None, 63], instances=[129, 64, 128, 0, 500, 63], what=kind + ", list")
    batch.free()


# ---- 5. after stepping, under the forced slow path
@pytest.mark.parametrize("force_slow", [False, True])
def test_exact_path_and_forced_slow_path(force_slow):
    batch, maps = _GW._arith(force_slow)
    n_slow = batch.stats()["n_slow_instances"]
    assert n_slow == batch.B if force_slow else 1 <= n_slow < batch.B
    slots, lengths = _check(batch, maps, list(range(batch.B)), what=f"arith force_slow={force_slow}")
    for j in (0, 7, 64, 129):
        assert _decoded(slots[j, :lengths[j]]) == maps[j]
    _check(batch, maps, list(range(batch.B)), witnesses=list(range(0, batch.nw, 3)) + [batch.nw + 2])


def test_after_solve_opcode_steps():
    from acvm_amd.acir import Circuit, Expression as E
    B = 70
    circ = Circuit(6, [E([], [(3, 1), (P - 1, 4)], 1), E([], [(1, 2)], P - 11), E([], [(3, 2), (P - 1, 5)], 1), E([], [(3, 3), (P - 1, 6)], 1)])
    batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, [1, 2, 3])
    batch.set_initial_witness(synth.values_from_rows([[EDGE[j % len(EDGE)] % P, 11 if j % 4 == 0 else 300 + j, 5 + j] for j in range(B)]))
    for step in range(3):
        batch.solve_opcode()
        maps = _maps_of(batch)
        _check(batch, maps, list(range(B)), what=f"after step {step}")
    assert len({len(m) for m in maps}) == 2
    batch.free()


# ---- 6. slot reuse
def test_slot_reuse_serves_the_kept_witnesses_and_refuses_the_whole_map():
    n_in, B = 9, 96
    keep = [n_in + 2, n_in + 6, 3]
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)), reuse_slots=True, keep=keep)
    batch.set_initial_witness(synth.values_from_rows(_rows(B, n_in, rot=2)))
    assert batch.solve() == 0
    ws = sorted(keep + [1, n_in])
    kept = batch.extract(ws)
    maps = [{w: int.from_bytes(kept[j, k].tobytes(), "big") for k, w in enumerate(ws)} for j in range(B)]
    _check(batch, maps, list(range(B)), witnesses=ws, what="reuse")
    _check(batch, maps, list(range(B)), witnesses=ws + [2 * n_in + 1, 5000], what="reuse, witnesses beyond the circuit")
    pitch = batch.wire_bound(GZIP_DEFLATE)
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (B * pitch))
    with pytest.raises(acvm_amd.AcvmError, match="error -5: .*full maps are not kept"):
        batch.witness_maps_wire_device(buf.ptr, GZIP_DEFLATE)
    with pytest.raises(acvm_amd.AcvmError, match="error -5: .*witness %d was not kept" % (n_in + 3)):
        batch.witness_maps_wire_device(buf.ptr, GZIP_DEFLATE, witnesses=sorted(ws + [n_in + 3]), pitch=pitch)
    assert set(buf.download()) == {PATTERN}
    buf.free()
    batch.free()


# ---- 7. round trip, the host form
def test_round_trip_through_the_host_import():
    """the downloaded rows are initial witness maps of a second handle; what the import leaves is what the BINCODE rows leave"""
    batch, maps = _case_handle()
    B, n_in = batch.B, cases.ROW_VALUES
    inputs = list(range(1, n_in + 1))
    states = []
    for container in (GZIP_DEFLATE, BINCODE):
        rows = batch.witness_maps_wire(container, witnesses=inputs)
        second = acvm_amd.Batch(_readback_circuit(n_in), B, inputs)
        second.set_initial_witness_maps_wire(rows)
        states.append(second.import_state())
        if container == GZIP_DEFLATE:
            assert second.solve() == 0 and _maps_of(second) == maps
        second.free()
    for key in ("rows", "planes", "events", "missing"):
        assert (states[0][key] == states[1][key]).all(), key


def test_host_form_equals_the_device_form_row_by_row():
    batch, maps = _GW._arith(False)
    B = batch.B
    got, lengths, pitch = _export(batch, GZIP_DEFLATE, B)
    slots = got[LEAD:LEAD + B * pitch].reshape(B, pitch)
    host = batch.witness_maps_wire(GZIP_DEFLATE)
    assert len(host) == B
    for j in range(B):
        assert host[j] == slots[j, :int(lengths[1 + j])].tobytes() == ref.encode(maps[j]), j
    part = batch.witness_maps_wire(GZIP_DEFLATE, witnesses=[1, 5, 17], first=60, n=10)
    assert part == [ref.encode(ref.restrict(maps[j], [1, 5, 17])) for j in range(60, 70)]
    assert batch.witness_maps_wire(GZIP_DEFLATE, n=0) == []


# ---- 8. refusals, host-to-device traffic
def test_refusals_name_their_cause_and_write_nothing():
    B = 65
    batch, maps = _GW._solved(3, B)
    bound = batch.wire_bound(GZIP_DEFLATE)
    assert bound == ref.bound(GZIP_DEFLATE, batch.nw) and batch.wire_bound(GZIP_DEFLATE, [1, 2]) == ref.bound(GZIP_DEFLATE, 2)
    assert bound < batch.wire_bound(_GW.GZIP_STORED)
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (B * (bound + 16) + TAIL))
    d_l = acvm_amd.DeviceBuffer(np.arange(4, dtype=np.uint32).tobytes())
    refused = [
        (dict(witnesses=[1, 3, 3]), "not strictly ascending"),
        (dict(pitch=bound - 16), "pitch %d is below the bound %d" % (bound - 16, bound)),
        (dict(pitch=bound + 8), "not a multiple of 16"),
        (dict(first=1, n=B), "beyond the 65 live instances"),
        (dict(first=1, n=3, d_instances=d_l.ptr), "first must be 0 for a list export"),
    ]
    for kw, message in refused:
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            batch.witness_maps_wire_device(buf.ptr, GZIP_DEFLATE, **kw)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*not aligned to 16 bytes"):
        batch.witness_maps_wire_device(buf.ptr + 8, GZIP_DEFLATE)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*null buffer"):
        batch.witness_maps_wire_device(None, GZIP_DEFLATE)
    for container in (2, 7, 9):  # through the Python view: refused as before this container existed (a CPU test cannot reach it: no handle)
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*unknown container %d" % container):
            batch.witness_maps_wire_device(buf.ptr, container)
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*unknown container %d" % container):
            batch.wire_bound(container)
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*unknown container %d" % container):
            batch.witness_maps_wire(container)
    fresh = acvm_amd.Batch(_readback_circuit(3), B, [1, 2, 3])
    fresh.set_initial_witness(synth.values_from_rows(_rows(B, 3)))
    with pytest.raises(acvm_amd.AcvmError, match="error -5"):
        fresh.witness_maps_wire_device(buf.ptr, GZIP_DEFLATE)
    # the import keeps refusing the container: inflating on the device is not part of it
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*unknown container 8"):
        fresh.import_device_wire(buf.ptr, GZIP_DEFLATE, bound)
    fresh.free()
    batch.witness_maps_wire_device(None, GZIP_DEFLATE, n=0)
    assert set(buf.download()) == {PATTERN}
    buf.free()
    d_l.free()


def test_host_to_device_traffic_is_the_plans_tables():
    batch, maps = _GW._arith(False)
    _export(batch, GZIP_DEFLATE, 64)  # (the exact lanes' map goes up once)
    grown = []
    for n in (64, 130):
        before = batch.export_h2d_bytes()
        _export(batch, GZIP_DEFLATE, n)
        grown.append(batch.export_h2d_bytes() - before)
    # the rank and power tables, the list mask, and the code table: 257 literals, 77 lengths, 12 words of head and header
    assert grown[0] == grown[1] == 4 * (2 * (batch.nw + 1) + (batch.nw + 31) // 32 + 257 + 77 + 12)
