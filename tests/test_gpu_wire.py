"""The batch-wide WitnessMap wire format (acvm_batch_witness_maps_wire_device, acvm_batch_witness_maps_wire, acvm_batch_wire_bound) on the
device: every output row's map as the reference's own bytes -- the bincode body, alone or in a stored-block gzip member -- in a slot at a pitch.
Expected buffers are built in Python (tests/wire_ref.py, pinned by tests/test_wire_ref.py) from Batch.witness_map and its assigned set, which
the other suites pin to the oracle. Every buffer is 16 + n * pitch + 64 bytes of 0xA5 and is compared WHOLE: the lead, the bytes behind each
row's length, the bytes between slots and the tail must still be 0xA5 afterwards; so must the lengths column around its n words."""
import functools
import gzip
import importlib.util
import os
import re

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import P, Brillig, Circuit, Expression as E
import wire_ref
from wire_ref import BINCODE, GZIP_STORED

pytestmark = pytest.mark.gpu
PATTERN, LEAD, TAIL = wire_ref.FILL, 16, 64
CONTAINERS = (BINCODE, GZIP_STORED)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = E.from_witness


def _load(name):
    spec = importlib.util.spec_from_file_location("_%s_for_wire" % name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GR = _load("test_gpu_records")
EDGE = _GR.EDGE
_readback_circuit = _GR._readback_circuit


def _window():
    """the kernel's window in list positions (wire_plan.hpp; kernels_wire.hip asserts that wire_encode.hpp's is the same)"""
    return int(re.search(r"WIRE_PLAN_WINDOW = (\d+)", open(os.path.join(ROOT, "acvm_amd", "csrc", "wire_plan.hpp")).read()).group(1))


def _maps_of(batch):
    """the map of every instance as it stands: {witness: int} from Batch.witness_map"""
    asg, vals = batch.witness_map()
    return [{int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])} for j in range(batch.B)]


def _export(batch, container, n, pitch=0, witnesses=None, first=0, instances=None, lengths=True):
    """(the whole buffer afterwards, the whole lengths column afterwards as words with one word of pattern on either side, the pitch)"""
    pitch = pitch or batch.wire_bound(container, witnesses)
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (LEAD + n * pitch + TAIL))
    d_len = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (8 * (n + 2)))
    d_l = acvm_amd.DeviceBuffer(np.array(instances, dtype=np.uint32).tobytes()) if instances is not None else None
    try:
        batch.witness_maps_wire_device(buf.ptr + LEAD, container, witnesses, first=first, n=n, pitch=pitch, d_instances=d_l.ptr if d_l else None,
                                       d_lengths=d_len.ptr + 8 if lengths else None)
        return np.frombuffer(buf.download(), dtype=np.uint8), np.frombuffer(d_len.download(), dtype=np.uint64), pitch
    finally:
        buf.free()
        d_len.free()
        if d_l:
            d_l.free()


def _assert_equal(got, want, pitch, what=""):
    want = np.frombuffer(want, dtype=np.uint8)
    assert got.size == want.size, what
    bad = np.flatnonzero(got != want)
    if bad.size:
        at = int(bad[0])
        where = "the lead" if at < LEAD else "row %d byte %d" % ((at - LEAD) // pitch, (at - LEAD) % pitch)
        raise AssertionError("%s: byte %d (%s) is %#x, expected %#x (%d bytes differ)" % (what, at, where, got[at], want[at], bad.size))


PATTERN64 = int.from_bytes(bytes([PATTERN]) * 8, "little")


def _check(batch, maps, container, rows, pitch_extra=0, witnesses=None, first=0, instances=None, what=""):
    """rows: per output row the instance whose map it holds, or None = an instance that assigned nothing. Returns the slots and the lengths."""
    n = len(rows)
    pitch = batch.wire_bound(container, witnesses) + pitch_extra
    n_positions = batch.nw if witnesses is None else len(witnesses)
    assert pitch - pitch_extra == wire_ref.bound(container, n_positions), what
    want_maps = [({} if j is None else maps[j]) if witnesses is None else wire_ref.restrict({} if j is None else maps[j], witnesses) for j in rows]
    want, want_lengths = wire_ref.slots(want_maps, container, pitch, tail=TAIL)
    got, lengths, _ = _export(batch, container, n, pitch, witnesses, first, instances)
    _assert_equal(got, bytes([PATTERN]) * LEAD + want, pitch, what)
    assert list(lengths[1:n + 1]) == want_lengths and lengths[0] == PATTERN64 and lengths[n + 1] == PATTERN64, what
    return got[LEAD:LEAD + n * pitch].reshape(n, pitch) if n else got[:0], want_lengths


# ---- 1. the size sweep
def _rows(B, n_in, rot=0):
    """the 256-bit edge strings mod p: 0, p - 1 and values with leading zero nibbles among them"""
    return [[EDGE[(j + k + rot) % len(EDGE)] % P for k in range(n_in)] for j in range(B)]


@functools.lru_cache(maxsize=None)
def _solved(n_in, B):
    """a solved handle of the read-back circuit and its maps: shared, read only"""
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    batch.set_initial_witness(synth.values_from_rows(_rows(B, n_in)))
    assert batch.solve() == 0
    return batch, _maps_of(batch)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("container", CONTAINERS)
def test_sizes_containers_and_pitches(container, B):
    batch, maps = _solved(3, B)
    for extra in (0, 48):
        _check(batch, maps, container, list(range(B)), extra, what=f"container {container} B={B} pitch=bound+{extra}")


def test_the_sweep_has_the_edge_values():
    _, maps = _solved(3, 130)
    values = {v for m in maps for v in m.values()}
    assert 0 in values and P - 1 in values and any(0 < v < 1 << 200 for v in values) and all(len(m) == 6 for m in maps)


# ---- 2. stored-block boundaries
@functools.lru_cache(maxsize=None)
def _chain(n_assigned, B=65):
    """w1 is the input, w(k) = 3 w(k - 1) + 1: witnesses 1 .. n_assigned are assigned, witness 0 is not"""
    ops = [E([], [(3, k - 1), (P - 1, k)], 1) for k in range(2, n_assigned + 1)]
    batch = acvm_amd.Batch(acvm_amd.Circuit(Circuit(n_assigned, ops).to_bytes()), B, [1])
    batch.set_initial_witness(synth.values_from_rows([[EDGE[j % len(EDGE)] % P] for j in range(B)]))
    assert batch.solve() == 0
    return batch, _maps_of(batch)


@pytest.mark.parametrize("n_assigned", [862, 863, 1724, 1725])
def test_stored_block_boundaries(n_assigned):
    B = 65
    batch, maps = _chain(n_assigned, B)
    assert all(len(m) == n_assigned for m in maps)
    for container in CONTAINERS:
        slots, lengths = _check(batch, maps, container, list(range(B)), what=f"{n_assigned} entries, container {container}")
        if container == GZIP_STORED:
            assert lengths[0] == 16 + 8 + 76 * n_assigned + 20 * ({862: 1, 863: 2, 1724: 2, 1725: 3}[n_assigned] - 1) + 8
            for j in (0, 1, 63, 64):
                assert gzip.decompress(slots[j, :lengths[j]].tobytes()) == wire_ref.body(maps[j])


def test_a_window_boundary_meets_an_entry_that_crosses_a_block_boundary():
    """From the plan: the whole map's list position is the witness, witness 0 is unassigned, so the entry of rank r is position r + 1. The entry
    that holds body byte 65 532 is cut by the first stored-block boundary; it is the last position of its window, so the joint lies inside the
    last entry of one block's run and the next window's run starts right behind it."""
    window = _window()
    batch, maps = _chain(863)
    rank = (wire_ref.BLOCK - 8) // wire_ref.ENTRY
    assert (wire_ref.BLOCK - 8) % wire_ref.ENTRY not in (0,) and rank == 862  # the boundary falls inside the entry, not between two
    position = sorted(maps[0])[rank]
    assert position == rank + 1 and position % window == window - 1


# ---- 3. scaled and relaxed rows, the exact path
@functools.lru_cache(maxsize=None)
def _arith(force_slow):
    B = 130
    circ, ids = synth.arithmetic_circuit(300)
    batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
    batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(synth.witness_batch(B))  # (instances 0 .. 7: config 2's edge cases -- zero denominators, the exact path)
    batch.solve()
    return batch, _maps_of(batch)


@pytest.mark.parametrize("force_slow", [False, True])
def test_scaled_and_relaxed_rows_and_the_exact_path(force_slow):
    batch, maps = _arith(force_slow)
    B = batch.B
    n_slow = batch.stats()["n_slow_instances"]
    assert n_slow == B if force_slow else 1 <= n_slow < B
    for container in CONTAINERS:
        _check(batch, maps, container, list(range(B)), what=f"arith force_slow={force_slow} container {container}")


# ---- 4. partial maps in lanes 0, 63 and 64 of a batch of 130
SPECIAL = (0, 63, 64)


def _partial(kind):
    B = 130
    if kind == "assert":  # w4 = 3 w1 + 1; assert w2 == 11; w5 = 3 w2 + 1; w6 = 3 w3 + 1: a failing instance never assigns w5, w6
        circ = Circuit(6, [E([], [(3, 1), (P - 1, 4)], 1), E([], [(1, 2)], P - 11), E([], [(3, 2), (P - 1, 5)], 1), E([], [(3, 3), (P - 1, 6)], 1)])
        batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, [1, 2, 3])
        batch.set_initial_witness(synth.values_from_rows([[EDGE[j % len(EDGE)] % P, 300 + j if j in SPECIAL else 11, 5 + j] for j in range(B)]))
        batch.solve()
        want_status = acvm_amd.STATUS_FAILURE
    elif kind == "masked":  # the special instances lack input 2
        batch = acvm_amd.Batch(_readback_circuit(3), B, [1, 2, 3])
        mask = np.ones((B, 3), dtype=np.uint8)
        mask[list(SPECIAL), 1] = 0
        d_v, d_m = acvm_amd.DeviceBuffer(synth.values_from_rows(_rows(B, 3, rot=5))), acvm_amd.DeviceBuffer(mask.tobytes())
        batch.import_device_masked(d_v.ptr, d_m.ptr)
        batch.solve()
        d_v.free()
        d_m.free()
        want_status = None
    else:  # the special instances wait inside a Brillig opcode (the circuit of tests/test_gpu_outcomes.py)
        br = Brillig(inputs=[W(1), E(), W(2)], outputs=[5, 6, 7, 8],
                     bytecode=[("ForeignCall", "invert", [("Register", 1)], [("Register", 0)]),
                               ("ForeignCall", "invert", [("Register", 3)], [("Register", 2)])], predicate=W(3))
        circ = Circuit(10, [E([(1, 1, 2)], [(P - 1, 4)], 0), E([], [(1, 4), (P - 1, 9)], 1), br, E([(1, 1, 6)], [(P - 1, 10)], 0)])
        batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, [1, 2, 3])
        batch.set_initial_witness(synth.values_from_rows([[3 + j, 7 * j + 1, 1 if j in SPECIAL else 0] for j in range(B)]))
        batch.solve()
        want_status = acvm_amd.STATUS_REQUIRES_FOREIGN_CALL
    if want_status is not None:
        res = batch.results()
        assert [j for j in range(B) if res[j].status == want_status] == list(SPECIAL)
        assert all(res[j].status == acvm_amd.STATUS_SOLVED for j in range(B) if j not in SPECIAL)
    return batch, _maps_of(batch)


@pytest.mark.parametrize("kind", ["assert", "masked", "waiting"])
def test_partial_maps_in_lanes_0_63_and_64(kind):
    batch, maps = _partial(kind)
    full = len(maps[1])
    assert all(len(maps[j]) < full for j in SPECIAL) and all(len(maps[j]) == full for j in range(batch.B) if j not in SPECIAL)
    for container in CONTAINERS:
        slots, lengths = _check(batch, maps, container, list(range(batch.B)), 48, what=f"{kind} container {container}")
        assert len(set(lengths)) == 2 and all(lengths[j] < lengths[1] for j in SPECIAL)  # the lengths column differs per row
        for j in SPECIAL:
            assert (slots[j, lengths[j]:] == PATTERN).all()
    batch.free()


# ---- 5. the list form
def test_list_form_descending_repeats_and_entries_beyond_the_batch():
    batch, maps = _arith(False)
    B = batch.B
    lst = list(range(B - 1, -1, -1)) + [3, 3, 1, B, 0xFFFFFFFF, 0, B + 5, 68]
    rows = [j if j < B else None for j in lst]
    for container in CONTAINERS:
        slots, lengths = _check(batch, maps, container, rows, instances=lst, what=f"list container {container}")
        for i, j in enumerate(lst):
            if j >= B:
                assert lengths[i] == wire_ref.length(container, 0)  # count 0
    batch, maps = _solved(3, 65)  # a handle nobody left the generic path of
    lst = [64, 0, 0, 70, 33] + list(range(64, -1, -1))
    _check(batch, maps, GZIP_STORED, [j if j < 65 else None for j in lst], 48, instances=lst)


def test_list_form_reads_the_selection_outcomes_device_wrote():
    batch, maps = _partial("assert")
    B = batch.B
    d_sel = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (4 * B))
    for status, want in ((acvm_amd.STATUS_FAILURE, list(SPECIAL)), (acvm_amd.STATUS_SOLVED, [j for j in range(B) if j not in SPECIAL])):
        count = batch.outcomes_device(select_mask=1 << status, d_selected=d_sel.ptr)
        assert count == len(want)
        pitch = batch.wire_bound(GZIP_STORED)
        buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (count * pitch + TAIL))
        batch.witness_maps_wire_device(buf.ptr, GZIP_STORED, n=count, d_instances=d_sel.ptr)
        assert buf.download() == wire_ref.slots([maps[j] for j in want], GZIP_STORED, pitch, tail=TAIL)[0]
        buf.free()
    d_sel.free()
    batch.free()


# ---- 6. a witness list
def test_witness_lists():
    for batch, maps in (_arith(False), _chain(863)):
        B, nw = batch.B, batch.nw
        for witnesses in (list(range(0, nw, 3)), list(range(1, nw, 3)), [2, 5, nw - 1, nw, nw + 7, 0xFFFFFFFF], [nw], [], [nw - 1]):
            for container in CONTAINERS:
                _check(batch, maps, container, list(range(B)), witnesses=witnesses, what=f"list of {len(witnesses)} container {container}")
    batch, maps = _arith(False)
    lst = [7, 0, 129, 200, 3]
    _check(batch, maps, GZIP_STORED, [7, 0, 129, None, 3], 48, witnesses=list(range(0, batch.nw, 3)), instances=lst)
    _check(batch, maps, BINCODE, list(range(60, 130)), witnesses=list(range(2, batch.nw, 3)), first=60)


def test_slot_reuse_serves_the_kept_witnesses_and_refuses_the_whole_map():
    n_in, B = 9, 96
    keep = [n_in + 2, n_in + 6, 3]
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)), reuse_slots=True, keep=keep)
    batch.set_initial_witness(synth.values_from_rows(_rows(B, n_in, rot=2)))
    assert batch.solve() == 0
    ws = sorted(keep + [1, n_in])
    kept = batch.extract(ws)
    maps = [{w: int.from_bytes(kept[j, k].tobytes(), "big") for k, w in enumerate(ws)} for j in range(B)]
    for container in CONTAINERS:
        _check(batch, maps, container, list(range(B)), witnesses=ws, what=f"reuse container {container}")
        _check(batch, maps, container, list(range(B)), witnesses=ws + [2 * n_in + 1, 5000], what="reuse, witnesses beyond the circuit")
    pitch = batch.wire_bound(GZIP_STORED)
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (B * pitch))
    with pytest.raises(acvm_amd.AcvmError, match="error -5: .*full maps are not kept"):
        batch.witness_maps_wire_device(buf.ptr, GZIP_STORED)
    with pytest.raises(acvm_amd.AcvmError, match="error -5: .*witness %d was not kept" % (n_in + 3)):
        batch.witness_maps_wire_device(buf.ptr, GZIP_STORED, witnesses=sorted(ws + [n_in + 3]), pitch=pitch)
    assert set(buf.download()) == {PATTERN}
    buf.free()
    batch.free()


# ---- 7. agreement with the one-instance call, the host form, the library's decoder
def test_agreement_with_witness_map_bytes_the_host_form_and_decompress_witness():
    batch, maps = _arith(False)
    B = batch.B
    got, lengths, pitch = _export(batch, BINCODE, B)
    slots = got[LEAD:LEAD + B * pitch].reshape(B, pitch)
    for j in list(range(8)) + [63, 64, 65, 100, 126, 127, 128, 129]:  # the edge-case instances of the exact path among them
        assert slots[j, :int(lengths[1 + j])].tobytes() == gzip.decompress(batch.witness_map_bytes(j)), j
    for container in CONTAINERS:
        got, lengths, pitch = _export(batch, container, B)
        slots = got[LEAD:LEAD + B * pitch].reshape(B, pitch)
        host = batch.witness_maps_wire(container)
        assert len(host) == B
        for j in range(B):
            assert host[j] == slots[j, :int(lengths[1 + j])].tobytes(), (container, j)
            assert acvm_amd.decompress_witness(host[j]) == maps[j], (container, j)
        part = batch.witness_maps_wire(container, witnesses=[1, 5, 17], first=60, n=10)
        assert part == [wire_ref.encode(wire_ref.restrict(maps[j], [1, 5, 17]), container) for j in range(60, 70)]
    assert batch.witness_maps_wire(GZIP_STORED, n=0) == []


def test_host_form_in_more_than_one_chunk():
    """1 100 slots of 65 728 bytes are more than the 64 MiB of staging the host form takes at a time (batch_export.cpp WIRE_HOST_CHUNK_BYTES: 960
    rows a chunk here): the second chunk starts at another instance, reuses the CRC words and lands behind the first in the caller's buffer"""
    B = 1100
    pitch = wire_ref.bound(GZIP_STORED, 864)
    assert pitch == 65728 and 64 * (((64 << 20) // pitch) // 64) == 960
    ops = [E([], [(3, k - 1), (P - 1, k)], 1) for k in range(2, 864)]
    batch = acvm_amd.Batch(acvm_amd.Circuit(Circuit(863, ops).to_bytes()), B, [1])
    batch.set_initial_witness(synth.values_from_rows([[(EDGE[j % len(EDGE)] + j) % P] for j in range(B)]))
    assert batch.solve() == 0
    got, lengths, _ = _export(batch, GZIP_STORED, B, pitch)
    slots = got[LEAD:LEAD + B * pitch].reshape(B, pitch)
    assert (lengths[1:B + 1] == wire_ref.length(GZIP_STORED, 863)).all()
    host = batch.witness_maps_wire(GZIP_STORED)
    n = wire_ref.length(GZIP_STORED, 863)
    assert len(host) == B and b"".join(host) == slots[:, :n].tobytes()
    assert len({bytes(h[-8:-4]) for h in host}) > B // 2  # (the rows differ: so do their CRCs)
    for j in (0, 959, 960, 1099):
        assert acvm_amd.decompress_witness(host[j])[1] == (EDGE[j % len(EDGE)] + j) % P
    batch.free()


def test_after_solve_opcode_steps():
    """it answers after stepping: the maps as they stand"""
    B = 70
    circ = Circuit(6, [E([], [(3, 1), (P - 1, 4)], 1), E([], [(1, 2)], P - 11), E([], [(3, 2), (P - 1, 5)], 1), E([], [(3, 3), (P - 1, 6)], 1)])
    batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, [1, 2, 3])
    batch.set_initial_witness(synth.values_from_rows([[EDGE[j % len(EDGE)] % P, 11 if j % 4 == 0 else 300 + j, 5 + j] for j in range(B)]))
    for step in range(3):
        batch.solve_opcode()
        maps = _maps_of(batch)
        _check(batch, maps, GZIP_STORED, list(range(B)), what=f"after step {step}")
    assert len({len(m) for m in maps}) == 2
    batch.free()


# ---- 8. refusals, host-to-device traffic
def test_refusals_write_nothing():
    B = 65
    batch, maps = _solved(3, B)
    bound = batch.wire_bound(GZIP_STORED)
    assert bound == wire_ref.bound(GZIP_STORED, batch.nw) and batch.wire_bound(BINCODE, [1, 2]) == wire_ref.bound(BINCODE, 2)
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (B * (bound + 16) + TAIL))
    d_l = acvm_amd.DeviceBuffer(np.arange(4, dtype=np.uint32).tobytes())
    refused = [
        (dict(container=2), "unknown container 2"),
        (dict(witnesses=[1, 3, 3]), "not strictly ascending"),
        (dict(witnesses=[4, 1]), "not strictly ascending"),
        (dict(pitch=bound - 16), "pitch %d is below the bound %d" % (bound - 16, bound)),
        (dict(pitch=bound + 8), "not a multiple of 16"),
        (dict(first=1, n=B), "beyond the 65 live instances"),
        (dict(first=1, n=3, d_instances=d_l.ptr), "first must be 0 for a list export"),
    ]
    h2d = batch.export_h2d_bytes()
    for kw, message in refused:
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            batch.witness_maps_wire_device(buf.ptr, **kw)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*not aligned to 16 bytes"):
        batch.witness_maps_wire_device(buf.ptr + 8)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*null buffer"):
        batch.witness_maps_wire_device(None)
    L = acvm_amd.lib()
    assert L.acvm_batch_witness_maps_wire_device(batch._h, None, None, buf.ptr, None) == -1 and b"null argument" in L.acvm_last_error()
    desc, _keep = acvm_amd.wire_desc(2, 0, 0)
    assert L.acvm_batch_wire_bound(batch._h, desc) == -1 and b"unknown container" in L.acvm_last_error()
    # not solved: ACVM_E_STATE as acvm_batch_export_device
    fresh = acvm_amd.Batch(_readback_circuit(3), B, [1, 2, 3])
    fresh.set_initial_witness(synth.values_from_rows(_rows(B, 3)))
    with pytest.raises(acvm_amd.AcvmError, match="error -5"):
        fresh.witness_maps_wire_device(buf.ptr)
    fresh.free()
    batch.witness_maps_wire_device(None, n=0)  # nothing to write succeeds, with any pointer
    assert batch.export_h2d_bytes() == h2d and set(buf.download()) == {PATTERN}
    buf.free()
    d_l.free()


def test_after_solve_then_import_the_initial_witnesses_are_refused():
    B, n_in = 65, 3
    rows = _rows(B, n_in, rot=4)
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, [1, 2, 3])
    d_in, d_next = acvm_amd.DeviceBuffer(synth.values_from_rows(rows)), acvm_amd.DeviceBuffer(synth.values_from_rows(_rows(B, n_in, rot=9)))
    batch.set_initial_witness_device(d_in.ptr)
    assert batch.solve(then_import=d_next.ptr) == 0
    maps = [{n_in + 1 + k: (3 * x + 1) % P for k, x in enumerate(r)} for r in rows]
    _check(batch, maps, GZIP_STORED, list(range(B)), witnesses=[4, 5, 6])  # the gate outputs are still there
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (B * batch.wire_bound(GZIP_STORED)))
    for witnesses in (None, [2, 4]):
        with pytest.raises(acvm_amd.AcvmError, match="error -5: .*initial witnesses"):
            batch.witness_maps_wire_device(buf.ptr, GZIP_STORED, witnesses=witnesses)
    assert set(buf.download()) == {PATTERN}
    for x in (buf, d_in, d_next):
        x.free()
    batch.free()


def test_host_to_device_traffic_does_not_grow_with_n():
    batch, maps = _arith(False)
    _export(batch, GZIP_STORED, 64)  # (the exact lanes' map goes up once)
    grown = []
    for n in (64, 130):
        before = batch.export_h2d_bytes()
        _export(batch, GZIP_STORED, n)
        grown.append(batch.export_h2d_bytes() - before)
    assert grown[0] == grown[1] and 0 < grown[0] <= 4 * (2 * (batch.nw + 1) + (batch.nw + 31) // 32)  # the rank and power tables, the list mask
    lst = list(range(100))
    before = batch.export_h2d_bytes()
    _export(batch, GZIP_STORED, len(lst), instances=lst)
    assert batch.export_h2d_bytes() - before == grown[0]
