"""Packed wire buffers on the device (acvm_batch_witness_maps_wire_packed_device / _packed, acvm_batch_import_device_wire_packed,
acvm_debug_wire_repitch): row i occupies bytes [offsets[i], offsets[i + 1]) of one buffer, no byte between rows. Expected bytes are
b"".join(...) of tests/wire_ref.py and tests/wire_deflate_ref.py rows and expected offsets their running sums: no tolerance anywhere. The
import's yardstick is the pitched import of the same rows, compared bit for bit through acvm_debug_import_state."""
import ctypes as C
import gzip
import importlib.util
import os
import random

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import P, Circuit, Expression as E
import wire_deflate_ref
import wire_ref
from wire_ref import BINCODE, GZIP_STORED
from wire_deflate_ref import GZIP_DEFLATE

pytestmark = pytest.mark.gpu
FILL, LEAD, TAIL = wire_ref.FILL, 16, 64
CONTAINERS = (BINCODE, GZIP_STORED, GZIP_DEFLATE)
FILL64 = int.from_bytes(bytes([FILL]) * 8, "little")
LENGTHS = list(range(0, 41)) + [63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537]


def _load(name):
    spec = importlib.util.spec_from_file_location("_%s_for_wire_packed" % name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GW = _load("test_gpu_wire")
_solved, _partial, _arith, SPECIAL = _GW._solved, _GW._partial, _GW._arith, _GW.SPECIAL


def _model(maps, container, witnesses=None):
    """(the rows, their running sums)"""
    rows = [wire_deflate_ref.encode(m if witnesses is None else wire_ref.restrict(m, witnesses), container) for m in maps]
    offsets = [0]
    for r in rows:
        offsets.append(offsets[-1] + len(r))
    return rows, offsets


def _export(batch, container, n, capacity, size=None, witnesses=None, first=0, instances=None, null=False):
    """(the whole buffer afterwards: LEAD bytes of fill, `size` bytes, TAIL; the offsets column with a word of fill on either side; total; n_fit)"""
    size = capacity if size is None else size
    buf = acvm_amd.DeviceBuffer(bytes([FILL]) * (LEAD + size + TAIL))
    d_off = acvm_amd.DeviceBuffer(bytes([FILL]) * (8 * (n + 3)))
    d_l = acvm_amd.DeviceBuffer(np.array(instances, dtype=np.uint32).tobytes()) if instances is not None else None
    try:
        total, n_fit = batch.witness_maps_wire_packed_device(None if null else buf.ptr + LEAD, capacity, d_off.ptr + 8, container, witnesses, first=first, n=n,
                                                             d_instances=d_l.ptr if d_l else None)
        return buf.download(), np.frombuffer(d_off.download(), dtype=np.uint64), total, n_fit
    finally:
        buf.free()
        d_off.free()
        if d_l:
            d_l.free()


def _check(batch, maps, container, rows, witnesses=None, first=0, instances=None, what=""):
    """rows: per output row the instance whose map it holds, or None = an instance that assigned nothing. Returns the model's rows and offsets."""
    want_rows, want_offsets = _model([{} if j is None else maps[j] for j in rows], container, witnesses)
    n, total = len(rows), want_offsets[-1]
    got, offsets, got_total, n_fit = _export(batch, container, n, total, witnesses=witnesses, first=first, instances=instances)
    assert list(offsets[1:n + 2]) == want_offsets and offsets[0] == FILL64 and offsets[n + 2] == FILL64, what
    assert (got_total, n_fit) == (total, n), what
    want = bytes([FILL]) * LEAD + b"".join(want_rows) + bytes([FILL]) * TAIL
    if got != want:
        at = next(k for k in range(len(want)) if got[k] != want[k])
        row = max(i for i in range(n + 1) if want_offsets[i] <= max(at - LEAD, 0))
        raise AssertionError("%s: byte %d (row %d byte %d) is %#x, expected %#x" % (what, at, row, at - LEAD - want_offsets[row], got[at], want[at]))
    return want_rows, want_offsets


# ---- 1. the probe: any bytes at any lengths, both directions, every displacement of the packed base
def _probe_rows(n, seed):
    rng = random.Random(seed)
    lens = [LENGTHS[(7 * i + seed) % len(LENGTHS)] for i in range(n)]
    if n >= 63:  # (every length of the list is there, the zero-length row and the three around 2^16 among them)
        assert set(lens) == set(LENGTHS)
    return [rng.randbytes(k) for k in lens]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_probe_pack_every_displacement(n):
    pitch = 65539  # (odd: the rows' source alignments differ)
    for displacement in range(16):
        rows = _probe_rows(n, displacement)
        want = b"".join(rows)
        packed, offsets, total, n_fit = acvm_amd.debug_wire_repitch(rows=rows, packed=len(want) + TAIL, pitch=pitch, displacement=displacement, capacity=len(want), scan_chunk=64)
        assert (total, n_fit) == (len(want), n)
        assert list(offsets) == [sum(len(r) for r in rows[:i]) for i in range(n + 1)]
        assert packed.tobytes() == want + bytes([FILL]) * TAIL, (n, displacement)  # the fill behind the rows is left alone
    # a capacity in the middle of a row: the rows in front of it complete, nothing at or behind their end
    rows = _probe_rows(n, 3)
    ends = np.cumsum([len(r) for r in rows])
    k = n // 2
    packed, offsets, total, n_fit = acvm_amd.debug_wire_repitch(rows=rows, packed=int(ends[-1]) + TAIL, pitch=pitch, displacement=9, capacity=max(int(ends[k]) - 1, 0), scan_chunk=64)
    fit = int(np.searchsorted(ends, max(int(ends[k]) - 1, 0), side="right"))
    assert (total, n_fit) == (int(ends[-1]), fit) and list(offsets[1:]) == list(ends)
    kept = b"".join(rows[:fit])
    assert packed.tobytes() == kept + bytes([FILL]) * (int(ends[-1]) + TAIL - len(kept))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_probe_unpack_every_displacement(n):
    pitch = 65539  # (odd: the rows' destination alignments differ)
    for displacement in range(16):
        rows = _probe_rows(n, displacement + 16)
        offsets = [sum(len(r) for r in rows[:i]) for i in range(n + 1)]
        out, lengths, findings, count, key = acvm_amd.debug_wire_repitch(packed=b"".join(rows), offsets=offsets, pitch=pitch, displacement=displacement)
        assert count == 0 and not findings.any() and list(lengths) == [len(r) for r in rows]
        want = np.full((n, pitch), FILL, dtype=np.uint8)
        for i, r in enumerate(rows):
            want[i, :len(r)] = np.frombuffer(r, dtype=np.uint8)
        assert np.array_equal(out, want), (n, displacement)  # the rows, and the fill behind each of them


def test_probe_unpack_findings():
    rows = [bytes([i]) * 40 for i in range(70)]
    offsets = [40 * i for i in range(71)]
    offsets[6] = 100       # row 5: 200 .. 100 descending (class 1); row 6: 100 .. 280 is 180 bytes: class 3 at a pitch of 48
    offsets[65] = 2801     # row 64: 2560 .. 2801 is beyond the buffer (class 2); row 65 descends
    out, lengths, findings, count, key = acvm_amd.debug_wire_repitch(packed=b"".join(rows), offsets=offsets, pitch=48, displacement=3)
    want_findings = np.zeros(70, dtype=np.uint32)
    want_findings[[5, 6, 64, 65]] = [1, 3, 2, 1]
    assert list(findings) == list(want_findings) and count == 4 and key == (~(5 << 4 | 1)) & ((1 << 64) - 1)
    for i in range(70):
        if want_findings[i]:
            assert (out[i] == FILL).all() and lengths[i] == 0  # a row with a finding copies nothing
        else:
            assert out[i, :40].tobytes() == rows[i] and (out[i, 40:] == FILL).all() and lengths[i] == 40


# ---- 2. the export: containers and sizes
def test_the_deflate_joints_reach_every_residue():
    """bincode and stored rows are multiples of 4 bytes long (8 + 76 N, 32 + 76 N + 20 k): only deflated rows put joints inside a dword"""
    _, maps = _solved(3, 130)
    for container in (BINCODE, GZIP_STORED):
        assert {o % 4 for o in _model(maps, container)[1]} == {0}
    assert {o % 16 for o in _model(maps, GZIP_DEFLATE)[1]} == set(range(16))


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("container", CONTAINERS)
def test_sizes_and_containers(container, B):
    batch, maps = _solved(3, B)
    rows, offsets = _check(batch, maps, container, list(range(B)), what=f"container {container} B={B}")
    if container != BINCODE:  # a packed buffer of gzip members is one multi-member .gz file
        assert gzip.decompress(b"".join(rows)) == b"".join(wire_ref.body(m) for m in maps)
    host, host_offsets = batch.witness_maps_wire_packed(container)
    assert host == b"".join(rows) and list(host_offsets) == offsets


# ---- 3. partial maps and the list form
@pytest.mark.parametrize("kind", ["assert", "masked", "waiting"])
def test_partial_maps_in_lanes_0_63_and_64(kind):
    batch, maps = _partial(kind)
    for container in CONTAINERS:
        rows, _ = _check(batch, maps, container, list(range(batch.B)), what=f"{kind} container {container}")
        if container != GZIP_DEFLATE:  # the lengths differ per row
            assert all(len(rows[j]) < len(rows[1]) for j in SPECIAL)
    batch.free()


def test_list_form_descending_repeats_and_entries_beyond_the_batch():
    batch, maps = _arith(False)
    B = batch.B
    lst = list(range(B - 1, -1, -1)) + [3, 3, 1, B, 0xFFFFFFFF, 0, B + 5, 68]
    for container, empty in zip(CONTAINERS, (8, 32, 63)):
        rows, _ = _check(batch, maps, container, [j if j < B else None for j in lst], instances=lst, what=f"list container {container}")
        assert [len(rows[i]) for i, j in enumerate(lst) if j >= B] == [empty] * 3  # maps of 0 entries
    _check(batch, maps, GZIP_DEFLATE, [7, 0, 129, None, 3], witnesses=list(range(0, batch.nw, 3)), instances=[7, 0, 129, 200, 3])
    _check(batch, maps, GZIP_STORED, list(range(60, 130)), witnesses=list(range(2, batch.nw, 3)), first=60)


# ---- 4. a capacity
@pytest.mark.parametrize("container", CONTAINERS)
def test_capacities_around_a_rows_end(container):
    B = 65
    batch, maps = _solved(3, B)
    rows, offsets = _model(maps, container)
    total = offsets[-1]
    got, sized, sized_total, sized_fit = _export(batch, container, B, 0, size=total, null=True)  # the sizing call
    assert list(sized[1:B + 2]) == offsets and (sized_total, sized_fit) == (total, 0) and set(got) == {FILL}
    L = acvm_amd.lib()
    for k in (1, 33, B):  # the end of the first, of a middle and of the last row
        for capacity in (offsets[k] - 1, offsets[k], offsets[k] + 1):
            fit = k - 1 if capacity < offsets[k] else k
            got, offs, got_total, n_fit = _export(batch, container, B, capacity, size=total)
            assert (got_total, n_fit) == (total, fit) and list(offs[1:B + 2]) == offsets, (k, capacity)
            assert got == bytes([FILL]) * LEAD + b"".join(rows[:fit]) + bytes([FILL]) * (total - offsets[fit] + TAIL), (k, capacity)
            # the host form at the same capacity
            out, host_offsets = np.full(total + TAIL, FILL, dtype=np.uint8), np.zeros(B + 1, dtype=np.uint64)
            desc, _keep = acvm_amd.wire_desc(container, 0, B)
            t, f = C.c_uint64(), C.c_uint32()
            assert L.acvm_batch_witness_maps_wire_packed(batch._h, C.byref(desc), out.ctypes.data, capacity, host_offsets.ctypes.data, C.byref(t), C.byref(f)) == 0
            assert (t.value, f.value) == (total, fit) and list(host_offsets) == offsets
            assert out.tobytes() == b"".join(rows[:fit]) + bytes([FILL]) * (total - offsets[fit] + TAIL), (k, capacity)
    # a caller whose buffer was too small continues with the list form on the remaining instances
    fit = 33
    rest = list(range(fit, B))
    got, offs, got_total, n_fit = _export(batch, container, len(rest), offsets[-1] - offsets[fit], instances=rest)
    assert n_fit == len(rest) and got[LEAD:LEAD + got_total] == b"".join(rows[fit:])


# ---- 5. more than one chunk
def test_more_than_one_chunk():
    """1 100 slots of 65 728 bytes are more than the 64 MiB of staging a chunk takes (960 rows here): the base carries over row 960"""
    B = 1100
    assert wire_ref.bound(GZIP_STORED, 864) == 65728
    ops = [E([], [(3, k - 1), (P - 1, k)], 1) for k in range(2, 864)]
    batch = acvm_amd.Batch(acvm_amd.Circuit(Circuit(863, ops).to_bytes()), B, [1])
    batch.set_initial_witness(synth.values_from_rows([[(_GW.EDGE[j % len(_GW.EDGE)] + j) % P] for j in range(B)]))
    assert batch.solve() == 0
    n = wire_ref.length(GZIP_STORED, 863)
    got, offsets, total, n_fit = _export(batch, GZIP_STORED, B, B * n)
    assert (total, n_fit) == (B * n, B) and list(offsets[1:B + 2]) == [n * i for i in range(B + 1)]
    assert set(got[:LEAD]) == {FILL} and set(got[LEAD + total:]) == {FILL}
    host, host_offsets = batch.witness_maps_wire_packed(GZIP_STORED)
    assert host == got[LEAD:LEAD + total] and list(host_offsets) == [n * i for i in range(B + 1)]
    maps = {j: acvm_amd.decompress_witness(host[n * j:n * (j + 1)]) for j in (0, 959, 960, 1099)}
    for j, m in maps.items():
        assert m[1] == (_GW.EDGE[j % len(_GW.EDGE)] + j) % P and host[n * j:n * (j + 1)] == wire_ref.encode(m, GZIP_STORED)
    batch.free()


# ---- 6. the round trip: packed export, packed import on a second handle
def _two_circuits(n):
    circ_a = Circuit(8, [E([], [(3, 1), (P - 1, 5)], 1), E([], [(3, 2), (P - 1, 6)], 1), E([], [(1, 3), (P - 1, 4)], 0), E([], [(3, 3), (P - 1, 7)], 1),
                         E([], [(3, 4), (P - 1, 8)], 1)])
    circ_b = Circuit(10, [E([], [(1, 6), (P - 1, 8)], 2), E([], [(3, 5), (P - 1, 9)], 1), E([], [(3, 7), (P - 1, 10)], 1)])
    rng = random.Random(0x1F8B6004)
    rows_a = []
    for j in range(n):
        x = rng.randrange(P)
        rows_a.append([rng.randrange(P), x, (3 * x + 2) * pow(3, -1, P) % P, 0])
        rows_a[-1][3] = rows_a[-1][2] if j % 3 else (rows_a[-1][2] + 1) % P  # every third instance of A fails: its map lacks w7, w8
    ga = acvm_amd.Batch(acvm_amd.Circuit(circ_a.to_bytes()), n, [1, 2, 3, 4])
    ga.set_initial_witness(synth.values_from_rows(rows_a))
    ga.solve()
    return ga, circ_b, [5, 6, 7, 8]


def _pitched_import(ga, gb, container, ids, n):
    pitch = ga.wire_bound(container, ids)
    d_bytes, d_len = acvm_amd.DeviceBuffer(bytes([FILL]) * (n * pitch)), acvm_amd.DeviceBuffer(bytes(8 * n))
    ga.witness_maps_wire_device(d_bytes.ptr, container, ids, n=n, pitch=pitch, d_lengths=d_len.ptr)
    if container == GZIP_DEFLATE:
        gb.import_device_wire_gzip(d_bytes.ptr, pitch, d_len.ptr)
    else:
        gb.import_device_wire(d_bytes.ptr, container, pitch, d_len.ptr)
    d_bytes.free()
    d_len.free()


@pytest.mark.parametrize("container", CONTAINERS)
def test_round_trip_equals_the_pitched_import(container):
    n = 130
    ga, circ_b, ids = _two_circuits(n)
    pitch = ga.wire_bound(container, ids)
    d_off = acvm_amd.DeviceBuffer(bytes(8 * (n + 1)))
    total, _ = ga.witness_maps_wire_packed_device(None, 0, d_off.ptr, container, ids)
    d_bytes = acvm_amd.DeviceBuffer(bytes([FILL]) * total)  # exactly the rows: the buffer ends with the last row's last byte
    assert ga.witness_maps_wire_packed_device(d_bytes.ptr, total, d_off.ptr, container, ids) == (total, n)
    if container == GZIP_DEFLATE:
        assert total % 4 != 0 or len({o % 4 for o in np.frombuffer(d_off.download(), dtype=np.uint64)}) > 1  # joints inside dwords
    new, old = (acvm_amd.Batch(acvm_amd.Circuit(circ_b.to_bytes()), n, ids) for _ in range(2))
    new.import_device_wire_packed(d_bytes.ptr, total, d_off.ptr, container, pitch)
    _pitched_import(ga, old, container, ids, n)
    assert new.import_missing() == old.import_missing() == len(range(0, n, 3))
    sn, so = new.import_state(), old.import_state()
    for key in ("missing", "events", "planes", "rows"):
        assert np.array_equal(sn[key], so[key]), (container, key)
    new.solve()
    old.solve()
    assert [r.as_tuple() for r in new.results()] == [r.as_tuple() for r in old.results()]
    (an, vn), (ao, vo) = new.witness_map(), old.witness_map()
    assert np.array_equal(an, ao) and np.array_equal(vn[an.astype(bool)], vo[ao.astype(bool)])
    res = [r.as_tuple() for r in new.results()]
    assert any(r[0] != 0 for r in res) and any(r[0] == 0 for r in res)
    for x in (d_bytes, d_off, ga, new, old):
        x.free()


# ---- 7. findings of the offsets leave the handle as it was
def test_import_findings_leave_the_handle_as_it_was():
    n = 130
    ga, circ_b, ids = _two_circuits(n)
    container = GZIP_DEFLATE
    pitch = ga.wire_bound(container, ids)
    packed, offsets = ga.witness_maps_wire_packed(container, ids)
    offsets = [int(o) for o in offsets]
    d_bytes = acvm_amd.DeviceBuffer(packed)
    new, old = (acvm_amd.Batch(acvm_amd.Circuit(circ_b.to_bytes()), n, ids) for _ in range(2))

    def imported(column, n_bytes=len(packed), pitch=pitch):
        d_off = acvm_amd.DeviceBuffer(np.array(column, dtype=np.uint64).tobytes())
        try:
            new.import_device_wire_packed(d_bytes.ptr, n_bytes, d_off.ptr, container, pitch)
        finally:
            d_off.free()

    imported(offsets)
    before = (new.import_state(), new.import_missing())
    longest = max(offsets[i + 1] - offsets[i] for i in range(n))
    texts = {1: "in front of its start", 2: "beyond the buffer", 3: "longer than the pitch"}

    def judged(column, n_bytes=len(packed), pitch=pitch):
        """the findings as (instance, class), ascending"""
        out = []
        for j in range(n):
            lo, hi = column[j], column[j + 1]
            cls = 1 if hi < lo else 2 if hi > n_bytes else 3 if hi - lo > pitch else 0
            if cls:
                out.append((j, cls))
        return out

    cases = []
    bad = list(offsets)
    bad[65] = offsets[64] - 1                       # row 64 descends; row 65 then starts in front of row 64
    cases.append((bad, {}, (64, 1)))
    bad = list(offsets)
    bad[64], bad[101] = offsets[63] - 5, offsets[100] - 1
    cases.append((bad, {}, (63, 1)))
    cases.append((offsets, dict(n_bytes=offsets[100] + 3), (100, 2)))   # rows 100 .. 129 end beyond the buffer
    bad = list(offsets)
    bad[n] = len(packed) + 1
    cases.append((bad, {}, (n - 1, 2)))
    small = (longest - 1) // 16 * 16
    cases.append((offsets, dict(pitch=small), (next(i for i in range(n) if offsets[i + 1] - offsets[i] > small), 3)))
    bad = list(offsets)
    bad[1], bad[65] = len(packed) + 7, offsets[64] - 1  # class 2 in row 0, class 1 in rows 1 and 64: the smallest (instance, class) is named
    cases.append((bad, {}, (0, 2)))
    assert {c[2][1] for c in cases} == {1, 2, 3}
    for column, kw, first in cases:
        found = judged(column, **kw)
        assert found[0] == first
        count, (instance, cls), text = len(found), first, texts[first[1]]
        with pytest.raises(acvm_amd.AcvmError, match=rf"error -1: wire offsets: {count} findings, the first of them instance {instance}, class {cls} \(.*{text}.*\); the handle stays as it was"):
            imported(column, **kw)
        state, missing = new.import_state(), new.import_missing()
        for key in before[0]:
            assert np.array_equal(before[0][key], state[key]), (cls, key)
        assert missing == before[1]
    new.solve()  # the previous import still solves
    _pitched_import(ga, old, container, ids, n)
    old.solve()
    assert [r.as_tuple() for r in new.results()] == [r.as_tuple() for r in old.results()]
    # what the import behind the offsets finds is its own: a row cut short is the inflater's finding, and the handle is as ITS rule says
    cut = list(offsets)
    cut[n] = offsets[n] - 1
    with pytest.raises(acvm_amd.AcvmError, match=rf"error -1: wire inflate: 1 findings, the first of them instance {n - 1}, class 7 "):
        imported(cut)
    for x in (d_bytes, ga, new, old):
        x.free()


# ---- 8. refusals, host-to-device traffic
def test_refusals_write_nothing():
    B = 65
    batch, maps = _solved(3, B)
    total = _model(maps, GZIP_STORED)[1][-1]
    buf = acvm_amd.DeviceBuffer(bytes([FILL]) * (total + TAIL))
    d_off = acvm_amd.DeviceBuffer(bytes([FILL]) * (8 * (B + 1)))
    d_l = acvm_amd.DeviceBuffer(np.arange(4, dtype=np.uint32).tobytes())
    L = acvm_amd.lib()
    h2d = batch.export_h2d_bytes()

    def call(ptr=buf.ptr, capacity=total, offsets=d_off.ptr, pitch=0, container=GZIP_STORED, first=0, n=B, instances=None, witnesses=None):
        desc, _keep = acvm_amd.wire_desc(container, first, n, witnesses, pitch)
        t, f = C.c_uint64(0xABCD), C.c_uint32(0xABCD)
        rc = L.acvm_batch_witness_maps_wire_packed_device(batch._h, C.byref(desc), instances, ptr, capacity, offsets, C.byref(t), C.byref(f))
        assert (t.value, f.value) == (0xABCD, 0xABCD) or rc == 0
        return rc, L.acvm_last_error()

    bound = batch.wire_bound(GZIP_STORED)
    for kw, message in [(dict(pitch=bound), b"a packed export has no pitch"), (dict(pitch=16), b"a packed export has no pitch"), (dict(ptr=buf.ptr + 8), b"not aligned to 16 bytes"),
                        (dict(offsets=None), b"null offsets"), (dict(first=1), b"beyond the 65 live instances"), (dict(first=1, n=3, instances=d_l.ptr), b"first must be 0 for a list export"),
                        (dict(ptr=None), b"null buffer with a capacity"), (dict(container=2), b"unknown container 2"), (dict(witnesses=[4, 1]), b"not strictly ascending")]:
        rc, err = call(**kw)
        assert rc == -1 and message in err, (kw, err)
    assert L.acvm_batch_witness_maps_wire_packed_device(batch._h, None, None, buf.ptr, total, d_off.ptr, None, None) == -1 and b"null argument" in L.acvm_last_error()
    fresh = acvm_amd.Batch(_GW._readback_circuit(3), B, [1, 2, 3])  # not solved: ACVM_E_STATE as the pitched export
    fresh.set_initial_witness(synth.values_from_rows(_GW._rows(B, 3)))
    with pytest.raises(acvm_amd.AcvmError, match="error -5"):
        fresh.witness_maps_wire_packed_device(buf.ptr, total, d_off.ptr)
    fresh.free()
    assert batch.export_h2d_bytes() == h2d and set(buf.download()) == {FILL} and set(d_off.download()) == {FILL}
    # the import's own: a staging pitch that is no multiple of 16, null offsets, a misaligned buffer
    imp = acvm_amd.Batch(_GW._readback_circuit(3), B, [1, 2, 3])
    for kw, message in [(dict(pitch=0), "pitch 0"), (dict(pitch=72), "not a multiple of 16"), (dict(d_offsets=None), "null offsets"), (dict(d_ptr=buf.ptr + 4), "not aligned to 16 bytes"),
                        (dict(container=5), "unknown container 5")]:
        args = dict(d_ptr=buf.ptr, n_bytes=total, d_offsets=d_off.ptr, container=GZIP_STORED, pitch=bound)
        args.update(kw)
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            imp.import_device_wire_packed(**args)
    for x in (buf, d_off, d_l, imp):
        x.free()


def test_host_to_device_traffic_does_not_grow_with_n():
    batch, maps = _arith(False)
    total = _model(maps, GZIP_DEFLATE)[1][-1]
    _export(batch, GZIP_DEFLATE, 64, total)  # (the exact lanes' map goes up once)
    grown = []
    for n in (64, 130):
        before = batch.export_h2d_bytes()
        _export(batch, GZIP_DEFLATE, n, total)
        grown.append(batch.export_h2d_bytes() - before)
    assert grown[0] == grown[1] > 0
    pitch = batch.wire_bound(GZIP_DEFLATE)
    buf = acvm_amd.DeviceBuffer(size=130 * pitch)
    before = batch.export_h2d_bytes()
    batch.witness_maps_wire_device(buf.ptr, GZIP_DEFLATE)
    assert batch.export_h2d_bytes() - before == grown[0]  # the pitched export's traffic, nothing more
    buf.free()
