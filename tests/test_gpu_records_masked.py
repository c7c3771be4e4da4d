"""The masked record import (acvm_batch_import_device_records_masked, acvm_batch_set_initial_witness_records_masked) on the device: packed records
whose fields carry presence bytes, for instances that do not all hold every initial witness.

The yardstick for STATE is acvm_batch_import_device_masked on a second handle, fed the same values (as BE32 columns) and the same presence bits (as
a column mask): rows, byte planes, event words, missing-set words (acvm_debug_import_state) and acvm_debug_import_missing are compared bit for bit.
The yardstick for OUTCOMES is the CPU oracle, through the circuits, absence patterns and checks of tests/test_gpu_import_masked.py.

Record shapes (37 initial witnesses: two words of the missing set):
  a  pitch <= 256, odd: {valid, value} pairs, mostly narrow encodings -- one window, every mask byte in the LDS image
  b  pitch > 256, odd: {valid, value} pairs of mixed encodings -- at least three windows, every mask byte beside its element
  c  the encodings of b with all 37 mask bytes gathered at the record's head -- the first few are near, the rest further than a window from their
     element: the far form, one byte load per lane
Buffers hold 0xA5 wherever neither a field nor a mask byte lies, 0xEE under an absent element, and are exactly lead + B * pitch bytes."""
import functools
import importlib.util
import os
import random

import numpy as np
import pytest

import acvm_amd
import records_ref as rr
from records_ref import BE32, LE32, MONT, P, U8, U16, U32, U64, U128

pytestmark = pytest.mark.gpu
IM = acvm_amd.LAYOUT_INSTANCE_MAJOR


def _sibling(name):
    spec = importlib.util.spec_from_file_location("_for_records_masked_" + name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GM = _sibling("test_gpu_import_masked")
_GR = _sibling("test_gpu_records")
N_IN, PATTERNS = _GM.N_IN, _GM.PATTERNS
BMAX = _GM.B  # 300: the batch of the oracle's cases; the state tests take the first B instances of everything
CAP = 256
ENC_A = [(U8, U16, U32, U8, U64, U8, U16)[k % 7] for k in range(N_IN)]
ENC_A[20], ENC_A[33] = U128, BE32
ENC_B = [(BE32, U8, LE32, U32, MONT, U16, U128, U64)[k % 8] for k in range(N_IN)]
ENC_C = [(BE32, LE32, MONT)[k % 3] for k in range(N_IN)]  # 32-byte encodings only: any field element


# ---- record layouts: (pitch, [(position, encoding, offset, mask_offset)])
@functools.lru_cache(maxsize=None)
def _layout(shape, encs):
    fields, at = [], N_IN if shape == "c" else 0
    for k, e in enumerate(encs):
        if shape == "c":
            fields.append((k, e, at, k))
            at += rr.size_of(e)
        else:
            fields.append((k, e, at + 1, at))
            at += 1 + rr.size_of(e)
    pitch = at + 2 if at % 2 else at + 1  # odd, with at least one byte of padding behind the last field
    if shape == "b":
        fields = fields[::-1]              # (the caller's order is any order)
    return pitch, tuple(fields)


def test_the_shapes_are_what_the_cases_need():
    """(no device) shape a is one window; b has at least three with every mask byte near; c has near and far mask bytes"""
    pa, fa = _layout("a", tuple(ENC_A))
    pb, fb = _layout("b", tuple(ENC_B))
    pc, fc = _layout("c", tuple(ENC_B))
    assert pa <= CAP and pa % 2 == 1 and pb > 2 * CAP and pb % 2 == 1 and pc > CAP and pc % 2 == 1
    span = lambda f: max(f[2] + rr.size_of(f[1]), f[3] + 1) - min(f[2], f[3])
    assert all(span(f) <= 33 for f in fa + fb)
    assert sum(span(f) <= CAP for f in fc) >= 3 and sum(span(f) > CAP for f in fc) >= 20
    assert {rr.size_of(e) for e in ENC_A} == {1, 2, 4, 8, 16, 32} and {rr.size_of(e) for e in ENC_B} == {1, 2, 4, 8, 16, 32}


# ---- values: vals[j][k] Python integers; raws[k] the element bytes [BMAX][size]; be[k] the same values as BE32 [BMAX][32]
@functools.lru_cache(maxsize=None)
def _values(kind, encs):
    rng = random.Random(0x4EC3A5 + len(kind))
    vals = []
    for j in range(BMAX):
        row = []
        for k, e in enumerate(encs):
            top = 256 if kind == "bytes" else P if rr.size_of(e) == 32 else 1 << (8 * rr.size_of(e))
            edges = [0, 1, 255, min(256, top - 1), top - 1]
            row.append(edges[(j + k) % 5] if (j + 2 * k) % 7 == 0 else rng.randrange(top))
        vals.append(row)
    return vals


@functools.lru_cache(maxsize=None)
def _raws_of(source, encs):
    """source: a _values kind, or "circuit:NAME" -- the values of a circuit of tests/test_gpu_import_masked.py"""
    vals = _GM._circuit(source[8:])[2] if source.startswith("circuit:") else _values(source, encs)
    raws = [np.frombuffer(b"".join(rr.element(vals[j][k], e) for j in range(BMAX)), dtype=np.uint8).reshape(BMAX, rr.size_of(e)) for k, e in enumerate(encs)]
    be = [np.frombuffer(b"".join(int(vals[j][k]).to_bytes(32, "big") for j in range(BMAX)), dtype=np.uint8).reshape(BMAX, 32) for k in range(len(encs))]
    return raws, be


def _records(B, pitch, fields, raws, held, lead=0, under_absent=0xEE, edit=None):
    """the buffer: `lead` bytes, B records. held[j][k] = 1 where instance j holds position k; edit(buf [B][pitch]) may change it last"""
    buf = np.full((B, pitch), rr.PATTERN, dtype=np.uint8)
    for k, e, off, m in fields:
        buf[:, off:off + rr.size_of(e)] = raws[k][:B]
    for k, e, off, m in fields:
        if m is not None:
            buf[held[:B, k] == 0, off:off + rr.size_of(e)] = under_absent
    for k, e, off, m in fields:
        if m is not None:
            buf[:, m] = held[:B, k]
    if edit is not None:
        edit(buf)
    return bytes([rr.PATTERN]) * lead + buf.tobytes()


def _import_records(batch, B, pitch, fields, raws, held, lead=0, **kw):
    data = _records(B, pitch, fields, raws, held, lead, **kw)
    assert len(data) == lead + B * pitch
    buf = acvm_amd.DeviceBuffer(data)
    try:
        batch.import_device_records_masked(buf.ptr + lead, pitch, fields)
    finally:
        buf.free()


def _import_columns(batch, B, be, held):
    """the yardstick: the same values as dense BE32 columns and the same presence as a column mask, through acvm_batch_import_device_masked"""
    values = np.stack([b[:B] for b in be], axis=1).copy()
    values[held[:B] == 0] = 0x5A  # (absent: any bytes)
    dv, dm = acvm_amd.DeviceBuffer(values.tobytes()), acvm_amd.DeviceBuffer(np.ascontiguousarray(held[:B]).tobytes())
    try:
        batch.import_device(dv.ptr, encoding=BE32, layout=IM, d_assigned=dm.ptr)
    finally:
        dv.free()
        dm.free()


def _assert_same_import_state(got, want, what):
    sg, sw = got.import_state(), want.import_state()
    for key in ("missing", "events", "planes", "rows"):
        bad = np.argwhere(sg[key] != sw[key])
        assert bad.size == 0, f"{what}: {key}{tuple(bad[0])} is {sg[key][tuple(bad[0])]:#x}, the column import's {sw[key][tuple(bad[0])]:#x} ({len(bad)} words differ)"
    assert got.import_missing() == want.import_missing(), what
    return sg


def _circuit_of(kind):
    return "b" if kind == "bytes" else "a"  # "b": the first 32 inputs have byte planes; "a": none, any field element


def _pair(kind, B, **kw):
    name = _circuit_of(kind)
    return (acvm_amd.Batch(_GM._device_circuit(name), B, _GM._circuit(name)[1], **kw), acvm_amd.Batch(_GM._device_circuit(name), B, _GM._circuit(name)[1], **kw))


# ---- 1. sizes, bases, absence patterns, shapes
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("shape,kind", [("a", "mixed"), ("a", "bytes"), ("b", "mixed"), ("b", "bytes"), ("c", "mixed"), ("c", "bytes")])
def test_state_equals_the_masked_column_import(shape, kind, B):
    encs = tuple(ENC_A if shape == "a" else ENC_B)
    pitch, fields = _layout(shape, encs)
    raws, be = _raws_of(kind, encs)
    new, ref = _pair(kind, B)
    assert (new.stats()["n_byte_planes"] > 0) == (kind == "bytes")
    for q, pattern in enumerate(PATTERNS):
        held = _GM._held(pattern)
        _import_records(new, B, pitch, fields, raws, held, lead=(q + B) % 4)
        _import_columns(ref, B, be, held)
        state = _assert_same_import_state(new, ref, f"shape {shape} {kind} B={B} pattern {pattern} base+{(q + B) % 4}")
        assert new.import_missing() == int((held[:B] == 0).any(axis=1).sum())
        # (the yardstick's own meaning, once more in plain numpy: bit k & 31 of word k >> 5 is set exactly where the instance lacks position k)
        want = np.zeros((2, B), dtype=np.uint32)
        for k in range(N_IN):
            want[k >> 5] |= (held[:B, k] == 0).astype(np.uint32) << np.uint32(k & 31)
        assert np.array_equal(state["missing"], want) and (state["events"][2:] == 0xFFFFFFFF).all()
    for x in (new, ref):
        x.free()


# ---- 2. garbage under an absent element
@pytest.mark.parametrize("shape", ["b", "c"])
def test_garbage_under_an_absent_element_changes_nothing(shape):
    """0xFF .. FF and a value >= p under absent 32-byte elements, a narrow non-byte under an absent lane of a wave of bytes: the state is the one
    with zero bytes there and the column import's, the other 63 lanes of those waves included"""
    B, encs = 130, tuple(ENC_B)
    pitch, fields = _layout(shape, encs)
    raws, be = _raws_of("bytes", encs)  # every present value a byte: whole waves take the closed form of the row
    by_position = {f[0]: f for f in fields}
    held = np.ones((BMAX, N_IN), dtype=np.uint8)
    spots = [(70, 0, b"\xff" * 32), (3, 8, P.to_bytes(32, "big")), (64, 2, (P + 5).to_bytes(32, "little")), (129, 4, b"\xff" * 32),
             (5, 5, b"\xff\xff"), (100, 3, b"\x00\x01\x00\x00"), (66, 6, b"\xff" * 16), (0, 36, b"\xff" * 32), (65, 35, b"\xff" * 4)]
    for j, k, raw in spots:
        assert len(raw) == rr.size_of(encs[k])
        held[j, k] = 0

    def garbage(buf):
        for j, k, raw in spots:
            off = by_position[k][2]
            buf[j, off:off + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    new, ref = _pair("bytes", B)
    _import_columns(ref, B, be, held)
    _import_records(new, B, pitch, fields, raws, held, lead=1, under_absent=0)
    clean = _assert_same_import_state(new, ref, f"shape {shape}, zero bytes under the absent elements")
    _import_records(new, B, pitch, fields, raws, held, lead=3, edit=garbage)
    dirty = _assert_same_import_state(new, ref, f"shape {shape}, garbage under the absent elements")
    for key in clean:
        assert np.array_equal(clean[key], dirty[key])
    for j, k, _ in spots:  # the absent rows are zero, their plane word says "the byte zero"
        assert not dirty["rows"][k, :, j].any() and dirty["planes"][k, j] in (0, 0x80000000)  # (0: an input without a plane)
    for x in (new, ref):
        x.free()


# ---- 3. shared and overlapping mask bytes
@pytest.mark.parametrize("long_record", [False, True])
def test_shared_mask_bytes_and_a_mask_byte_inside_a_field(long_record):
    """positions 0 .. 7 share ONE valid byte, positions 8 .. 11 another; the mask byte of position 13 is byte 1 of position 12's U32, that of
    position 14 is the first byte of its own element (so the element, where present, begins with the byte 1); the rest carry no mask"""
    B, encs = 130, [U32] * N_IN
    encs[13], encs[14], encs[20] = BE32, U16, MONT
    encs = tuple(encs)
    at, offs = 2, []
    for e in encs:
        offs.append(at)
        at += rr.size_of(e) + (9 if long_record else 0)
    pitch = at + 1
    assert (pitch > 2 * CAP) == long_record
    mask_of = {k: 0 for k in range(8)}
    mask_of.update({k: 1 for k in range(8, 12)})
    mask_of[13], mask_of[14] = offs[12] + 1, offs[14]
    fields = tuple((k, e, offs[k], mask_of.get(k)) for k, e in enumerate(encs))
    raws, be = _raws_of("mixed", encs)
    raws, be = [r.copy() for r in raws], [b.copy() for b in be]
    rng = np.random.default_rng(0x3A5CE)
    struct0, struct1, h13, h14 = (rng.random(BMAX) < 0.7, rng.random(BMAX) < 0.5, rng.random(BMAX) < 0.6, rng.random(BMAX) < 0.5)
    held = np.ones((BMAX, N_IN), dtype=np.uint8)
    held[:, :8], held[:, 8:12], held[:, 13], held[:, 14] = struct0[:, None], struct1[:, None], h13, h14
    # the overlapped elements hold the mask bytes: position 12 (always held) has byte 1 = held[13]; position 14 begins with its own presence
    raws[12][:, 1] = held[:, 13]
    raws[14][:, 0] = held[:, 14]
    for k in (12, 14):
        be[k] = np.frombuffer(b"".join(int.from_bytes(raws[k][j].tobytes(), "little").to_bytes(32, "big") for j in range(BMAX)), dtype=np.uint8).reshape(BMAX, 32)

    def overlapped(buf):  # (_records put 0xEE under the absent position 14, its own mask byte included: the presence byte again)
        buf[:, offs[14]] = held[:B, 14]
    new, ref = _pair("mixed", B)
    _import_records(new, B, pitch, fields, raws, held, lead=2, edit=overlapped)
    _import_columns(ref, B, be, held)
    _assert_same_import_state(new, ref, "shared and overlapping mask bytes")
    assert 0 < new.import_missing() < B
    for x in (new, ref):
        x.free()


# ---- 4. stale bits
def test_no_bit_of_an_earlier_import_survives():
    B, encs = 257, tuple(ENC_B)
    raws, be = _raws_of("bytes", encs)
    new, ref = _pair("bytes", B)
    for shape in ("b", "c"):
        pitch, fields = _layout(shape, encs)
        _import_records(new, B, pitch, fields, raws, _GM._held("everyone"))
        assert new.import_missing() == B and new.import_state()["missing"].any(axis=0).all()
        _import_records(new, B, pitch, fields, raws, _GM._held("none"))
        assert new.import_missing() == 0 and not new.import_state()["missing"].any()
        assert new.solve() == 0 and new.stats()["n_slow_instances"] == 0  # nobody was flagged: no flag pass, no exact lane
        _import_records(new, B, pitch, fields, raws, _GM._held("everyone"))
        _import_records(new, B, pitch, fields, raws, _GM._held("pos36"))
        _import_columns(ref, B, be, _GM._held("pos36"))
        _assert_same_import_state(new, ref, f"shape {shape}: pos36 behind everyone")
        # the unmasked record import clears the missing state
        _import_records(new, B, pitch, fields, raws, _GM._held("everyone"))
        data = _records(B, pitch, fields, raws, _GM._held("none"))
        buf = acvm_amd.DeviceBuffer(data)
        new.import_device_records(buf.ptr, pitch, [f[:3] for f in fields])
        buf.free()
        assert new.import_missing() == 0
        assert new.solve() == 0 and new.stats()["n_slow_instances"] == 0
    for x in (new, ref):
        x.free()


# ---- 5. bad bytes
@pytest.mark.parametrize("byte", [2, 255])
@pytest.mark.parametrize("lowest", [0, 64])
def test_bad_mask_bytes_fail_closed(byte, lowest):
    """shape c: the mask bytes of positions 0, 3, 5 are near, that of position 36 far"""
    B, encs = 257, tuple(ENC_B)
    pitch, fields = _layout("c", encs)
    kinds = {f[0]: max(f[2] + rr.size_of(f[1]), f[3] + 1) - min(f[2], f[3]) > CAP for f in fields}
    assert not kinds[0] and not kinds[3] and not kinds[5] and kinds[36]
    raws, be = _raws_of("bytes", encs)
    ids = _GM._circuit("b")[1]
    new, ref = _pair("bytes", B)
    _import_records(new, B, pitch, fields, raws, _GM._held("pos0"))  # a good import first: the refusal below takes it away
    bad = [(200, 5), (lowest, 36), (lowest, 3), (256, 0)]

    def spoil(buf):
        for j, k in bad:
            buf[j, k] = byte  # (shape c: the mask byte of position k is byte k of the record)
    with pytest.raises(acvm_amd.AcvmError, match=rf"error -1: .*\b4 elements .*instance {lowest}, position 3 \(initial witness {ids[3]}\)"):
        _import_records(new, B, pitch, fields, raws, _GM._held("random"), lead=1, edit=spoil)
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        new.solve()
    # a far byte alone, in a later instance
    with pytest.raises(acvm_amd.AcvmError, match=rf"error -1: .*\b1 elements .*instance 130, position 36 \(initial witness {ids[36]}\)"):
        _import_records(new, B, pitch, fields, raws, _GM._held("none"), edit=lambda buf: buf.__setitem__((130, 36), byte))
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        new.solve()
    _import_records(new, B, pitch, fields, raws, _GM._held("random"), lead=2)  # a following good import recovers
    _import_columns(ref, B, be, _GM._held("random"))
    _assert_same_import_state(new, ref, "after the refused bytes")
    new.solve()
    ref.solve()
    assert [r.as_tuple() for r in new.results()] == [r.as_tuple() for r in ref.results()]
    for x in (new, ref):
        x.free()


# ---- 6. host refusals
def test_host_refusals_leave_the_previous_import_in_place():
    B, encs = 65, tuple(ENC_A)
    pitch, fields = _layout("a", encs)
    raws, be = _raws_of("mixed", encs)
    new, ref = _pair("mixed", B)
    _import_records(new, B, pitch, fields, raws, _GM._held("random"))
    before = new.import_state()
    ptr = 1 << 20  # (never read: every call below is refused by the host checks)
    with_mask = lambda f, m: [f[0][:3] + (m,)] + list(f[1:])
    refused = [
        (pitch, with_mask(fields, pitch), "field 0 .*mask_offset %d is not below the pitch %d" % (pitch, pitch)),
        (pitch, with_mask(fields, (1 << 64) - 2), "field 0 .*mask_offset"),
        (pitch, list(fields[:-1]), "position .*no field"),
        (pitch, list(fields) + [(1, U8, 6, 0)], "position 1 is supplied twice"),
        (pitch, [(0, U32, pitch - 3, pitch)] + list(fields[1:]), "field 0 .*beyond the pitch"),  # the unmasked refusal comes first
    ]
    for pt, fl, message in refused:
        copies = new.import_list_copies()
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            new.import_device_records_masked(ptr, pt, fl)
        assert new.import_list_copies() == copies
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*null records"):
        new.import_device_records_masked(None, pitch, fields)
    L = acvm_amd.lib()
    assert L.acvm_batch_import_device_records_masked(new._h, None, ptr) == -1 and b"null argument" in L.acvm_last_error()
    after = new.import_state()
    for key in before:
        assert np.array_equal(before[key], after[key])
    _import_columns(ref, B, be, _GM._held("random"))
    _assert_same_import_state(new, ref, "after the refusals")
    for x in (new, ref):
        x.free()


# ---- 7. no masks at all
def test_without_masks_it_is_the_record_import():
    B, encs = 130, tuple(ENC_B)
    pitch, fields = _layout("b", encs)
    raws, _ = _raws_of("bytes", encs)
    plain = [f[:3] for f in fields]
    data = _records(B, pitch, fields, raws, _GM._held("none"), lead=1)
    buf = acvm_amd.DeviceBuffer(data)
    new, ref = _pair("bytes", B)
    ref.import_device_records(buf.ptr + 1, pitch, plain)
    new.import_device_records_masked(buf.ptr + 1, pitch, plain)
    _assert_same_import_state(new, ref, "no masks")
    assert new.import_missing() == 0 and new.import_list_copies() == 1
    # the same table as the unmasked call's: neither order of the two uploads it again; a table with masks is another one
    new.import_device_records(buf.ptr + 1, pitch, plain)
    new.import_device_records_masked(buf.ptr + 1, pitch, [f[:3] + (None,) for f in fields])
    assert new.import_list_copies() == 1
    new.import_device_records_masked(buf.ptr + 1, pitch, fields)
    new.import_device_records_masked(buf.ptr + 1, pitch, fields)
    assert new.import_list_copies() == 2 and new.import_missing() == 0
    _assert_same_import_state(new, ref, "masks of all ones against no masks")
    assert new.solve() == 0 and ref.solve() == 0 and new.stats()["n_slow_instances"] == 0
    _GR._assert_same_state(_GR._whole_state(new), _GR._whole_state(ref), "solved")
    buf.free()
    for x in (new, ref):
        x.free()


# ---- 8. end to end against the oracle
def _case(name):
    """circuit b (black box inputs, bytes): shape a, narrow encodings, near masks; circuit c (Brillig inputs, field elements): shape c, far masks"""
    shape, encs = ("a", tuple(ENC_A)) if name == "b" else ("c", tuple(ENC_C))
    pitch, fields = _layout(shape, encs)
    return pitch, fields, _raws_of("circuit:" + name, encs)[0]


@pytest.mark.parametrize("name", ["b", "c"])
@pytest.mark.parametrize("pattern", ["random", "pos31"])
def test_black_box_and_brillig_inputs_against_the_oracle(name, pattern):
    pitch, fields, raws = _case(name)
    ids = _GM._circuit(name)[1]
    batch = acvm_amd.Batch(_GM._device_circuit(name), BMAX, ids)
    _import_records(batch, BMAX, pitch, fields, raws, _GM._held(pattern), lead=3)
    assert batch.import_missing() == _GM._n_missing(pattern)
    # the host form equals the device form
    host = acvm_amd.Batch(_GM._device_circuit(name), BMAX, ids)
    host.set_initial_witness_records_masked(_records(BMAX, pitch, fields, raws, _GM._held(pattern)), pitch, fields)
    _assert_same_import_state(host, batch, "host form against device form")
    batch.solve()
    _GM._assert_expected(batch, name, pattern, f"circuit {name} pattern {pattern}")
    first = _GR._whole_state(batch)
    batch.reset()  # solve, reset, solve: the reset keeps what the import said
    assert batch.import_missing() == _GM._n_missing(pattern)
    batch.solve()
    _GM._assert_expected(batch, name, pattern, f"circuit {name} pattern {pattern}, behind reset")
    _GR._assert_same_state(_GR._whole_state(batch), first, "solve behind reset")
    host.solve()
    _GR._assert_same_state(_GR._whole_state(host), first, "host form")
    with pytest.raises(ValueError):
        host.set_initial_witness_records_masked(b"\0" * (BMAX * pitch - 1), pitch, fields)
    for x in (batch, host):
        x.free()


def test_forced_slow_path():
    pitch, fields, raws = _case("c")
    batch = acvm_amd.Batch(_GM._device_circuit("c"), BMAX, _GM._circuit("c")[1])
    batch.set_force_slow_path(True)
    _import_records(batch, BMAX, pitch, fields, raws, _GM._held("random"))
    batch.solve()
    _GM._assert_expected(batch, "c", "random", "forced slow path")
    batch.free()


def test_reuse_slots_handle():
    """rows are not ids; what can be read back under slot reuse is the results, the digests and the kept witnesses"""
    ob = _GM._oracle()
    pitch, fields, raws = _case("b")
    ids, keep = _GM._circuit("b")[1], [38, 39, 70, 71]
    batch = acvm_amd.Batch(_GM._device_circuit("b"), BMAX, ids, reuse_slots=True, keep=keep)
    for pattern in ("random", "pos31"):
        _import_records(batch, BMAX, pitch, fields, raws, _GM._held(pattern), lead=1)
        batch.solve()
        res, asg, values = _GM._expected("b", pattern)
        assert [r.as_tuple() for r in batch.results()] == res, pattern
        dig = batch.digest()
        for j in range(0, BMAX, 7):
            assert bytes(dig[j]) == ob.witness_map_digest(asg[j], values[j]), (pattern, j)
        solved = [j for j in range(BMAX) if res[j][0] == 0]
        for j in solved[:3] + solved[-3:]:
            assert np.array_equal(batch.extract(keep + ids, first=j, n=1)[0], values[j][keep + ids]), (pattern, j)
    batch.free()


# ---- 9. the chain: A's record export, mask bytes and all, is B's masked record import
def test_chain_of_two_circuits_through_records():
    from acvm_amd.acir import Circuit, Expression as E
    ob = _GM._oracle()
    n = 130
    # A: w4 = w1 w2 + w3; assert w3 = 5 (fails for a third, behind w4); w5 = w4^2 + 7; w6 = w4 + w1. Every fifth instance lacks w2: nothing is solved.
    circ_a = Circuit(6, [E([(1, 1, 2)], [(1, 3), (P - 1, 4)], 0), E([], [(1, 3)], P - 5), E([(1, 4, 4)], [(P - 1, 5)], 7), E([], [(1, 4), (1, 1), (P - 1, 6)], 0)])
    ids_a = [1, 2, 3]
    rng = random.Random(0x3A5CF)
    rows = [[rng.randrange(P), rng.randrange(P), 5 if j % 3 else 6] for j in range(n)]
    held_a = np.ones((n, 3), dtype=np.uint8)
    held_a[::5, 1] = 0
    # B reads A's w4, w5, w6 and (as a byte: 5 or 6 fits) w3 as its w1 .. w4: w5 = 2 w1 + 1; w6 = w2 + w1; w7 = w3 w1; w8 = w4 + 1
    circ_b = Circuit(8, [E([], [(2, 1), (P - 1, 5)], 1), E([], [(1, 2), (1, 1), (P - 1, 6)], 0), E([(1, 3, 1)], [(P - 1, 7)], 0), E([], [(1, 4), (P - 1, 8)], 1)])
    ids_b, position_of = [1, 2, 3, 4], {4: 0, 5: 1, 6: 2, 3: 3}
    oa, obc = ob.Circuit(circ_a.to_bytes()), ob.Circuit(circ_b.to_bytes())
    want = []
    for j in range(n):
        a = ob.ACVM(oa, {ids_a[k]: rows[j][k] for k in range(3) if held_a[j, k]})
        a.solve()
        map_a = a.witness_map()
        b = ob.ACVM(obc, {ids_b[pos]: map_a[w] for w, pos in position_of.items() if w in map_a})
        b.solve()
        want.append((b.result().as_tuple(), b.witness_map()))
    # A's inputs arrive as masked records themselves
    enc_in = (BE32, LE32, U8)
    in_fields = [(0, BE32, 1, 0), (1, LE32, 34, 33), (2, U8, 67, None)]
    raws_in = [np.frombuffer(b"".join(rr.element(rows[j][k], enc_in[k]) for j in range(n)), dtype=np.uint8).reshape(n, -1) for k in range(3)]
    ga = acvm_amd.Batch(acvm_amd.Circuit(circ_a.to_bytes()), n, ids_a)
    ga.set_initial_witness_records_masked(_records(n, 69, in_fields, raws_in, held_a), 69, in_fields)
    assert ga.import_missing() == (n + 4) // 5
    ga.solve()
    # the export: {valid, w4: Montgomery}, {valid, w5: BE32}, w3 as a byte with its valid byte at the record's end, {valid, w6: LE32}; pitch 107
    pitch, out_fields = 107, [(4, MONT, 1, 0), (5, BE32, 34, 33), (3, U8, 66, 106), (6, LE32, 70, 69), (2, BE32, 71, None)]
    d_records = acvm_amd.DeviceBuffer(bytes([rr.PATTERN]) * (3 + n * pitch))
    ga.export_device_records(d_records.ptr + 3, pitch, out_fields[:4])
    in_b = acvm_amd.record_masked_fields_from_out(out_fields, position_of)
    assert in_b == [(0, MONT, 1, 0), (1, BE32, 34, 33), (3, U8, 66, 106), (2, LE32, 70, 69)]  # (w2 is none of B's: padding to the import)
    gb = acvm_amd.Batch(acvm_amd.Circuit(circ_b.to_bytes()), n, ids_b)
    gb.import_device_records_masked(d_records.ptr + 3, pitch, in_b)
    gb.solve()
    res = [r.as_tuple() for r in gb.results()]
    asg, vals = gb.witness_map()
    for j in range(n):
        assert res[j] == want[j][0], (j, res[j], want[j][0])
        assert {w for w in range(asg.shape[1]) if asg[j, w]} == set(want[j][1]), j
        for w, v in want[j][1].items():
            assert bytes(vals[j, w]) == v.to_bytes(32, "big"), (j, w)
    assert any(r[0] != 0 for r in res) and any(r[0] == 0 for r in res)
    assert gb.import_missing() == sum(1 for j in range(n) if j % 3 == 0 or j % 5 == 0)
    for x in (d_records, ga, gb):
        x.free()
