"""acvm_batch_import_device_wire_gzip / acvm_batch_set_initial_witness_maps_gzip / acvm_debug_inflate_rows on the device: gzip members
inflated one row per lane, then read as initial witness maps.

The yardstick for the INFLATER is tests/wire_inflate_ref.py (pinned against zlib on the CPU by tests/test_wire_inflate_cases.py) over the rows
of tests/wire_inflate_cases.py. The yardstick for STATE is acvm_batch_import_device_wire(BINCODE) on a second handle, fed the inflated bodies:
rows, byte planes, event words and missing-set words (acvm_debug_import_state) are compared bit for bit. The yardstick for OUTCOMES is the CPU
oracle."""
import ctypes as C
import functools
import importlib.util
import os
import random

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import P, Circuit, Expression as E
import wire_in_cases as wc
import wire_inflate_cases as cases
import wire_inflate_ref as ref
import wire_ref
from wire_ref import BINCODE, GZIP_STORED

pytestmark = pytest.mark.gpu
FILL = 0xA5
GZIP_DEFLATE = acvm_amd.WIRE_GZIP_DEFLATE


def _load(name):
    spec = importlib.util.spec_from_file_location("_%s_for_wire_inflate" % name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_WI = _load("test_gpu_wire_in")
_GR, _GM = _WI._GR, _WI._GM
_readback_circuit, _values, _held, _rows, _assert_same_import_state = _WI._readback_circuit, _WI._values, _WI._held, _WI._rows, _WI._assert_same_import_state


def _round16(n):
    return (n + 15) // 16 * 16


def _writer(j):
    """how row j's body is compressed: every writer of list A in turn, the project's own stored member and a head with every optional field"""
    kinds = [lambda b, kw=kw: cases.deflated(b, **kw) for _, kw in cases.WRITERS] + [wire_ref.member, lambda b: cases.member(cases.deflated(b, wbits=-15), b, head=cases.head_of(
        fextra=b"xy", fname=b"w", fcomment=b"c", fhcrc=True))]
    return kinds[j % len(kinds)]


def _members(bodies):
    return [_writer(j)(b) for j, b in enumerate(bodies)]


# ---- 1. the inflater alone, on bytes that need not be witness maps
def _assert_inflated(rows, cap, what, **kw):
    out, lengths, findings, crcs = acvm_amd.debug_inflate_rows(rows, cap, fill=FILL, **kw)
    for i, row in enumerate(rows):
        m = cases.judged(row, cap)
        n = int(lengths[i])
        assert (int(findings[i, 0]), int(findings[i, 1]), n, int(crcs[i])) == (m.cls, m.block, len(m.out), m.crc), (what, i, row[:16].hex(), m.cause)
        assert bytes(out[i, :n]) == m.out, (what, i)
        assert (out[i, n:] == FILL).all(), (what, i, "bytes at or behind the row's length were written")
    return findings


def test_every_case_row_against_the_model():
    everything = cases.everything()
    for cap in sorted({c.cap for c in everything if c.cap is not None}):
        _assert_inflated([c.row for c in everything if c.cap == cap], cap, f"cap {cap}")
    plain = [c.row for c in everything if c.cap is None]
    findings = _assert_inflated(plain, cases.CAP, "the lists at the common cap")
    assert set(findings[:, 0].tolist()) == set(range(0, 11)) - {ref.OUTPUT}
    # the small accepted rows with a cap of exactly their output and of four bytes less
    small = [c.row for c in cases.list_a() + cases.list_b() if 4 <= len(cases.judged(c.row, cases.CAP).out) <= 464]
    for n in sorted({len(cases.judged(r, cases.CAP).out) for r in small}):
        rows = [r for r in small if len(cases.judged(r, cases.CAP).out) == n]
        if n % 4 == 0:
            assert not _assert_inflated(rows, n, f"cap = the output {n}")[:, 0].any()
            assert (_assert_inflated(rows, n - 4, f"cap = the output {n} - 4")[:, 0] == ref.OUTPUT).all()


@functools.lru_cache(maxsize=None)
def _pools():
    good, bad = [], []
    for c in cases.everything():
        if c.cap is None and len(c.row) <= 400:
            m = cases.judged(c.row, 3072)
            (bad if m.cls else good).append((c.row, m))
    return good, bad


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_batch_sizes_and_where_the_failing_rows_stand(B):
    """stored, fixed, dynamic and failing rows interleaved in one wave; a failing row in the first, a middle and the last lane of a wave and in
    the partial last wave; every class of finding somewhere"""
    good, bad = _pools()
    kinds = {k: [r for r, m in good if k in m.labels and len(m.labels & {"block.stored", "block.fixed", "block.dynamic"}) == 1] for k in ("block.stored", "block.fixed", "block.dynamic")}
    assert all(len(v) >= 3 for v in kinds.values())
    rng = random.Random(0x1F8B6000 + B)
    for failing in ([], [0], [B // 2], [B - 1], sorted({0, 31 % B, 63 % B, B - 1})):
        rows = [rng.choice(kinds[("block.stored", "block.fixed", "block.dynamic")[i % 3]]) for i in range(B)]
        for q, at in enumerate(failing):
            rows[at] = bad[(7 * B + 13 * q + at) % len(bad)][0]
        findings = _assert_inflated(rows, 3072, f"B={B} failing at {failing}")
        assert sorted(np.nonzero(findings[:, 0])[0].tolist()) == failing
    # lengths NULL: the bound is the pitch, and what lies behind a member is nobody's
    rows = [rng.choice(good)[0] for _ in range(B)]
    pitch = _round16(max(len(r) for r in rows)) + 16
    flat = wc.slots(rows, pitch, rng=random.Random(B))
    out, lengths, findings, crcs = acvm_amd.debug_inflate_rows(flat, 3072, fill=FILL, pitch=pitch)
    for i, r in enumerate(rows):
        m = cases.judged(r, 3072)
        assert (int(findings[i, 0]), int(lengths[i]), int(crcs[i]), bytes(out[i, :len(m.out)])) == (0, len(m.out), m.crc, m.out), i


# ---- 2. the import is the BINCODE import of the inflated bodies
def _import_gzip(batch, members, pitch=None, lengths=True, rng=None, fill=FILL):
    pitch = pitch or _round16(max(len(m) for m in members))
    data = wc.slots(members, pitch, fill=fill, rng=rng)
    buf, d_len = acvm_amd.DeviceBuffer(data), acvm_amd.DeviceBuffer(np.array([len(m) for m in members], dtype=np.uint64).tobytes())
    try:
        batch.import_device_wire_gzip(buf.ptr, pitch, d_len.ptr if lengths else None)
    finally:
        buf.free()
        d_len.free()


def _import_bodies(batch, bodies, n_in):
    _WI._import_wire(batch, bodies, BINCODE, wire_ref.bound(BINCODE, n_in))


@pytest.mark.parametrize("B", [1, 64, 65, 130])
@pytest.mark.parametrize("n_in", [3, 40])
def test_state_equals_the_bincode_import(n_in, B):
    """full and partial maps, values at or above p, either letter case; d_lengths given and NULL; pitches of the longest member and beyond"""
    ids = list(range(1, n_in + 1))
    new, old = (acvm_amd.Batch(_readback_circuit(n_in), B, ids) for _ in range(2))
    vals = _values(B, n_in)
    for q, pattern in enumerate(("all", "random", "none", "last-lane")):
        bodies = _rows(ids, vals, _held(pattern, B, n_in), BINCODE)
        members = _members(bodies)
        _import_bodies(old, bodies, n_in)
        for lengths, extra in ((True, 0), (False, 48)) if pattern == "random" else [((True, 0), (False, 48))[q % 2]]:
            what = f"n_in={n_in} B={B} pattern {pattern} lengths {lengths}"
            _import_gzip(new, members, _round16(max(len(m) for m in members)) + extra, lengths, rng=random.Random(q))
            _assert_same_import_state(new, old, what)
            assert new.import_missing() == old.import_missing(), what
    bodies = _rows(ids, vals, _held("all", B, n_in), BINCODE)
    _import_gzip(new, _members(bodies))
    assert new.solve() == 0 and new.stats()["n_slow_instances"] == 0
    _GR._assert_read_back(new, [[v % P for v in r] for r in vals], "solved behind the gzip import")
    for x in (new, old):
        x.free()


def test_a_handle_of_440_initial_witnesses():
    """33 448 bytes a body: matches more than 16 384 bytes back, many blocks (memLevel 1), the longest body exactly at the bound"""
    n_in, B = 440, 66
    ids = list(range(1, n_in + 1))
    new, old = (acvm_amd.Batch(_readback_circuit(n_in), B, ids) for _ in range(2))
    list_a = {c.name: c.row for c in cases.list_a() if c.name.startswith("A 440")}
    assert len(list_a) >= 12
    members = [list(list_a.values())[j % len(list_a)] for j in range(B)]
    bodies = [cases.judged(m, cases.CAP).out for m in members]
    assert all(len(b) == 8 + 76 * n_in for b in bodies)
    _import_bodies(old, bodies, n_in)
    _import_gzip(new, members, lengths=False)
    _assert_same_import_state(new, old, "440 initial witnesses")
    assert new.import_missing() == 0 and new.solve() == 0
    for x in (new, old):
        x.free()


def _compressed_rows(name, pattern):
    _, ids, vals = _GM._circuit(name)
    bodies = _rows(ids, vals, _GM._held(pattern), BINCODE)
    return ids, bodies, _members(bodies)


@pytest.mark.parametrize("name", ["b", "c"])
def test_black_box_and_brillig_inputs_against_the_oracle(name):
    """"b": byte-plane inputs"""
    ids, bodies, members = _compressed_rows(name, "random")
    batch, old = (acvm_amd.Batch(_GM._device_circuit(name), _GM.B, ids) for _ in range(2))
    _import_gzip(batch, members, lengths=name == "b", rng=random.Random(5))
    _import_bodies(old, bodies, len(ids))
    _assert_same_import_state(batch, old, f"circuit {name}")
    assert batch.import_missing() == _GM._n_missing("random")
    batch.solve()
    _GM._assert_expected(batch, name, "random", f"circuit {name}")
    for x in (batch, old):
        x.free()


def test_reuse_slots_handle():
    ob = _GM._oracle()
    keep = [38, 39, 70, 71]
    for pattern in ("random", "pos31"):
        ids, bodies, members = _compressed_rows("b", pattern)
        batch, old = (acvm_amd.Batch(_GM._device_circuit("b"), _GM.B, ids, reuse_slots=True, keep=keep) for _ in range(2))
        _import_gzip(batch, members)
        _import_bodies(old, bodies, len(ids))
        _assert_same_import_state(batch, old, f"reuse_slots {pattern}")
        batch.solve()
        res, asg, values = _GM._expected("b", pattern)
        assert [r.as_tuple() for r in batch.results()] == res, pattern
        dig = batch.digest()
        for j in range(0, _GM.B, 7):
            assert bytes(dig[j]) == ob.witness_map_digest(asg[j], values[j]), (pattern, j)
        for x in (batch, old):
            x.free()


# ---- 3. the round trips
@pytest.mark.parametrize("container", [GZIP_DEFLATE, GZIP_STORED])
def test_the_exports_buffer_is_the_imports_input(container):
    """circuit A's maps, written by the device in either gzip container, are circuit B's initial witnesses with nothing in between"""
    ob = _GM._oracle()
    n = 130
    circ_a = Circuit(8, [E([], [(3, 1), (P - 1, 5)], 1), E([], [(3, 2), (P - 1, 6)], 1), E([], [(1, 3), (P - 1, 4)], 0), E([], [(3, 3), (P - 1, 7)], 1),
                         E([], [(3, 4), (P - 1, 8)], 1)])
    circ_b = Circuit(10, [E([], [(1, 6), (P - 1, 8)], 2), E([], [(3, 5), (P - 1, 9)], 1), E([], [(3, 7), (P - 1, 10)], 1)])
    ids_b = [5, 6, 7, 8]
    rng = random.Random(0x1F8B6003)
    rows_a = []
    for j in range(n):
        x = rng.randrange(P)
        rows_a.append([rng.randrange(P), x, (3 * x + 2) * pow(3, -1, P) % P, 0])
        rows_a[-1][3] = rows_a[-1][2] if j % 3 else (rows_a[-1][2] + 1) % P
    oa, obc = ob.Circuit(circ_a.to_bytes()), ob.Circuit(circ_b.to_bytes())
    want = []
    for j in range(n):
        a = ob.ACVM(oa, dict(zip([1, 2, 3, 4], rows_a[j])))
        a.solve()
        map_a = a.witness_map()
        b = ob.ACVM(obc, {w: map_a[w] for w in ids_b if w in map_a})
        b.solve()
        want.append((b.result().as_tuple(), b.witness_map()))
    ga = acvm_amd.Batch(acvm_amd.Circuit(circ_a.to_bytes()), n, [1, 2, 3, 4])
    ga.set_initial_witness(synth.values_from_rows(rows_a))
    ga.solve()
    pitch = ga.wire_bound(container, ids_b)
    d_bytes, d_len = acvm_amd.DeviceBuffer(bytes([FILL]) * (n * pitch)), acvm_amd.DeviceBuffer(bytes(8 * n))
    ga.witness_maps_wire_device(d_bytes.ptr, container, ids_b, n=n, pitch=pitch, d_lengths=d_len.ptr)
    gb = acvm_amd.Batch(acvm_amd.Circuit(circ_b.to_bytes()), n, ids_b)
    gb.import_device_wire_gzip(d_bytes.ptr, pitch, d_len.ptr)  # the same device buffer and lengths column, no pass in between
    assert gb.import_missing() == len(range(0, n, 3))
    gb.solve()
    res = [r.as_tuple() for r in gb.results()]
    asg, vals = gb.witness_map()
    for j in range(n):
        assert res[j] == want[j][0], (j, res[j], want[j][0])
        assert {w for w in range(asg.shape[1]) if asg[j, w]} == set(want[j][1]), j
        for w, v in want[j][1].items():
            assert bytes(vals[j, w]) == v.to_bytes(32, "big"), (j, w)
    assert any(r[0] != 0 for r in res) and any(r[0] == 0 for r in res)
    for x in (d_bytes, d_len, ga, gb):
        x.free()


def test_the_references_own_member_in_65_slots():
    member, witness_map = cases.pinned()
    B, ids = 65, sorted(witness_map)
    batch = acvm_amd.Batch(_readback_circuit(len(ids)), B, ids)
    _import_gzip(batch, [member] * B, lengths=False, rng=random.Random(1))  # 106 bytes in slots of 112: random bytes behind the trailer
    assert batch.import_missing() == 0 and batch.solve() == 0
    _GR._assert_read_back(batch, [[witness_map[w] for w in ids]] * B, "expectedWitnessMap")
    batch.free()


# ---- 4. findings
def _state(batch):
    return batch.import_state(), batch.import_missing()


def _assert_state_is(batch, before, what):
    state, missing = _state(batch)
    for key in before[0]:
        assert np.array_equal(before[0][key], state[key]), (what, key)
    assert missing == before[1], what


def test_inflate_findings_leave_the_handle_as_it_was():
    B, n_in = 130, 12
    ids = list(range(1, n_in + 1))
    vals = [[(0x1234567890 << (8 * k)) + 1000 * j + k for k in range(n_in)] for j in range(B)]
    held = _held("random", B, n_in)
    good = _members(_rows(ids, vals, held, BINCODE))
    cap = 8 + 76 * n_in
    new = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    _import_gzip(new, good)
    before = _state(new)
    bad = {}
    for c in cases.list_c():  # one row per class, short enough for the slot; class 8 against this handle's own bound
        m = cases.judged(c.row, cap)
        if m.cls and len(c.row) <= 1100 and m.cls not in bad:
            bad[m.cls] = (c.row, m)
    row = cases.built(lambda w: cases.fixed(w, [97, ("m", 258, 1)] * 4, 1))  # 1 036 bytes: more than this handle's longest body
    bad[ref.OUTPUT] = (row, cases.judged(row, cap))
    assert set(bad) == set(range(1, 11)) and all(m.cls == cls for cls, (_, m) in bad.items())
    order = sorted(bad)
    for q, cls in enumerate(order):
        row, m = bad[cls]
        other_row, other = bad[order[(q + 3) % len(order)]]
        for first, second in ((0, 101), (64, 129), (129, 64)):  # the first of the two rows in either order of their places
            rows = list(good)
            rows[first], rows[second] = row, other_row
            lo, lo_m = (first, m) if first < second else (second, other)
            with pytest.raises(acvm_amd.AcvmError, match=rf"error -1: wire inflate: 2 findings, the first of them instance {lo}, class {lo_m.cls} \(.*\), block {lo_m.block}; the handle stays as it was"):
                _import_gzip(new, rows, 1104, lengths=True, rng=random.Random(q))
            _assert_state_is(new, before, f"behind class {cls}")
    new.solve()  # the previous import still solves
    ref_batch = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    _import_bodies(ref_batch, _rows(ids, vals, held, BINCODE), n_in)
    ref_batch.solve()
    assert [r.as_tuple() for r in new.results()] == [r.as_tuple() for r in ref_batch.results()]
    for x in (new, ref_batch):
        x.free()


def test_a_body_that_is_no_canonical_map_is_the_body_imports_finding():
    B, n_in, window = 130, 12, _WI.WINDOW
    ids = list(range(1, n_in + 1))
    vals = [[(0x1234567890 << (8 * k)) + 1000 * j + k for k in range(n_in)] for j in range(B)]
    held = _held("random", B, n_in).copy()
    held[[0, 64, 101], :] = 1
    good = _members(_rows(ids, vals, held, BINCODE))
    new = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    rows_d = cases.list_d(ids, vals[0], window)
    assert {b.cls for b, _ in rows_d} == {1, 2, 3, 4, 5}
    trailing = cases.deflated(wire_ref.body({1: 5}) + b"\x00")  # bytes behind the map: the inflater's length is the row's d_lengths
    for q, (b, row) in enumerate(rows_d):
        for at in (0, 64):
            rows = list(good)
            rows[at], rows[101] = row, trailing
            _import_gzip(new, good)
            with pytest.raises(acvm_amd.AcvmError, match=rf"error -1: wire import: 2 findings, the first of them instance {at}, class {b.cls} \(.*\), entry {b.rank}; .*without initial witnesses"):
                _import_gzip(new, rows, rng=random.Random(q))
            with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
                new.solve()
    rows = list(good)
    rows[129] = trailing
    with pytest.raises(acvm_amd.AcvmError, match=r"error -1: wire import: 1 findings, the first of them instance 129, class 1 \(.*\), entry 0; "):
        _import_gzip(new, rows)
    _import_gzip(new, good)  # a following good import works: partial maps, so some instances lack an input
    assert new.import_missing() == int((held == 0).any(axis=1).sum())
    new.solve()
    new.free()


# ---- 5. nothing outside a row's bound has any influence
def test_bytes_outside_a_rows_bound_influence_nothing():
    B, n_in = 130, 9
    ids = list(range(1, n_in + 1))
    vals, held = _values(B, n_in), _held("random", B, n_in)
    members = _members(_rows(ids, vals, held, BINCODE))
    new = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    pitch = _round16(max(len(m) for m in members)) + 32
    states = []
    for fill in (0x00, 0xFF):
        _import_gzip(new, members, pitch, lengths=True, fill=fill)
        states.append(_state(new))
    _assert_state_is(new, states[0], "two fills")
    # a failing batch: a row cut short by its length; the bytes behind the cut are the member's own in one run and other bytes in the next
    cut = dict((j, len(members[j]) - 9) for j in (3, 64, 129))
    messages = []
    for fill in (None, 0x00, 0xFF):
        data = bytearray(wc.slots(members, pitch, fill=fill or 0))
        if fill is not None:
            for j, n in cut.items():
                data[j * pitch + n:(j + 1) * pitch] = bytes([fill]) * (pitch - n)
        words = [cut.get(j, len(m)) for j, m in enumerate(members)]
        buf, d_len = acvm_amd.DeviceBuffer(bytes(data)), acvm_amd.DeviceBuffer(np.array(words, dtype=np.uint64).tobytes())
        with pytest.raises(acvm_amd.AcvmError, match="wire inflate: 3 findings, the first of them instance 3, class 7 ") as e:
            new.import_device_wire_gzip(buf.ptr, pitch, d_len.ptr)
        messages.append(str(e.value))
        buf.free()
        d_len.free()
        _assert_state_is(new, states[0], f"fill {fill}")
    assert len(set(messages)) == 1
    new.free()


# ---- 6. the host form
def test_host_form():
    B, n_in = 67, 12
    ids = list(range(1, n_in + 1))
    vals, held = _values(B, n_in), _held("random", B, n_in)
    bodies = _rows(ids, vals, held, BINCODE)
    members = _members(bodies)
    new, dev, old = (acvm_amd.Batch(_readback_circuit(n_in), B, ids) for _ in range(3))
    new.set_initial_witness_maps_gzip(members)
    _import_gzip(dev, members)
    _assert_same_import_state(new, dev, "the host form and the device form")
    old.set_initial_witness_maps_wire(members)  # the old host form stages canonical bodies as they are
    _assert_same_import_state(new, old, "the new host form and the old")
    assert new.import_missing() == dev.import_missing() == old.import_missing()
    before = _state(new)
    # refusals: nothing enqueued, the handle as it was
    for spoiled, message in (([bodies[0]] + members[1:], "instance 0: the row does not start 1f 8b"), (members[:5] + [b"\x1f"] + members[6:], "instance 5: the row does not start 1f 8b"),
                             (members[:-1] + [b""], f"instance {B - 1}: the row does not start 1f 8b")):
        with pytest.raises(acvm_amd.AcvmError, match="error -1: " + message):
            new.set_initial_witness_maps_gzip(spoiled)
        _assert_state_is(new, before, message)
    with pytest.raises(ValueError):
        new.set_initial_witness_maps_gzip(members[:-1])
    L = acvm_amd.lib()
    buf = bytes(64 * B)
    assert L.acvm_batch_set_initial_witness_maps_gzip(new._h, buf, 64, None) == -1 and b"null lengths" in L.acvm_last_error()
    assert L.acvm_batch_set_initial_witness_maps_gzip(new._h, None, 64, (C.c_uint64 * B)()) == -1 and b"null buffer" in L.acvm_last_error()
    _assert_state_is(new, before, "null arguments")
    # a finding of the inflater names its instance and leaves the handle as it was; a body out of canonical shape is the body import's finding
    corrupt = bytearray(members[9])
    corrupt[-6] ^= 0x10
    with pytest.raises(acvm_amd.AcvmError, match=r"wire inflate: 1 findings, the first of them instance 9, class 9 "):
        new.set_initial_witness_maps_gzip(members[:9] + [bytes(corrupt)] + members[10:])
    _assert_state_is(new, before, "a wrong CRC")
    loose = cases.deflated(wire_ref.body({2: 7, 1: 5})[:8] + wire_ref.body({2: 7})[8:] + wire_ref.body({1: 5})[8:])  # keys descending: the old form reorders them
    old.set_initial_witness_maps_wire(members[:9] + [loose] + members[10:])
    with pytest.raises(acvm_amd.AcvmError, match=r"wire import: 1 findings, the first of them instance 9, class 5 "):
        new.set_initial_witness_maps_gzip(members[:9] + [loose] + members[10:])
    new.set_initial_witness_maps_gzip(members)
    new.solve()
    dev.solve()
    assert [r.as_tuple() for r in new.results()] == [r.as_tuple() for r in dev.results()]
    for x in (new, dev, old):
        x.free()


# ---- 7. sequences on one handle against fresh ones; host refusals
def test_sequences_and_host_refusals():
    name = "b"
    ids, bodies, members = _compressed_rows(name, "everyone")
    one = acvm_amd.Batch(_GM._device_circuit(name), _GM.B, ids)
    _import_gzip(one, members)
    one.solve()
    _GM._assert_expected(one, name, "everyone", "gzip import, solve")
    first = _GR._whole_state(one)
    one.reset()
    one.solve()
    _GR._assert_same_state(_GR._whole_state(one), first, "solve behind reset")
    ids, bodies2, members2 = _compressed_rows(name, "pos36")
    _import_bodies(one, bodies2, len(ids))  # a BINCODE import behind it
    fresh = acvm_amd.Batch(_GM._device_circuit(name), _GM.B, ids)
    _import_bodies(fresh, bodies2, len(ids))
    _assert_same_import_state(one, fresh, "BINCODE behind gzip")
    one.solve()
    _GM._assert_expected(one, name, "pos36", "BINCODE import behind the gzip import")
    _import_gzip(one, members)  # and gzip again behind that
    fresh2 = acvm_amd.Batch(_GM._device_circuit(name), _GM.B, ids)
    _import_gzip(fresh2, members)
    _assert_same_import_state(one, fresh2, "gzip behind BINCODE")
    before = _state(one)
    ptr, pitch = 1 << 20, 1024  # (never read: every call below is refused by the host checks)
    L = acvm_amd.lib()
    for container, p, d_ptr, message in ((BINCODE, pitch, ptr, "container 0 is not ACVM_WIRE_GZIP_DEFLATE"), (GZIP_STORED, pitch, ptr, "container 1 is not"),
                                         (GZIP_DEFLATE, 0, ptr, "pitch 0"), (GZIP_DEFLATE, 24, ptr, "pitch 24 is not a multiple of 16"),
                                         (GZIP_DEFLATE, pitch, ptr + 8, "not aligned to 16 bytes"), (GZIP_DEFLATE, pitch, None, "null buffer")):
        desc = acvm_amd.WireInDesc(container=container, pitch=p)
        assert L.acvm_batch_import_device_wire_gzip(one._h, C.byref(desc), d_ptr, None) == -1 and message.encode() in L.acvm_last_error(), message
    assert L.acvm_batch_import_device_wire_gzip(one._h, None, ptr, None) == -1 and b"null argument" in L.acvm_last_error()
    # the old entry point still refuses the container (its message is its own)
    with pytest.raises(acvm_amd.AcvmError, match="unknown container 8"):
        one.import_device_wire(ptr, GZIP_DEFLATE, pitch)
    _assert_state_is(one, before, "host refusals")
    one.solve()
    _GM._assert_expected(one, name, "everyone", "behind the refusals")
    for x in (one, fresh, fresh2):
        x.free()
