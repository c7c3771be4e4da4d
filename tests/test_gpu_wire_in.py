"""acvm_batch_import_device_wire / acvm_batch_set_initial_witness_maps_wire on the device: the batch-wide WitnessMap wire format read as
per-instance, possibly partial, initial witness maps.

The yardstick for STATE is acvm_batch_import_device_masked on a second handle, fed the same values (as BE32 columns, unreduced) and the same
presence (as a column mask): rows, byte planes, event words, missing-set words (acvm_debug_import_state) and acvm_debug_import_missing are
compared bit for bit. The yardstick for OUTCOMES is the CPU oracle. Rows come from tests/wire_ref.py and tests/wire_in_cases.py (pinned on
the CPU by tests/test_wire_in_cases.py); what the device must find in a slot is wire_in_cases.findings."""
import functools
import gzip
import importlib.util
import os
import random
import re
import struct

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import P, Circuit, Expression as E
import wire_in_cases as wc
import wire_ref
from wire_ref import BINCODE, GZIP_STORED

pytestmark = pytest.mark.gpu
CONTAINERS = (BINCODE, GZIP_STORED)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE32, IM = acvm_amd.ENC_BE32, acvm_amd.LAYOUT_INSTANCE_MAJOR
CASES = ("lower", "upper", "mixed")


def _load(name):
    spec = importlib.util.spec_from_file_location("_%s_for_wire_in" % name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GR = _load("test_gpu_records")
_GM = _load("test_gpu_import_masked")
EDGE = _GR.EDGE
_readback_circuit = _GR._readback_circuit
WINDOW = int(re.search(r"WIRE_PLAN_WINDOW = (\d+)", open(os.path.join(ROOT, "acvm_amd", "csrc", "wire_plan.hpp")).read()).group(1))


# ---- values and presence
def _values(B, n_in, rot=0):
    """cell (instance j, position k): the 256-bit edge strings as they are (>= p and all ones among them, 0, p - 1); position 1 holds bytes in
    every instance, so that whole waves take the closed form of the row"""
    assert 0 in EDGE and P - 1 in EDGE and (1 << 256) - 1 in EDGE and any(P <= v for v in EDGE)
    return [[(7 * j + rot) % 256 if k == 1 else EDGE[(j + k + rot) % len(EDGE)] for k in range(n_in)] for j in range(B)]


def _held(pattern, B, n_in):
    h = np.ones((B, n_in), dtype=np.uint8)
    if pattern == "none":                 # N = 0 everywhere
        h[:] = 0
    elif pattern == "random":
        h = (np.random.default_rng(0x31BE5000 + B + n_in).random((B, n_in)) >= 0.3).astype(np.uint8)
    elif pattern.startswith("only"):      # one position and nothing else: 31 and 32 are either side of a missing-set word boundary
        h[:] = 0
        h[:, min(int(pattern[4:]), n_in - 1)] = 1
    elif pattern == "last-lane":          # the last lane of a partial wave differs from the rest, both ways
        h[B - 1, :] = 0
        h[B - 1, n_in - 1] = 1
        if B > 1:
            h[B - 2, 0] = 0
    else:
        assert pattern == "all"
    return h


PATTERNS = ["all", "none", "random", "only31", "only32", "last-lane"]


def _import_columns(ref, vals, held):
    """the yardstick: BE32 columns, unreduced, and mask bytes; 0xA5 under the absent elements"""
    B, n_in = held.shape
    v = np.full((B, n_in, 32), 0xA5, dtype=np.uint8)
    for j in range(B):
        for k in range(n_in):
            if held[j, k]:
                v[j, k] = np.frombuffer(vals[j][k].to_bytes(32, "big"), dtype=np.uint8)
    dv, dm = acvm_amd.DeviceBuffer(v.tobytes()), acvm_amd.DeviceBuffer(held.tobytes())
    try:
        ref.import_device_masked(dv.ptr, dm.ptr, BE32, IM)
    finally:
        dv.free()
        dm.free()


def _rows(ids, vals, held, container):
    """instance j's row: the witnesses it holds, its letter case by j"""
    return [wc.good_row({ids[k]: vals[j][k] for k in range(len(ids)) if held[j, k]}, container, CASES[j % 3], seed=j) for j in range(held.shape[0])]


def _import_wire(batch, rows, container, pitch, lengths=True, rng=None, exact=False, wrong_lengths=None):
    """the rows at the pitch in a device buffer of 0xA5 (or random bytes); exact: the buffer ends with the last row's last byte"""
    data = wc.slots(rows, pitch, rng=rng)
    if exact:
        data = data[:(len(rows) - 1) * pitch + len(rows[-1])]
    words = [len(r) for r in rows]
    for j, n in (wrong_lengths or {}).items():
        words[j] = n
    buf, d_len = acvm_amd.DeviceBuffer(data), acvm_amd.DeviceBuffer(np.array(words, dtype=np.uint64).tobytes())
    try:
        batch.import_device_wire(buf.ptr, container, pitch, d_len.ptr if lengths else None)
    finally:
        buf.free()
        d_len.free()


def _assert_same_import_state(got, want, what):
    sg, sw = got.import_state(), want if isinstance(want, dict) else want.import_state()
    for key in ("missing", "events", "planes", "rows"):
        bad = np.argwhere(sg[key] != sw[key])
        assert bad.size == 0, f"{what}: {key}{tuple(bad[0])} is {sg[key][tuple(bad[0])]:#x}, the column import's {sw[key][tuple(bad[0])]:#x} ({len(bad)} words differ)"
    return sg


@functools.lru_cache(maxsize=None)
def _reference(n_in, B, pattern, rot=0):
    """(state, missing count) the masked column import leaves: once per shape and pattern, read only"""
    ref = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    _import_columns(ref, _values(B, n_in, rot), _held(pattern, B, n_in))
    out = ref.import_state(), ref.import_missing()
    ref.free()
    return out


# ---- 1. the state is the masked column import's
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("n_in", [3, WINDOW + 1, 40])
@pytest.mark.parametrize("container", CONTAINERS)
def test_state_equals_the_masked_column_import(container, n_in, B):
    ids = list(range(1, n_in + 1))
    new = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    vals, bound = _values(B, n_in), wire_ref.bound(container, n_in)
    forms = [(bound, True), (bound + 48, False), (bound, False), (bound + 48, True)]
    for q, pattern in enumerate(PATTERNS):
        held = _held(pattern, B, n_in)
        rows = _rows(ids, vals, held, container)
        state, missing = _reference(n_in, B, pattern)
        for pitch, lengths in (forms if pattern == "random" else [forms[q % 4]]):
            what = f"container {container} n_in={n_in} B={B} pattern {pattern} pitch {pitch} lengths {lengths}"
            _import_wire(new, rows, container, pitch, lengths)
            _assert_same_import_state(new, state, what)
            assert new.import_missing() == missing == int((held == 0).any(axis=1).sum()), what
    # every input held: nobody is flagged, the solve reads back every value reduced
    _import_wire(new, _rows(ids, vals, _held("all", B, n_in), container), container, bound)
    assert new.solve() == 0 and new.stats()["n_slow_instances"] == 0
    _GR._assert_read_back(new, [[v % P for v in r] for r in vals], "solved behind the wire import")
    new.free()


# ---- 2. the block joint
@pytest.mark.parametrize("B", [3, 65])
def test_a_body_across_the_block_joint(B):
    """870 entries are 66 128 body bytes: two stored blocks, entry 862 spans body bytes 65 520 .. 65 595 across the joint at 65 532"""
    n_in = 870
    assert wire_ref.n_blocks(8 + 76 * n_in) == 2 and 8 + 76 * 862 == 65520
    ids = list(range(1, n_in + 1))
    vals = _values(B, n_in)
    new, ref = (acvm_amd.Batch(_readback_circuit(n_in), B, ids) for _ in range(2))
    pitch = wire_ref.bound(GZIP_STORED, n_in)
    for pattern in ("all", "some-862"):
        held = np.ones((B, n_in), dtype=np.uint8)
        if pattern == "some-862":  # one block, 65 520 bytes, in every other row
            held[::2, 862:] = 0
        rows = _rows(ids, vals, held, GZIP_STORED)
        assert {len(r) for r in rows} == {wire_ref.length(GZIP_STORED, n) for n in ((870,) if pattern == "all" else (862, 870)[:B])}
        _import_wire(new, rows, GZIP_STORED, pitch, lengths=pattern == "all")
        _import_columns(ref, vals, held)
        _assert_same_import_state(new, ref, f"B={B} {pattern}")
        assert new.import_missing() == int((held == 0).any(axis=1).sum())
        if pattern == "all":
            assert new.solve() == 0
            _GR._assert_read_back(new, [[v % P for v in r] for r in vals], "across the joint")
    for x in (new, ref):
        x.free()


# ---- 3. round trip with the export
@pytest.mark.parametrize("container", CONTAINERS)
def test_the_exports_buffer_is_the_imports_input(container):
    ob = _GM._oracle()
    n = 130
    # A: w5 = 3 w1 + 1; w6 = 3 w2 + 1; assert w3 = w4 (fails for every third instance, in mid-circuit); w7 = 3 w3 + 1; w8 = 3 w4 + 1
    circ_a = Circuit(8, [E([], [(3, 1), (P - 1, 5)], 1), E([], [(3, 2), (P - 1, 6)], 1), E([], [(1, 3), (P - 1, 4)], 0), E([], [(3, 3), (P - 1, 7)], 1),
                         E([], [(3, 4), (P - 1, 8)], 1)])
    # B reads A's w5 .. w8 under the same numbers: w8 = w6 + 2 (an assert where w8 is held, the gate that solves it where not); w9 = 3 w5 + 1;
    # w10 = 3 w7 + 1 (MissingAssignment where A never reached w7)
    circ_b = Circuit(10, [E([], [(1, 6), (P - 1, 8)], 2), E([], [(3, 5), (P - 1, 9)], 1), E([], [(3, 7), (P - 1, 10)], 1)])
    ids_b = [5, 6, 7, 8]
    rng = random.Random(0x31BE5003)
    rows_a = []
    for j in range(n):
        x = rng.randrange(P)
        rows_a.append([rng.randrange(P), x, (3 * x + 2) * pow(3, -1, P) % P, 0])  # 3 w4 + 1 = (3 w2 + 1) + 2
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
    d_bytes, d_len = acvm_amd.DeviceBuffer(bytes([wire_ref.FILL]) * (n * pitch)), acvm_amd.DeviceBuffer(bytes(8 * n))
    ga.witness_maps_wire_device(d_bytes.ptr, container, ids_b, n=n, pitch=pitch, d_lengths=d_len.ptr)
    gb = acvm_amd.Batch(acvm_amd.Circuit(circ_b.to_bytes()), n, ids_b)
    gb.import_device_wire(d_bytes.ptr, container, pitch, d_len.ptr)  # the same device buffer and lengths column, no pass in between
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
    assert all(8 in want[j][1] and 10 not in want[j][1] for j in range(0, n, 3))  # w8 solved from its gate, w10 never
    for x in (d_bytes, d_len, ga, gb):
        x.free()


# ---- 4. garbage is not read
@pytest.mark.parametrize("container", CONTAINERS)
def test_nothing_behind_a_rows_length_is_read(container):
    B, n_in = 130, WINDOW + 1
    ids = list(range(1, n_in + 1))
    vals, held = _values(B, n_in), _held("random", B, n_in).copy()
    held[B - 1, 3:] = 0  # a short last slot
    rows = _rows(ids, vals, held, container)
    new, ref = (acvm_amd.Batch(_readback_circuit(n_in), B, ids) for _ in range(2))
    _import_columns(ref, vals, held)
    want = ref.import_state()
    pitch = wire_ref.bound(container, n_in) + 48
    states = []
    for what, kw in (("0xA5", {}), ("random", dict(rng=random.Random(0x31BE5004))), ("nothing behind the last row", dict(exact=True)),
                     ("random, no lengths", dict(rng=random.Random(0x31BE5005), lengths=False))):
        _import_wire(new, rows, container, pitch, **kw)
        states.append(_assert_same_import_state(new, want, what))
        assert new.import_missing() == ref.import_missing()
    for x in (new, ref):
        x.free()


# ---- 5. every finding class, fail closed
def _expected_findings(rows, container, ids, pitch, lengths=None):
    per_row = [wc.findings(wc.slots([r], pitch), container, ids, None if lengths is None else lengths[j]) for j, r in enumerate(rows)]
    first = min((j, cls, rank) for j, f in enumerate(per_row) for cls, rank in f)
    return sum(len(f) for f in per_row), first


@pytest.mark.parametrize("container", CONTAINERS)
def test_every_finding_class_fails_closed(container):
    B, n_in = 130, 12
    assert n_in > WINDOW
    ids = list(range(1, n_in + 1))
    vals = [[(0x1234567890 << (8 * k)) + 1000 * j + k for k in range(n_in)] for j in range(B)]
    held = _held("random", B, n_in).copy()
    held[[0, 64, 101], :] = 1
    good = _rows(ids, vals, held, container)
    new, ref = (acvm_amd.Batch(_readback_circuit(n_in), B, ids) for _ in range(2))
    _import_columns(ref, vals, held)
    want = ref.import_state()
    pitch = wire_ref.bound(container, n_in)
    bad = wc.bad_rows(ids, vals[0], container, WINDOW)
    assert {b.cls for b in bad} == set(range(1, 8 if container == GZIP_STORED else 6))
    _import_wire(new, good, container, pitch)  # a good import first: the refusals below take it away
    for q, b in enumerate(bad):
        other = next(o for o in bad[q + 1:] + bad[:q] if o.cls != b.cls)
        for at in (0, 64):
            rows = list(good)
            rows[at], rows[101] = b.row, other.row
            count, (j, cls, rank) = _expected_findings(rows, container, ids, pitch)
            assert (j, cls, rank) == (at, b.cls, b.rank) and count == 2, b
            with pytest.raises(acvm_amd.AcvmError, match=rf"error -1: .*\b2 findings, the first of them instance {at}, class {b.cls} \(.*\), entry {b.rank}; .*without initial witnesses"):
                _import_wire(new, rows, container, pitch, lengths=False, rng=random.Random(q))
            with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
                new.solve()
        _import_wire(new, good, container, pitch)  # a following good import works and leaves no bit of the bad one
        _assert_same_import_state(new, want, f"behind {b}")
        assert new.import_missing() == ref.import_missing()
    # a length that is not the map's is a count finding, alone in its row
    with pytest.raises(acvm_amd.AcvmError, match=r"error -1: .*\b2 findings, the first of them instance 64, class 1 \(.*\), entry 0; "):
        _import_wire(new, good, container, pitch, wrong_lengths={64: len(good[64]) + 4, 129: 0})
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        new.solve()
    _import_wire(new, good, container, pitch)
    _assert_same_import_state(new, want, "behind the wrong lengths")
    new.solve()
    ref.solve()
    assert [r.as_tuple() for r in new.results()] == [r.as_tuple() for r in ref.results()]
    for x in (new, ref):
        x.free()


# ---- 6. host refusals
def test_host_refusals_leave_the_previous_import_in_place():
    B, n_in = 65, 5
    ids = list(range(1, n_in + 1))
    vals, held = _values(B, n_in), _held("random", B, n_in)
    new = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    pitch = wire_ref.bound(GZIP_STORED, n_in)
    _import_wire(new, _rows(ids, vals, held, GZIP_STORED), GZIP_STORED, pitch)
    before, missing = new.import_state(), new.import_missing()
    ptr = 1 << 20  # (never read: every call below is refused by the host checks)
    for kw, message in ((dict(container=2, pitch=pitch), "unknown container 2"), (dict(container=GZIP_STORED, pitch=8), "pitch 8 is not a multiple of 16"),
                        (dict(container=GZIP_STORED, pitch=0), "pitch 0"), (dict(container=BINCODE, pitch=pitch, d_ptr=ptr + 8), "not aligned to 16 bytes"),
                        (dict(container=BINCODE, pitch=pitch, d_ptr=None), "null buffer")):
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            new.import_device_wire(kw.pop("d_ptr", ptr), **kw)
    L = acvm_amd.lib()
    assert L.acvm_batch_import_device_wire(new._h, None, ptr, None) == -1 and b"null argument" in L.acvm_last_error()
    after = new.import_state()
    for key in before:
        assert np.array_equal(before[key], after[key])
    assert new.import_missing() == missing
    new.solve()  # the handle still has its initial witnesses
    new.free()


# ---- 7. the host form
def _loose_body(entries):
    """entries: (key, characters) in the order given, any length"""
    return struct.pack("<Q", len(entries)) + b"".join(struct.pack("<IQ", w, len(s)) + s for w, s in entries)


def test_host_form_reads_what_the_reference_reads():
    B, n_in = 67, 12
    ids = list(range(1, n_in + 1))
    rng = random.Random(0x31BE5007)
    vals, held = _values(B, n_in), _held("random", B, n_in)
    maps = [{ids[k]: vals[j][k] for k in range(n_in) if held[j, k]} for j in range(B)]
    hexs = lambda v: b"%064x" % v
    short = lambda v: (b"%x" % v).rjust(2 * ((len(b"%x" % v) + 1) // 2), b"0")
    rows = []
    for j, m in enumerate(maps):
        canonical = wire_ref.body(m)
        keys = sorted(m)
        shuffled = rng.sample(keys, len(keys))
        rows.append([
            acvm_amd.compress_witness({w: v % P for w, v in m.items()}),             # real deflate, what compressWitness writes
            gzip.compress(canonical),                                                   # any gzip stream
            canonical,                                                                  # the raw body
            wire_ref.member(canonical),                                                 # the export's own member
            _loose_body([(w, hexs(m[w])) for w in shuffled]),                           # unordered keys
            _loose_body([(w, hexs(0x77)) for w in keys[:1]] + [(w, hexs(m[w])) for w in shuffled]),  # a repeated key: the last one wins
            gzip.compress(_loose_body([(w, b"0x" + hexs(m[w])) for w in keys])),        # prefixed strings
            _loose_body([(w, short(m[w])) for w in keys]),                              # strings of another even length
            wc.good_row(m, BINCODE, "upper"),
        ][j % 9])
    got = [acvm_amd.decompress_witness(r) for r in rows]
    assert got == [wc.decoded(m) for m in maps]  # every spelling means the map
    new, ref = (acvm_amd.Batch(_readback_circuit(n_in), B, ids) for _ in range(2))
    new.set_initial_witness_maps_wire(rows)
    held_got = np.array([[ids[k] in g for k in range(n_in)] for g in got], dtype=np.uint8)
    _import_columns(ref, [[g.get(ids[k], 0) for k in range(n_in)] for g in got], held_got)
    state = _assert_same_import_state(new, ref, "host form")
    assert new.import_missing() == ref.import_missing() == int((held == 0).any(axis=1).sum())
    # refusals name the instance and leave the handle as it was
    corrupt = bytearray(rows[9])
    corrupt[len(corrupt) // 2] ^= 0x10
    assert rows[9][:2] == b"\x1f\x8b"
    for at, row, message in ((9, bytes(corrupt), "instance 9: gzip stream is corrupt"), (20, rows[2] + b"\x00", "instance 20: trailing bytes after the witness map"),
                             (66, wire_ref.body({1: 5, n_in + 1: 6}), f"instance 66: witness {n_in + 1} is not an initial witness of this handle"),
                             (3, _loose_body([(1, b"zz")]), "instance 3: bad field element hex")):
        spoiled = list(rows)
        spoiled[at] = row
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            new.set_initial_witness_maps_wire(spoiled)
        after = new.import_state()
        for key in state:
            assert np.array_equal(state[key], after[key]), (message, key)
    with pytest.raises(ValueError):
        new.set_initial_witness_maps_wire(rows[:-1])
    new.solve()
    ref.solve()
    assert [r.as_tuple() for r in new.results()] == [r.as_tuple() for r in ref.results()]
    for x in (new, ref):
        x.free()


# ---- 8. behind it: the solve, against the oracle
def _import_circuit(batch, name, pattern, container=GZIP_STORED):
    """the masked import suite's circuit, values and absence pattern as wire rows"""
    _, ids, vals = _GM._circuit(name)
    held = _GM._held(pattern)
    rows = _rows(ids, vals, held, container)
    _import_wire(batch, rows, container, wire_ref.bound(container, len(ids)), lengths=container == BINCODE, rng=random.Random(7))
    assert batch.import_missing() == _GM._n_missing(pattern)


@pytest.mark.parametrize("name", ["b", "c"])
def test_black_box_and_brillig_inputs_against_the_oracle(name):
    batch = acvm_amd.Batch(_GM._device_circuit(name), _GM.B, _GM._circuit(name)[1])
    _import_circuit(batch, name, "random", BINCODE if name == "b" else GZIP_STORED)
    batch.solve()
    _GM._assert_expected(batch, name, "random", f"circuit {name}")
    first = _GR._whole_state(batch)
    batch.reset()  # solve, reset, solve: the reset keeps what the import said
    assert batch.import_missing() == _GM._n_missing("random")
    batch.solve()
    _GR._assert_same_state(_GR._whole_state(batch), first, "solve behind reset")
    batch.free()


def test_forced_slow_path():
    batch = acvm_amd.Batch(_GM._device_circuit("c"), _GM.B, _GM._circuit("c")[1])
    batch.set_force_slow_path(True)
    _import_circuit(batch, "c", "random")
    batch.solve()
    _GM._assert_expected(batch, "c", "random", "forced slow path")
    batch.free()


def test_reuse_slots_handle():
    """rows are not ids; what can be read back under slot reuse is the results, the digests and the kept witnesses"""
    ob = _GM._oracle()
    ids, keep = _GM._circuit("b")[1], [38, 39, 70, 71]
    batch = acvm_amd.Batch(_GM._device_circuit("b"), _GM.B, ids, reuse_slots=True, keep=keep)
    for pattern in ("random", "pos31"):
        _import_circuit(batch, "b", pattern)
        batch.solve()
        res, asg, values = _GM._expected("b", pattern)
        assert [r.as_tuple() for r in batch.results()] == res, pattern
        dig = batch.digest()
        for j in range(0, _GM.B, 7):
            assert bytes(dig[j]) == ob.witness_map_digest(asg[j], values[j]), (pattern, j)
    batch.free()


def test_no_bit_of_an_earlier_import_survives():
    name = "b"
    ids, vals = _GM._circuit(name)[1:]
    new, ref = (acvm_amd.Batch(_GM._device_circuit(name), _GM.B, ids) for _ in range(2))
    _import_circuit(new, name, "everyone")
    assert new.import_state()["missing"].any(axis=0).all()
    new.solve()
    _GM._assert_expected(new, name, "everyone", "everyone")
    _import_circuit(new, name, "none")  # import, solve, import again with other presence
    assert not new.import_state()["missing"].any()
    assert new.solve() == 0 and new.stats()["n_slow_instances"] == 0  # nobody was flagged: no flag pass, no exact lane
    _import_circuit(new, name, "everyone")
    _import_circuit(new, name, "pos36", BINCODE)
    _import_columns(ref, vals, _GM._held("pos36"))
    _assert_same_import_state(new, ref, "pos36 behind everyone")
    new.solve()
    _GM._assert_expected(new, name, "pos36", "pos36 behind everyone")
    for x in (new, ref):
        x.free()
