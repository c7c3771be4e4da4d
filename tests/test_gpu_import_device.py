"""acvm_batch_import_device / acvm_batch_solve_then_import_ex on the device: the initial witnesses read from a caller's device buffer in every
encoding and layout of the device export, with strides and column lists, judged by Python integers through the read-back circuit of
tests/test_gpu_import.py (w[n_in + k] = 3 w[k] + 1: the initial witness read back checks the value, the gate output that the row really is
x * 2^261 mod p) and, where a real circuit runs, by the CPU oracle. Buffers are pre-filled with a pattern wherever no described element lies:
a value read from there shows in the result."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import Circuit, Expression as E, P

pytestmark = pytest.mark.gpu
BE32, LE32, MONT = acvm_amd.ENC_BE32, acvm_amd.ENC_LE32, acvm_amd.ENC_MONT256_LE
IM, WM = acvm_amd.LAYOUT_INSTANCE_MAJOR, acvm_amd.LAYOUT_WITNESS_MAJOR
ENCODINGS, LAYOUTS = (BE32, LE32, MONT), (IM, WM)
PATTERN = 0xA5
R256_INV = pow(1 << 256, -1, P)


def _gpu_import_module():
    spec = importlib.util.spec_from_file_location("_gpu_import_for_import_device", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_import.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GI = _gpu_import_module()
EDGE = _GI.EDGE                          # the 72 reduction-edge strings
_readback_circuit = _GI._readback_circuit


# ---- what the bytes mean, and how a buffer is laid out (Python integers and index arithmetic only)
def _string_bytes(s, encoding):
    """the 256-bit string s as the element's 32 bytes: s is the integer the decoder reads in that encoding"""
    return s.to_bytes(32, "big" if encoding == BE32 else "little")


def _string_value(s, encoding):
    """the field element those bytes mean"""
    return s * R256_INV % P if encoding == MONT else s % P


def _value_bytes(v, encoding):
    """32 bytes that mean v mod p in the encoding, as an exporter would write them (v itself may be an unreduced big-endian input)"""
    if encoding == BE32:
        return v.to_bytes(32, "big")
    if encoding == LE32:
        return v.to_bytes(32, "little")
    return ((v << 256) % P).to_bytes(32, "little")


def _buffer(elements, layout, stride=0):
    """elements[i][c]: the 32 bytes of (instance i, column c) -> the bytes of the whole buffer; everything else holds PATTERN"""
    n, n_columns = len(elements), len(elements[0])
    rows, dense = (n_columns, n) if layout == WM else (n, n_columns)
    stride = stride or dense
    assert stride >= dense
    buf = np.full((rows * stride, 32), PATTERN, dtype=np.uint8)
    view = buf.reshape(rows, stride, 32)
    arr = np.frombuffer(b"".join(e for row in elements for e in row), dtype=np.uint8).reshape(n, n_columns, 32)
    view[:, :dense] = arr.transpose(1, 0, 2) if layout == WM else arr
    return buf.tobytes()


def _be_rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for r in vals for v in r), dtype=np.uint8).reshape(len(vals), -1, 32)


def _assert_read_back(batch, vals, what="", initial=True):
    """vals[j][k]: the field element input k of instance j means. Every initial witness reads back as it, every gate output as 3 x + 1."""
    n_in = len(vals[0])
    assert all(r.status == acvm_amd.STATUS_SOLVED for r in batch.results()), what
    want_in, want_out = _be_rows(vals), _be_rows([[(3 * x + 1) % P for x in r] for r in vals])
    for k in range(n_in):
        for w, want, name in ((1 + k, want_in, "initial witness"), (1 + n_in + k, want_out, "gate output")):
            if name == "initial witness" and not initial:
                continue
            got, asg = batch.witness(w)
            assert asg.all(), (what, w)
            bad = np.nonzero((got != want[:, k]).any(axis=1))[0]
            assert bad.size == 0, (f"{what}: {name} {w} of instance {bad[0]} is {got[bad[0]].tobytes().hex()}, expected {want[bad[0], k].tobytes().hex()} "
                                   f"({bad.size} instances differ)")


def _edge_columns(B, n_columns, rot=0):
    return [[EDGE[(j + c + rot) % len(EDGE)] for c in range(n_columns)] for j in range(B)]


def _import_strings(batch, strings, encoding, layout, columns=None, stride=0):
    """strings[j][c]: the 256-bit string in column c of instance j. Imports them and returns the field elements the inputs then hold."""
    n_in = len(batch.ids)
    data = _buffer([[_string_bytes(s, encoding) for s in row] for row in strings], layout, stride)
    buf = acvm_amd.DeviceBuffer(data)
    try:
        batch.import_device(buf.ptr, encoding=encoding, layout=layout, columns=columns, n_columns=None if columns is None else len(strings[0]), stride=stride)
    finally:
        buf.free()  # (the call returns after the stream is synchronised: the buffer is the caller's again)
    cols = list(range(n_in)) if columns is None else columns
    return [[_string_value(row[c], encoding) for c in cols] for row in strings]


def _whole_state(batch):
    asg, vals = batch.witness_map()
    return [r.as_tuple() for r in batch.results()], asg, vals


def _assert_same_state(got, want, what=""):
    assert got[0] == want[0], what
    assert np.array_equal(got[1], want[1]), what
    bad = np.argwhere((got[2] != want[2]).any(axis=2))
    assert bad.size == 0, f"{what}: witness {bad[0][1]} of instance {bad[0][0]} differs ({len(bad)} differ)"


# ---- 1. every encoding x layout on the edge values
# one instance, below / on / above one block of 64 instances (and of the streaming kernel's 256: 130 < 256, the shapes of the issue), ragged last groups of four inputs
@pytest.mark.parametrize("n_in,B", [(1, 130), (3, 64), (4, 65), (5, 1), (9, 130), (5, 63)])
def test_every_encoding_and_layout_on_the_edge_values(n_in, B):
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    rot = 0
    for encoding in ENCODINGS:
        for layout in LAYOUTS:
            vals = _import_strings(batch, _edge_columns(B, n_in, rot), encoding, layout)
            assert batch.solve() == 0
            _assert_read_back(batch, vals, f"encoding {encoding} layout {layout} n_in {n_in} B {B}")
            rot += 11
    batch.free()


def test_streaming_kernel_more_than_one_block():
    """the witness-major kernel's blocks hold 256 instances: below / above one and two blocks, every edge value in the last live lane of a block"""
    n_in = 2
    for B in (255, 257, 513):
        batch = acvm_amd.Batch(_readback_circuit(n_in), B, [1, 2])
        for encoding in ENCODINGS:
            vals = _import_strings(batch, _edge_columns(B, n_in, encoding), encoding, WM)
            assert batch.solve() == 0
            _assert_read_back(batch, vals, f"encoding {encoding} B {B}")
        batch.free()


def test_byte_shortcut_is_decided_per_wave():
    """waves whose 64 values are all bytes take the closed form, a wave with one value that is no byte takes the product: same rows either way.
    The read-back circuit has no byte plane, so Montgomery-256 inputs never take the shortcut here (test 4 covers them with planes)."""
    n_in, B = 4, 130
    rng = np.random.default_rng(0xB17E)
    strings = [[int(b) for b in rng.integers(0, 256, n_in)] for _ in range(B)]
    strings[0][:2], strings[129][2:] = [0, 255], [255, 0]
    strings[70][1] = 256        # witness-major: the second wave of input 1; instance-major: the wave of instances [64, 80)
    strings[20][3] = P + 200    # a byte once reduced
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    for encoding in (BE32, LE32):
        for layout in LAYOUTS:
            vals = _import_strings(batch, strings, encoding, layout)
            assert vals[20][3] == 200
            assert batch.solve() == 0
            _assert_read_back(batch, vals, f"encoding {encoding} layout {layout}")
    batch.free()


# ---- 2. stride and columns
@pytest.mark.parametrize("layout", LAYOUTS)
def test_stride_and_column_lists(layout):
    n_in, B = 5, 70
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    wide = 2 * n_in + 3
    cases = [(None, n_in), ([4, 2, 0, 1, 3], n_in), ([1, 1, 3, 0, 3], n_in), ([12, 0, 7, 7, 3], wide)]
    rot = 0
    for encoding in ENCODINGS:
        for columns, n_columns in cases:
            dense = B if layout == WM else n_columns
            for stride in (0, dense + 7):
                vals = _import_strings(batch, _edge_columns(B, n_columns, rot), encoding, layout, columns=columns, stride=stride)
                assert batch.solve() == 0
                _assert_read_back(batch, vals, f"encoding {encoding} layout {layout} columns {columns} of {n_columns} stride {stride}")
                rot += 5
    batch.free()


# ---- 3. refusals
def test_refusals_leave_the_handle_usable():
    n_in, B = 5, 65
    ids = list(range(1, n_in + 1))
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, ids)
    strings = _edge_columns(B, n_in)
    vals = _import_strings(batch, strings, BE32, IM)  # a good import first: a refused call must leave it in place
    buf = acvm_amd.DeviceBuffer(size=(B + 8) * (2 * n_in + 3) * 32 + 16)
    invalid = r"error -1: "
    with pytest.raises(acvm_amd.AcvmError, match=invalid + ".*stride"):
        batch.import_device(buf.ptr, layout=IM, stride=n_in - 1)
    with pytest.raises(acvm_amd.AcvmError, match=invalid + ".*stride"):
        batch.import_device(buf.ptr, layout=WM, stride=B - 1)
    with pytest.raises(acvm_amd.AcvmError, match=invalid + ".*stride"):
        batch.import_device(buf.ptr, layout=IM, columns=[0, 1, 2, 3, 4], n_columns=7, stride=6)
    with pytest.raises(acvm_amd.AcvmError, match=invalid + ".*column"):
        batch.import_device(buf.ptr, columns=[0, 1, 2, 3, 7], n_columns=7)
    with pytest.raises(acvm_amd.AcvmError, match=invalid + ".*encoding"):
        batch.import_device(buf.ptr, encoding=3)
    with pytest.raises(acvm_amd.AcvmError, match=invalid + ".*layout"):
        batch.import_device(buf.ptr, layout=2)
    with pytest.raises(acvm_amd.AcvmError, match=invalid + ".*aligned"):
        batch.import_device(buf.ptr + 8, encoding=LE32)
    with pytest.raises(acvm_amd.AcvmError, match=invalid + ".*aligned"):
        batch.import_device(buf.ptr + 8, encoding=BE32, stride=n_in + 1)  # (not the plain shape: a stride above dense)
    with pytest.raises(acvm_amd.AcvmError, match=invalid):
        batch.import_device(0)
    with pytest.raises(acvm_amd.AcvmError, match=invalid + ".*stride"):
        batch.solve(then_import=buf.ptr, then_import_desc=dict(layout=WM, stride=B - 1))
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "after the refusals")
    want = _whole_state(batch)
    # a misaligned pointer with the plain descriptor is acvm_batch_set_initial_witness_device: both succeed and agree
    rows = _buffer([[_string_bytes(s, BE32) for s in row] for row in strings], IM)
    for off in (4, 8):
        buf.upload(rows, offset=off)
        batch.import_device(buf.ptr + off)
        assert batch.solve() == 0
        _assert_same_state(_whole_state(batch), want, f"plain descriptor, offset {off}")
        batch.set_initial_witness_device(buf.ptr + off)
        assert batch.solve() == 0
        _assert_same_state(_whole_state(batch), want, f"set_initial_witness_device, offset {off}")
    buf.free()
    batch.free()


# ---- 4. byte planes and event words
def test_hash_circuit_byte_planes_and_event_words(oracle):
    """SHA256 / Keccak256 read the plane words the import wrote, RANGE the rows; one handle takes two different batches one after the other, each
    with one instance whose input is no byte: a plane left from the first batch, or event words the second import did not reset, would show"""
    B = 70
    circ, ids = synth.hash_circuit(n_msg=8)
    n_in = len(ids)
    data = circ.to_bytes()
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), B, ids)
    assert batch.stats()["n_byte_planes"] == n_in
    for seed, bad, (encoding, layout) in ((0xAC1D0003, (5, 2), (MONT, WM)), (0xAC1D0B0B, (9, n_in - 1), (LE32, IM)), (0xAC1D0C0C, (64, 0), (MONT, IM))):
        values = np.frombuffer(synth.byte_batch(B, n_in, seed=seed), dtype=np.uint8).reshape(B, n_in, 32).copy()
        values[bad[0], bad[1]] = np.frombuffer((256).to_bytes(32, "big"), dtype=np.uint8)
        ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values.tobytes(), B)
        assert ores[bad[0]].status == 2 and sum(r.status != 0 for r in ores) == 1
        ints = [[int.from_bytes(values[j, k].tobytes(), "big") for k in range(n_in)] for j in range(B)]
        buf = acvm_amd.DeviceBuffer(_buffer([[_value_bytes(v, encoding) for v in row] for row in ints], layout))
        batch.import_device(buf.ptr, encoding=encoding, layout=layout)
        buf.free()
        assert batch.solve() == 1
        res = batch.results()
        for j in range(B):
            assert res[j].as_tuple() == ores[j].as_tuple(), f"encoding {encoding} layout {layout} instance {j}: {res[j].as_tuple()}, the oracle's {ores[j].as_tuple()}"
        asg, vals = batch.witness_map()
        nw = min(oasg.shape[1], asg.shape[1])
        assert np.array_equal(asg[:, :nw], oasg[:, :nw])
        wrong = np.argwhere((vals[:, :nw] != ovals[:, :nw]).any(axis=2))
        assert wrong.size == 0, f"encoding {encoding} layout {layout}: witness {wrong[0][1]} of instance {wrong[0][0]} differs from the oracle's"
    batch.free()


# ---- 5. hand-over without a chosen order
def test_hand_over_the_whole_map_to_the_next_circuit(oracle):
    """batch A exports its WHOLE map as a prover keeps it (Montgomery-256, one column per witness, a padded stride); batch B picks its three
    inputs out of it by a column list"""
    B, stride = 130, 192
    circ_a, ids_a = synth.arithmetic_circuit(200, seed=0xAC1D0E05)
    data_a = circ_a.to_bytes()
    values = synth.witness_batch(B, seed=0xAC1D0E05, edge_cases=False)
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data_a), ids_a, values, B)
    a = acvm_amd.Batch(acvm_amd.Circuit(data_a), B, ids_a)
    a.set_initial_witness(values)
    assert a.solve() == 0
    chosen = [a.nw - 1, a.nw // 2, ids_a[0]]
    assert oasg[:, chosen].all()
    d = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (a.nw * stride * 32))
    a.export_device(d.ptr, encoding=MONT, layout=WM, stride=stride)
    circ_b = Circuit(5, [E([(1, 1, 2)], [(1, 3), (P - 1, 4)], 0), E([(1, 4, 4)], [(P - 1, 5)], 7)])  # w4 = w1 w2 + w3, w5 = w4^2 + 7
    ids_b = [1, 2, 3]
    data_b = circ_b.to_bytes()
    b = acvm_amd.Batch(acvm_amd.Circuit(data_b), B, ids_b)
    b.import_device(d.ptr, encoding=MONT, layout=WM, columns=chosen, n_columns=a.nw, stride=stride)
    assert b.solve() == 0
    gasg, gvals = b.witness_map()
    bres, basg, bvals = oracle.solve_batch(oracle.Circuit(data_b), ids_b, np.ascontiguousarray(ovals[:, chosen]).tobytes(), B)
    assert all(r.status == 0 for r in bres)
    nw = min(basg.shape[1], gasg.shape[1])
    assert np.array_equal(gasg[:, :nw], basg[:, :nw]) and np.array_equal(gvals[:, :nw], bvals[:, :nw])
    for x in (a, b, d):
        x.free()


# ---- 6. tiles through one handle
@functools.lru_cache(maxsize=None)
def _tile_circuit(n_in):
    """the read-back gates and one that fails where w1 = 0: w1 * u = 1"""
    ops = [E([], [(3, k), (P - 1, n_in + k)], 1) for k in range(1, n_in + 1)] + [E([(1, 1, 2 * n_in + 1)], [], P - 1)]
    return acvm_amd.Circuit(Circuit(2 * n_in + 1, ops).to_bytes())


def _fresh_state(circuit, ids, rows):
    f = acvm_amd.Batch(circuit, len(rows), ids)
    f.set_initial_witness(synth.values_from_rows(rows))
    f.solve()
    st = _whole_state(f)
    f.free()
    return st


def test_tiles_through_one_handle():
    n_in, B, stride = 5, 65, 70
    ids = list(range(1, n_in + 1))
    circuit = _tile_circuit(n_in)
    desc = dict(encoding=MONT, layout=WM, columns=[3, 0, 4, 1, 2], n_columns=n_in, stride=stride)
    other = dict(desc, columns=[0, 3, 4, 1, 2])
    tiles = []
    for t in range(3):
        cols = [[EDGE[(j + c + 7 * t) % len(EDGE)] % P for c in range(n_in)] for j in range(B)]
        for row in cols:
            row[3] = row[3] or 1  # (w1 is column 3 under `desc`: nobody fails ...)
        if t == 1:
            cols[17][3] = 0       # (... but instance 17 of the second tile)
        tiles.append(cols)
    rows_of = lambda cols, d: [[row[c] for c in d["columns"]] for row in cols]
    bufs = [acvm_amd.DeviceBuffer(_buffer([[_value_bytes(v, MONT) for v in row] for row in cols], WM, stride)) for cols in tiles]
    want = [_fresh_state(circuit, ids, rows_of(cols, desc)) for cols in tiles]
    assert [sum(r[0] != 0 for r in w[0]) for w in want] == [0, 1, 0]
    h = acvm_amd.Batch(circuit, B, ids)
    outputs = list(range(n_in + 1, 2 * n_in + 2))

    def assert_outputs(st, what):
        assert [r.as_tuple() for r in h.results()] == st[0], what
        for w in outputs:
            got, asg = h.witness(w)
            assert np.array_equal(asg, st[1][:, w]) and np.array_equal(got, st[2][:, w]), (what, w)

    h.import_device(bufs[0].ptr, **desc)
    assert h.solve(then_import=bufs[1].ptr, then_import_desc=desc) == 0
    # tile 0 solved clean: the gated import of tile 1 ran, the rows of the initial witnesses hold tile 1
    assert_outputs(want[0], "tile 0")
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        h.witness(1)
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        h.witness_map()
    h.import_device(bufs[1].ptr, **desc)  # costs nothing
    assert h.solve(then_import=bufs[2].ptr, then_import_desc=desc) == 1
    # tile 1 has a failing instance: the import of tile 2 was held back, everything of tile 1 is still there
    _assert_same_state(_whole_state(h), want[1], "tile 1")
    h.import_device(bufs[2].ptr, **desc)  # performs it
    assert h.solve(then_import=bufs[0].ptr, then_import_desc=desc) == 0
    assert_outputs(want[2], "tile 2")
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        h.witness(1)
    # the same pointer read by ANOTHER descriptor: the import behind the solve does not count, the values are the other descriptor's
    h.import_device(bufs[0].ptr, **other)
    h.solve()
    _assert_same_state(_whole_state(h), _fresh_state(circuit, ids, rows_of(tiles[0], other)), "tile 0 by the other descriptor")
    assert rows_of(tiles[0], other) != rows_of(tiles[0], desc)
    # and the plain entry point with the same pointer imports too: its shape is not the descriptor's. It reads the first B x n_in elements of
    # the buffer as big-endian strings, whatever they were written as
    h.import_device(bufs[2].ptr, **desc)
    assert h.solve(then_import=bufs[1].ptr, then_import_desc=desc) == 0
    h.set_initial_witness_device(bufs[1].ptr)
    h.solve()
    raw = bufs[1].download(B * n_in * 32)
    as_plain = [[int.from_bytes(raw[(j * n_in + k) * 32:(j * n_in + k + 1) * 32], "big") for k in range(n_in)] for j in range(B)]
    _assert_same_state(_whole_state(h), _fresh_state(circuit, ids, as_plain), "tile 1's buffer through the plain entry point")
    for x in bufs + [h]:
        x.free()


# ---- 7. fewer live instances than the handle's capacity
def test_live_count_below_capacity_witness_major_dense():
    """set_instances(n): the dense witness-major stride is the LIVE count, not the capacity; the buffer holds exactly n_in x n elements. The lanes
    behind n cannot be read through the ABI; that nothing is written there is kernels_import.hip's `j >= a.B` in both kernels."""
    n_in, cap, n = 3, 130, 70
    batch = acvm_amd.Batch(_readback_circuit(n_in), cap, list(range(1, n_in + 1)))
    vals = _import_strings(batch, _edge_columns(cap, n_in), LE32, WM)
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "capacity")
    batch.set_instances(n)
    for encoding in ENCODINGS:
        vals = _import_strings(batch, _edge_columns(n, n_in, 3 + encoding), encoding, WM)
        assert batch.solve() == 0
        assert len(batch.results()) == n
        _assert_read_back(batch, vals, f"{n} live instances, encoding {encoding}")
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*stride"):
        batch.import_device(16, layout=WM, stride=n - 1)
    batch.set_instances(cap)
    vals = _import_strings(batch, _edge_columns(cap, n_in, 9), MONT, WM)
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "capacity again")
    batch.free()


# ---- 8. slot reuse
def test_slot_reuse_rows(oracle):
    """ACVM_BATCH_REUSE_SLOTS: the rows of the initial witnesses are the plan's (d_init_rows), and the exact path gathers them from there"""
    B = 96
    circ, ids = synth.arithmetic_circuit(1000, seed=0xAC1D0E01)
    data = circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    values = synth.witness_batch(B, seed=0xAC1D0E01)
    n_in = len(ids)
    ints = [[int.from_bytes(values[(j * n_in + k) * 32:(j * n_in + k + 1) * 32], "big") for k in range(n_in)] for j in range(B)]
    keep = [gc.num_witnesses - 1, gc.num_witnesses // 2]
    old = acvm_amd.Batch(gc, B, ids, reuse_slots=True, keep=keep)
    d_old = acvm_amd.DeviceBuffer(values)
    old.set_initial_witness_device(d_old.ptr)
    old.solve()
    assert old.stats()["n_slow_instances"] > 0 and old.stats()["n_table_rows"] < old.stats()["n_witnesses"]
    want = ([r.as_tuple() for r in old.results()], old.digest())
    solved = [j for j, r in enumerate(want[0]) if r[0] == 0]
    perm = [(5 * k + 3) % n_in for k in range(n_in)]  # input k lies in column perm[k]
    for encoding, layout in ((LE32, WM), (MONT, IM), (BE32, WM)):
        new = acvm_amd.Batch(gc, B, ids, reuse_slots=True, keep=keep)
        elements = [[None] * n_in for _ in range(B)]
        for j in range(B):
            for k in range(n_in):
                elements[j][perm[k]] = _value_bytes(ints[j][k], encoding)
        buf = acvm_amd.DeviceBuffer(_buffer(elements, layout, (B if layout == WM else n_in) + 2))
        new.import_device(buf.ptr, encoding=encoding, layout=layout, columns=perm, n_columns=n_in, stride=(B if layout == WM else n_in) + 2)
        buf.free()
        new.solve()
        assert [r.as_tuple() for r in new.results()] == want[0]
        assert np.array_equal(new.digest(), want[1])
        for j in solved[:3] + solved[-3:]:
            assert np.array_equal(new.extract(keep + ids, first=j, n=1), old.extract(keep + ids, first=j, n=1)), j
        new.free()
    # and the oracle agrees with the old path about who is solved (the old path is the yardstick above)
    ores, _, _ = oracle.solve_batch(oracle.Circuit(data), ids, values, B)
    assert [r.as_tuple() for r in ores] == want[0]
    d_old.free()
    old.free()
