"""The narrow encodings of the device I/O (ACVM_ENC_U8 .. ACVM_ENC_U128: an element is an unsigned little-endian integer of 1 .. 16 bytes) through
acvm_batch_import_device, acvm_batch_solve_then_import_ex and acvm_batch_export_device, and acvm_batch_import_device_parts (several buffers,
broadcast columns), on the device. Imports are judged by Python integers through the read-back circuit of tests/test_gpu_import.py
(w[n_in + k] = 3 w[k] + 1) and, where a real circuit runs, by the CPU oracle and by the same values fed as ACVM_ENC_BE32; exports by the oracle's
map. Buffers hold a pattern wherever no described element lies: a value read from there shows in the result, a byte written there in the buffer."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import BlackBoxFuncCall as BB, Circuit, Expression as E, FunctionInput as FI, P

pytestmark = pytest.mark.gpu
BE32, LE32, MONT = acvm_amd.ENC_BE32, acvm_amd.ENC_LE32, acvm_amd.ENC_MONT256_LE
U8, U16, U32, U64, U128 = acvm_amd.ENC_U8, acvm_amd.ENC_U16, acvm_amd.ENC_U32, acvm_amd.ENC_U64, acvm_amd.ENC_U128
NARROW = (U8, U16, U32, U64, U128)
IM, WM, BC = acvm_amd.LAYOUT_INSTANCE_MAJOR, acvm_amd.LAYOUT_WITNESS_MAJOR, acvm_amd.LAYOUT_BROADCAST
LAYOUTS = (IM, WM)
PATTERN = 0xA5
SIZE = acvm_amd.element_size


def _gpu_import_module():
    spec = importlib.util.spec_from_file_location("_gpu_import_for_typed_io", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_import.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GI = _gpu_import_module()
EDGE = _GI.EDGE
_readback_circuit = _GI._readback_circuit


# ---- values and buffers (Python integers and index arithmetic only)
@functools.lru_cache(maxsize=None)
def _edges(encoding):
    """the value edges of a width: 0, 1, the byte and plane-word boundaries, the top bit, all ones, alternating bits, and the reduction-edge
    strings of the 32-byte import cut to the width"""
    size, bits = SIZE(encoding), 8 * SIZE(encoding)
    vals = [0, 1, 255, 256, 257, (1 << 29) - 1, 1 << 29, (1 << 29) + 7, 1 << (bits - 1), (1 << bits) - 1, int("55" * size, 16), int("aa" * size, 16)]
    vals = [v for v in vals if v < (1 << bits)] + [e % (1 << bits) for e in EDGE]
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return out


def _edge_columns(encoding, B, n_columns, rot=0):
    ed = _edges(encoding)
    return [[ed[(j + c + rot) % len(ed)] for c in range(n_columns)] for j in range(B)]


def _element(v, encoding):
    if encoding == BE32:
        return int(v).to_bytes(32, "big")
    if encoding == LE32:
        return int(v).to_bytes(32, "little")
    if encoding == MONT:
        return ((int(v) << 256) % P).to_bytes(32, "little")
    return int(v).to_bytes(SIZE(encoding), "little")


def _buffer(vals, encoding, layout, stride=0, lead=0):
    """vals[i][c] -> the bytes of the whole buffer behind `lead` bytes of pattern; everything that is no described element holds PATTERN"""
    n, n_columns, size = len(vals), len(vals[0]), SIZE(encoding)
    if layout == BC:
        return bytes([PATTERN]) * lead + b"".join(_element(v, encoding) for v in vals[0])
    rows, dense = (n_columns, n) if layout == WM else (n, n_columns)
    stride = stride or dense
    assert stride >= dense
    buf = np.full((rows, stride, size), PATTERN, dtype=np.uint8)
    arr = np.frombuffer(b"".join(_element(v, encoding) for row in vals for v in row), dtype=np.uint8).reshape(n, n_columns, size)
    buf[:, :dense] = arr.transpose(1, 0, 2) if layout == WM else arr
    return bytes([PATTERN]) * lead + buf.tobytes()


def _be_rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for r in vals for v in r), dtype=np.uint8).reshape(len(vals), -1, 32)


def _assert_read_back(batch, vals, what=""):
    """vals[j][k]: the value input k of instance j holds. Every initial witness reads back as it, every gate output as 3 x + 1."""
    n_in = len(vals[0])
    assert all(r.status == acvm_amd.STATUS_SOLVED for r in batch.results()), what
    want_in, want_out = _be_rows(vals), _be_rows([[(3 * x + 1) % P for x in r] for r in vals])
    for k in range(n_in):
        for w, want, name in ((1 + k, want_in, "initial witness"), (1 + n_in + k, want_out, "gate output")):
            got, asg = batch.witness(w)
            assert asg.all(), (what, w)
            bad = np.nonzero((got != want[:, k]).any(axis=1))[0]
            assert bad.size == 0, (f"{what}: {name} {w} of instance {bad[0]} is {got[bad[0]].tobytes().hex()}, expected {want[bad[0], k].tobytes().hex()} "
                                   f"({bad.size} instances differ)")


def _import(batch, vals, encoding, layout, columns=None, stride=0, lead=0):
    """vals[j][c]: the value in column c of instance j. Imports them and returns the values the inputs then hold."""
    buf = acvm_amd.DeviceBuffer(_buffer(vals, encoding, layout, stride, lead))
    try:
        batch.import_device(buf.ptr + lead, encoding=encoding, layout=layout, columns=columns, n_columns=None if columns is None else len(vals[0]), stride=stride)
    finally:
        buf.free()
    cols = list(range(len(batch.ids))) if columns is None else columns
    return [[row[c] for c in cols] for row in vals]


def _whole_state(batch):
    asg, vals = batch.witness_map()
    return [r.as_tuple() for r in batch.results()], asg, vals


def _assert_same_state(got, want, what=""):
    assert got[0] == want[0], what
    nw = min(got[1].shape[1], want[1].shape[1])
    assert np.array_equal(got[1][:, :nw], want[1][:, :nw]), what
    bad = np.argwhere((got[2][:, :nw] != want[2][:, :nw]).any(axis=2))
    assert bad.size == 0, f"{what}: witness {bad[0][1]} of instance {bad[0][0]} differs ({len(bad)} differ)"


def _oracle_state(oracle, data, ids, rows):
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, synth.values_from_rows(rows), len(rows))
    return [r.as_tuple() for r in ores], oasg, ovals


def _be32_state(gc, ids, rows, **kw):
    """the same values through ACVM_ENC_BE32 on a fresh handle"""
    f = acvm_amd.Batch(gc, len(rows), ids, **kw)
    buf = acvm_amd.DeviceBuffer(synth.values_from_rows(rows))
    f.import_device(buf.ptr, encoding=BE32, layout=IM)
    buf.free()
    f.solve()
    return f


# ---- 1. every width x layout on the value edges
# B: one instance, below / on / above a wave and the 64-instance tile, three tiles with a ragged last one, above the 256-lane block;
# n_in: ragged and full groups of four
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130, 257])
@pytest.mark.parametrize("n_in", [1, 3, 4, 5, 9])
def test_every_width_and_layout_on_the_value_edges(n_in, B):
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    rot = 0
    for encoding in NARROW:
        for layout in LAYOUTS:
            vals = _import(batch, _edge_columns(encoding, B, n_in, rot), encoding, layout)
            assert batch.solve() == 0
            _assert_read_back(batch, vals, f"encoding {encoding} layout {layout} n_in {n_in} B {B}")
            rot += 11
    batch.free()


# ---- 2. strides, pointers, column lists
@pytest.mark.parametrize("layout", LAYOUTS)
def test_strides_pointers_and_column_lists(layout):
    n_in, B = 5, 70
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    wide = 2 * n_in + 3
    rot = 0
    for encoding in NARROW:
        for columns, n_columns in ((None, n_in), ([1, 1, 3, 0, 3], n_in), ([12, 0, 7, 7, 3], wide)):
            dense = B if layout == WM else n_columns
            for stride in (0, dense + 1, dense + 7):  # (U8 / U16 rows then start off any 4-byte boundary)
                vals = _import(batch, _edge_columns(encoding, B, n_columns, rot), encoding, layout, columns=columns, stride=stride)
                assert batch.solve() == 0
                _assert_read_back(batch, vals, f"encoding {encoding} layout {layout} columns {columns} of {n_columns} stride {stride}")
                rot += 5
    # a pointer is aligned to the element's size, no further
    for encoding, lead in ((U8, 1), (U8, 3), (U16, 2), (U32, 4), (U64, 8)):
        vals = _import(batch, _edge_columns(encoding, B, n_in, rot), encoding, layout, lead=lead, stride=(B if layout == WM else n_in) + 1)
        assert batch.solve() == 0
        _assert_read_back(batch, vals, f"encoding {encoding} layout {layout} from ptr + {lead}")
        rot += 5
    want = _whole_state(batch)
    buf = acvm_amd.DeviceBuffer(size=(B + 8) * wide * 16 + 16)
    for encoding, lead in ((U16, 1), (U32, 2), (U64, 4), (U128, 8)):
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*aligned"):
            batch.import_device(buf.ptr + lead, encoding=encoding, layout=layout)
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*aligned"):
            batch.solve(then_import=buf.ptr + lead, then_import_desc=dict(encoding=encoding, layout=layout))
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*stride"):
        batch.import_device(buf.ptr, encoding=U8, layout=layout, stride=(B if layout == WM else n_in) - 1)
    buf.free()
    assert batch.solve() == 0  # a refused call leaves the handle as it was
    _assert_same_state(_whole_state(batch), want, "after the refusals")
    batch.free()


# ---- 3. bytes with planes
def test_hash_circuit_bytes_as_u8_equal_be32_and_the_oracle(oracle):
    """SHA256 -> Keccak256 + RANGE read the plane words and rows the U8 import wrote: results, assigned sets and the whole map equal those of the
    same values through BE32 on a fresh handle, and the oracle's"""
    B = 70
    circ, ids = synth.hash_circuit(n_msg=8)
    n_in, data = len(ids), circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    rows = [[int(v) for v in r] for r in np.frombuffer(synth.byte_batch(B, n_in, seed=0xAC1D0710), dtype=np.uint8).reshape(B, n_in, 32)[:, :, 31]]
    rows[0][:2], rows[B - 1][-2:] = [0, 255], [255, 0]
    want = _oracle_state(oracle, data, ids, rows)
    assert all(r[0] == 0 for r in want[0])
    ref = _be32_state(gc, ids, rows)
    ref_state = _whole_state(ref)
    ref.free()
    _assert_same_state(ref_state, want, "BE32 against the oracle")
    batch = acvm_amd.Batch(gc, B, ids)
    assert batch.stats()["n_byte_planes"] == n_in
    for layout in LAYOUTS:
        _import(batch, rows, U8, layout)
        assert batch.solve() == 0
        got = _whole_state(batch)
        _assert_same_state(got, ref_state, f"U8 layout {layout} against BE32")
        _assert_same_state(got, want, f"U8 layout {layout} against the oracle")
    batch.free()


@pytest.mark.parametrize("encoding", [U16, U32, U64, U128])
def test_hash_circuit_wider_inputs_with_values_that_are_no_bytes(oracle, encoding):
    """the wave [0, 64) holds bytes only (the closed form), the wave [64, 128) one value that is no byte (the product), the ragged last wave two
    more: those instances fail at the same opcode with the same error as through BE32, everybody else solves"""
    B = 130
    circ, ids = synth.hash_circuit(n_msg=8)
    n_in, data = len(ids), circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    rows = [[int(v) for v in r] for r in np.frombuffer(synth.byte_batch(B, n_in, seed=0xAC1D0711), dtype=np.uint8).reshape(B, n_in, 32)[:, :, 31]]
    top = (1 << (8 * SIZE(encoding))) - 1
    rows[70][3], rows[128][n_in - 1], rows[129][0] = 256, top, (1 << 29) + 7 if encoding != U16 else 0x8007
    want = _oracle_state(oracle, data, ids, rows)
    assert [j for j, r in enumerate(want[0]) if r[0] != 0] == [70, 128, 129]
    ref = _be32_state(gc, ids, rows)
    ref_state = _whole_state(ref)
    ref.free()
    _assert_same_state(ref_state, want, "BE32 against the oracle")
    batch = acvm_amd.Batch(gc, B, ids)
    for layout in LAYOUTS:
        _import(batch, rows, encoding, layout)
        assert batch.solve() == 3
        got = _whole_state(batch)
        _assert_same_state(got, ref_state, f"encoding {encoding} layout {layout} against BE32")
        _assert_same_state(got, want, f"encoding {encoding} layout {layout} against the oracle")
    batch.free()


def test_closed_form_and_product_give_the_same_rows():
    """without planes: per wave all bytes, or bytes and a single value that is none, in every width above one byte"""
    n_in, B = 4, 130
    rng = np.random.default_rng(0xB17E)
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    for encoding in (U16, U32, U64, U128):
        vals = [[int(b) for b in rng.integers(0, 256, n_in)] for _ in range(B)]
        vals[0][:2], vals[129][2:] = [0, 255], [255, 0]
        vals[70][1] = 256  # witness-major: the second wave of input 1; instance-major: the second tile's wave of input 1
        for layout in LAYOUTS:
            got = _import(batch, vals, encoding, layout)
            assert batch.solve() == 0
            _assert_read_back(batch, got, f"encoding {encoding} layout {layout}")
    batch.free()


# ---- 4. tiles through solve(then_import_desc=...)
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


def test_three_tiles_of_bytes_through_one_handle():
    n_in, B, stride = 5, 65, 71
    ids = list(range(1, n_in + 1))
    circuit = _tile_circuit(n_in)
    desc = dict(encoding=U8, layout=WM, columns=[3, 0, 4, 1, 2], n_columns=n_in, stride=stride)
    other = dict(desc, columns=[0, 3, 4, 1, 2])
    tiles = []
    for t in range(3):
        cols = [[(37 * j + 11 * c + 5 * t) % 256 for c in range(n_in)] for j in range(B)]
        for row in cols:
            row[3] = row[3] or 1  # (w1 is column 3 under `desc`: nobody fails ...)
        if t == 1:
            cols[17][3] = 0       # (... but instance 17 of the second tile)
        tiles.append(cols)
    rows_of = lambda cols, d: [[row[c] for c in d["columns"]] for row in cols]
    bufs = [acvm_amd.DeviceBuffer(_buffer(cols, U8, WM, stride)) for cols in tiles]
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
    h.import_device(bufs[1].ptr, **desc)  # costs nothing
    assert h.solve(then_import=bufs[2].ptr, then_import_desc=desc) == 1
    # tile 1 has a failing instance: the import of tile 2 was held back, everything of tile 1 is still there
    _assert_same_state(_whole_state(h), want[1], "tile 1")
    h.import_device(bufs[2].ptr, **desc)  # performs it
    assert h.solve(then_import=bufs[0].ptr, then_import_desc=desc) == 0
    assert_outputs(want[2], "tile 2")
    # the same pointer read by a changed descriptor: the import behind the solve does not count
    h.import_device(bufs[0].ptr, **other)
    h.solve()
    _assert_same_state(_whole_state(h), _fresh_state(circuit, ids, rows_of(tiles[0], other)), "tile 0 by the other descriptor")
    assert rows_of(tiles[0], other) != rows_of(tiles[0], desc)
    for x in bufs + [h]:
        x.free()


# ---- 5. parts
@functools.lru_cache(maxsize=None)
def _mixed_input_circuit():
    """fn main(msg: [u8; 8], a: Field, b: Field, root: Field): SHA256 over the bytes (RANGE on each), w44 = a b + root, w45 = w44^2 + 7 w12"""
    ids = list(range(1, 12))
    sha_out = list(range(12, 44))
    ops = [BB("RANGE", {"input": FI(w, 8)}) for w in ids[:8]]
    ops.append(BB("SHA256", {"inputs": [FI(w, 8) for w in ids[:8]], "outputs": sha_out}))
    ops.append(E([(1, 9, 10)], [(1, 11), (P - 1, 44)], 0))
    ops.append(E([(1, 44, 44)], [(7, 12), (P - 1, 45)], 0))
    circ = Circuit(current_witness_index=45, opcodes=ops, private_parameters=ids, return_values=[45])
    return circ.to_bytes(), ids


def _mixed_rows(B, seed):
    rng = np.random.default_rng(seed)
    root = EDGE[5] % P
    return [[int(b) for b in rng.integers(0, 256, 8)] + [EDGE[(j + 3) % len(EDGE)] % P, EDGE[(2 * j + 1) % len(EDGE)] % P, root] for j in range(B)]


def _mixed_parts(rows, bufs):
    """the bytes as U8 witness-major, the two field inputs as Montgomery-256 instance-major, the root as BE32 broadcast"""
    bufs += [acvm_amd.DeviceBuffer(_buffer([r[:8] for r in rows], U8, WM)), acvm_amd.DeviceBuffer(_buffer([r[8:10] for r in rows], MONT, IM)),
             acvm_amd.DeviceBuffer(_buffer([r[10:] for r in rows], BE32, BC))]
    return [dict(d_ptr=bufs[-3].ptr, encoding=U8, layout=WM, positions=range(8)), dict(d_ptr=bufs[-2].ptr, encoding=MONT, layout=IM, positions=[8, 9]),
            dict(d_ptr=bufs[-1].ptr, encoding=BE32, layout=BC, positions=[10])]


@pytest.mark.parametrize("B", [70, 257])
def test_parts_bytes_fields_and_a_broadcast_root(oracle, B):
    data, ids = _mixed_input_circuit()
    gc = acvm_amd.Circuit(data)
    rows = _mixed_rows(B, 0xAC1D0712)
    want = _oracle_state(oracle, data, ids, rows)
    assert all(r[0] == 0 for r in want[0])
    ref = _be32_state(gc, ids, rows)
    ref_state = _whole_state(ref)
    ref.free()
    batch = acvm_amd.Batch(gc, B, ids)
    assert batch.stats()["n_byte_planes"] > 0
    bufs = []
    parts = _mixed_parts(rows, bufs)
    assert batch.import_list_copies() == 0
    batch.import_device_parts(parts)
    assert batch.import_list_copies() == 1
    assert batch.solve() == 0
    got = _whole_state(batch)
    _assert_same_state(got, ref_state, "parts against one BE32 import")
    _assert_same_state(got, want, "parts against the oracle")
    # the same call again: the lists are on the device already
    batch.import_device_parts(parts)
    assert batch.import_list_copies() == 1
    assert batch.solve() == 0
    _assert_same_state(_whole_state(batch), want, "the same parts again")
    # other values in the order [root, bytes, fields], a part without inputs among them: other lists, one more copy
    rows2 = _mixed_rows(B, 0xAC1D0713)
    parts2 = _mixed_parts(rows2, bufs)
    batch.import_device_parts([parts2[2], dict(d_ptr=0, encoding=U64, layout=WM, positions=[]), parts2[0], parts2[1]])
    assert batch.import_list_copies() == 2
    assert batch.solve() == 0
    _assert_same_state(_whole_state(batch), _oracle_state(oracle, data, ids, rows2), "the parts in another order")
    for x in bufs + [batch]:
        x.free()


@pytest.mark.parametrize("encoding", NARROW + (LE32, MONT))
def test_broadcast_columns(encoding):
    """inputs 0 and 2 from a broadcast buffer of five columns (columns 4 and 1), input 1 per instance as U8: one value for all 130 instances"""
    n_in, B = 3, 130
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, [1, 2, 3])
    ed = _edges(encoding) if encoding in NARROW else [e % P for e in EDGE]
    for rot in (0, 4, 9):
        common = [ed[(rot + c) % len(ed)] for c in range(5)]
        mine = [[(3 * j + rot) % 256] for j in range(B)]
        d_c, d_m = acvm_amd.DeviceBuffer(_buffer([common], encoding, BC)), acvm_amd.DeviceBuffer(_buffer(mine, U8, WM))
        batch.import_device_parts([dict(d_ptr=d_c.ptr, encoding=encoding, layout=BC, positions=[0, 2], columns=[4, 1], n_columns=5),
                                   dict(d_ptr=d_m.ptr, encoding=U8, layout=WM, positions=[1])])
        assert batch.solve() == 0
        _assert_read_back(batch, [[common[4], mine[j][0], common[1]] for j in range(B)], f"encoding {encoding} rot {rot}")
        d_c.free()
        d_m.free()
    batch.free()


def test_parts_refusals_leave_the_previous_import_in_place():
    n_in, B = 4, 65
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    vals = _import(batch, _edge_columns(U32, B, n_in), U32, WM)
    buf = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (B * n_in * 32 + 64))
    part = lambda positions, **kw: dict(dict(d_ptr=buf.ptr, encoding=U8, layout=WM, positions=positions), **kw)
    refused = [
        ([part([0, 1]), part([3])], "position 2 .*no part"),                                  # uncovered
        ([part([0, 1, 2]), part([2, 3])], "position 2 .*twice"),                              # doubly covered
        ([part([0, 1, 1, 2, 3])], "position 1 .*twice"),                                      # ... inside one part
        ([part([0, 1, 2]), part([4])], "position 4 "),                                        # out of range
        ([part([0, 1]), part([2, 3], d_ptr=buf.ptr + 8, encoding=U128)], "part 1: .*aligned"),    # a misaligned part
        ([part([0, 1]), part([2, 3], d_ptr=buf.ptr + 8, encoding=LE32)], "part 1: .*aligned"),
        ([part([0, 1]), part([2, 3], encoding=21)], "part 1: .*encoding"),                    # an unknown encoding in the second part
        ([part([0, 1]), part([2, 3], layout=2)], "part 1: .*layout"),
        ([part([0, 1]), part([2, 3], stride=B - 1)], "part 1: .*stride"),
        ([part([0, 1]), part([2, 3], columns=[0, 2], n_columns=2)], "part 1: .*column"),
        ([part([0, 1]), part([2, 3], d_ptr=0)], "part 1: .*null"),
        ([], "position 0 .*no part"),                                                         # no parts for a circuit with initial witnesses
    ]
    for parts, message in refused:
        copies = batch.import_list_copies()
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            batch.import_device_parts(parts)
        assert batch.import_list_copies() == copies  # nothing was copied or enqueued
        assert batch.solve() == 0
        _assert_read_back(batch, vals, f"after the refusal {message!r}")
    # the broadcast layout belongs to parts, the old refusals hold
    for kw, message in ((dict(layout=BC), "layout"), (dict(layout=2), "layout"), (dict(encoding=3), "encoding"), (dict(encoding=15), "encoding"), (dict(encoding=21), "encoding")):
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            batch.import_device(buf.ptr, **kw)
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            batch.solve(then_import=buf.ptr, then_import_desc=kw)
    for kw, message in ((dict(layout=BC), "layout"), (dict(layout=2), "layout"), (dict(encoding=3), "encoding"), (dict(encoding=21), "encoding")):
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*" + message):
            batch.export_device(buf.ptr, **kw)
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "after the old refusals")
    buf.free()
    batch.free()


def test_parts_for_a_circuit_without_initial_witnesses():
    circuit = acvm_amd.Circuit(Circuit(1, [E([], [(1, 1)], P - 5)]).to_bytes())  # w1 = 5
    batch = acvm_amd.Batch(circuit, 3, [])
    batch.import_device_parts([])
    assert batch.solve() == 0
    got, asg = batch.witness(1)
    assert asg.all() and all(int.from_bytes(g.tobytes(), "big") == 5 for g in got)
    batch.free()


# ---- 6. live count below capacity, slot reuse
def test_live_count_below_capacity():
    """set_instances(n): the dense witness-major stride is the live count; the buffers hold exactly n elements per column"""
    n_in, cap, n = 3, 130, 70
    batch = acvm_amd.Batch(_readback_circuit(n_in), cap, [1, 2, 3])
    vals = _import(batch, _edge_columns(U8, cap, n_in), U8, WM)
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "capacity")
    batch.set_instances(n)
    for encoding in (U8, U32):
        for layout in LAYOUTS:
            vals = _import(batch, _edge_columns(encoding, n, n_in, 3 + encoding), encoding, layout)
            assert batch.solve() == 0
            assert len(batch.results()) == n
            _assert_read_back(batch, vals, f"{n} live instances, encoding {encoding} layout {layout}")
    cols = _edge_columns(U16, n, n_in, 7)
    d_a, d_b = acvm_amd.DeviceBuffer(_buffer([r[:2] for r in cols], U16, WM)), acvm_amd.DeviceBuffer(_buffer([r[2:] for r in cols], U16, IM))
    batch.import_device_parts([dict(d_ptr=d_a.ptr, encoding=U16, layout=WM, positions=[1, 0]), dict(d_ptr=d_b.ptr, encoding=U16, layout=IM, positions=[2])])
    assert batch.solve() == 0
    _assert_read_back(batch, [[r[1], r[0], r[2]] for r in cols], f"{n} live instances, parts")
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*stride"):
        batch.import_device(16, encoding=U8, layout=WM, stride=n - 1)
    batch.set_instances(cap)
    vals = _import(batch, _edge_columns(U64, cap, n_in, 9), U64, WM)
    assert batch.solve() == 0
    _assert_read_back(batch, vals, "capacity again")
    for x in (d_a, d_b, batch):
        x.free()


def test_slot_reuse_rows(oracle):
    """ACVM_BATCH_REUSE_SLOTS: the rows of the initial witnesses are the plan's (d_init_rows), for the U8 import and for parts"""
    B = 96
    data, ids = _mixed_input_circuit()
    gc = acvm_amd.Circuit(data)
    rows = _mixed_rows(B, 0xAC1D0714)
    rows[40][2] = 0  # (nobody fails here; zero is a byte like any other)
    keep = [45, 20]
    ref = _be32_state(gc, ids, rows, reuse_slots=True, keep=keep)
    want = ([r.as_tuple() for r in ref.results()], ref.digest(), ref.extract(keep + ids))
    ref.free()
    ores = _oracle_state(oracle, data, ids, rows)[0]
    assert ores == want[0]
    new = acvm_amd.Batch(gc, B, ids, reuse_slots=True, keep=keep)
    bufs = []
    new.import_device_parts(_mixed_parts(rows, bufs))
    new.solve()
    assert [r.as_tuple() for r in new.results()] == want[0]
    assert np.array_equal(new.digest(), want[1]) and np.array_equal(new.extract(keep + ids), want[2])
    for x in bufs + [new]:
        x.free()
    # all inputs as bytes through the plain U8 import
    rows8 = [r[:8] + [r[0], r[1], 7] for r in rows]
    ref = _be32_state(gc, ids, rows8, reuse_slots=True, keep=keep)
    want = ([r.as_tuple() for r in ref.results()], ref.digest(), ref.extract(keep + ids))
    ref.free()
    for layout in LAYOUTS:
        new = acvm_amd.Batch(gc, B, ids, reuse_slots=True, keep=keep)
        _import(new, rows8, U8, layout)
        new.solve()
        assert [r.as_tuple() for r in new.results()] == want[0]
        assert np.array_equal(new.digest(), want[1]) and np.array_equal(new.extract(keep + ids), want[2])
        new.free()


# ---- 7. export
TAIL = 96


def _expected_narrow(oasg, ovals, encoding, layout, witnesses, first, n, stride):
    """the whole output buffers (values, mask) as they must read afterwards, TAIL pattern elements behind the last row included: the low bytes of
    the oracle's value, little-endian; mask 0 unassigned (zero bytes), 1 the value fits, 2 it does not"""
    size, nw_o = SIZE(encoding), oasg.shape[1]
    low = np.zeros((n, len(witnesses), size), dtype=np.uint8)
    mask = np.zeros((n, len(witnesses)), dtype=np.uint8)
    for k, w in enumerate(witnesses):
        if w < nw_o:
            asg = oasg[first:first + n, w] != 0
            be = ovals[first:first + n, w]
            fits = ~be[:, :32 - size].any(axis=1)
            low[:, k] = np.where(asg[:, None], be[:, ::-1][:, :size], 0)
            mask[:, k] = np.where(asg, np.where(fits, 1, 2), 0)
    rows, dense = (len(witnesses), n) if layout == WM else (n, len(witnesses))
    stride = stride or dense
    vals = np.full((rows * stride + TAIL, size), PATTERN, dtype=np.uint8)
    m = np.full(rows * stride + TAIL, PATTERN, dtype=np.uint8)
    v, mm = vals[:rows * stride].reshape(rows, stride, size), m[:rows * stride].reshape(rows, stride)
    if layout == WM:
        v[:, :dense], mm[:, :dense] = low.transpose(1, 0, 2), mask.T
    else:
        v[:, :dense], mm[:, :dense] = low, mask
    return vals, m


def _check_export(batch, oasg, ovals, encoding, layout, witnesses=None, first=0, n=None, stride=0, with_mask=True, lead=0):
    n = batch.B - first if n is None else n
    ws = list(range(batch.nw)) if witnesses is None else list(witnesses)
    want_v, want_m = _expected_narrow(oasg, ovals, encoding, layout, ws, first, n, stride)
    d_v = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (want_v.size + lead))
    d_m = acvm_amd.DeviceBuffer(bytes([PATTERN]) * want_m.size) if with_mask else None
    try:
        batch.export_device(d_v.ptr + lead, encoding=encoding, layout=layout, witnesses=witnesses, first=first, n=n, stride=stride, d_assigned=d_m.ptr if with_mask else None)
        raw = d_v.download()
        assert raw[:lead] == bytes([PATTERN]) * lead
        got_v = np.frombuffer(raw[lead:], dtype=np.uint8).reshape(-1, SIZE(encoding))
        what = f"encoding {encoding} layout {layout} first {first} n {n} stride {stride}"
        if with_mask:
            got_m = np.frombuffer(d_m.download(), dtype=np.uint8)
            bad = np.nonzero(got_m != want_m)[0]
            assert bad.size == 0, f"{what}: mask differs at element {bad[0]} ({bad.size} in all): {got_m[bad[0]]} != {want_m[bad[0]]}"
        bad = np.nonzero((got_v != want_v).any(axis=1))[0]
        assert bad.size == 0, f"{what}: values differ at element {bad[0]} ({bad.size} in all): {got_v[bad[0]].tobytes().hex()} != {want_v[bad[0]].tobytes().hex()}"
        return want_m
    finally:
        d_v.free()
        if d_m is not None:
            d_m.free()


def _solved(oracle, data, ids, values, B, force_slow=False, **kw):
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values, B)
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), B, ids, **kw)
    batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(values)
    batch.solve()
    return batch, ores, oasg, ovals


@pytest.mark.parametrize("force_slow", [False, True])
def test_export_digest_bytes_of_the_hash_circuit(oracle, force_slow):
    """the 64 digest witnesses as U8 in both layouts with the mask; instance 9 fails its RANGE check and lives on the exact path (its digests are
    unassigned: mask 0), with the forced slow path every instance does; sub-ranges across a 64-instance tile, strides, no mask"""
    B = 150
    circ, ids = synth.hash_circuit(n_msg=8)
    n_in = len(ids)
    values = np.frombuffer(synth.byte_batch(B, n_in, seed=0xAC1D0715), dtype=np.uint8).reshape(B, n_in, 32).copy()
    values[9, 2] = np.frombuffer((256).to_bytes(32, "big"), dtype=np.uint8)
    batch, ores, oasg, ovals = _solved(oracle, circ.to_bytes(), ids, values.tobytes(), B, force_slow=force_slow)
    assert [j for j, r in enumerate(ores) if r.status != 0] == [9]
    digests = list(range(n_in + 1, n_in + 65))
    for layout in LAYOUTS:
        m = _check_export(batch, oasg, ovals, U8, layout, witnesses=digests)
        assert set(m[m != PATTERN]) == {0, 1}
        _check_export(batch, oasg, ovals, U8, layout, witnesses=digests, first=37, n=101)
        _check_export(batch, oasg, ovals, U8, layout, witnesses=digests, first=3, n=70, stride=(70 if layout == WM else 64) + 3, lead=1)
        _check_export(batch, oasg, ovals, U8, layout, witnesses=digests, with_mask=False)
        _check_export(batch, oasg, ovals, U16, layout, witnesses=digests + ids[:3] + [batch.nw + 4], first=60, n=10, stride=83 if layout == IM else 17, lead=2)
    _check_export(batch, oasg, ovals, U32, IM)  # the whole map
    batch.free()


@pytest.mark.parametrize("force_slow", [False, True])
def test_export_full_size_values_unassigned_and_unknown_witnesses(oracle, force_slow):
    """arithmetic witnesses of full size: mask 2 and the value mod 2^w; unassigned witnesses of the mixed circuit and listed indices beyond the
    circuit: mask 0 and zero bytes; scaled columns and exact lanes (the edge cases of witness_batch put a few instances there)"""
    B = 150
    circ, ids = synth.mixed_circuit(600, seed=0xAC1D0E02)
    batch, ores, oasg, ovals = _solved(oracle, circ.to_bytes(), ids, synth.witness_batch(B, seed=0xAC1D0E02), B, force_slow=force_slow)
    if not force_slow:
        assert 1 <= batch.stats()["n_slow_instances"] < B
    assert not oasg[0].all()
    nw = batch.nw
    sel = [nw - 1, 3, 3, nw + 5, 0xFFFFFFFF, nw // 2, 1] + list(range(20, 90))
    seen = set()
    for encoding in NARROW:
        for layout in LAYOUTS:
            m = _check_export(batch, oasg, ovals, encoding, layout)
            seen |= set(m[m != PATTERN])
            _check_export(batch, oasg, ovals, encoding, layout, witnesses=sel, first=37, n=101, stride=(101 if layout == WM else len(sel)) + 5)
        _check_export(batch, oasg, ovals, encoding, IM, witnesses=[nw - 1, nw + 1, 7], first=3, n=140, stride=5)  # (a short list: the direct kernel)
        _check_export(batch, oasg, ovals, encoding, IM, witnesses=[ids[0]])
    assert seen == {0, 1, 2}
    batch.free()


def test_export_scaled_columns_of_an_arithmetic_circuit(oracle):
    B = 130
    circ, ids = synth.arithmetic_circuit(1000, seed=0xAC1D0E01)
    batch, ores, oasg, ovals = _solved(oracle, circ.to_bytes(), ids, synth.witness_batch(B, seed=0xAC1D0E01), B)
    assert batch.stats()["n_scaled_witnesses"] > 0
    for encoding in (U64, U128):
        for layout in LAYOUTS:
            m = _check_export(batch, oasg, ovals, encoding, layout)
            assert (m == 2).sum() > B  # full-size values: the low bytes, and the mask says so
    for encoding, lead in ((U16, 1), (U64, 4), (U128, 8)):
        d = acvm_amd.DeviceBuffer(size=B * batch.nw * 16 + 16)
        with pytest.raises(acvm_amd.AcvmError, match="error -1: .*aligned"):
            batch.export_device(d.ptr + lead, encoding=encoding)
        d.free()
    batch.free()


def test_export_after_solve_then_import_and_slot_reuse_refuse_as_before():
    n_in, B = 5, 65
    ids = list(range(1, n_in + 1))
    circuit = _tile_circuit(n_in)
    cols = [[(j + c) % 255 + 1 for c in range(n_in)] for j in range(B)]
    buf = acvm_amd.DeviceBuffer(_buffer(cols, U8, WM))
    out = acvm_amd.DeviceBuffer(size=B * (2 * n_in + 2) * 16)
    h = acvm_amd.Batch(circuit, B, ids)
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        h.export_device(out.ptr, encoding=U8)  # not solved
    h.import_device(buf.ptr, encoding=U8, layout=WM)
    assert h.solve(then_import=buf.ptr, then_import_desc=dict(encoding=U8, layout=WM)) == 0
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        h.export_device(out.ptr, encoding=U8)  # the whole map
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        h.export_device(out.ptr, encoding=U8, witnesses=[1])  # an initial witness
    h.export_device(out.ptr, encoding=U64, layout=WM, witnesses=[n_in + 1])  # a gate output is still there
    got = np.frombuffer(out.download(B * 8), dtype="<u8")
    assert list(got) == [3 * r[0] + 1 for r in cols]
    h.free()
    r = acvm_amd.Batch(circuit, B, ids, reuse_slots=True, keep=[n_in + 2])
    r.import_device(buf.ptr, encoding=U8, layout=WM)
    assert r.solve() == 0
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        r.export_device(out.ptr, encoding=U8)
    with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
        r.export_device(out.ptr, encoding=U8, witnesses=[n_in + 3])  # not kept
    r.export_device(out.ptr, encoding=U32, layout=IM, witnesses=[n_in + 2, 1])
    got = np.frombuffer(out.download(B * 8), dtype="<u4").reshape(B, 2)
    assert [list(g) for g in got] == [[3 * row[1] + 1, row[0]] for row in cols]
    for x in (r, buf, out):
        x.free()


def test_digest_bytes_of_batch_a_are_the_inputs_of_batch_b(oracle):
    """A's 64 digest bytes leave as U8 and enter B as U8 without a conversion in between: B's state equals B fed the same bytes through BE32"""
    B = 130
    circ, ids = synth.hash_circuit(n_msg=32)  # 64 byte inputs
    n_in, data = len(ids), circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    a, ores, oasg, ovals = _solved(oracle, data, ids, synth.byte_batch(B, n_in, seed=0xAC1D0716), B)
    assert all(r.status == 0 for r in ores)
    digests = list(range(n_in + 1, n_in + 65))
    rows = [[int(ovals[j, w, 31]) for w in digests] for j in range(B)]
    ref = _be32_state(gc, ids, rows)
    want = _whole_state(ref)
    ref.free()
    b = acvm_amd.Batch(gc, B, ids)
    for layout, stride in ((WM, 0), (IM, 0), (WM, B + 3), (IM, 67)):
        d = acvm_amd.DeviceBuffer(bytes([PATTERN]) * ((stride or max(B, 64)) * max(B, 64)))
        a.export_device(d.ptr, encoding=U8, layout=layout, witnesses=digests, stride=stride)
        b.import_device(d.ptr, encoding=U8, layout=layout, stride=stride)
        d.free()
        assert b.solve() == 0
        _assert_same_state(_whole_state(b), want, f"layout {layout} stride {stride}")
    a.free()
    b.free()
