"""acvm_batch_import_device_masked / acvm_batch_set_initial_witness_masked on the device: per-instance partial initial witness maps. The expected
outcome of every case is the CPU oracle's ACVM fed, instance by instance, with exactly the ids that instance holds; the result tuple, the
assigned set and every assigned value are compared bit for bit.

Shapes: B = 300 crosses the 64-, 128- and 256-instance block edges of the import kernels; 37 initial witnesses cross the 32-bit word of the missing
set and are no multiple of the instance-major group of 4. Wherever no described element lies, value and mask buffers hold a pattern: a value or
a mask byte read from there shows (a pattern byte in the mask is a refusal). The values of absent elements are the pattern too."""
import functools
import random

import numpy as np
import pytest

import acvm_amd
from acvm_amd.acir import BlackBoxFuncCall as BB, Brillig, Circuit, Expression as E, FunctionInput as FI, P

pytestmark = pytest.mark.gpu
BE32, LE32, MONT, U8 = acvm_amd.ENC_BE32, acvm_amd.ENC_LE32, acvm_amd.ENC_MONT256_LE, acvm_amd.ENC_U8
IM, WM = acvm_amd.LAYOUT_INSTANCE_MAJOR, acvm_amd.LAYOUT_WITNESS_MAJOR
FORMS = [(e, l) for e in (BE32, LE32, MONT) for l in (IM, WM)]
PATTERN = 0xA5
B, N_IN = 300, 37
W = E.from_witness


# ---- the circuits: (Circuit, initial ids, values[j][k])
@functools.lru_cache(maxsize=None)
def _circuit(name):
    rng = random.Random(0x3A5C0 + ord(name))
    if name == "a":
        # gates w[37 + k] = 3 w[k] + 1 for k = 1 .. 30; the outputs of gates 1 .. 7 (38 .. 44) are initial ids themselves (positions 30 .. 36): with
        # both present the gate is an assert, with one absent it is solved from the other -- backwards for an absent w[k] -- with both absent it cannot be
        ids = list(range(1, 31)) + list(range(38, 45))
        circ = Circuit(67, [E([], [(3, k), (P - 1, 37 + k)], 1) for k in range(1, 31)])
        vals = []
        for j in range(B):
            x = [rng.randrange(P) if (j + k) % 5 else [0, 1, P - 1, 255, 256][k % 5] for k in range(30)]
            out = [(3 * v + 1) % P for v in x[:7]]
            if j % 50 == 7:
                out[j % 7] = (out[j % 7] + 1) % P  # (an assert that fails where both are present)
            vals.append(x + out)
    elif name == "b":
        # a RANGE on every input, an AND and a SHA256 that read initial witnesses (the message bytes have byte planes)
        ids = list(range(1, N_IN + 1))
        ops = [BB("RANGE", {"input": FI(w, 8)}) for w in ids]
        ops.append(BB("AND", {"lhs": FI(33, 8), "rhs": FI(34, 8), "output": 38}))
        ops.append(BB("SHA256", {"inputs": [FI(w, 8) for w in ids[:32]], "outputs": list(range(39, 71))}))
        ops.append(BB("AND", {"lhs": FI(37, 8), "rhs": FI(1, 8), "output": 71}))
        circ = Circuit(71, ops)
        vals = [[rng.randrange(256) for _ in range(N_IN)] for _ in range(B)]
    else:
        # Brillig opcodes with initial witnesses as inputs (inlined, and through the VM: the backward jump), read-back gates for the other inputs
        ids = list(range(1, N_IN + 1))
        ops = [Brillig(inputs=[W(1), W(2)], outputs=[38], bytecode=[("BinaryFieldOp", 0, "Add", 0, 1), ("Stop",)]),
               Brillig(inputs=[W(32), W(33)], outputs=[39], bytecode=[("BinaryFieldOp", 0, "Mul", 0, 1), ("Const", 1, 0), ("JumpIf", 1, 0), ("Stop",)]),
               Brillig(inputs=[W(36), W(37)], outputs=[40], bytecode=[("BinaryFieldOp", 0, "Sub", 0, 1), ("Stop",)])]
        ops += [E([], [(3, k), (P - 1, 40 + k)], 1) for k in range(3, 32)]
        circ = Circuit(71, ops)
        vals = [[rng.randrange(P) for _ in range(N_IN)] for _ in range(B)]
    return circ, ids, vals


@functools.lru_cache(maxsize=None)
def _device_circuit(name):
    return acvm_amd.Circuit(_circuit(name)[0].to_bytes())


# ---- absence patterns: held[j][k] = 1 where instance j holds the initial witness at position k
@functools.lru_cache(maxsize=None)
def _held(pattern):
    h = np.ones((B, N_IN), dtype=np.uint8)
    if pattern.startswith("pos"):       # one position, a third of the instances
        h[::3, int(pattern[3:])] = 0
    elif pattern == "one-instance":      # every position of one instance
        h[77, :] = 0
    elif pattern == "edges":             # the first and last instances of the import kernels' blocks
        for j in (0, 63, 64, 255, 256, 299):
            h[j, (5 * j) % N_IN] = 0
    elif pattern == "everyone":          # every instance lacks something
        for j in range(B):
            h[j, j % N_IN] = 0
            if j % 4 == 0:
                h[j, (j + 30) % N_IN] = 0
    elif pattern == "random":            # a seeded 10 % of the elements
        h = (np.random.default_rng(0x3A5C7).random((B, N_IN)) >= 0.10).astype(np.uint8)
    else:
        assert pattern == "none"
    h.setflags(write=False)
    return h


PATTERNS = ["none", "pos0", "pos31", "pos32", "pos36", "one-instance", "edges", "everyone", "random"]


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import binding
    binding.build()
    binding.lib()
    return binding


# ---- the oracle's answer, once per (circuit, pattern)
@functools.lru_cache(maxsize=None)
def _expected(name, pattern):
    ob = _oracle()
    circ, ids, vals = _circuit(name)
    held = _held(pattern)
    oc = ob.Circuit(circ.to_bytes())
    nw = oc.num_witnesses
    res, asg, values = [], np.zeros((B, nw), dtype=np.uint8), np.zeros((B, nw, 32), dtype=np.uint8)
    for j in range(B):
        a = ob.ACVM(oc, {ids[k]: vals[j][k] for k in range(N_IN) if held[j, k]})
        a.solve()
        res.append(a.result().as_tuple())
        for w, v in a.witness_map().items():
            asg[j, w] = 1
            values[j, w] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    return res, asg, values


def _assert_expected(batch, name, pattern, what):
    res, asg, values = _expected(name, pattern)
    got = [r.as_tuple() for r in batch.results()]
    bad = [j for j in range(B) if got[j] != res[j]]
    assert not bad, f"{what}: instance {bad[0]} is {got[bad[0]]}, the oracle's {res[bad[0]]} ({len(bad)} differ)"
    gasg, gvals = batch.witness_map()
    nw = asg.shape[1]
    assert gasg.shape[1] >= nw and not gasg[:, nw:].any(), what
    wrong = np.argwhere(gasg[:, :nw] != asg)
    assert wrong.size == 0, f"{what}: witness {wrong[0][1]} of instance {wrong[0][0]} is assigned {gasg[wrong[0][0], wrong[0][1]]}, the oracle's {asg[wrong[0][0], wrong[0][1]]}"
    wrong = np.argwhere(((gvals[:, :nw] != values).any(axis=2)) & (asg == 1))
    assert wrong.size == 0, f"{what}: witness {wrong[0][1]} of instance {wrong[0][0]} differs from the oracle's"


# ---- buffers
def _element_bytes(v, encoding):
    if encoding == BE32:
        return v.to_bytes(32, "big")
    if encoding == LE32:
        return v.to_bytes(32, "little")
    if encoding == MONT:
        return ((v << 256) % P).to_bytes(32, "little")
    return v.to_bytes(1 << (encoding - U8), "little")


def _laid_out(arr, layout, stride):
    """arr [n][n_columns][size] -> the bytes of the buffer, PATTERN wherever no element lies"""
    n, n_columns, size = arr.shape
    rows, dense = (n_columns, n) if layout == WM else (n, n_columns)
    stride = stride or dense
    assert stride >= dense
    buf = np.full((rows, stride, size), PATTERN, dtype=np.uint8)
    buf[:, :dense] = arr.transpose(1, 0, 2) if layout == WM else arr
    return buf.tobytes()


def _buffers(vals, held, encoding, layout, columns=None, n_columns=None, stride=0):
    """(value bytes, mask bytes) of the batch; input k in column columns[k]; absent elements and unused columns hold PATTERN in both"""
    size = 32 if encoding < U8 else 1 << (encoding - U8)
    cols = list(range(N_IN)) if columns is None else columns
    n_columns = N_IN if columns is None else n_columns
    v = np.full((B, n_columns, size), PATTERN, dtype=np.uint8)
    m = np.full((B, n_columns, 1), PATTERN, dtype=np.uint8)
    for j in range(B):
        for k in range(N_IN):
            m[j, cols[k], 0] = held[j, k]
            if held[j, k]:
                v[j, cols[k]] = np.frombuffer(_element_bytes(vals[j][k], encoding), dtype=np.uint8)
    return _laid_out(v, layout, stride), _laid_out(m, layout, stride)


def _import(batch, name, pattern, encoding, layout, columns=None, n_columns=None, stride=0, mask_offset=0):
    values, mask = _buffers(_circuit(name)[2], _held(pattern), encoding, layout, columns, n_columns, stride)
    dv, dm = acvm_amd.DeviceBuffer(values), acvm_amd.DeviceBuffer(bytes(mask_offset) + mask)
    try:
        batch.import_device(dv.ptr, encoding=encoding, layout=layout, columns=columns, n_columns=n_columns, stride=stride, d_assigned=dm.ptr + mask_offset)
    finally:
        dv.free()
        dm.free()


def _n_missing(pattern):
    return int((_held(pattern) == 0).any(axis=1).sum())


@pytest.fixture(scope="module")
def batches():
    made = {}

    def get(name):
        if name not in made:
            made[name] = acvm_amd.Batch(_device_circuit(name), B, _circuit(name)[1])
        return made[name]
    yield get
    for b in made.values():
        b.free()


# ---- 1. every absence pattern, every 32-byte encoding x both layouts (the forms rotate over the patterns; test 2 runs all six on one pattern)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_absence_patterns_against_the_oracle(batches, pattern):
    batch = batches("a")
    q = PATTERNS.index(pattern)
    for encoding, layout in (FORMS[q % 6], FORMS[(q + 3) % 6]):
        _import(batch, "a", pattern, encoding, layout, mask_offset=q % 3)
        assert batch.import_missing() == _n_missing(pattern)
        batch.solve()
        _assert_expected(batch, "a", pattern, f"pattern {pattern} encoding {encoding} layout {layout}")
        if pattern == "none":  # nothing absent: no exact lane but the instances whose assert fails, exactly as the unmasked import
            want = ([r.as_tuple() for r in batch.results()], batch.stats()["n_slow_instances"])
            values, _ = _buffers(_circuit("a")[2], _held("none"), encoding, layout)
            dv = acvm_amd.DeviceBuffer(values)
            batch.import_device(dv.ptr, encoding=encoding, layout=layout)
            dv.free()
            batch.solve()
            assert ([r.as_tuple() for r in batch.results()], batch.stats()["n_slow_instances"]) == want
            assert want[1] == sum(r[0] != 0 for r in want[0]) == B // 50


@pytest.mark.parametrize("name", ["b", "c"])
def test_nothing_absent_is_the_unmasked_import(batches, name):
    """a mask of all ones: nobody is missing anything, no instance takes the exact path, and the outcome is the unmasked import's"""
    batch = batches(name)
    states = []
    for masked in (True, False):
        values, mask = _buffers(_circuit(name)[2], _held("none"), MONT, WM)
        dv, dm = acvm_amd.DeviceBuffer(values), acvm_amd.DeviceBuffer(mask)
        batch.import_device(dv.ptr, encoding=MONT, layout=WM, d_assigned=dm.ptr if masked else None)
        dv.free()
        dm.free()
        assert batch.import_missing() == 0
        assert batch.solve() == 0
        assert batch.stats()["n_slow_instances"] == 0
        _assert_expected(batch, name, "none", f"circuit {name}, mask of ones" if masked else f"circuit {name}, unmasked")
        states.append(([r.as_tuple() for r in batch.results()],) + batch.witness_map())
    assert states[0][0] == states[1][0] and np.array_equal(states[0][1], states[1][1]) and np.array_equal(states[0][2], states[1][2])


@pytest.mark.parametrize("encoding,layout", FORMS)
def test_every_encoding_and_layout(batches, encoding, layout):
    batch = batches("a")
    _import(batch, "a", "random", encoding, layout, mask_offset=1)
    assert batch.import_missing() == _n_missing("random")
    batch.solve()
    _assert_expected(batch, "a", "random", f"encoding {encoding} layout {layout}")


# ---- 2. black-box opcodes and Brillig: MissingAssignment of the right witness at the right opcode
@pytest.mark.parametrize("name", ["b", "c"])
@pytest.mark.parametrize("pattern", ["everyone", "random", "pos31"])
def test_black_box_and_brillig_inputs(batches, name, pattern):
    batch = batches(name)
    encoding, layout = FORMS[(PATTERNS.index(pattern) + ord(name)) % 6]
    _import(batch, name, pattern, encoding, layout)
    batch.solve()
    _assert_expected(batch, name, pattern, f"circuit {name} pattern {pattern} encoding {encoding} layout {layout}")
    res = _expected(name, pattern)[0]
    assert any(r[0] != 0 for r in res) and (pattern == "everyone" or any(r[0] == 0 for r in res))


def test_narrow_encoding(batches):
    batch = batches("b")
    for layout in (IM, WM):
        _import(batch, "b", "random", U8, layout, mask_offset=3)
        batch.solve()
        _assert_expected(batch, "b", "random", f"U8 layout {layout}")


# ---- 3. strides, column lists, the host form
@pytest.mark.parametrize("layout", [IM, WM])
def test_stride_above_dense_and_permuted_columns(batches, layout):
    batch = batches("a")
    _import(batch, "a", "random", LE32, layout, stride=(B if layout == WM else N_IN) + 11)
    batch.solve()
    _assert_expected(batch, "a", "random", f"padded stride, layout {layout}")
    perm = [(5 * k + 3) % (N_IN + 4) for k in range(N_IN)]  # input k lies in column perm[k] of 41
    assert len(set(perm)) == N_IN
    _import(batch, "a", "everyone", MONT, layout, columns=perm, n_columns=N_IN + 4, stride=(B if layout == WM else N_IN + 4) + 3)
    batch.solve()
    _assert_expected(batch, "a", "everyone", f"column list, layout {layout}")


def _host_form(batch, name, pattern):
    values, mask = _buffers(_circuit(name)[2], _held(pattern), BE32, IM)
    batch.set_initial_witness_masked(values, mask)


def test_host_form(batches):
    batch = batches("a")
    _host_form(batch, "a", "random")
    assert batch.import_missing() == _n_missing("random")
    batch.solve()
    _assert_expected(batch, "a", "random", "host form")


# ---- 4. the other ways through a solve
def test_forced_slow_path():
    batch = acvm_amd.Batch(_device_circuit("a"), B, _circuit("a")[1])
    batch.set_force_slow_path(True)
    _import(batch, "a", "random", MONT, WM)
    batch.solve()
    _assert_expected(batch, "a", "random", "forced slow path")
    batch.free()


def test_stepping_to_the_end():
    batch = acvm_amd.Batch(_device_circuit("a"), B, _circuit("a")[1])
    _import(batch, "a", "everyone", BE32, IM)
    for _ in range(len(_circuit("a")[0].opcodes)):
        batch.solve_opcode()
    _assert_expected(batch, "a", "everyone", "stepping")
    batch.free()


def test_reuse_slots_handle():
    """the rows of the initial witnesses are the plan's, the exact lanes start over in the side table; what can be read back under slot reuse is
    the results, the digests and the kept witnesses"""
    ob = _oracle()
    circ, ids, _ = _circuit("b")
    keep = [38, 39, 70, 71]
    batch = acvm_amd.Batch(_device_circuit("b"), B, ids, reuse_slots=True, keep=keep)
    for pattern, (encoding, layout) in (("random", (LE32, WM)), ("pos31", (MONT, IM))):
        _import(batch, "b", pattern, encoding, layout)
        batch.solve()
        res, asg, values = _expected("b", pattern)
        assert [r.as_tuple() for r in batch.results()] == res, pattern
        dig = batch.digest()
        for j in range(B):
            assert bytes(dig[j]) == ob.witness_map_digest(asg[j], values[j]), (pattern, j)
        solved = [j for j in range(B) if res[j][0] == 0]
        assert solved or pattern == "random"
        for j in solved[:3] + solved[-3:]:
            assert np.array_equal(batch.extract(keep + ids, first=j, n=1)[0], values[j][keep + ids]), (pattern, j)
    batch.free()


# ---- 5. sequences on one handle
def test_masked_then_unmasked_import():
    circ, ids, vals = _circuit("a")
    batch = acvm_amd.Batch(_device_circuit("a"), B, ids)
    _import(batch, "a", "random", MONT, IM)
    batch.solve()
    _assert_expected(batch, "a", "random", "masked")
    values, _ = _buffers(vals, _held("none"), MONT, IM)
    dv = acvm_amd.DeviceBuffer(values)
    batch.import_device(dv.ptr, encoding=MONT, layout=IM)
    assert batch.import_missing() == 0
    batch.solve()
    _assert_expected(batch, "a", "none", "unmasked behind masked")
    fresh = acvm_amd.Batch(_device_circuit("a"), B, ids)
    fresh.import_device(dv.ptr, encoding=MONT, layout=IM)
    fresh.solve()
    assert [r.as_tuple() for r in batch.results()] == [r.as_tuple() for r in fresh.results()]
    assert batch.stats()["n_slow_instances"] == fresh.stats()["n_slow_instances"]
    for x, y in zip(batch.witness_map(), fresh.witness_map()):
        assert np.array_equal(x, y)
    for x in (dv, batch, fresh):
        x.free()


def test_masked_import_solve_reset_solve():
    batch = acvm_amd.Batch(_device_circuit("a"), B, _circuit("a")[1])
    _import(batch, "a", "everyone", LE32, WM)
    batch.solve()
    _assert_expected(batch, "a", "everyone", "first solve")
    first = ([r.as_tuple() for r in batch.results()],) + batch.witness_map()
    batch.reset()
    assert batch.import_missing() == B
    batch.solve()
    _assert_expected(batch, "a", "everyone", "solve behind reset")
    assert [r.as_tuple() for r in batch.results()] == first[0]
    for x, y in zip(batch.witness_map(), first[1:]):
        assert np.array_equal(x, y)
    batch.free()


# ---- 6. refusals
@pytest.mark.parametrize("byte", [2, 255])
def test_bad_mask_bytes_fail_closed(byte):
    circ, ids, vals = _circuit("a")
    batch = acvm_amd.Batch(_device_circuit("a"), B, ids)
    _import(batch, "a", "pos0", BE32, WM)  # a good import first: the refusal below takes it away
    for layout in (IM, WM):
        values, mask = _buffers(vals, _held("random"), BE32, layout)
        m = np.frombuffer(mask, dtype=np.uint8).copy()
        for j, k in ((200, 5), (64, 36), (64, 3), (299, 0)):
            m[k * B + j if layout == WM else j * N_IN + k] = byte
        dv, dm = acvm_amd.DeviceBuffer(values), acvm_amd.DeviceBuffer(m.tobytes())
        with pytest.raises(acvm_amd.AcvmError, match=rf"error -1: .*\b4 elements .*instance 64, position 3 \(initial witness {ids[3]}\)"):
            batch.import_device(dv.ptr, layout=layout, d_assigned=dm.ptr)
        with pytest.raises(acvm_amd.AcvmError, match="error -5: "):
            batch.solve()
        dv.free()
        dm.free()
        _import(batch, "a", "random", BE32, layout)  # a following good import solves
        batch.solve()
        _assert_expected(batch, "a", "random", f"after the refused byte {byte}, layout {layout}")
    batch.free()


def test_descriptor_refusals_leave_the_handle_as_it_was():
    circ, ids, vals = _circuit("a")
    batch = acvm_amd.Batch(_device_circuit("a"), B, ids)
    _import(batch, "a", "edges", LE32, IM)
    buf = acvm_amd.DeviceBuffer(size=(B + 8) * (N_IN + 8) * 32 + 16)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*stride"):
        batch.import_device(buf.ptr, layout=IM, stride=N_IN - 1, d_assigned=buf.ptr)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*stride"):
        batch.import_device(buf.ptr, layout=WM, stride=B - 1, d_assigned=buf.ptr)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*aligned"):
        batch.import_device(buf.ptr + 8, encoding=LE32, d_assigned=buf.ptr)
    with pytest.raises(acvm_amd.AcvmError, match="error -1: .*column"):
        batch.import_device(buf.ptr, columns=list(range(N_IN - 1)) + [N_IN + 9], n_columns=N_IN + 4, d_assigned=buf.ptr)
    buf.free()
    assert batch.import_missing() == 6
    batch.solve()
    _assert_expected(batch, "a", "edges", "after the refusals")
    batch.free()


def test_null_mask_is_the_unmasked_import():
    circ, ids, vals = _circuit("a")
    batch = acvm_amd.Batch(_device_circuit("a"), B, ids)
    values, _ = _buffers(vals, _held("none"), LE32, WM)
    dv = acvm_amd.DeviceBuffer(values)
    batch.import_device(dv.ptr, encoding=LE32, layout=WM, d_assigned=None)
    assert batch.import_missing() == 0
    batch.solve()
    _assert_expected(batch, "a", "none", "d_assigned=None")
    batch.import_device_masked(dv.ptr, None, encoding=LE32, layout=WM)
    batch.solve()
    _assert_expected(batch, "a", "none", "import_device_masked(d_assigned=None)")
    desc, _keep = batch._import_desc(LE32, WM)
    import ctypes as C
    assert acvm_amd.lib().acvm_batch_import_device_masked(batch._h, C.byref(desc), dv.ptr, None) == 0
    batch.solve()
    _assert_expected(batch, "a", "none", "acvm_batch_import_device_masked(NULL)")
    dv.free()
    batch.free()


# ---- 7. two circuits on the device: A's export, whole map and mask, is B's masked import
def test_pipeline_of_two_circuits_on_the_device():
    ob = _oracle()
    n, stride = 130, 192
    # A: w4 = w1 w2 + w3; assert w3 = 5 (fails for a third); w5 = w4^2 + 7; w6 = w4 + w1
    circ_a = Circuit(6, [E([(1, 1, 2)], [(1, 3), (P - 1, 4)], 0), E([], [(1, 3)], P - 5), E([(1, 4, 4)], [(P - 1, 5)], 7), E([], [(1, 4), (1, 1), (P - 1, 6)], 0)])
    ids_a = [1, 2, 3]
    rng = random.Random(0x3A5C9)
    rows = [[rng.randrange(P), rng.randrange(P), 5 if j % 3 else 6] for j in range(n)]
    # B reads A's w4, w5, w6 as its w1, w2, w3: w4 = 2 w1 + 1; w5 = w2 + w1; w6 = w3 w1
    circ_b = Circuit(6, [E([], [(2, 1), (P - 1, 4)], 1), E([], [(1, 2), (1, 1), (P - 1, 5)], 0), E([(1, 3, 1)], [(P - 1, 6)], 0)])
    ids_b, picked = [1, 2, 3], [4, 5, 6]
    oa, obc = ob.Circuit(circ_a.to_bytes()), ob.Circuit(circ_b.to_bytes())
    want = []
    for j in range(n):
        a = ob.ACVM(oa, dict(zip(ids_a, rows[j])))
        a.solve()
        map_a = a.witness_map()
        assert (a.result().status != 0) == (j % 3 == 0) and (5 in map_a) == (j % 3 != 0)
        b = ob.ACVM(obc, {ids_b[k]: map_a[picked[k]] for k in range(3) if picked[k] in map_a})
        b.solve()
        want.append((b.result().as_tuple(), b.witness_map()))
    ga = acvm_amd.Batch(acvm_amd.Circuit(circ_a.to_bytes()), n, ids_a)
    ga.set_initial_witness(b"".join(v.to_bytes(32, "big") for r in rows for v in r))
    assert ga.solve() == (n + 2) // 3
    d_vals, d_mask = acvm_amd.DeviceBuffer(bytes([PATTERN]) * (ga.nw * stride * 32)), acvm_amd.DeviceBuffer(bytes([PATTERN]) * (ga.nw * stride))
    ga.export_device(d_vals.ptr, encoding=MONT, layout=WM, stride=stride, d_assigned=d_mask.ptr)
    gb = acvm_amd.Batch(acvm_amd.Circuit(circ_b.to_bytes()), n, ids_b)
    gb.import_device(d_vals.ptr, encoding=MONT, layout=WM, columns=picked, n_columns=ga.nw, stride=stride, d_assigned=d_mask.ptr)
    assert gb.import_missing() == (n + 2) // 3
    gb.solve()
    res = [r.as_tuple() for r in gb.results()]
    asg, vals = gb.witness_map()
    for j in range(n):
        assert res[j] == want[j][0], (j, res[j], want[j][0])
        assert {w for w in range(asg.shape[1]) if asg[j, w]} == set(want[j][1]), j
        for w, v in want[j][1].items():
            assert bytes(vals[j, w]) == v.to_bytes(32, "big"), (j, w)
    assert any(r[0] != 0 for r in res) and any(r[0] == 0 for r in res)
    for x in (d_vals, d_mask, ga, gb):
        x.free()
