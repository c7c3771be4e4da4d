"""Device-resident outcomes: acvm_batch_outcomes_device (status columns and the ordered selection), acvm_batch_export_device_list (the map of
listed instances) and the selection probe acvm_debug_select, on the device. Outcomes are compared field by field with acvm_batch_results and
with the CPU oracle; exported maps bit for bit with the oracle's maps converted with Python integers and with rows of the range export of the
same handle. Every output buffer is pre-filled with a pattern, and everything outside the described elements must still hold it."""
import random

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import P, Brillig, Circuit, Expression as E
from acvm_amd.synth import values_from_rows

pytestmark = pytest.mark.gpu
M1 = P - 1
W = E.from_witness
WIDE = (acvm_amd.ENC_BE32, acvm_amd.ENC_LE32, acvm_amd.ENC_MONT256_LE)
NARROW = (acvm_amd.ENC_U8, acvm_amd.ENC_U16, acvm_amd.ENC_U32, acvm_amd.ENC_U64, acvm_amd.ENC_U128)
ENCODINGS = WIDE + NARROW
IM, WM = acvm_amd.LAYOUT_INSTANCE_MAJOR, acvm_amd.LAYOUT_WITNESS_MAJOR
LAYOUTS = (IM, WM)
PATTERN, TAIL = 0xA5, 96
PATTERN32 = 0xA5A5A5A5
SOLVED, IN_PROGRESS, FAILURE, WAITING = (acvm_amd.STATUS_SOLVED, acvm_amd.STATUS_IN_PROGRESS, acvm_amd.STATUS_FAILURE,
                                         acvm_amd.STATUS_REQUIRES_FOREIGN_CALL)
SPAN = 1024  # elements per block of the selection (select_scan.hpp SELECT_SPAN; tests/test_select_on_host.py reads it from the header)


def SIZE(encoding):
    return 32 if encoding < 16 else 1 << (encoding - 16)


# ------------------------------------------------------------------------------------------------ 1. the selection kernels on any pattern
def _patterns(n, rng):
    yield "none", [0] * n
    yield "all", [2] * n
    yield "alternating", [2 * (i & 1) for i in range(n)]
    yield "first", [2 if i == 0 else 0 for i in range(n)]
    yield "last", [2 if i == n - 1 else 0 for i in range(n)]
    yield "random", [rng.choice((0, 2)) for _ in range(n)]


def _select_case(st, mask):
    n = len(st)
    want = np.array([i for i, s in enumerate(st) if s < 32 and (mask >> s) & 1], dtype=np.uint32)
    st = np.asarray(st, dtype=np.uint8)
    got, count = acvm_amd.debug_select(st, mask, out=np.full(n, PATTERN32, dtype=np.uint32))
    assert count == want.size, (n, mask)
    assert np.array_equal(got[:count], want), (n, mask)
    assert (got[count:] == PATTERN32).all(), (n, mask)
    assert acvm_amd.debug_select(st, mask, want_list=False)[1] == want.size  # the count alone


def test_select_against_numpy_nonzero():
    rng = random.Random(0x5E1EC7)
    for n in list(range(0, 301)) + [SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 1]:
        for _, st in _patterns(n, rng):
            _select_case(st, 1 << 2)


def test_select_masks_over_status_bytes():
    rng = random.Random(0x5E1EC8)
    for n in (1, 63, 64, 65, 300, SPAN + 1, 3 * SPAN + 1):
        st = [rng.randrange(4) for _ in range(n)]
        for mask in (1, 2, 4, 8, 0b1101):
            _select_case(st, mask)
    _select_case([0, 32, 33, 255, 3, 1] * 50, 0xFFFFFFFF)  # a status byte of 32 or more is selected by nothing


def test_select_scan_carries_across_steps():
    """more blocks than one step of select_scan_kernel takes (256 totals per step): the running carry and the re-use of its LDS sums. Two steps with
    one block in the second, and three steps with a ragged last block"""
    rng = np.random.default_rng(0x5E1EC9)
    for n in (256 * SPAN + 1, 2 * 256 * SPAN + SPAN + 77):
        for st in (np.full(n, 2, dtype=np.uint8), rng.integers(0, 4, size=n, dtype=np.uint8), (np.arange(n) == n - 1).astype(np.uint8) * 2):
            want = np.nonzero(st == 2)[0].astype(np.uint32)
            got, count = acvm_amd.debug_select(st, 1 << 2, out=np.full(n, PATTERN32, dtype=np.uint32))
            assert count == want.size, n
            assert np.array_equal(got[:count], want) and (got[count:] == PATTERN32).all(), n


# ------------------------------------------------------------------------------------------------ 2. outcomes on a real batch
def _check_outcomes(batch, want, first, n, mask, null=()):
    """want: (status, err, opcode_index) per instance of the batch; null: names of the descriptor's pointers left NULL"""
    bufs = {"d_status": acvm_amd.DeviceBuffer(bytes([PATTERN]) * (n + TAIL)), "d_err": acvm_amd.DeviceBuffer(bytes([PATTERN]) * (n + TAIL)),
            "d_opcode_index": acvm_amd.DeviceBuffer(bytes([PATTERN]) * 4 * (n + TAIL)), "d_selected": acvm_amd.DeviceBuffer(bytes([PATTERN]) * 4 * (n + TAIL))}
    try:
        ptr = {k: (None if k in null else v.ptr) for k, v in bufs.items()}
        count = batch.outcomes_device(first=first, n=n, select_mask=mask, count="count" not in null, **ptr)
        what = f"first {first} n {n} mask {mask} null {null}"
        w = np.array(want[first:first + n], dtype=np.int64).reshape(n, 3)
        got = {"d_status": np.frombuffer(bufs["d_status"].download(), dtype=np.uint8), "d_err": np.frombuffer(bufs["d_err"].download(), dtype=np.uint8),
               "d_opcode_index": np.frombuffer(bufs["d_opcode_index"].download(), dtype=np.uint32),
               "d_selected": np.frombuffer(bufs["d_selected"].download(), dtype=np.uint32)}
        for col, name in enumerate(("d_status", "d_err", "d_opcode_index")):
            pat = PATTERN32 if name == "d_opcode_index" else PATTERN
            if name in null:
                assert (got[name] == pat).all(), f"{what}: {name} was written"
                continue
            assert np.array_equal(got[name][:n].astype(np.int64), w[:, col]), f"{what}: {name} differs: {got[name][:n]} != {w[:, col]}"
            assert (got[name][n:] == pat).all(), f"{what}: {name} written behind n"
        sel = [first + i for i in range(n) if (mask >> int(w[i, 0])) & 1]
        if "count" not in null:
            assert count == len(sel), what
        if "d_selected" in null:
            assert (got["d_selected"] == PATTERN32).all(), what
        else:
            assert list(got["d_selected"][:len(sel)]) == sel, what
            assert (got["d_selected"][len(sel):] == PATTERN32).all(), f"{what}: d_selected written behind the count"
    finally:
        for v in bufs.values():
            v.free()


def _sweep(batch, want, masks):
    """every sub-range of the issue with every pointer given, then each pointer NULL in turn"""
    B = batch.B
    k = 0
    for first in (0, 1, 64):
        for n in (1, 63, 64, 65, B - first):
            _check_outcomes(batch, want, first, n, masks[k % len(masks)])
            k += 1
    for name in ("d_status", "d_err", "d_opcode_index", "d_selected", "count"):
        _check_outcomes(batch, want, 1, 65, masks[0], null=(name,))
        _check_outcomes(batch, want, 0, B, masks[-1], null=(name,))
    _check_outcomes(batch, want, 0, B, masks[0], null=("d_status", "d_err", "d_opcode_index", "d_selected"))  # the count alone
    _check_outcomes(batch, want, 0, B, masks[0], null=("d_selected", "count"))  # no selection
    _check_outcomes(batch, want, B, 0, masks[0])  # an empty range at the end is a range


def _triples(results):
    return [(r.status, r.err, r.opcode_index) for r in results]


OUT_B = 200
OUT_FAIL = sorted({0, 63, 64, 65, 199} | set(random.Random(0x0C0DE5).sample(range(OUT_B), 9)))
OUT_ZERO_SOLVED, OUT_ZERO_FAILED = 7, 8  # zero denominators: the gate holds without assigning (Solved on the exact path) / does not hold


def _outcomes_circuit():
    """w4 = w1 w2; assert w4 == w6 (w6 is an input: it decides satisfaction); w5 = w4 / w3 (w3 == 0: the instance leaves the generic path); w7 = w4 + w3"""
    circ = Circuit(7, [E([(1, 1, 2)], [(M1, 4)], 0), E([], [(1, 4), (M1, 6)], 0), E([(1, 3, 5)], [(M1, 4)], 0), E([], [(1, 4), (1, 3), (M1, 7)], 0)])
    ids = [1, 2, 3, 6]
    rows = []
    for j in range(OUT_B):
        a, b, c = 3 + j, 7 * j + 2, j + 1
        rows.append([a, b, c, a * b + (1 if j in OUT_FAIL and j not in (OUT_ZERO_SOLVED, OUT_ZERO_FAILED) else 0)])
    rows[OUT_ZERO_SOLVED] = [0, 5, 0, 0]
    rows[OUT_ZERO_FAILED] = [2, 3, 0, 6]
    return circ.to_bytes(), ids, values_from_rows(rows)


@pytest.fixture(scope="module")
def outcomes_ref(oracle):
    data, ids, values = _outcomes_circuit()
    ores, _, _ = oracle.solve_batch(oracle.Circuit(data), ids, values, OUT_B, want_witness=False)
    want = _triples(ores)
    failed = (set(OUT_FAIL) | {OUT_ZERO_FAILED}) - {OUT_ZERO_SOLVED}
    assert [j for j in range(OUT_B) if want[j][0] == FAILURE] == sorted(failed) and all(want[j] == (SOLVED, 0, 0) for j in range(OUT_B) if j not in failed)
    assert {want[j][2] for j in failed} == {1, 2}  # the assert gate and the division
    return data, ids, values, want


MASKS = (1 << SOLVED, 1 << FAILURE, (1 << SOLVED) | (1 << FAILURE), 1 << WAITING, 1 << IN_PROGRESS, 0)


@pytest.mark.parametrize("mode", ["plain", "force_slow", "reuse_slots"])
def test_outcomes_equal_results_and_the_oracle(outcomes_ref, mode):
    data, ids, values, want = outcomes_ref
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), OUT_B, ids, **({"reuse_slots": True, "keep": [7]} if mode == "reuse_slots" else {}))
    batch.set_force_slow_path(mode == "force_slow")
    batch.set_initial_witness(values)
    batch.solve()
    n_slow = batch.stats()["n_slow_instances"]
    assert n_slow == OUT_B if mode == "force_slow" else 1 <= n_slow < OUT_B  # (the zero denominator ends Solved ON the exact path)
    assert _triples(batch.results()) == want
    _sweep(batch, want, MASKS)
    h2d = batch.export_h2d_bytes()
    batch.outcomes_device(select_mask=1)
    assert batch.export_h2d_bytes() - h2d <= 16 * n_slow  # the exact lanes' records and nothing else
    batch.free()


def test_outcomes_after_solve_opcode_steps(outcomes_ref):
    data, ids, values, want = outcomes_ref
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), OUT_B, ids)
    batch.set_initial_witness(values)
    for _ in range(2):
        batch.solve_opcode()
        stepped = _triples(batch.results())
        _check_outcomes(batch, stepped, 0, OUT_B, 1 << IN_PROGRESS)
        _check_outcomes(batch, stepped, 64, 65, 1 << FAILURE)
    assert any(t[0] == IN_PROGRESS for t in stepped) and any(t[0] == FAILURE for t in stepped)
    batch.solve()
    assert _triples(batch.results()) == want
    _sweep(batch, want, MASKS)
    batch.free()


def test_outcomes_not_solved_range_and_descriptor_refusals(outcomes_ref):
    data, ids, values, want = outcomes_ref
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), OUT_B, ids)
    d = acvm_amd.DeviceBuffer(size=OUT_B * 4)
    with pytest.raises(acvm_amd.AcvmError, match="not solved"):
        batch.outcomes_device(d_status=d.ptr)
    batch.set_initial_witness(values)
    batch.solve()
    with pytest.raises(acvm_amd.AcvmError, match="out of bounds"):
        batch.outcomes_device(first=OUT_B - 1, n=2, d_status=d.ptr)
    with pytest.raises(acvm_amd.AcvmError, match="nothing to write"):
        batch.outcomes_device(count=False)
    d.free()
    batch.free()


def test_outcomes_with_instances_waiting_at_a_foreign_call(oracle):
    """the circuit of tests/test_gpu_foreign_call.py: instances that fail early, instances that never wait, instances waiting inside a Brillig opcode"""
    br = Brillig(inputs=[W(1), E(), W(2)], outputs=[5, 6, 7, 8],
                 bytecode=[("ForeignCall", "invert", [("Register", 1)], [("Register", 0)]),
                           ("ForeignCall", "invert", [("Register", 3)], [("Register", 2)])], predicate=W(3))
    circ = Circuit(10, [E([(1, 1, 2)], [(M1, 4)], 0), E([], [(1, 4), (M1, 9)], 1), br, E([(1, 1, 6)], [(M1, 10)], 0)])
    ids = [1, 2, 3]
    rows = [[3 + j, 7 * j + 1, 1 if j % 4 else 0] for j in range(OUT_B)]
    data = circ.to_bytes()
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), OUT_B, ids)
    batch.set_initial_witness(values_from_rows(rows))
    batch.solve()
    want = _triples(batch.results())
    for j in range(OUT_B):  # acvm_result_t.opcode_index of a waiting instance is the oracle's instruction pointer
        a = oracle.ACVM(oracle.Circuit(data), dict(zip(ids, rows[j])))
        a.solve()
        o = a.result().as_tuple()
        assert want[j] == (o[0], o[1], a.instruction_pointer() if o[0] == oracle.ST_REQUIRES_FOREIGN_CALL else o[2]), j
    assert sum(t[0] == WAITING for t in want) >= OUT_B // 2
    _sweep(batch, want, (1 << WAITING, 1 << SOLVED, (1 << WAITING) | (1 << FAILURE)))
    batch.free()


def test_outcomes_after_solve_then_import(oracle):
    B = 130
    circ = Circuit(5, [E([(1, 1, 2)], [(M1, 3)], 0), E([], [(1, 3), (1, 4), (M1, 5)], 0)])
    ids = [1, 2, 4]
    values = values_from_rows([[j + 2, 3 * j + 1, j + 9] for j in range(B)])
    nxt = values_from_rows([[j + 5, 7 * j + 1, j] for j in range(B)])
    batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
    d_in, d_next = acvm_amd.DeviceBuffer(values), acvm_amd.DeviceBuffer(nxt)
    batch.set_initial_witness_device(d_in.ptr)
    assert batch.solve(then_import=d_next.ptr) == 0
    want = _triples(batch.results())
    assert want == [(SOLVED, 0, 0)] * B
    _check_outcomes(batch, want, 0, B, 1 << SOLVED)
    _check_outcomes(batch, want, 1, 65, 1 << FAILURE)
    for x in (d_in, d_next):
        x.free()
    batch.free()


# ------------------------------------------------------------------------------------------------ 3. the list export
LIST_B = 200
LENGTHS = (1, 63, 64, 65, 200)
KINDS = ("identity", "descending", "repeats", "exact", "out_of_range")


class ListRef:
    """one solved handle, the oracle's maps of its batch and, per encoding, every element of the batch as the export must write it (row B: an instance
    that assigned nothing -- what an out-of-range list entry reads as). The ones of the `arith` fixture are computed once and shared, and no test
    solves, imports into or otherwise modifies their handle; a test that must do so builds a ListRef of its own with like=<the shared one>, which
    takes over the oracle's answer and the exact set and solves a fresh handle."""

    def __init__(self, oracle, circ, ids, values, B, like=None, **kw):
        data = circ.to_bytes()
        self.solved = like.solved if like is not None else oracle.solve_batch(oracle.Circuit(data), ids, values, B)
        self.ores, oasg, ovals = self.solved
        force_slow = kw.pop("force_slow", False)
        self.batch = acvm_amd.Batch(acvm_amd.Circuit(data), B, ids, **kw)
        self.batch.set_force_slow_path(force_slow)
        self.batch.set_initial_witness(values)
        self.batch.solve()
        self.B, self.nw = B, self.batch.nw
        self.NW = self.nw + 8  # columns behind the circuit's witnesses: a listed index beyond the circuit is unassigned
        self.asg = np.zeros((B + 1, self.NW), dtype=np.uint8)
        self.be = np.zeros((B + 1, self.NW, 32), dtype=np.uint8)
        k = min(self.nw, oasg.shape[1])
        self.asg[:B, :k] = oasg[:, :k]
        self.be[:B, :k] = ovals[:, :k]
        self.be[self.asg == 0] = 0
        self.tables, self.ranges = {}, {}
        # the instances of the exact path, from the solver's own statistics and nothing of the exports: whether an instance leaves the generic path
        # depends on its inputs alone, so it is one iff a batch of that instance alone counts one. witness_batch plants its edge cases in instances
        # 0 .. 7; that none sits further back is what the comparison with this batch's count says
        if like is not None:
            self.exact = list(like.exact)
        elif force_slow:
            self.exact = list(range(B))
        else:
            self.exact = []
            gc, per = acvm_amd.Circuit(data), len(values) // B
            for j in range(min(B, 16)):
                one = acvm_amd.Batch(gc, 1, ids)
                one.set_initial_witness(values[j * per:(j + 1) * per])
                one.solve()
                if one.stats()["n_slow_instances"] == 1:
                    self.exact.append(j)
                one.free()
        assert len(self.exact) == self.batch.stats()["n_slow_instances"]

    def table(self, encoding):
        if encoding not in self.tables:
            size = SIZE(encoding)
            if encoding == acvm_amd.ENC_BE32:
                vals, mask = self.be, self.asg
            elif encoding == acvm_amd.ENC_LE32:
                vals, mask = np.ascontiguousarray(self.be[..., ::-1]), self.asg
            elif encoding == acvm_amd.ENC_MONT256_LE:
                flat = self.be.reshape(-1, 32)
                out = np.zeros_like(flat)
                for r in np.nonzero(self.asg.reshape(-1))[0]:
                    v = int.from_bytes(flat[r].tobytes(), "big")
                    out[r] = np.frombuffer(((v << 256) % P).to_bytes(32, "little"), dtype=np.uint8)
                vals, mask = out.reshape(self.be.shape), self.asg
            else:  # the low bytes, little-endian; mask 1: the value fits, 2: it does not
                vals = np.ascontiguousarray(self.be[..., ::-1][..., :size])
                fits = ~self.be[..., :32 - size].any(axis=-1)
                mask = np.where(self.asg != 0, np.where(fits, 1, 2), 0).astype(np.uint8)
            self.tables[encoding] = (vals, mask)
        return self.tables[encoding]

    def range_rows(self, encoding, ws):
        """the second witness: the range export of the whole batch for this witness list, instance-major and dense -> ([B][k][size], [B][k])"""
        key = (encoding, None if ws is None else tuple(ws))
        if key not in self.ranges:
            k, size = self.nw if ws is None else len(ws), SIZE(encoding)
            d_v, d_m = acvm_amd.DeviceBuffer(size=self.B * k * size), acvm_amd.DeviceBuffer(size=self.B * k)
            self.batch.export_device(d_v.ptr, encoding=encoding, layout=IM, witnesses=ws, d_assigned=d_m.ptr)
            self.ranges[key] = (np.frombuffer(d_v.download(), dtype=np.uint8).reshape(self.B, k, size), np.frombuffer(d_m.download(), dtype=np.uint8).reshape(self.B, k))
            d_v.free()
            d_m.free()
        return self.ranges[key]

    def instances(self, kind, n):
        B = self.B
        if kind == "identity":
            return list(range(n))
        if kind == "descending":
            return [B - 1 - i for i in range(n)]
        if kind == "repeats":
            return [(i // 3 * 37 + 5) % B for i in range(n)]
        if kind == "exact":
            return [self.exact[i % len(self.exact)] for i in range(n)]
        return [(B, 1 << 31, 0xFFFFFFFF, (11 * i) % B, B + 1, B - 1)[i % 6] for i in range(n)]


def _check_list(ref, encoding, layout, L, ws=None, stride=0, with_mask=True, second_witness=True):
    batch, size, n = ref.batch, SIZE(encoding), len(L)
    cols = list(range(ref.nw)) if ws is None else [w if w < ref.NW else ref.NW - 1 for w in ws]
    rows = [j if j < ref.B else ref.B for j in L]
    vals, mask = ref.table(encoding)
    enc, msk = vals[rows][:, cols], mask[rows][:, cols]
    nrows, dense = (len(cols), n) if layout == WM else (n, len(cols))
    st = stride or dense
    want_v = np.full((nrows * st + TAIL, size), PATTERN, dtype=np.uint8)
    want_m = np.full(nrows * st + TAIL, PATTERN, dtype=np.uint8)
    v, m = want_v[:nrows * st].reshape(nrows, st, size), want_m[:nrows * st].reshape(nrows, st)
    if layout == WM:
        v[:, :dense], m[:, :dense] = enc.transpose(1, 0, 2), msk.T
    else:
        v[:, :dense], m[:, :dense] = enc, msk
    d_l = acvm_amd.DeviceBuffer(np.array(L, dtype=np.uint32).tobytes())
    d_v = acvm_amd.DeviceBuffer(bytes([PATTERN]) * want_v.size)
    d_m = acvm_amd.DeviceBuffer(bytes([PATTERN]) * want_m.size) if with_mask else None
    try:
        batch.export_device_list(d_l.ptr, n, d_v.ptr, encoding=encoding, layout=layout, witnesses=ws, stride=stride, d_assigned=d_m.ptr if with_mask else None)
        what = f"encoding {encoding} layout {layout} n {n} list {L[:6]}.. witnesses {None if ws is None else len(ws)} stride {stride}"
        got_v = np.frombuffer(d_v.download(), dtype=np.uint8).reshape(-1, size)
        if with_mask:
            got_m = np.frombuffer(d_m.download(), dtype=np.uint8)
            bad = np.nonzero(got_m != want_m)[0]
            assert bad.size == 0, f"{what}: mask differs at element {bad[0]} ({bad.size} in all): {got_m[bad[0]]} != {want_m[bad[0]]}"
        bad = np.nonzero((got_v != want_v).any(axis=1))[0]
        assert bad.size == 0, f"{what}: values differ at element {bad[0]} ({bad.size} in all): {got_v[bad[0]].tobytes().hex()} != {want_v[bad[0]].tobytes().hex()}"
        if second_witness:  # rows L of the range export of the same handle
            rv, rm = ref.range_rows(encoding, ws)
            g = got_v[:nrows * st].reshape(nrows, st, size)[:, :dense]
            g = g.transpose(1, 0, 2) if layout == WM else g
            inside = [i for i, j in enumerate(L) if j < ref.B]
            assert np.array_equal(g[inside], rv[[L[i] for i in inside]]), f"{what}: differs from the range export"
            if with_mask:
                gm = got_m[:nrows * st].reshape(nrows, st)[:, :dense]
                gm = gm.T if layout == WM else gm
                assert np.array_equal(gm[inside], rm[[L[i] for i in inside]]), f"{what}: mask differs from the range export"
    finally:
        for x in (d_l, d_v, d_m):
            if x is not None:
                x.free()


def _witness_lists(pool, nw, rng):
    """lists of 1, 4, 15, 16 and 17 positions (the direct / tiled switch at 4, the tile of 16): any order, a repeat, and in the longest an index beyond the circuit"""
    out = []
    for k in (1, 4, 15, 16, 17):
        ws = [pool[rng.randrange(len(pool))] for _ in range(k)]
        if k >= 15:
            ws[3] = ws[9]
        if k == 17 and nw is not None:
            ws[11] = nw + 3
        out.append(ws)
    return out


def _list_sweep(ref, encoding, layout, wlists, seed):
    rng = random.Random(seed)
    kinds = [k for k in KINDS if k != "exact" or ref.exact]
    combos = [(n, ws) for n in LENGTHS for ws in wlists]
    for idx, (n, ws) in enumerate(combos):
        L = ref.instances(kinds[idx % len(kinds)], n)
        if idx % 7 == 3:
            rng.shuffle(L)
        _check_list(ref, encoding, layout, L, ws)
    ws = wlists[-2]
    dense = 65 if layout == WM else len(ws)
    _check_list(ref, encoding, layout, ref.instances("out_of_range", 65), ws, stride=dense + 5)  # a stride above the dense one
    _check_list(ref, encoding, layout, ref.instances("repeats", 65), ws, with_mask=False)         # no mask


@pytest.fixture(scope="module")
def arith(oracle):
    circ, ids = synth.arithmetic_circuit(1000, seed=0xAC1D0E01)
    values = synth.witness_batch(LIST_B, seed=0xAC1D0E01)
    refs = {}

    def get(mode):
        if mode not in refs:
            kw = {"force_slow": True} if mode == "force_slow" else {}
            if mode == "reuse_slots":
                gc = acvm_amd.Circuit(circ.to_bytes())
                kw = {"reuse_slots": True, "keep": gc.witness_set("return_values") + [gc.num_witnesses // 2, gc.num_witnesses // 3]}
            refs[mode] = ListRef(oracle, circ, ids, values, LIST_B, **kw)
            refs[mode].ids, refs[mode].keep = ids, kw.get("keep", [])
            refs[mode].own = lambda mode=mode, kw=kw: ListRef(oracle, circ, ids, values, LIST_B, like=refs[mode], **kw)
        return refs[mode]
    yield get
    for r in refs.values():
        r.batch.free()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_list_export_every_encoding_and_layout(arith, encoding, layout):
    """generic and exact lanes in one batch (the edge cases of witness_batch put a few instances on the exact path)"""
    ref = arith("plain")
    assert 1 <= len(ref.exact) < LIST_B
    wlists = _witness_lists(list(range(1, ref.nw)), ref.nw, random.Random(0x715700 + encoding)) + [None]
    _list_sweep(ref, encoding, layout, wlists, 0x5EED00 + 16 * encoding + layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_list_export_forced_slow_path(arith, encoding, layout):
    """every instance is an exact lane"""
    ref = arith("force_slow")
    assert len(ref.exact) == LIST_B
    wlists = _witness_lists(list(range(1, ref.nw)), ref.nw, random.Random(0x715701 + encoding)) + [None]
    _list_sweep(ref, encoding, layout, wlists, 0x5EED01 + 16 * encoding + layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_list_export_slot_reuse_kept_witnesses(arith, encoding, layout):
    """rows are recycled and the exact lanes live in the side table: the initial witnesses and keep_ids equal the oracle"""
    ref = arith("reuse_slots")
    assert ref.batch.stats()["n_slow_instances"] > 0 and ref.batch.stats()["n_table_rows"] < ref.batch.stats()["n_witnesses"]
    wlists = _witness_lists(ref.keep + ref.ids, None, random.Random(0x715702 + encoding))
    _list_sweep(ref, encoding, layout, wlists, 0x5EED02 + 16 * encoding + layout)


def test_list_export_refusals_equal_the_range_exports(arith):
    ref = arith("reuse_slots")
    b = ref.batch
    d = acvm_amd.DeviceBuffer(size=LIST_B * b.nw * 32)
    d_l = acvm_amd.DeviceBuffer(np.arange(LIST_B, dtype=np.uint32).tobytes())
    not_kept = [ref.ids[-1] + 3]
    assert not_kept[0] not in ref.keep
    for kw in ({"witnesses": not_kept}, {}, {"witnesses": ref.keep, "stride": len(ref.keep) - 1}, {"witnesses": ref.keep, "encoding": 3},
               {"witnesses": ref.keep, "layout": 2}):
        with pytest.raises(acvm_amd.AcvmError) as of_range:
            b.export_device(d.ptr, **kw)
        with pytest.raises(acvm_amd.AcvmError) as of_list:
            b.export_device_list(d_l.ptr, LIST_B, d.ptr, **kw)
        assert str(of_list.value) == str(of_range.value), kw
    with pytest.raises(acvm_amd.AcvmError, match="recycles"):
        b.export_device_list(d_l.ptr, LIST_B, d.ptr)
    with pytest.raises(acvm_amd.AcvmError, match="not kept"):
        b.export_device_list(d_l.ptr, LIST_B, d.ptr, witnesses=not_kept)
    with pytest.raises(acvm_amd.AcvmError, match="aligned"):
        b.export_device_list(d_l.ptr, LIST_B, d.ptr + 8, witnesses=ref.keep)
    b.export_device_list(d_l.ptr, 0, d.ptr, witnesses=ref.keep)  # an empty list writes nothing
    fresh = acvm_amd.Batch(acvm_amd.Circuit(synth.arithmetic_circuit(10, seed=1)[0].to_bytes()), 4, synth.arithmetic_circuit(10, seed=1)[1])
    with pytest.raises(acvm_amd.AcvmError, match="not solved"):
        fresh.export_device_list(d_l.ptr, 4, d.ptr)
    fresh.free()
    d.free()
    d_l.free()


def test_list_export_after_solve_then_import_refuses_like_the_range_export():
    B = 130
    circ = Circuit(5, [E([(1, 1, 2)], [(M1, 3)], 0), E([], [(1, 3), (1, 4), (M1, 5)], 0)])
    ids = [1, 2, 4]
    batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
    d_in = acvm_amd.DeviceBuffer(values_from_rows([[j + 2, 3 * j + 1, j + 9] for j in range(B)]))
    d_next = acvm_amd.DeviceBuffer(values_from_rows([[j + 5, 7 * j + 1, j] for j in range(B)]))
    batch.set_initial_witness_device(d_in.ptr)
    assert batch.solve(then_import=d_next.ptr) == 0
    d = acvm_amd.DeviceBuffer(size=B * batch.nw * 32)
    d_l = acvm_amd.DeviceBuffer(np.arange(B, dtype=np.uint32)[::-1].copy().tobytes())
    batch.export_device_list(d_l.ptr, B, d.ptr, encoding=acvm_amd.ENC_LE32, witnesses=[5, 3])
    got = np.frombuffer(d.download(B * 2 * 32), dtype=np.uint8).reshape(B, 2, 32)
    for i in (0, 1, B - 1):
        j = B - 1 - i
        w3 = (j + 2) * (3 * j + 1)
        assert int.from_bytes(got[i, 1].tobytes(), "little") == w3 and int.from_bytes(got[i, 0].tobytes(), "little") == w3 + j + 9
    with pytest.raises(acvm_amd.AcvmError, match="initial witnesses"):
        batch.export_device_list(d_l.ptr, B, d.ptr, witnesses=[3, 1])
    with pytest.raises(acvm_amd.AcvmError, match="initial witnesses"):
        batch.export_device_list(d_l.ptr, B, d.ptr)
    for x in (d, d_l, d_in, d_next):
        x.free()
    batch.free()


# ------------------------------------------------------------------------------------------------ 4. the pipeline and the transfers
def test_pipeline_select_solved_then_export_their_maps(arith):
    """outcomes_device(select Solved) -> export_device_list(d_selected, n_selected): the oracle's maps of exactly the solved instances, dense"""
    for mode in ("plain", "force_slow"):
        ref = arith(mode)
        solved = [j for j in range(LIST_B) if ref.ores[j].status == SOLVED]
        d_sel = acvm_amd.DeviceBuffer(bytes([PATTERN]) * 4 * LIST_B)
        n_sel = ref.batch.outcomes_device(select_mask=1 << SOLVED, d_selected=d_sel.ptr)
        assert n_sel == len(solved) and list(np.frombuffer(d_sel.download(4 * n_sel), dtype=np.uint32)) == solved
        vals, mask = ref.table(acvm_amd.ENC_MONT256_LE)
        for layout in LAYOUTS:
            d_v, d_m = acvm_amd.DeviceBuffer(size=n_sel * ref.nw * 32), acvm_amd.DeviceBuffer(size=n_sel * ref.nw)
            ref.batch.export_device_list(d_sel.ptr, n_sel, d_v.ptr, encoding=acvm_amd.ENC_MONT256_LE, layout=layout, d_assigned=d_m.ptr)
            shape = (ref.nw, n_sel) if layout == WM else (n_sel, ref.nw)
            got_v, got_m = np.frombuffer(d_v.download(), dtype=np.uint8).reshape(shape + (32,)), np.frombuffer(d_m.download(), dtype=np.uint8).reshape(shape)
            if layout == WM:
                got_v, got_m = got_v.transpose(1, 0, 2), got_m.T
            assert np.array_equal(got_m, mask[solved][:, :ref.nw]) and np.array_equal(got_v, vals[solved][:, :ref.nw])
            d_v.free()
            d_m.free()
        d_sel.free()


H2D_CONSTANT = 16  # bytes a list export may copy to the device besides its witness list and the exact lanes' words (today: none)


def test_transfers_are_the_witness_list_and_the_exact_lanes(oracle, arith):
    """host-to-device bytes of a list export: <= 4 n_sel + H2D_CONSTANT without exact lanes, + 16 n_slow with them; never per instance or per list entry"""
    circ, ids = synth.arithmetic_circuit(300, seed=0xAC1D0E07)
    B = 4096
    batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
    batch.set_initial_witness(synth.witness_batch(B, seed=0xAC1D0E07, edge_cases=False))
    assert batch.solve() == 0 and batch.stats()["n_slow_instances"] == 0
    d_l = acvm_amd.DeviceBuffer(np.arange(B, dtype=np.uint32).tobytes())
    d_v = acvm_amd.DeviceBuffer(size=B * batch.nw * 32)
    for ws in (None, [5, 9, batch.nw - 1], list(range(1, 41))):
        for enc in (acvm_amd.ENC_BE32, acvm_amd.ENC_U64):
            h = batch.export_h2d_bytes()
            batch.export_device_list(d_l.ptr, B, d_v.ptr, encoding=enc, witnesses=ws)
            assert batch.export_h2d_bytes() - h <= 4 * (0 if ws is None else len(ws)) + H2D_CONSTANT, (ws, enc)
    batch.solve()  # a solve that flags nothing changes nothing
    h = batch.export_h2d_bytes()
    batch.export_device_list(d_l.ptr, B, d_v.ptr, witnesses=[5])
    assert batch.export_h2d_bytes() - h <= 4 + H2D_CONSTANT
    for x in (d_l, d_v):
        x.free()
    batch.free()
    for mode in ("plain", "force_slow"):
        ref = arith(mode).own()  # a handle of this test's: it is solved again below
        n_slow = ref.batch.stats()["n_slow_instances"]
        ref.batch.set_initial_witness(synth.witness_batch(LIST_B, seed=0xAC1D0E01))
        ref.batch.solve()  # the same inputs again: the set of exact lanes is rebuilt, the map on the device is stale
        d_l = acvm_amd.DeviceBuffer(np.arange(LIST_B, dtype=np.uint32)[::-1].copy().tobytes())
        d_v = acvm_amd.DeviceBuffer(size=LIST_B * 8 * 32)
        ws = [3, 4, 5, 6, 7, 8, 9, 10]
        for _ in range(2):
            h = ref.batch.export_h2d_bytes()
            ref.batch.export_device_list(d_l.ptr, LIST_B, d_v.ptr, witnesses=ws)
            assert ref.batch.export_h2d_bytes() - h <= 4 * len(ws) + H2D_CONSTANT + 16 * n_slow
        assert ref.batch.export_h2d_bytes() - h <= 4 * len(ws) + H2D_CONSTANT  # the second export found the map current
        _check_list(ref, acvm_amd.ENC_BE32, IM, list(range(LIST_B))[::-1], ws)
        for x in (d_l, d_v):
            x.free()
        ref.batch.free()
