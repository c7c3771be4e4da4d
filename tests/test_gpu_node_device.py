"""The device form of the node driver (acvm_node_solve_device, node.cpp run_lane_device_body): every lane reads its initial witnesses from, and writes
kept witnesses, outcome columns, digests and the selection into, device memory of the caller. The shapes are those of tests/test_gpu_node.py (one
GPU: "several devices" is device 0 listed several times). Every output buffer holds a pattern plus a tail before the call, and everything outside
the described elements must still hold it afterwards. All-zero input rows are planted at the first and the last row of every tile of every lane:
they fail, so they take the exact path -- asynchronously, beside the next tile -- and their rows are written one tile later."""
import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import Brillig, Circuit, Expression as E, P

pytestmark = pytest.mark.gpu
BE32, LE32, MONT, U8 = acvm_amd.ENC_BE32, acvm_amd.ENC_LE32, acvm_amd.ENC_MONT256_LE, acvm_amd.ENC_U8
IM, WM = acvm_amd.LAYOUT_INSTANCE_MAJOR, acvm_amd.LAYOUT_WITNESS_MAJOR
SIZE = acvm_amd.element_size
PATTERN, TAIL = 0xA5, 96
SOLVED, FAILURE, FOREIGN = acvm_amd.STATUS_SOLVED, acvm_amd.STATUS_FAILURE, acvm_amd.STATUS_REQUIRES_FOREIGN_CALL
# The mixed circuit of this seed has both kinds of exact lane among the rows every test feeds it: the all-zero row fails, and the all-ones row (edge
# case 1 of synth.witness_batch, global row 1) is Solved with an assigned set that is not the generic one -- a gate with a zero multiplicand holds
# without assigning -- which only the exact path can produce. Found with the CPU oracle; test_device_form_equals_node_solve asserts both.
CIRCUIT_SEED = 0x40DE0105


# ---- values and buffers
def planted_rows(lanes_n, tile):
    """global numbers of the first and the last row of every tile of every lane (the last, partial tile included)"""
    out, base = [], 0
    for n in lanes_n:
        for first in range(0, n, tile):
            out += [base + first, base + min(first + tile, n) - 1]
        base += n
    return sorted(set(out))


def mixed_values(total, seed, lanes_n, tile, edge_cases=True):
    v = np.frombuffer(synth.witness_batch(total, seed=seed, edge_cases=edge_cases), dtype=np.uint8).reshape(total, 16, 32).copy()
    v[planted_rows(lanes_n, tile)] = 0
    return v


def element(v, encoding):
    if encoding == BE32:
        return int(v).to_bytes(32, "big")
    if encoding == LE32:
        return int(v).to_bytes(32, "little")
    if encoding == MONT:
        return ((int(v) << 256) % P).to_bytes(32, "little")
    return int(v).to_bytes(SIZE(encoding), "little")


def decode(b, encoding):
    if encoding == BE32:
        return int.from_bytes(b, "big")
    if encoding == MONT:
        return int.from_bytes(b, "little") * pow(2, -256, P) % P
    return int.from_bytes(b, "little")


def input_buffer(rows, encoding, layout, stride=0, columns=None, n_columns=None, lead=0):
    """rows[i][k]: the value of initial witness k of row i, put where `columns` says (column k by default); every byte that is no element the
    import reads holds PATTERN, `lead` elements in front of the base included"""
    n, n_in, size = len(rows), len(rows[0]) if len(rows) else 0, SIZE(encoding)
    cols = list(range(n_in)) if columns is None else list(columns)
    width = n_in if columns is None else n_columns
    if not n:
        return bytes([PATTERN]) * 64
    r, dense = (width, n) if layout == WM else (n, width)
    stride = stride or dense
    buf = np.full((r, stride, size), PATTERN, dtype=np.uint8)
    for k, c in enumerate(cols):
        col = np.frombuffer(b"".join(element(row[k], encoding) for row in rows), dtype=np.uint8).reshape(n, size)
        if layout == WM:
            buf[c, :n] = col
        else:
            buf[:, c] = col
    return bytes([PATTERN]) * (lead * size) + buf.tobytes()


class Outputs:
    """the output buffers of one lane, pattern-filled, each with TAIL elements behind its last described one (and `lead` in front of kept / mask)"""

    def __init__(self, n, n_keep, encoding=BE32, layout=IM, stride=0, lead=0):
        self.n, self.n_keep, self.encoding, self.layout, self.lead = n, n_keep, encoding, layout, lead
        rows, dense = (n_keep, n) if layout == WM else (n, n_keep)
        self.stride = stride or dense
        self.elems = rows * self.stride + TAIL + lead
        size = SIZE(encoding)
        fill = lambda nbytes: acvm_amd.DeviceBuffer(bytes([PATTERN]) * nbytes)
        self.kept, self.mask = fill(self.elems * size), fill(self.elems)
        self.status, self.err, self.opcode, self.digests, self.selected = fill(n + TAIL), fill(n + TAIL), fill(4 * (n + TAIL)), fill(32 * (n + TAIL)), fill(4 * (n + TAIL))

    def fields(self, select_mask=0, stride=None, **null):
        """the output fields of the lane's dict; name=None passes that pointer as NULL"""
        size = SIZE(self.encoding)
        d = dict(d_kept=self.kept.ptr + self.lead * size, d_kept_assigned=self.mask.ptr + self.lead, kept_encoding=self.encoding, kept_layout=self.layout,
                 kept_stride=self.stride if stride is None else stride, d_status=self.status.ptr, d_err=self.err.ptr, d_opcode_index=self.opcode.ptr, d_digests32=self.digests.ptr,
                 select_mask=select_mask, d_selected=self.selected.ptr)
        d.update(null)
        return d

    def refill(self):
        for b in self.buffers():
            b.upload(bytes([PATTERN]) * b.size)

    def buffers(self):
        return (self.kept, self.mask, self.status, self.err, self.opcode, self.digests, self.selected)

    def get(self):
        g = lambda b, dtype=np.uint8: np.frombuffer(b.download(), dtype=dtype)
        return dict(kept=g(self.kept).reshape(-1, SIZE(self.encoding)), mask=g(self.mask), status=g(self.status), err=g(self.err), opcode=g(self.opcode, np.uint32),
                    digests=g(self.digests).reshape(-1, 32), selected=g(self.selected, np.uint32))

    def untouched(self, *names):
        got = self.get()
        return all((got[k].view(np.uint8) == PATTERN).all() for k in names)

    def free(self):
        for b in self.buffers():
            b.free()


PATTERN32 = int.from_bytes(bytes([PATTERN]) * 4, "little")


def expect_columns(n, results, digests, select_mask):
    """the columns of one lane as they must read afterwards, tails included: results = the n result tuples of the lane's rows, digests [n][32]"""
    status = np.full(n + TAIL, PATTERN, dtype=np.uint8)
    err, opcode = status.copy(), np.full(n + TAIL, PATTERN32, dtype=np.uint32)
    dig = np.full((n + TAIL, 32), PATTERN, dtype=np.uint8)
    status[:n], err[:n], opcode[:n] = [r[0] for r in results], [r[1] for r in results], [r[2] for r in results]
    dig[:n] = digests
    chosen = np.nonzero((select_mask >> status[:n].astype(np.uint32)) & 1)[0]
    selected = np.full(n + TAIL, PATTERN32, dtype=np.uint32)
    selected[:chosen.size] = chosen
    return dict(status=status, err=err, opcode=opcode, digests=dig, selected=selected), chosen.size


def assert_lane(out, got, want_cols, what, skip=()):
    for name, want in want_cols.items():
        if name in skip:
            continue
        bad = np.nonzero((got[name].reshape(want.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs at row {bad[0]} ({bad.size} in all): {got[name][bad[0]]} != {want[bad[0]]}"


def expect_kept_be32(out, kept, asg):
    """BE32, instance-major, dense: the lane's slice of acvm_node_solve's kept_be32 / kept_assigned, then the pattern"""
    v = np.full((out.elems, 32), PATTERN, dtype=np.uint8)
    m = np.full(out.elems, PATTERN, dtype=np.uint8)
    v[:out.n * out.n_keep], m[:out.n * out.n_keep] = kept.reshape(-1, 32), asg.reshape(-1)
    return dict(kept=v, mask=m)


def plain_batch(data, ids, values, B, **kw):
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), B, ids, **kw)
    batch.set_initial_witness(values)
    batch.solve()
    return batch


def expect_kept_of_plain(plain, out, first, keep):
    """what acvm_batch_export_device of a plain batch writes for the lane's rows into buffers of the same shape, whole buffers"""
    ref = Outputs(out.n, out.n_keep, out.encoding, out.layout, out.stride, out.lead)
    try:
        if out.n:
            f = ref.fields()
            plain.export_device(f["d_kept"], encoding=out.encoding, layout=out.layout, witnesses=keep, first=first, n=out.n, stride=out.stride, d_assigned=f["d_kept_assigned"])
        got = ref.get()
        return dict(kept=got["kept"], mask=got["mask"])
    finally:
        ref.free()


def offsets(lanes_n):
    return [sum(lanes_n[:q]) for q in range(len(lanes_n))]


# ---- 1. against acvm_node_solve
@pytest.mark.parametrize("devices,tile,lanes_n", [([0], 256, [1000]), ([0, 0], 192, [577, 423]), ([0, 0], 64, [130, 0]), ([0] * 3, 512, [3, 600, 97]),
                                                 ([0] * 8, 128, [700, 0, 3, 129, 640, 128, 500, 400])])
def test_device_form_equals_node_solve(devices, tile, lanes_n):
    """BE32, instance-major, dense: kept, assigned, digests and the status / err / opcode columns equal acvm_node_solve's for the same values, lane by
    lane; twice on one node, the second time with other values in the same buffers"""
    total, off = sum(lanes_n), offsets(lanes_n)
    circ, ids = synth.mixed_circuit(500, seed=CIRCUIT_SEED)
    data = circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    keep = gc.witness_set("return_values") + [ids[0], 7, 1 << 30]
    node = acvm_amd.Node(gc, ids, keep=keep, devices=devices, tile=tile)
    outs = [Outputs(n, len(keep)) for n in lanes_n]
    ins = [acvm_amd.DeviceBuffer(bytes([PATTERN]) * max(n * len(ids) * 32, 64)) for n in lanes_n]
    mask = (1 << SOLVED) | (1 << FAILURE)
    planted = planted_rows(lanes_n, tile)
    for rnd, seed in enumerate((0x40DE0001, 0x40DE0D02)):
        values = mixed_values(total, seed, lanes_n, tile)
        not_solved, res, kept, asg, dig = node.solve(values.tobytes(), total)  # the host form, on the same node
        res = [r.as_tuple() for r in res]
        # the planted rows took the exact path: they fail; and among the exact lanes of the whole set some fail and some solve
        plain = plain_batch(data, ids, values.tobytes(), total)
        n_exact = plain.stats()["n_slow_instances"]
        plain.free()
        n_failed = sum(r[0] == FAILURE for r in res)
        assert all(res[j][0] == FAILURE for j in planted) and n_failed >= len(planted) >= 2
        one = plain_batch(data, ids, values[1:2].tobytes(), 1)  # (whether an instance leaves the generic path depends on its inputs alone)
        assert res[1][0] == SOLVED and one.stats()["n_slow_instances"] == 1 and n_exact > n_failed >= 1, "no Solved exact lane among the expected outcomes"
        one.free()
        for q, n in enumerate(lanes_n):
            outs[q].refill()
            if n:
                ins[q].upload(values[off[q]:off[q] + n].tobytes())
        got = node.solve_device([dict(n=n, d_values=ins[q].ptr, **outs[q].fields(select_mask=mask)) for q, n in enumerate(lanes_n)])
        st = node.stats()
        assert all(st["async_exact"]) and sum(st["exact_instances"]) == n_exact and st["n_instances"] == total
        assert sum(st["tiles"]) == sum((n + tile - 1) // tile for n in lanes_n)
        assert node.last_not_solved == not_solved == sum(g[0] for g in got)
        for q, n in enumerate(lanes_n):
            lo, hi = off[q], off[q] + n
            want, n_sel = expect_columns(n, res[lo:hi], dig[lo:hi], mask)
            want.update(expect_kept_be32(outs[q], kept[lo:hi], asg[lo:hi]))
            assert_lane(outs[q], outs[q].get(), want, f"round {rnd} lane {q}")
            assert got[q] == (sum(r[0] != SOLVED for r in res[lo:hi]), n_sel)
    for b in ins:
        b.free()
    for o in outs:
        o.free()
    node.free()


# ---- 2. encodings and layouts, on both sides
def test_every_wide_encoding_layout_and_stride(oracle):
    """every 32-byte encoding x both layouts x dense and padded strides for the inputs and for the kept witnesses, with a column list that permutes
    and repeats: the kept witnesses equal what acvm_batch_export_device of one plain batch writes (whole buffers: mask bytes, zero bytes for
    unassigned elements, the pattern between rows) and, on every 7th instance, the oracle's values through Python integers"""
    lanes_n, tile = [333, 140], 128
    total, off = sum(lanes_n), offsets(lanes_n)
    circ, ids = synth.mixed_circuit(500, seed=CIRCUIT_SEED)
    n_in, data = len(ids), circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    keep = gc.witness_set("return_values") + [ids[0], 7, 1 << 30]
    values = mixed_values(total, 0x40DE0E03, lanes_n, tile)
    values[:, 5] = values[:, 2]  # (the column list below reads initial witnesses 2 and 5 from one column)
    rows = [[int.from_bytes(values[j, k].tobytes(), "big") % P for k in range(n_in)] for j in range(total)]
    columns, n_columns = [(5 * k + 3) % 19 for k in range(n_in)], 19  # a permutation of 16 of 19 columns ...
    columns[5] = columns[2]                                           # ... with a repeat
    plain = plain_batch(data, ids, values.tobytes(), total)
    res, dig = [r.as_tuple() for r in plain.results()], plain.digest()
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values.tobytes(), total)
    assert res == [r.as_tuple() for r in ores]
    node = acvm_amd.Node(gc, ids, keep=keep, devices=[0, 0], tile=tile)
    seen_masks = set()
    for case, (enc_in, lay_in, enc_k, lay_k, padded) in enumerate((e, l, (LE32, MONT, BE32)[i], (WM, IM)[j], p) for i, e in enumerate((BE32, LE32, MONT)) for j, l in enumerate((IM, WM))
                                                                  for p in (False, True)):
        use_columns = case % 3 != 0
        outs, ins, lanes = [], [], []
        for q, n in enumerate(lanes_n):
            dense_in = n if lay_in == WM else (n_columns if use_columns else n_in)
            dense_k = n if lay_k == WM else len(keep)
            out = Outputs(n, len(keep), enc_k, lay_k, dense_k + 5 if padded else 0)
            buf = acvm_amd.DeviceBuffer(input_buffer(rows[off[q]:off[q] + n], enc_in, lay_in, dense_in + 3 if padded else 0, columns if use_columns else None, n_columns))
            outs.append(out)
            ins.append(buf)
            lanes.append(dict(n=n, d_values=buf.ptr, encoding=enc_in, layout=lay_in, stride=dense_in + 3 if padded else 0, columns=columns if use_columns else None,
                              n_columns=n_columns, **out.fields(select_mask=1 << SOLVED, stride=None if padded else 0)))
        got = node.solve_device(lanes)
        what = f"in {enc_in}/{lay_in} kept {enc_k}/{lay_k} padded {padded} columns {use_columns}"
        for q, n in enumerate(lanes_n):
            lo, hi = off[q], off[q] + n
            want, n_sel = expect_columns(n, res[lo:hi], dig[lo:hi], 1 << SOLVED)
            want.update(expect_kept_of_plain(plain, outs[q], lo, keep))
            g = outs[q].get()
            assert_lane(outs[q], g, want, f"{what} lane {q}")
            assert got[q] == (sum(r[0] != SOLVED for r in res[lo:hi]), n_sel)
            for j in range(lo, hi, 7):  # the oracle's values through Python integers
                for k, w in enumerate(keep):
                    at = (k * outs[q].stride + (j - lo)) if lay_k == WM else ((j - lo) * outs[q].stride + k)
                    assigned = w < oasg.shape[1] and bool(oasg[j, w])
                    assert g["mask"][at] == assigned, (what, j, w)
                    assert decode(g["kept"][at].tobytes(), enc_k) == (int.from_bytes(ovals[j, w].tobytes(), "big") if assigned else 0), (what, j, w)
            seen_masks |= set(g["mask"][g["mask"] != PATTERN])
        for b in ins:
            b.free()
        for o in outs:
            o.free()
    assert seen_masks == {0, 1}
    plain.free()
    node.free()


# ---- 3. narrow encodings
def test_bytes_in_and_digest_bytes_out(oracle):
    """the hash circuit fed U8 bytes, its 32 Keccak output bytes kept as U8, in both layouts, every base pointer one element behind its allocation;
    one more kept witness (3 x + 1000) never fits a byte: mask 2, low byte written"""
    circ, ids = synth.hash_circuit(n_msg=8)
    n_in = len(ids)
    big = circ.current_witness_index + 1
    circ.opcodes.append(E([], [(3, ids[0]), (P - 1, big)], 1000))
    circ.current_witness_index = big
    data = circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    keep = gc.witness_set("return_values") + [big, ids[3]]
    lanes_n, tile = [150, 70], 64
    total, off = sum(lanes_n), offsets(lanes_n)
    values = synth.byte_batch(total, n_in, seed=0xAC1D0D10)
    rows = [[int(v) for v in r] for r in np.frombuffer(values, dtype=np.uint8).reshape(total, n_in, 32)[:, :, 31]]
    plain = plain_batch(data, ids, values, total)
    res, dig = [r.as_tuple() for r in plain.results()], plain.digest()
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values, total)
    assert res == [r.as_tuple() for r in ores] and all(r[0] == SOLVED for r in res)
    node = acvm_amd.Node(gc, ids, keep=keep, devices=[0, 0], tile=tile)
    for lay_in, lay_k in ((IM, WM), (WM, IM)):
        outs, ins, lanes = [], [], []
        for q, n in enumerate(lanes_n):
            out = Outputs(n, len(keep), U8, lay_k, lead=1)
            buf = acvm_amd.DeviceBuffer(input_buffer(rows[off[q]:off[q] + n], U8, lay_in, lead=1))
            outs.append(out)
            ins.append(buf)
            lanes.append(dict(n=n, d_values=buf.ptr + 1, encoding=U8, layout=lay_in, **out.fields()))
        got = node.solve_device(lanes)
        for q, n in enumerate(lanes_n):
            lo, hi = off[q], off[q] + n
            want, n_sel = expect_columns(n, res[lo:hi], dig[lo:hi], 0)
            want.update(expect_kept_of_plain(plain, outs[q], lo, keep))
            g = outs[q].get()
            assert_lane(outs[q], g, want, f"U8 in {lay_in} kept {lay_k} lane {q}")
            assert got[q] == (0, 0) and g["kept"][0, 0] == PATTERN and g["mask"][0] == PATTERN  # (the element in front of the base)
            k_big = keep.index(big)
            for j in range(lo, hi, 7):
                for k, w in enumerate(keep):
                    at = 1 + ((k * outs[q].stride + (j - lo)) if lay_k == WM else ((j - lo) * outs[q].stride + k))
                    v = int.from_bytes(ovals[j, w].tobytes(), "big")
                    assert oasg[j, w] and g["kept"][at, 0] == v % 256 and g["mask"][at] == (2 if v > 255 else 1)
                    assert (k == k_big) == (g["mask"][at] == 2)
        for b in ins:
            b.free()
        for o in outs:
            o.free()
    plain.free()
    node.free()


# ---- 4. selection, NULL outputs
def _small_case(reuse_slots=False, seed=CIRCUIT_SEED, gates=500):
    lanes_n, tile = [130, 70], 64
    total = sum(lanes_n)
    circ, ids = synth.mixed_circuit(gates, seed=seed)
    data = circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    keep = gc.witness_set("return_values")
    values = mixed_values(total, seed, lanes_n, tile)
    node = acvm_amd.Node(gc, ids, keep=keep, devices=[0, 0], tile=tile, reuse_slots=reuse_slots)
    not_solved, res, kept, asg, dig = node.solve(values.tobytes(), total)
    ins = [acvm_amd.DeviceBuffer(values[o:o + n].tobytes()) for o, n in zip(offsets(lanes_n), lanes_n)]
    return node, lanes_n, keep, ins, not_solved, [r.as_tuple() for r in res], kept, asg, dig


def _want_of(out, q, lanes_n, res, kept, asg, dig, mask):
    lo = offsets(lanes_n)[q]
    hi = lo + lanes_n[q]
    want, n_sel = expect_columns(lanes_n[q], res[lo:hi], dig[lo:hi], mask)
    want.update(expect_kept_be32(out, kept[lo:hi], asg[lo:hi]))
    return want, (sum(r[0] != SOLVED for r in res[lo:hi]), n_sel)


@pytest.mark.parametrize("mask", [1 << SOLVED, 1 << FAILURE, (1 << SOLVED) | (1 << FAILURE)])
def test_selection_and_counts(mask):
    """d_selected / n_selected against numpy.nonzero of the status column the call itself wrote; not_solved per lane and in total"""
    node, lanes_n, keep, ins, not_solved, res, kept, asg, dig = _small_case()
    outs = [Outputs(n, len(keep)) for n in lanes_n]
    got = node.solve_device([dict(n=n, d_values=ins[q].ptr, **outs[q].fields(select_mask=mask)) for q, n in enumerate(lanes_n)])
    assert node.last_not_solved == not_solved == sum(g[0] for g in got) and not_solved >= 2
    for q, n in enumerate(lanes_n):
        g = outs[q].get()
        chosen = np.nonzero((mask >> g["status"][:n].astype(np.uint32)) & 1)[0]
        assert got[q][1] == chosen.size and np.array_equal(g["selected"][:chosen.size], chosen) and (g["selected"][chosen.size:] == PATTERN32).all()
        assert got[q][0] == np.count_nonzero(g["status"][:n] != SOLVED)
        want, counts = _want_of(outs[q], q, lanes_n, res, kept, asg, dig, mask)
        assert_lane(outs[q], g, want, f"mask {mask} lane {q}")
        assert got[q] == counts and (mask == 1 << SOLVED or chosen.size > 0)
    for b in ins + outs:
        b.free()
    node.free()


@pytest.mark.parametrize("reuse_slots", [False, True])
def test_null_outputs_and_slot_reuse(reuse_slots):
    """each output NULL in turn, then all of them (the counts alone): what is given is right, what is not given is not written -- also with
    recycled witness rows (tests/test_gpu_node.py test_node_with_slot_reuse_and_null_outputs)"""
    node, lanes_n, keep, ins, not_solved, res, kept, asg, dig = _small_case(reuse_slots, *((0x40DE0002, 400) if reuse_slots else ()))
    outs = [Outputs(n, len(keep)) for n in lanes_n]
    mask = 1 << SOLVED
    cases = [{}, dict(d_kept=None, d_kept_assigned=None), dict(d_kept_assigned=None), dict(d_status=None), dict(d_err=None), dict(d_opcode_index=None), dict(d_digests32=None),
             dict(d_selected=None), dict(d_kept=None, d_kept_assigned=None, d_status=None, d_err=None, d_opcode_index=None, d_digests32=None, d_selected=None)]
    names = dict(d_kept="kept", d_kept_assigned="mask", d_status="status", d_err="err", d_opcode_index="opcode", d_digests32="digests", d_selected="selected")
    for null in cases:
        for o in outs:
            o.refill()
        got = node.solve_device([dict(n=n, d_values=ins[q].ptr, **outs[q].fields(select_mask=mask, **null)) for q, n in enumerate(lanes_n)])
        assert node.last_not_solved == not_solved
        skipped = [names[k] for k in null]
        for q in range(len(lanes_n)):
            want, counts = _want_of(outs[q], q, lanes_n, res, kept, asg, dig, mask)
            assert got[q] == counts, null  # (n_selected is counted without d_selected, and without d_status)
            assert_lane(outs[q], outs[q].get(), want, f"null {sorted(null)} lane {q}", skip=skipped)
            assert outs[q].untouched(*skipped), null
    assert all(node.stats()["async_exact"])
    for b in ins + outs:
        b.free()
    node.free()


# ---- 5. handles that stay synchronous
def test_foreign_calls_stay_synchronous():
    """the foreign-call circuit of tests/test_gpu_node.py: every row is RequiresForeignCall, written right after the solve (async_exact is 0)"""
    circ = Circuit(3, [Brillig(inputs=[E.from_witness(1)], outputs=[2], bytecode=[("ForeignCall", "f", [("Register", 0)], [("Register", 0)]), ("Stop",)])])
    node = acvm_amd.Node(acvm_amd.Circuit(circ.to_bytes()), [1], keep=[2, 1], devices=[0], tile=64)
    n = 150
    values = synth.values_from_rows([[5 + j] for j in range(n)])
    not_solved, res, kept, asg, dig = node.solve(values, n)
    res = [r.as_tuple() for r in res]
    out, buf = Outputs(n, 2), acvm_amd.DeviceBuffer(values)
    mask = 1 << FOREIGN
    got = node.solve_device([dict(n=n, d_values=buf.ptr, **out.fields(select_mask=mask))])
    assert got == [(n, n)] and node.last_not_solved == n == not_solved and not any(node.stats()["async_exact"])
    want, _ = expect_columns(n, res, dig, mask)
    want.update(expect_kept_be32(out, kept, asg))
    g = out.get()
    assert_lane(out, g, want, "foreign calls")
    assert (g["status"][:n] == FOREIGN).all() and g["mask"][:2 * n].reshape(n, 2)[:, 1].all() and not g["mask"][:2 * n].reshape(n, 2)[:, 0].any()
    out.free()
    buf.free()
    node.free()


# ---- 6. refusals
def test_refusals_start_nothing_and_leave_the_node_usable():
    node, lanes_n, keep, ins, not_solved, res, kept, asg, dig = _small_case()
    outs = [Outputs(n, len(keep)) for n in lanes_n]
    good = [dict(n=n, d_values=ins[q].ptr, **outs[q].fields()) for q, n in enumerate(lanes_n)]
    bad = [
        (dict(stride=15), "lane 1: input: stride 15 is below the dense stride 16 of the layout"),
        (dict(layout=WM, stride=64), "lane 1: input: stride 64 is below the dense stride 70 of the layout"),  # (the stride is judged against n, not the tile)
        (dict(columns=list(range(15)) + [16], n_columns=16), "lane 1: input: column 16 of initial witness 15 is not below n_columns 16"),
        (dict(encoding=7), "lane 1: input: unknown encoding 7"),
        (dict(encoding=LE32, d_values=ins[1].ptr + 8), "lane 1: input: d_values must be 16-byte aligned"),
        (dict(d_values=None), "lane 1: input: null values"),
        (dict(kept_layout=16), "lane 1: kept: unknown layout 16"),
        (dict(kept_encoding=MONT, d_kept=outs[1].kept.ptr + 8), "lane 1: kept: d_values must be 16-byte aligned"),
        (dict(kept_layout=WM, kept_stride=69), "lane 1: kept: stride 69 is below the dense stride 70 of the layout"),
        (dict(d_kept=None), "lane 1: kept: d_kept_assigned without d_kept"),
        (dict(n=1 << 32), "lane 1: n 4294967296 is not below 2^32"),
    ]
    for change, text in bad:
        with pytest.raises(acvm_amd.AcvmError) as e:
            node.solve_device([good[0], dict(good[1], **change)])
        assert text in str(e.value), (change, str(e.value))
    for lanes in ([good[0]], good + [good[1]], []):
        with pytest.raises(acvm_amd.AcvmError) as e:
            node.solve_device(lanes)
        assert "n_lanes %d is not the node's number of handles, 2" % len(lanes) in str(e.value)
    assert all(o.untouched("kept", "mask", "status", "err", "opcode", "digests", "selected") for o in outs)  # lane 0 was never started either
    # a host-form solve follows and matches; then the device form
    values = b"".join(b.download() for b in ins)
    n2, res2, kept2, asg2, dig2 = node.solve(values, sum(lanes_n))
    assert n2 == not_solved and [r.as_tuple() for r in res2] == res and np.array_equal(kept2, kept) and np.array_equal(asg2, asg) and np.array_equal(dig2, dig)
    got = node.solve_device(good)
    for q in range(len(lanes_n)):
        want, counts = _want_of(outs[q], q, lanes_n, res, kept, asg, dig, 0)
        assert got[q] == counts
        assert_lane(outs[q], outs[q].get(), want, f"after the refusals, lane {q}")
    for b in ins + outs:
        b.free()
    node.free()


# ---- 7. the traffic condition
def test_nothing_proportional_to_the_instance_count_is_copied():
    """a condition, not a measurement: the same number of tiles and the same planted exact lanes -- B instances at tile T, 2 B at tile 2 T -- copy the
    same bytes in both directions"""
    circ, ids = synth.mixed_circuit(500, seed=CIRCUIT_SEED)
    gc = acvm_amd.Circuit(circ.to_bytes())
    keep = gc.witness_set("return_values")
    seen = []
    for tile, n in ((64, 3 * 64 - 10), (128, 2 * (3 * 64 - 10))):
        values = mixed_values(n, 0x40DE0F07, [n], tile, edge_cases=False)
        keep_rows = np.ones(n, dtype=bool)
        keep_rows[planted_rows([n], tile)] = False
        values[keep_rows] = values[1]  # one generic row everywhere else: the exact lanes are the planted rows in both shapes
        node = acvm_amd.Node(gc, ids, keep=keep, devices=[0], tile=tile)
        out, buf = Outputs(n, len(keep)), acvm_amd.DeviceBuffer(values.tobytes())
        assert node.io_bytes(0) == (0, 0)
        got = node.solve_device([dict(n=n, d_values=buf.ptr, **out.fields(select_mask=1 << FAILURE))])
        st = node.stats()
        assert st["tiles"] == [3] and st["exact_instances"] == [6] and got == [(6, 6)]  # the planted rows, two per tile, and nobody else
        seen.append(node.io_bytes(0))
        got = node.solve_device([dict(n=n, d_values=buf.ptr, **out.fields(select_mask=1 << FAILURE))])
        assert node.io_bytes(0) == (2 * seen[-1][0], 2 * seen[-1][1])  # cumulative
        out.free()
        buf.free()
        node.free()
    assert seen[0] == seen[1] and seen[0][0] > 0 and seen[0][1] > 0, seen
