"""acvm_batch_export_device on the device: the witness map written into device memory in the consumer's encoding and layout, against the
CPU oracle's maps converted with Python integers. Every comparison is bit-exact, values and mask; the output buffers are pre-filled with a
pattern, and everything outside the described elements must still hold it."""
import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import P, Brillig, Circuit, Expression as E
from acvm_amd.synth import values_from_rows

pytestmark = pytest.mark.gpu
M1 = P - 1
W = E.from_witness
ENCODINGS = (acvm_amd.ENC_BE32, acvm_amd.ENC_LE32, acvm_amd.ENC_MONT256_LE)
LAYOUTS = (acvm_amd.LAYOUT_INSTANCE_MAJOR, acvm_amd.LAYOUT_WITNESS_MAJOR)
PATTERN, TAIL = 0xA5, 96


def _encode(be, encoding):
    """[..., 32] canonical big-endian bytes (the oracle's) -> the encoding's bytes, through Python integers where arithmetic is involved"""
    if encoding == acvm_amd.ENC_BE32:
        return be
    if encoding == acvm_amd.ENC_LE32:
        return be[..., ::-1]
    flat = be.reshape(-1, 32)
    out = np.empty_like(flat)
    for r in range(flat.shape[0]):
        v = int.from_bytes(flat[r].tobytes(), "big")
        out[r] = np.frombuffer(((v << 256) % P).to_bytes(32, "little"), dtype=np.uint8)
    return out.reshape(be.shape)


def _expected(oasg, ovals, encoding, layout, witnesses, first, n, stride):
    """the whole output buffers (values, mask) as they must read afterwards, TAIL pattern elements behind the last row included"""
    nw_o = oasg.shape[1]
    be = np.zeros((n, len(witnesses), 32), dtype=np.uint8)
    asg = np.zeros((n, len(witnesses)), dtype=np.uint8)
    for k, w in enumerate(witnesses):
        if w < nw_o:
            asg[:, k] = oasg[first:first + n, w]
            be[:, k] = ovals[first:first + n, w]
    be[asg == 0] = 0
    enc = np.ascontiguousarray(_encode(be, encoding))
    enc[asg == 0] = 0
    rows, dense = (len(witnesses), n) if layout == acvm_amd.LAYOUT_WITNESS_MAJOR else (n, len(witnesses))
    stride = stride or dense
    vals = np.full((rows * stride + TAIL, 32), PATTERN, dtype=np.uint8)
    mask = np.full(rows * stride + TAIL, PATTERN, dtype=np.uint8)
    v, m = vals[:rows * stride].reshape(rows, stride, 32), mask[:rows * stride].reshape(rows, stride)
    if layout == acvm_amd.LAYOUT_WITNESS_MAJOR:
        v[:, :dense], m[:, :dense] = enc.transpose(1, 0, 2), asg.T
    else:
        v[:, :dense], m[:, :dense] = enc, asg
    return vals, mask


def _check(batch, oasg, ovals, encoding, layout, witnesses=None, first=0, n=None, stride=0, with_mask=True):
    n = batch.B - first if n is None else n
    ws = list(range(batch.nw)) if witnesses is None else list(witnesses)
    want_v, want_m = _expected(oasg, ovals, encoding, layout, ws, first, n, stride)
    d_v = acvm_amd.DeviceBuffer(bytes([PATTERN]) * want_v.size)
    d_m = acvm_amd.DeviceBuffer(bytes([PATTERN]) * want_m.size) if with_mask else None
    try:
        batch.export_device(d_v.ptr, encoding=encoding, layout=layout, witnesses=witnesses, first=first, n=n, stride=stride,
                            d_assigned=d_m.ptr if with_mask else None)
        got_v = np.frombuffer(d_v.download(), dtype=np.uint8).reshape(-1, 32)
        what = f"encoding {encoding} layout {layout} first {first} n {n} stride {stride}"
        if with_mask:
            got_m = np.frombuffer(d_m.download(), dtype=np.uint8)
            bad = np.nonzero(got_m != want_m)[0]
            assert bad.size == 0, f"{what}: mask differs at element {bad[0]} ({bad.size} in all)"
        bad = np.nonzero((got_v != want_v).any(axis=1))[0]
        assert bad.size == 0, f"{what}: values differ at element {bad[0]} ({bad.size} in all): {got_v[bad[0]].tobytes().hex()} != {want_v[bad[0]].tobytes().hex()}"
    finally:
        d_v.free()
        if d_m is not None:
            d_m.free()


def _solved(oracle, circ, ids, values, B, force_slow=False, oracle_threads=1, **kw):
    data = circ.to_bytes()
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values, B, n_threads=oracle_threads)
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), B, ids, **kw)
    batch.set_force_slow_path(force_slow)
    batch.set_initial_witness(values)
    batch.solve()
    return batch, oasg, ovals


def test_arithmetic_circuit_every_encoding_and_layout(oracle):
    """scaled and relaxed columns; the edge cases of witness_batch put a few instances on the exact path, so both kinds of lane are there"""
    B = 200
    circ, ids = synth.arithmetic_circuit(1000, seed=0xAC1D0E01)
    batch, oasg, ovals = _solved(oracle, circ, ids, synth.witness_batch(B, seed=0xAC1D0E01), B)
    assert 1 <= batch.stats()["n_slow_instances"] < B
    for encoding in ENCODINGS:
        for layout in LAYOUTS:
            _check(batch, oasg, ovals, encoding, layout)
    # the host export as second witness
    gasg, gvals = batch.witness_map()
    d = acvm_amd.DeviceBuffer(size=B * batch.nw * 32)
    batch.export_device(d.ptr)
    assert d.download() == gvals.tobytes()
    d.free()
    _check(batch, oasg, ovals, acvm_amd.ENC_LE32, acvm_amd.LAYOUT_INSTANCE_MAJOR, with_mask=False)
    batch.free()


@pytest.mark.parametrize("force_slow", [False, True])
def test_mixed_circuit_whole_map_and_sub_range(oracle, force_slow):
    """unassigned witnesses, hashes, memory, Brillig; B no multiple of 64, a sub-range whose first instance is none either"""
    B = 200
    circ, ids = synth.mixed_circuit(600, seed=0xAC1D0E02)
    batch, oasg, ovals = _solved(oracle, circ, ids, synth.witness_batch(B, seed=0xAC1D0E02), B, force_slow=force_slow)
    if not force_slow:
        assert 1 <= batch.stats()["n_slow_instances"] < B
    assert not oasg[0].all()  # (some witness of the numbering is unassigned)
    for encoding in ENCODINGS:
        for layout in LAYOUTS:
            _check(batch, oasg, ovals, encoding, layout)
            _check(batch, oasg, ovals, encoding, layout, first=37, n=101)
    batch.free()


def test_selection_repeats_unknown_indices_and_strides(oracle):
    B = 150
    circ, ids = synth.arithmetic_circuit(300, seed=0xAC1D0E03)
    batch, oasg, ovals = _solved(oracle, circ, ids, synth.witness_batch(B, seed=0xAC1D0E03), B)
    nw = batch.nw
    sel = [nw - 1, 3, 3, nw + 5, 0xFFFFFFFF, nw // 2, 1, nw - 1] + list(range(20, 43))
    for encoding in ENCODINGS:
        _check(batch, oasg, ovals, encoding, acvm_amd.LAYOUT_INSTANCE_MAJOR, witnesses=sel, stride=len(sel) + 9)
        _check(batch, oasg, ovals, encoding, acvm_amd.LAYOUT_WITNESS_MAJOR, witnesses=sel, stride=B + 7)
        _check(batch, oasg, ovals, encoding, acvm_amd.LAYOUT_INSTANCE_MAJOR, witnesses=sel, first=65, n=70, stride=64)
        _check(batch, oasg, ovals, encoding, acvm_amd.LAYOUT_WITNESS_MAJOR, witnesses=sel, first=65, n=70, stride=71)
        # lists of one and of three: the two layouts of one position are the same bytes
        _check(batch, oasg, ovals, encoding, acvm_amd.LAYOUT_INSTANCE_MAJOR, witnesses=[nw - 1])
        _check(batch, oasg, ovals, encoding, acvm_amd.LAYOUT_INSTANCE_MAJOR, witnesses=[nw - 1, nw + 1, 7], first=3, n=140, stride=5)
    _check(batch, oasg, ovals, acvm_amd.ENC_LE32, acvm_amd.LAYOUT_INSTANCE_MAJOR, stride=nw + 3)
    _check(batch, oasg, ovals, acvm_amd.ENC_LE32, acvm_amd.LAYOUT_WITNESS_MAJOR, stride=B + 64)
    d = acvm_amd.DeviceBuffer(size=B * nw * 32 + 64)
    with pytest.raises(acvm_amd.AcvmError, match="stride"):
        batch.export_device(d.ptr, witnesses=sel, stride=len(sel) - 1)
    with pytest.raises(acvm_amd.AcvmError, match="stride"):
        batch.export_device(d.ptr, layout=acvm_amd.LAYOUT_WITNESS_MAJOR, witnesses=sel, stride=B - 1)
    with pytest.raises(acvm_amd.AcvmError, match="aligned"):
        batch.export_device(d.ptr + 8, witnesses=sel)
    with pytest.raises(acvm_amd.AcvmError, match="out of bounds"):
        batch.export_device(d.ptr, witnesses=sel, first=B - 1, n=2)
    d.free()
    batch.free()
    # a witness of the numbering that nothing produces, with and without recycled rows
    circ = Circuit(9, [E([(1, 1, 2)], [(M1, 3)], 0)])
    values = values_from_rows([[j + 1, j + 2] for j in range(70)])
    for reuse in (False, True):
        b, oasg, ovals = _solved(oracle, circ, [1, 2], values, 70, reuse_slots=reuse, keep=[3, 7])
        for layout in LAYOUTS:
            _check(b, oasg, ovals, acvm_amd.ENC_MONT256_LE, layout, witnesses=[3, 7, 1, 7, 2])
        b.free()


def test_not_solved_is_refused():
    circ, ids = synth.arithmetic_circuit(10, seed=1)
    b = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), 4, ids)
    d = acvm_amd.DeviceBuffer(size=4 * b.nw * 32)
    with pytest.raises(acvm_amd.AcvmError, match="not solved"):
        b.export_device(d.ptr)
    d.free()
    b.free()


def test_slot_reuse_kept_witnesses_and_side_table(oracle):
    """rows are recycled and the flagged instances live in the side table: kept + initial witnesses equal the oracle, the rest is refused"""
    B = 96
    circ, ids = synth.mixed_circuit(400, seed=0xAC1D0F03)
    data = circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    keep = gc.witness_set("return_values") + [gc.num_witnesses // 2]
    batch, oasg, ovals = _solved(oracle, circ, ids, synth.witness_batch(B, seed=0xAC1D0F03), B, reuse_slots=True, keep=keep)
    assert batch.stats()["n_slow_instances"] > 0 and batch.stats()["n_table_rows"] < batch.stats()["n_witnesses"]
    sel = keep + ids[:3] + keep[:1]
    for encoding in ENCODINGS:
        for layout in LAYOUTS:
            _check(batch, oasg, ovals, encoding, layout, witnesses=sel)
    _check(batch, oasg, ovals, acvm_amd.ENC_BE32, acvm_amd.LAYOUT_INSTANCE_MAJOR, witnesses=sel, first=5, n=70, stride=len(sel) + 1)
    d = acvm_amd.DeviceBuffer(size=B * batch.nw * 32)
    with pytest.raises(acvm_amd.AcvmError, match="not kept"):
        batch.export_device(d.ptr, witnesses=[ids[-1] + 3])
    with pytest.raises(acvm_amd.AcvmError, match="recycles"):
        batch.export_device(d.ptr)
    d.free()
    batch.free()


def test_after_solve_then_import(oracle):
    B = 130
    circ = Circuit(5, [E([(1, 1, 2)], [(M1, 3)], 0), E([], [(1, 3), (1, 4), (M1, 5)], 0)])
    ids = [1, 2, 4]
    values = values_from_rows([[j + 2, 3 * j + 1, j + 9] for j in range(B)])
    nxt = values_from_rows([[j + 5, 7 * j + 1, j] for j in range(B)])
    data = circ.to_bytes()
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values, B)
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), B, ids)
    d_in, d_next = acvm_amd.DeviceBuffer(values), acvm_amd.DeviceBuffer(nxt)
    batch.set_initial_witness_device(d_in.ptr)
    assert batch.solve(then_import=d_next.ptr) == 0
    for layout in LAYOUTS:
        _check(batch, oasg, ovals, acvm_amd.ENC_MONT256_LE, layout, witnesses=[5, 3])
    d = acvm_amd.DeviceBuffer(size=B * batch.nw * 32)
    with pytest.raises(acvm_amd.AcvmError, match="initial witnesses"):
        batch.export_device(d.ptr, witnesses=[3, 1])
    with pytest.raises(acvm_amd.AcvmError, match="initial witnesses"):
        batch.export_device(d.ptr)
    for x in (d, d_in, d_next):
        x.free()
    batch.free()


def test_batch_waiting_at_a_foreign_call(oracle):
    """the map as it stands: instances that failed early, instances that never wait and instances waiting inside a Brillig opcode"""
    br = Brillig(inputs=[W(1), E(), W(2)], outputs=[5, 6, 7, 8],
                 bytecode=[("ForeignCall", "invert", [("Register", 1)], [("Register", 0)]),
                           ("ForeignCall", "invert", [("Register", 3)], [("Register", 2)])], predicate=W(3))
    circ = Circuit(10, [E([(1, 1, 2)], [(M1, 4)], 0), E([], [(1, 4), (M1, 9)], 1), br, E([(1, 1, 6)], [(M1, 10)], 0)])
    ids = [1, 2, 3]
    rows = [[3 + j, 7 * j + 1, 1 if j % 4 else 0] for j in range(70)]
    data = circ.to_bytes()
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), len(rows), ids)
    batch.set_initial_witness(values_from_rows(rows))
    batch.solve()
    res = batch.results()
    assert any(r.status == acvm_amd.STATUS_REQUIRES_FOREIGN_CALL for r in res)
    oasg = np.zeros((len(rows), batch.nw), dtype=np.uint8)
    ovals = np.zeros((len(rows), batch.nw, 32), dtype=np.uint8)
    for j, row in enumerate(rows):
        a = oracle.ACVM(oracle.Circuit(data), dict(zip(ids, row)))
        a.solve()
        # acvm_result_t.opcode_index is ACVM::instruction_pointer (include/acvm_amd.h); the oracle's result carries an opcode index for failures only
        # and answers instruction_pointer() apart: a waiting instance is compared with that, every other one tuple against tuple
        got, want = res[j].as_tuple(), a.result().as_tuple()
        if want[0] == oracle.ST_REQUIRES_FOREIGN_CALL:
            want = want[:2] + (a.instruction_pointer(),) + want[3:]
        assert got == want, j
        for w, v in a.witness_map().items():
            oasg[j, w] = 1
            ovals[j, w] = np.frombuffer(int(v).to_bytes(32, "big"), dtype=np.uint8)
    for encoding in ENCODINGS:
        for layout in LAYOUTS:
            _check(batch, oasg, ovals, encoding, layout)
    batch.free()


def test_hand_over_to_the_next_circuit_without_the_host(oracle):
    """chosen witnesses of batch A, exported big-endian instance-major, ARE the initial witness buffer of batch B"""
    B = 130
    circ_a, ids_a = synth.arithmetic_circuit(200, seed=0xAC1D0E05)
    a, oasg, ovals = _solved(oracle, circ_a, ids_a, synth.witness_batch(B, seed=0xAC1D0E05, edge_cases=False), B)
    chosen = [a.nw - 1, a.nw // 2, ids_a[0]]
    assert oasg[:, chosen].all()
    d = acvm_amd.DeviceBuffer(size=B * len(chosen) * 32)
    a.export_device(d.ptr, encoding=acvm_amd.ENC_BE32, layout=acvm_amd.LAYOUT_INSTANCE_MAJOR, witnesses=chosen)
    circ_b = Circuit(5, [E([(1, 1, 2)], [(1, 3), (M1, 4)], 0), E([(1, 4, 4)], [(M1, 5)], 7)])  # w4 = w1 w2 + w3, w5 = w4^2 + 7
    ids_b = [1, 2, 3]
    data_b = circ_b.to_bytes()
    b = acvm_amd.Batch(acvm_amd.Circuit(data_b), B, ids_b)
    b.set_initial_witness_device(d.ptr)
    assert b.solve() == 0
    gasg, gvals = b.witness_map()
    ores, basg, bvals = oracle.solve_batch(oracle.Circuit(data_b), ids_b, np.ascontiguousarray(ovals[:, chosen]).tobytes(), B)
    assert all(r.status == 0 for r in ores)
    nw = min(basg.shape[1], gasg.shape[1])
    assert np.array_equal(gasg[:, :nw], basg[:, :nw]) and np.array_equal(gvals[:, :nw], bvals[:, :nw])
    for x in (a, b):
        x.free()
    d.free()


def test_larger_shape_many_blocks_in_both_dimensions(oracle):
    B = 1 << 14
    circ, ids = synth.arithmetic_circuit(3000, seed=0xAC1D0E06)
    batch, oasg, ovals = _solved(oracle, circ, ids, synth.witness_batch(B, seed=0xAC1D0E06), B, oracle_threads=16)
    for layout in LAYOUTS:
        _check(batch, oasg, ovals, acvm_amd.ENC_LE32, layout)
    # Montgomery-256 on a slice of it (Python integers judge every element: 257 instances x the whole map)
    for layout in LAYOUTS:
        _check(batch, oasg, ovals, acvm_amd.ENC_MONT256_LE, layout, first=8000 - 129, n=257)
    batch.free()
