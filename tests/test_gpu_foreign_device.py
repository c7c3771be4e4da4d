"""The Brillig foreign-call round trip for the whole batch on the device (acvm_batch_foreign_call_sites, acvm_batch_foreign_call_inputs_device,
acvm_batch_resolve_foreign_calls_device): the pending inputs of the waiting instances are read as device columns and the answers appended from device
columns, and every result, assigned set and witness map must equal the CPU oracle's -- driven through ACVM::resolve_pending_foreign_call
(acvm/src/pwg/mod.rs:203-228) -- and those of a second handle driven by the per-instance calls. Every output buffer here is pattern-filled with a tail
and compared whole; the expected inputs are what acvm_batch_pending_foreign_call_inputs returns on that second handle."""
import collections

import pytest

import acvm_amd
from acvm_amd import (ENC_BE32 as BE32, ENC_LE32 as LE32, ENC_MONT256_LE as MONT, ENC_U8 as U8, ENC_U64 as U64, LAYOUT_INSTANCE_MAJOR as IM,
                      LAYOUT_WITNESS_MAJOR as WM)
from acvm_amd.acir import P, Brillig, Circuit, Expression as E
from acvm_amd.synth import values_from_rows

pytestmark = pytest.mark.gpu
W = E.from_witness
WAITS = acvm_amd.STATUS_REQUIRES_FOREIGN_CALL
PAD, TAIL = 0xA5, 48
R256 = 1 << 256

# how a test reads the inputs and writes the answers: encoding, layout, elements added to the dense stride; extra: columns beyond the longest row
IO = collections.namedtuple("IO", "enc_in layout_in pad_in extra enc_out layout_out pad_out", defaults=(MONT, WM, 0, 0, BE32, IM, 0))


# ---- the caller's device buffers
class Out:
    """a device buffer of n bytes and a tail, filled with a pattern: what a call left of it is compared whole"""

    def __init__(self, n):
        self.n = n
        self.buf = acvm_amd.DeviceBuffer(data=bytes([PAD]) * (n + TAIL))
        self.ptr = self.buf.ptr

    def check(self, expected, what):
        got = self.buf.download()
        assert len(expected) == self.n
        assert got[:self.n] == bytes(expected), what
        assert got[self.n:] == bytes([PAD]) * TAIL, what + ": the tail"


def size_of(enc):
    return acvm_amd.element_size(enc)


def index(layout, stride, i, k):
    return k * stride + i if layout == WM else i * stride + k


def extent(layout, stride, n_rows, n_cols):
    """elements from the first to the last one of an n_rows x n_cols buffer"""
    return index(layout, stride, n_rows - 1, n_cols - 1) + 1 if n_rows and n_cols else 0


def encode(x, enc):
    """a value as the export encodes a witness, and its mask byte"""
    if enc == BE32:
        return x.to_bytes(32, "big"), 1
    if enc == LE32:
        return x.to_bytes(32, "little"), 1
    if enc == MONT:
        return (x * R256 % P).to_bytes(32, "little"), 1
    size = size_of(enc)
    return (x % (1 << 8 * size)).to_bytes(size, "little"), 1 if x < 1 << 8 * size else 2


def answer_bytes(v, enc):
    """a 256-bit string that means v to the import: v itself (v >= p is allowed), for Montgomery-256 a representative that is not below p where one exists"""
    if enc == BE32:
        return v.to_bytes(32, "big")
    if enc == LE32:
        return v.to_bytes(32, "little")
    if enc == MONT:
        m = v % P * R256 % P
        return (m + P if m + P < R256 and v >= P else m).to_bytes(32, "little")
    return v.to_bytes(size_of(enc), "little")


def flat(values):
    """a ForeignCallResult of the Python view -- int (single) or list (array) per output -- as its shape and its values back to back"""
    return tuple(None if isinstance(v, int) else len(v) for v in values), [x for v in values for x in ([v] if isinstance(v, int) else v)]


# ---- one site, both directions
def read_inputs(dev, site, io, instances, rows_inputs, first_row=0):
    """rows [first_row, first_row + len(instances)) of the site through the device form, every buffer compared whole with what the per-instance call
    returned for those instances (rows_inputs: per row the list of inputs, each a list of ints)"""
    op, bi, n_inputs = site["opcode_index"], site["brillig_index"], site["n_inputs"]
    n = len(instances)
    flats = [[x for inp in row for x in inp] for row in rows_inputs]
    longest = max((len(f) for f in flats), default=0)
    assert dev.foreign_call_inputs_device(op, bi, first_row=first_row, n_rows=n) == longest  # the sizing call
    n_columns = longest + io.extra
    size = size_of(io.enc_in)
    stride = (n if io.layout_in == WM else n_columns) + io.pad_in
    ext = extent(io.layout_in, stride, n, n_columns)
    d_inst, d_lens, d_vals, d_mask = Out(4 * n), Out(4 * n * n_inputs), Out(ext * size), Out(ext)
    got = dev.foreign_call_inputs_device(op, bi, first_row=first_row, n_rows=n, d_values=d_vals.ptr, encoding=io.enc_in, layout=io.layout_in, n_columns=n_columns,
                                         stride=stride if io.pad_in else 0, d_instances=d_inst.ptr, d_lens=d_lens.ptr, d_mask=d_mask.ptr)
    assert got == longest
    d_inst.check(b"".join(j.to_bytes(4, "little") for j in instances), "instances")
    lens = [[len(inp) for inp in row] + [0] * (n_inputs - len(row)) for row in rows_inputs]
    d_lens.check(b"".join(x.to_bytes(4, "little") for row in lens for x in row), "lens")
    vals, mask = bytearray([PAD]) * (ext * size), bytearray([PAD]) * ext
    for i, f in enumerate(flats):
        for k in range(n_columns):  # a column at or beyond the row's total: zero bytes, mask 0
            b, m = encode(f[k], io.enc_in) if k < len(f) else (bytes(size), 0)
            at = index(io.layout_in, stride, i, k)
            vals[at * size:(at + 1) * size] = b
            mask[at] = m
    d_vals.check(vals, "values")
    d_mask.check(mask, "mask")


def resolve_rows(dev, site, io, answers, first_row=0, n_columns=None, ptr_offset=0):
    """one ForeignCallResult per row (the same shape for all), written in the test's encoding and layout and appended by the device form"""
    shape, _ = flat(answers[0])
    assert all(flat(a)[0] == shape for a in answers)
    n, total = len(answers), len(flat(answers[0])[1])
    n_columns = total if n_columns is None else n_columns
    size = size_of(io.enc_out)
    stride = (n if io.layout_out == WM else n_columns) + io.pad_out
    buf = bytearray([PAD]) * (extent(io.layout_out, stride, n, n_columns) * size + 64)
    for i, a in enumerate(answers):
        for k, v in enumerate(flat(a)[1]):
            at = index(io.layout_out, stride, i, k)
            buf[at * size:(at + 1) * size] = answer_bytes(v, io.enc_out)
    d = acvm_amd.DeviceBuffer(data=bytes(buf))
    dev.resolve_foreign_calls_device(site["opcode_index"], site["brillig_index"], shape, d.ptr + ptr_offset, first_row=first_row, n_rows=n, encoding=io.enc_out,
                                     layout=io.layout_out, n_columns=n_columns, stride=stride if io.pad_out else 0)


def waiting_at(dev, ref, site):
    """the instances of the site's waiting list, their pending inputs on the per-instance handle"""
    res = dev.results()
    pend = {j: ref.get_pending_foreign_call(j) for j, r in enumerate(ref.results()) if r.status == WAITS}
    inst = [j for j in sorted(pend) if res[j].status == WAITS and res[j].opcode_index == site["opcode_index"] and pend[j][0] == site["function"]]
    assert len(inst) == site["n_waiting"]
    return inst, pend


def lockstep(dev, ref, respond, io=IO(), form=lambda rounds: "device", solve=lambda b: b.solve(), max_rounds=10):
    """Both handles solve, the per-instance handle says what waits, and every site is answered on `dev` by the device form (or, where form(round) says
    "instance", by the per-instance call: the two forms mixed on one handle) and on `ref` per instance. Returns the rounds."""
    rounds = 0
    while True:
        solve(dev)
        solve(ref)
        sites = dev.foreign_call_sites()
        n_ref = sum(r.status == WAITS for r in ref.results())
        assert sum(s["n_waiting"] for s in sites) == n_ref and all(s["n_resolved"] == 0 for s in sites)
        assert sites == sorted(sites, key=lambda s: (s["opcode_index"], s["brillig_index"]))
        if not sites:
            return rounds
        rounds += 1
        assert rounds <= max_rounds
        for site in sites:
            inst, pend = waiting_at(dev, ref, site)
            read_inputs(dev, site, io, inst, [pend[j][1] for j in inst])
            answers = [respond(j, site["function"], pend[j][1]) for j in inst]
            if form(rounds) == "device":
                resolve_rows(dev, site, io, answers)
            else:
                for j, a in zip(inst, answers):
                    dev.resolve_pending_foreign_call(j, a)
            for j, a in zip(inst, answers):
                ref.resolve_pending_foreign_call(j, a)
        after = {(s["opcode_index"], s["brillig_index"]): s for s in dev.foreign_call_sites()}
        assert all(after[(s["opcode_index"], s["brillig_index"])]["n_resolved"] == s["n_waiting"] for s in sites)  # answered rows stay listed


def snapshot(batch):
    asg, vals = batch.witness_map()
    return [r.as_tuple() for r in batch.results()], asg.tobytes(), vals.tobytes()


def check_against_oracle(oracle, data, ids, rows, respond, batch):
    res = batch.results()
    asg, vals = batch.witness_map()
    oc = oracle.Circuit(data)
    for j, row in enumerate(rows):
        a = oracle.ACVM(oc, dict(zip(ids, row)))
        st = a.solve()
        while st == oracle.ST_REQUIRES_FOREIGN_CALL:
            fn, inputs = a.get_pending_foreign_call()
            a.resolve_pending_foreign_call([v % P if isinstance(v, int) else [x % P for x in v] for v in respond(j, fn, inputs)])
            st = a.solve()
        r = a.result()
        assert res[j].as_tuple() == r.as_tuple(), (j, res[j].as_tuple(), r.as_tuple())
        assert res[j].message == r.message
        assert list(res[j].call_stack[:res[j].n_call_stack]) == list(r.call_stack[:r.n_call_stack])
        got = {w: int.from_bytes(vals[j, w].tobytes(), "big") for w in range(asg.shape[1]) if asg[j, w]}
        assert got == a.witness_map(), j


def two_handles(circ, ids, rows, **kw):
    data = circ.to_bytes()
    c = acvm_amd.Circuit(data)
    dev, ref = acvm_amd.Batch(c, len(rows), ids, **kw), acvm_amd.Batch(c, len(rows), ids, **kw)
    for b in (dev, ref):
        b.set_initial_witness(values_from_rows(rows))
    return data, dev, ref


# ---- the circuit of tests/test_gpu_foreign_relevel.py
def relevel_circuit(n_tail=40):
    """w3 = oracle 'invert'(w1) ; w4 = w3 * w1 (must be 1) ; w5 = oracle 'double'(w2 + w4) [2 results] ; then a tail of gates"""
    ops = [Brillig(inputs=[W(1)], outputs=[3], bytecode=[("ForeignCall", "invert", [("Register", 0)], [("Register", 0)]), ("Stop",)]),
           E([(1, 3, 1)], [(P - 1, 4)], 0),
           Brillig(inputs=[E([], [(1, 2), (1, 4)], 0)], outputs=[5, 6],
                   bytecode=[("ForeignCall", "double", [("Register", 0), ("Register", 1)], [("Register", 0)]), ("Stop",)])]
    nw = 6
    for i in range(n_tail):  # w_{k} = w_{k-1} * w_{k-2} + w5
        ops.append(E([(1, nw, nw - 1)], [(1, 5), (P - 1, nw + 1)], 0))
        nw += 1
    return Circuit(nw, ops), [1, 2]


def relevel_respond(j, fn, inputs):
    if fn == "invert":
        return [pow(inputs[0][0], P - 2, P)]
    assert fn == "double"
    return [inputs[0][0] * 2 % P, (inputs[0][0] * 2 + 1) % P]


def relevel_rows(B):
    rows = [[3 + j, 1000 + 7 * j] for j in range(B)]
    rows[min(5, B - 1)][0] = 0  # invert(0) = 0: w4 = 0, still solvable
    return rows


@pytest.mark.parametrize("mode", ["relevel", "exact"])
@pytest.mark.parametrize("B", [96, 1, 63, 64, 65, 257])
def test_relevel_circuit_driven_to_the_end_by_the_device_form(oracle, B, mode):
    circ, ids = relevel_circuit()
    rows = relevel_rows(B)
    with acvm_amd.tuning(fc_relevel=1 if mode == "relevel" else 0):
        data, dev, ref = two_handles(circ, ids, rows)
        assert lockstep(dev, ref, relevel_respond) == 2  # inputs read as Montgomery-256, witness-major
        if mode == "relevel":
            assert dev.stats()["n_slow_instances"] == 0  # everything behind the calls ran on the level kernels
    assert all(r[0] == acvm_amd.STATUS_SOLVED for r in snapshot(dev)[0])
    assert snapshot(dev) == snapshot(ref)
    check_against_oracle(oracle, data, ids, rows, relevel_respond, dev)


def above_p(respond):
    """the same answers as 256-bit strings that are not below p where one exists: the reduction of the device form against the per-instance call's"""
    def r(j, fn, inputs):
        out = respond(j, fn, inputs)
        return [v + P if isinstance(v, int) and j % 3 == 0 else v for v in out]
    return r


@pytest.mark.parametrize("layout", [IM, WM])
@pytest.mark.parametrize("enc", [BE32, LE32, MONT])
def test_every_wide_encoding_and_layout_at_a_padded_stride(oracle, enc, layout):
    circ, ids = relevel_circuit(4)
    rows = relevel_rows(70)
    data, dev, ref = two_handles(circ, ids, rows)
    respond = above_p(relevel_respond)
    assert any(v >= P for j in range(70) for v in respond(j, "invert", [[3 + j]]))
    assert lockstep(dev, ref, respond, IO(enc_in=enc, layout_in=layout, pad_in=5, extra=2, enc_out=enc, layout_out=layout, pad_out=3)) == 2
    assert snapshot(dev) == snapshot(ref)
    check_against_oracle(oracle, data, ids, rows, respond, dev)


@pytest.mark.parametrize("layout", [IM, WM])
@pytest.mark.parametrize("enc", [U8, U64])
def test_narrow_encodings_on_small_values(oracle, enc, layout):
    """inputs read and answers written as integers of 1 and 8 bytes; one input is 2^64 or more: its low bytes and mask 2"""
    circ = Circuit(3, [Brillig(inputs=[W(1), W(2)], outputs=[3],
                               bytecode=[("ForeignCall", "small", [("Register", 0)], [("Register", 0), ("Register", 1)]), ("Stop",)])])
    rows = [[j % 200, 3 * j % 251] for j in range(67)]
    rows[9][1] = (1 << 64) + 5
    rows[10][0] = 256  # fits eight bytes, not one

    def respond(j, fn, inputs):
        assert fn == "small"
        return [(inputs[0][0] + inputs[1][0]) % 256]
    data, dev, ref = two_handles(circ, [1, 2], rows)
    assert lockstep(dev, ref, respond, IO(enc_in=enc, layout_in=layout, pad_in=3, extra=1, enc_out=enc, layout_out=layout, pad_out=2)) == 1
    assert snapshot(dev) == snapshot(ref)
    check_against_oracle(oracle, data, [1, 2], rows, respond, dev)


@pytest.mark.parametrize("layout", [IM, WM])
def test_array_and_vector_shapes(oracle, layout):
    """a HeapArray input and output and a HeapVector input whose length is the instance's w4: d_lens, the zero-filled tail columns and max_values"""
    br = Brillig(inputs=[[W(1), W(2), W(3)], W(4)], outputs=[[10, 11], 12],
                 bytecode=[("Const", 3, 20),
                           ("ForeignCall", "shape", [("HeapArray", 3, 2), ("Register", 4)], [("HeapArray", 0, 3), ("HeapVector", 0, 1), ("Register", 1)]),
                           ("Mov", 0, 3), ("Mov", 1, 4), ("Stop",)])
    circ = Circuit(12, [br, E([(1, 10, 11)], [(P - 1, 9)], 0)])
    ids = [1, 2, 3, 4]
    rows = [[5 * j + 3, 3 * j + 1, 7 * j, (j * 5 + 1) % 4] for j in range(66)]

    def respond(j, fn, inputs):
        assert fn == "shape" and [len(x) for x in inputs] == [3, rows[j][3], 1]
        return [[sum(inputs[0]) % P, (sum(inputs[1]) + 1) % P], inputs[2][0] * 3 % P]
    data, dev, ref = two_handles(circ, ids, rows)
    assert lockstep(dev, ref, respond, IO(layout_in=layout, enc_out=MONT, layout_out=layout, extra=1)) == 1
    assert snapshot(dev) == snapshot(ref)
    check_against_oracle(oracle, data, ids, rows, respond, dev)


@pytest.mark.parametrize("order", [("instance", "device"), ("device", "instance"), ("device", "device")])
def test_a_second_result_appended_behind_the_first_in_one_slot(oracle, order):
    """one Brillig opcode, two ForeignCalls: the second answer goes behind the first in the opcode's slot, whichever form wrote the first"""
    br = Brillig(inputs=[W(1), W(2)], outputs=[5, 6],
                 bytecode=[("ForeignCall", "inv_a", [("Register", 0)], [("Register", 0)]), ("ForeignCall", "inv_b", [("Register", 1)], [("Register", 1)]), ("Stop",)])
    circ = Circuit(7, [br, E([(1, 1, 5)], [(P - 1, 7)], 0)])
    rows = [[3 + j, 7 * j + 1] for j in range(66)]

    def respond(j, fn, inputs):
        assert fn in ("inv_a", "inv_b") and len(inputs) == 1
        return [pow(inputs[0][0], P - 2, P)]
    data, dev, ref = two_handles(circ, [1, 2], rows)
    assert lockstep(dev, ref, respond, form=lambda rounds: order[rounds - 1]) == 2
    assert snapshot(dev) == snapshot(ref)
    check_against_oracle(oracle, data, [1, 2], rows, respond, dev)


def code_of(excinfo):
    return int(str(excinfo.value).split("error ")[1].split(":")[0])


def test_partial_ranges_and_a_refused_second_answer(oracle):
    circ, ids = relevel_circuit(4)
    B = 32
    rows = relevel_rows(B)
    data, dev, ref = two_handles(circ, ids, rows)
    dev.solve()
    ref.solve()
    (site,) = dev.foreign_call_sites()
    assert (site["function"], site["n_waiting"], site["n_resolved"], site["n_inputs"]) == ("invert", B, 0, 1)
    inst, pend = waiting_at(dev, ref, site)
    half = B // 2
    answers = [relevel_respond(j, "invert", pend[j][1]) for j in inst]
    resolve_rows(dev, site, IO(), answers[:half])
    for j, a in zip(inst[:half], answers[:half]):
        ref.resolve_pending_foreign_call(j, a)
    (site,) = dev.foreign_call_sites()
    assert (site["n_waiting"], site["n_resolved"]) == (B, half)
    read_inputs(dev, site, IO(), inst, [pend[j][1] for j in inst])  # the list is fixed until the next solve: answered rows are still rows
    # a second answer for an answered row -- alone, or as part of a range -- is refused as a whole and changes nothing
    for first, n in ((0, 1), (half - 1, 2), (0, B)):
        with pytest.raises(acvm_amd.AcvmError, match="was already answered since the last solve") as e:
            resolve_rows(dev, site, IO(), [[7]] * n, first_row=first)
        assert code_of(e) == -5
    assert dev.foreign_call_sites()[0]["n_resolved"] == half
    dev.solve()
    ref.solve()
    assert snapshot(dev) == snapshot(ref)  # the same maps as without the refused calls
    sites = dev.foreign_call_sites()
    assert [(s["function"], s["opcode_index"], s["n_waiting"], s["n_resolved"]) for s in sites] == [("invert", 0, B - half, 0), ("double", 2, half, 0)]
    rest, pend = waiting_at(dev, ref, sites[0])
    assert rest == inst[half:]
    read_inputs(dev, sites[0], IO(enc_in=BE32, layout_in=IM), rest, [[[rows[j][0]]] for j in rest])  # the rest still waits with the same inputs
    # a range in the middle of a list, then the list's ends
    resolve_rows(dev, sites[0], IO(), answers[half + 3:half + 9], first_row=3)
    resolve_rows(dev, sites[0], IO(layout_out=WM), answers[half:half + 3], first_row=0)
    resolve_rows(dev, sites[0], IO(enc_out=LE32), answers[half + 9:], first_row=9)
    for j, a in zip(inst[half:], answers[half:]):
        ref.resolve_pending_foreign_call(j, a)
    lockstep(dev, ref, relevel_respond)
    assert snapshot(dev) == snapshot(ref)
    check_against_oracle(oracle, data, ids, rows, relevel_respond, dev)


def test_interleaved_sites(oracle):
    """after one round the even instances wait at the second call and the odd ones at the first: a row of either list is not its lane"""
    circ, ids = relevel_circuit(4)
    B = 66
    rows = relevel_rows(B)
    seen = []

    def respond(j, fn, inputs):
        seen.append((fn, j))
        return relevel_respond(j, fn, inputs)
    with acvm_amd.tuning(fc_relevel=0):  # (the lanes stay the lanes of the first solve: lane = instance, row = instance / 2)
        data, dev, ref = two_handles(circ, ids, rows)
        dev.solve()
        ref.solve()
        for j in range(0, B, 2):
            fn, inputs = ref.get_pending_foreign_call(j)
            for b in (dev, ref):
                b.resolve_pending_foreign_call(j, relevel_respond(j, fn, inputs))
        assert lockstep(dev, ref, respond, IO(enc_in=LE32, layout_in=IM)) == 2
    first_round = seen[:B]
    assert [j for fn, j in first_round if fn == "invert"] == list(range(1, B, 2)) and [j for fn, j in first_round if fn == "double"] == list(range(0, B, 2))
    assert snapshot(dev) == snapshot(ref)
    check_against_oracle(oracle, data, ids, rows, relevel_respond, dev)


def test_wrong_result_shapes_fail_as_after_the_per_instance_call(oracle):
    """the cases of tests/test_gpu_foreign_call.py test_wrong_result_shapes through the device form (brillig_vm/src/lib.rs:262-270): the shape is not
    checked against the bytecode, the VM reports it"""
    last = Brillig(inputs=[W(1)], outputs=[2], bytecode=[("ForeignCall", "f", [("Register", 0), ("Register", 1)], [("Register", 0)])])
    mid = Brillig(inputs=[W(1)], outputs=[3], bytecode=[("ForeignCall", "g", [("HeapArray", 0, 2)], [("Register", 0)]), ("Stop",)])
    for circ, answer in [(Circuit(3, [last]), [5]), (Circuit(3, [mid]), [[1, 2, 3]]), (Circuit(3, [mid]), [4])]:
        rows = [[9], [10]]
        respond = lambda j, fn, inputs: answer  # noqa: E731
        data, dev, ref = two_handles(circ, [1], rows)
        lockstep(dev, ref, respond)
        assert snapshot(dev) == snapshot(ref)
        check_against_oracle(oracle, data, [1], rows, respond, dev)


def test_refusals_start_nothing(oracle):
    circ, ids = relevel_circuit(4)
    B = 8
    rows = relevel_rows(B)
    data = circ.to_bytes()
    c = acvm_amd.Circuit(data)
    good = acvm_amd.DeviceBuffer(data=bytes(64 * B))
    # a handle with a caller's BlackBoxFunctionSolver keeps its store on the host
    with_solver = acvm_amd.Batch(c, B, ids, solver=acvm_amd.bb_dummy())
    with_solver.set_initial_witness(values_from_rows(rows))
    with_solver.solve()
    assert with_solver.foreign_call_sites()[0]["n_waiting"] == B
    with pytest.raises(acvm_amd.AcvmError, match="BlackBoxFunctionSolver") as e:
        with_solver.resolve_foreign_calls_device(0, 0, [None], good.ptr)
    assert code_of(e) == -3 and with_solver.foreign_call_sites()[0]["n_resolved"] == 0
    data, dev, ref = two_handles(circ, ids, rows)
    # not solved
    assert dev.foreign_call_sites() == []
    for call in (lambda: dev.resolve_foreign_calls_device(0, 0, [None], good.ptr, n_rows=B), lambda: dev.foreign_call_inputs_device(0, 0, n_rows=B)):
        with pytest.raises(acvm_amd.AcvmError, match="batch not solved") as e:
            call()
        assert code_of(e) == -5
    dev.solve()
    ref.solve()
    site = dev.foreign_call_sites()[0]
    # a range past the list, a buffer narrower than the shape, a misaligned pointer
    for kw, text in ((dict(first_row=1, n_rows=B), r"rows \[1, 9\) are outside the 8 rows waiting at opcode 0, brillig index 0"),
                     (dict(n_rows=B, n_columns=0), "n_columns 0 is below the 1 values of the result's shape"),
                     (dict(n_rows=B, d_off=8), "d_values must be 16-byte aligned"),
                     (dict(n_rows=B, stride=B - 1, layout=WM), "stride 7 is below the dense stride 8 of the layout"),
                     (dict(n_rows=B, encoding=7), "unknown encoding 7")):
        off = kw.pop("d_off", 0)
        with pytest.raises(acvm_amd.AcvmError, match=text) as e:
            dev.resolve_foreign_calls_device(0, 0, [None], good.ptr + off, **kw)
        assert code_of(e) == -1
    # the inputs call: a buffer narrower than the longest row is refused with the needed width, and nothing is written
    out, mask, inst = Out(32 * B), Out(B), Out(4 * B)
    with pytest.raises(acvm_amd.AcvmError, match="n_columns 0 is below the 1 values of the longest row") as e:
        dev.foreign_call_inputs_device(0, 0, n_rows=B, d_values=out.ptr, d_mask=mask.ptr, d_instances=inst.ptr, n_columns=0)
    assert code_of(e) == -1
    for kw, text in ((dict(first_row=B, n_rows=1), r"rows \[8, 9\) are outside the 8 rows"), (dict(n_rows=B, d_values=out.ptr + 8, n_columns=1), "d_values must be 16-byte aligned")):
        with pytest.raises(acvm_amd.AcvmError, match=text) as e:
            dev.foreign_call_inputs_device(0, 0, d_mask=mask.ptr, d_instances=inst.ptr, **kw)
        assert code_of(e) == -1
    for o, n in ((out, 32 * B), (mask, B), (inst, 4 * B)):
        o.check(bytes([PAD]) * n, "a refused call wrote")
    assert dev.foreign_call_sites() == [site]  # nothing was started: nobody counts as answered
    dev.reset()
    ref.reset()
    assert lockstep(dev, ref, relevel_respond) == 2
    assert snapshot(dev) == snapshot(ref)
    check_against_oracle(oracle, data, ids, rows, relevel_respond, dev)


@pytest.mark.parametrize("how", ["new_inputs", "reset"])
def test_new_inputs_forget_the_device_resolved_answers(oracle, how):
    circ, ids = relevel_circuit(4)
    B = 65
    rows = relevel_rows(B)
    data, dev, ref = two_handles(circ, ids, rows)
    assert lockstep(dev, ref, relevel_respond) == 2
    first = snapshot(dev)
    for b in (dev, ref):
        b.set_initial_witness(values_from_rows(rows)) if how == "new_inputs" else b.reset()
    dev.solve()
    assert all(r.status == WAITS and r.opcode_index == 0 for r in dev.results())  # every instance waits again, at the first call
    assert [(s["function"], s["n_waiting"], s["n_resolved"]) for s in dev.foreign_call_sites()] == [("invert", B, 0)]
    # the second drive mixes the forms the other way round on a slot that was device-owned before
    assert lockstep(dev, ref, relevel_respond, form=lambda rounds: ("instance", "device")[rounds - 1]) == 2
    assert snapshot(dev) == first == snapshot(ref)
    check_against_oracle(oracle, data, ids, rows, relevel_respond, dev)


def test_the_round_trip_through_solve_opcode(oracle):
    circ, ids = relevel_circuit(4)
    B = 65
    rows = relevel_rows(B)
    data, dev, ref = two_handles(circ, ids, rows)
    steps, answered = 0, 0
    while True:
        left = dev.solve_opcode()
        assert ref.solve_opcode() == left
        steps += 1
        assert steps < 40
        for site in dev.foreign_call_sites():
            if site["n_resolved"]:
                continue
            inst, pend = waiting_at(dev, ref, site)
            read_inputs(dev, site, IO(), inst, [pend[j][1] for j in inst])
            answers = [relevel_respond(j, site["function"], pend[j][1]) for j in inst]
            resolve_rows(dev, site, IO(layout_out=WM), answers)
            for j, a in zip(inst, answers):
                ref.resolve_pending_foreign_call(j, a)
            answered += len(inst)
        if left == 0:
            break
    assert answered == 2 * B
    assert snapshot(dev) == snapshot(ref)
    check_against_oracle(oracle, data, ids, rows, relevel_respond, dev)


def test_many_calls_in_one_round_do_not_grow_the_store(oracle):
    """A column gains one result per round however many calls answer the round's rows: a handle answered row by row, in small ranges and per instance on
    its device-owned slots holds tables of the size of a handle answered by one call per site -- and computes the same."""
    circ, ids = relevel_circuit(4)
    B = 300
    rows = relevel_rows(B)
    data, many, one = two_handles(circ, ids, rows)
    sizes = []
    for rounds in range(1, 4):
        left = many.solve()
        assert one.solve() == left
        sites = many.foreign_call_sites()
        assert one.foreign_call_sites() == sites
        if not sites:
            break
        for site in sites:
            res = many.results()
            inst = [j for j in range(B) if res[j].status == WAITS and res[j].opcode_index == site["opcode_index"]]
            assert len(inst) == site["n_waiting"]
            answers = [relevel_respond(j, *many.get_pending_foreign_call(j)) for j in inst]
            resolve_rows(one, site, IO(), answers)
            resolve_rows(many, site, IO(), answers[:1])  # (the slot is device-owned from here on)
            r = 1
            while r < len(inst) // 2:  # ranges of 1 .. 7 rows
                n = min(1 + r % 7, len(inst) // 2 - r)
                resolve_rows(many, site, IO(layout_out=WM), answers[r:r + n], first_row=r)
                r += n
            for j, a in zip(inst[r:], answers[r:]):  # the rest per instance: one append each
                many.resolve_pending_foreign_call(j, a)
        sizes.append((many.foreign_call_stats()["store_bytes"], one.foreign_call_stats()["store_bytes"]))
    assert rounds == 3 and len(sizes) == 2
    assert all(m == o and m > 0 for m, o in sizes), sizes
    assert snapshot(many) == snapshot(one)
    check_against_oracle(oracle, data, ids, rows, relevel_respond, many)
