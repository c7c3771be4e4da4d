"""The node's foreign-call handler (acvm_node_set_foreign_call_handler, node.cpp foreign_rounds): behind a tile's solve every site the tile's handle lists
is handed to the handler, the answer goes through acvm_batch_resolve_foreign_calls_device_rows, and the tile is solved again. Both node forms
(acvm_node_solve, acvm_node_solve_device) times both handler spaces, one device listed once and twice, tile 64 with n = 165 (two full tiles and a
partial one) and n = 1. Expected: a plain Batch of the same instances driven per instance (acvm_batch_resolve_foreign_call), which is itself compared
with the CPU oracle driven through ACVM::resolve_pending_foreign_call (acvm/src/pwg/mod.rs:203-228)."""
import numpy as np
import pytest

import acvm_amd
from acvm_amd import ENC_BE32 as BE32, ENC_LE32 as LE32, ENC_MONT256_LE as MONT, LAYOUT_INSTANCE_MAJOR as IM, LAYOUT_WITNESS_MAJOR as WM
from acvm_amd.acir import P, Brillig, Circuit, Expression as E
from acvm_amd.synth import values_from_rows

import test_gpu_foreign_device as fd

pytestmark = pytest.mark.gpu
W = E.from_witness
WAITS, SOLVED = acvm_amd.STATUS_REQUIRES_FOREIGN_CALL, acvm_amd.STATUS_SOLVED
PAD = fd.PAD
TILE = 64
R256 = 1 << 256


# ---- circuits
def split_circuit():
    """w2 = 1: the instance waits at 'even' (opcode 0) and skips opcode 1; w3 = 1: the other way round. Instances of one tile wait at two sites at once."""
    code = lambda fn: [("ForeignCall", fn, [("Register", 0)], [("Register", 0)]), ("Stop",)]  # noqa: E731
    ops = [Brillig(inputs=[W(1)], outputs=[4], bytecode=code("even"), predicate=W(2)),
           Brillig(inputs=[W(1)], outputs=[5], bytecode=code("odd"), predicate=W(3)),
           E([], [(1, 4), (1, 5), (1, 1), (P - 1, 6)], 0)]
    return Circuit(6, ops), [1, 2, 3]


def split_rows(n):
    return [[100 + 3 * j, 1 - j % 2, j % 2] for j in range(n)]


def split_respond(j, fn, inputs):
    return [(inputs[0][0] * (2 if fn == "even" else 3) + j) % P]


def println_circuit():
    return Circuit(3, [Brillig(inputs=[W(1)], outputs=[2], bytecode=[("ForeignCall", "println", [], [("Register", 0)]), ("Stop",)]),
                       E([(1, 1, 2)], [(P - 1, 3)], 0)]), [1]


CIRCUITS = {"relevel": (lambda: fd.relevel_circuit(4), fd.relevel_rows, fd.relevel_respond, [5, 6, 9]),
            "split": (split_circuit, split_rows, split_respond, [4, 5, 6])}


# ---- the expected outcome: one plain batch, driven per instance
class Reference:
    def __init__(self, data, ids, rows, keep, respond, can_answer=lambda j, fn, rnd: True, max_rounds=256):
        n = len(rows)
        self.batch = b = acvm_amd.Batch(acvm_amd.Circuit(data), n, ids)
        b.set_initial_witness(values_from_rows(rows))
        self.waiting = []  # per round: {instance: function}
        rnd = 0
        while True:
            b.solve()
            waits = {j: b.get_pending_foreign_call(j) for j, r in enumerate(b.results()) if r.status == WAITS}
            if not waits or rnd >= max_rounds:
                break
            self.waiting.append({j: p[0] for j, p in waits.items()})
            answered = 0
            for j, (fn, inputs) in waits.items():
                if can_answer(j, fn, rnd):
                    b.resolve_pending_foreign_call(j, respond(j, fn, inputs))
                    answered += 1
            if not answered:
                break
            rnd += 1
        self.results = [r.as_tuple() for r in b.results()]
        self.digests = b.digest()
        self.kept = np.zeros((n, len(keep), 32), dtype=np.uint8)
        self.assigned = np.zeros((n, len(keep)), dtype=np.uint8)
        for k, w in enumerate(keep):
            self.kept[:, k], self.assigned[:, k] = b.witness(w)

    def check_oracle(self, oracle, data, ids, rows, respond, can_answer=lambda j, fn, rnd: True, max_rounds=256):
        res = self.batch.results()
        asg, vals = self.batch.witness_map()
        oc = oracle.Circuit(data)
        for j, row in enumerate(rows):
            a = oracle.ACVM(oc, dict(zip(ids, row)))
            st, rnd = a.solve(), 0
            while st == oracle.ST_REQUIRES_FOREIGN_CALL and rnd < max_rounds:
                fn, inputs = a.get_pending_foreign_call()
                if not can_answer(j, fn, rnd):
                    break
                a.resolve_pending_foreign_call([v % P if isinstance(v, int) else [x % P for x in v] for v in respond(j, fn, inputs)])
                st, rnd = a.solve(), rnd + 1
            want = a.result().as_tuple()  # (of an instance that still waits the oracle's record holds the status alone)
            assert res[j].as_tuple()[:1 if want[0] == WAITS else 5] == want[:1 if want[0] == WAITS else 5], j
            assert {w: int.from_bytes(vals[j, w].tobytes(), "big") for w in range(asg.shape[1]) if asg[j, w]} == a.witness_map(), j


# ---- a handler that decodes its inputs and encodes its answers on the host, in either space
def decode(b, enc):
    if enc == BE32:
        return int.from_bytes(b, "big")
    x = int.from_bytes(b, "little")
    return x * pow(R256, -1, P) % P if enc == MONT else x


class Handler:
    """respond(caller's row number, function, inputs) per row; seen: (lane, tile, round, function, caller-numbered rows) per call"""

    def __init__(self, space, respond, in_enc=BE32, in_layout=IM, out_enc=BE32, out_layout=IM, decline=lambda r: False, answers=None, returns=None, offsets=(0,)):
        self.space, self.respond, self.in_enc, self.in_layout, self.out_enc, self.out_layout = space, respond, in_enc, in_layout, out_enc, out_layout
        self.decline, self.answers, self.returns, self.offsets = decline, answers, returns, offsets
        self.seen, self.keep = [], {}

    def install(self, node, max_rounds=0):
        node.set_foreign_call_handler(self, space=self.space, in_encoding=self.in_enc, in_layout=self.in_layout, max_rounds=max_rounds)

    def __call__(self, r):
        assert (r.space, r.in_encoding, r.in_layout) == (self.space, self.in_enc, self.in_layout) and r.device == 0
        rows, lens, vals, mask = r.rows_list(), r.lens_list(), r.values_bytes(), r.mask_bytes()
        assert rows == sorted(rows) and len(rows) == r.n_rows and r.max_values == max(sum(x) for x in lens)
        numbers = [self.offsets[r.lane] + r.row_base + i for i in rows]  # global numbers (the device form numbers per lane)
        self.seen.append((r.lane, r.tile, r.round, r.function, numbers))
        if self.returns is not None and self.returns(r) is not None:
            return self.returns(r)
        if self.decline(r):
            return False
        size = acvm_amd.element_size(self.in_enc)
        stride = r.n_rows if self.in_layout == WM else r.max_values
        answers = []
        for i, g in enumerate(numbers):
            flat = []
            for v in range(sum(lens[i])):
                at = fd.index(self.in_layout, stride, i, v)
                assert mask[at] == 1
                flat.append(decode(vals[at * size:(at + 1) * size], self.in_enc))
            inputs, at = [], 0
            for n in lens[i]:
                inputs.append(flat[at:at + n])
                at += n
            answers.append(self.respond(g, r.function, inputs) if self.answers is None or self.answers(g, r.function, r.round) else None)
        given = [a for a in answers if a is not None]
        shape = list(fd.flat(given[0])[0]) if given else []
        total = len(fd.flat(given[0])[1]) if given else 0
        osize = acvm_amd.element_size(self.out_enc)
        ostride = r.n_rows if self.out_layout == WM else total
        buf = bytearray([PAD]) * (max(r.n_rows * total, 1) * osize)
        for i, a in enumerate(answers):
            for k, v in enumerate(fd.flat(a)[1] if a is not None else []):
                at = fd.index(self.out_layout, ostride, i, k)
                buf[at * osize:(at + 1) * osize] = fd.answer_bytes(v, self.out_enc)
        answered = bytes(0 if a is None else 1 + i % 200 for i, a in enumerate(answers)) if self.answers is not None else None
        out = dict(shape=shape, encoding=self.out_enc, layout=self.out_layout, n_columns=total)
        if self.space == acvm_amd.SPACE_HOST:
            out.update(values=bytes(buf) if total else None, answered=answered)
        else:  # the answer's device buffers live until this lane asks again
            d_vals = acvm_amd.DeviceBuffer(data=bytes(buf))
            d_ans = acvm_amd.DeviceBuffer(data=answered) if answered is not None else None
            self.keep[r.lane] = (d_vals, d_ans)
            out.update(values=d_vals.ptr if total else None, answered=d_ans.ptr if d_ans else None)
        return out


# ---- the two node forms behind one face: (results' first three fields, kept, assigned, digests), rows in global order
def lane_split(form, n, n_lanes):
    if form == "host":  # acvm_node_solve's contiguous split
        per = ((n + n_lanes - 1) // n_lanes + 63) // 64 * 64
        return [min(n, per * (d + 1)) - min(n, per * d) for d in range(n_lanes)]
    return [n] if n_lanes == 1 else [n - n // 3, n // 3] if n > 1 else [1, 0]


def run_node(node, form, rows, keep, lanes_n):
    n, nk = len(rows), len(keep)
    if form == "host":
        _, res, kept, asg, dig = node.solve(values_from_rows(rows), n)
        return [r.as_tuple()[:3] for r in res], kept, asg, dig
    lanes, bufs, at = [], [], 0
    for m in lanes_n:
        mk = lambda size: acvm_amd.DeviceBuffer(data=bytes([PAD]) * (size + 16))  # noqa: E731
        b = dict(values=acvm_amd.DeviceBuffer(data=values_from_rows(rows[at:at + m]) + bytes(16)), kept=mk(m * nk * 32), asg=mk(m * nk), status=mk(m), err=mk(m),
                 opcode=mk(4 * m), dig=mk(32 * m))
        bufs.append(b)
        lanes.append(dict(n=m, d_values=b["values"].ptr, d_kept=b["kept"].ptr, d_kept_assigned=b["asg"].ptr, d_status=b["status"].ptr, d_err=b["err"].ptr,
                          d_opcode_index=b["opcode"].ptr, d_digests32=b["dig"].ptr))
        at += m
    node.solve_device(lanes)
    res, kept, asg, dig = [], [], [], []
    for m, b in zip(lanes_n, bufs):
        g = lambda name, size, dtype=np.uint8: np.frombuffer(b[name].download(size), dtype=dtype)  # noqa: E731
        for name, size in (("kept", m * nk * 32), ("asg", m * nk), ("status", m), ("err", m), ("opcode", 4 * m), ("dig", 32 * m)):
            assert b[name].download()[size:] == bytes([PAD]) * 16, name  # the tail
        res += list(zip(g("status", m).tolist(), g("err", m).tolist(), g("opcode", 4 * m, np.uint32).tolist()))
        kept.append(g("kept", m * nk * 32).reshape(m, nk, 32))
        asg.append(g("asg", m * nk).reshape(m, nk))
        dig.append(g("dig", 32 * m).reshape(m, 32))
    return res, np.concatenate(kept), np.concatenate(asg), np.concatenate(dig)


def assert_equals_reference(got, ref):
    res, kept, asg, dig = got
    assert res == [r[:3] for r in ref.results]
    assert np.array_equal(asg, ref.assigned) and np.array_equal(kept, ref.kept) and np.array_equal(dig, ref.digests)


def offsets_of(form, lanes_n):
    return [0] * len(lanes_n) if form == "host" else [sum(lanes_n[:d]) for d in range(len(lanes_n))]


def assert_seen_is_the_waiting_rows(handler, ref):
    """every caller-numbered row the handler saw is exactly the set of waiting rows, once per round"""
    rounds = max((s[2] for s in handler.seen), default=-1) + 1
    assert rounds == len(ref.waiting)
    for rnd, waiting in enumerate(ref.waiting):
        for fn in set(waiting.values()):
            saw = sorted(g for s in handler.seen if s[2] == rnd and s[3] == fn for g in s[4])
            assert saw == sorted(j for j, f in waiting.items() if f == fn), (rnd, fn)


SPACES = {"device": acvm_amd.SPACE_DEVICE, "host": acvm_amd.SPACE_HOST}


@pytest.mark.parametrize("circuit", sorted(CIRCUITS))
@pytest.mark.parametrize("devices", [[0], [0, 0]])
@pytest.mark.parametrize("space", sorted(SPACES))
@pytest.mark.parametrize("form", ["host", "device"])
def test_both_node_forms_and_both_spaces_equal_a_batch_driven_per_instance(oracle, form, space, devices, circuit):
    make, make_rows, respond, keep = CIRCUITS[circuit]
    circ, ids = make()
    data = circ.to_bytes()
    node = acvm_amd.Node(acvm_amd.Circuit(data), ids, keep=keep, devices=devices, tile=TILE)
    io = dict(in_enc=MONT, in_layout=WM, out_enc=LE32, out_layout=WM) if space == "device" else {}
    for n in (165, 1):  # the node is reusable
        rows = make_rows(n)
        ref = Reference(data, ids, rows, keep, respond)
        assert all(r[0] == SOLVED for r in ref.results)
        ref.check_oracle(oracle, data, ids, rows, respond)
        lanes_n = lane_split(form, n, len(devices))
        handler = Handler(SPACES[space], respond, offsets=offsets_of(form, lanes_n), **io)
        handler.install(node)
        assert_equals_reference(run_node(node, form, rows, keep, lanes_n), ref)
        assert_seen_is_the_waiting_rows(handler, ref)
        stats = [node.foreign_stats(d) for d in range(len(devices))]
        assert sum(s["rows_answered"] for s in stats) == sum(len(w) for w in ref.waiting) and sum(s["handler_calls"] for s in stats) == len(handler.seen)
        assert all(s["rows_declined"] == s["rows_left_waiting"] == 0 for s in stats)
        if n == 165 and devices == [0]:
            assert {s[1] for s in handler.seen} == {0, 1, 2}  # two full tiles and a partial one
            assert stats[0]["rounds"] == 3 * len(ref.waiting)
    node.free()


def test_a_declined_site_leaves_exactly_its_rows_waiting(oracle):
    circ, ids = split_circuit()
    data, keep, n = circ.to_bytes(), [4, 5, 6], 165
    rows = split_rows(n)
    can = lambda j, fn, rnd: fn != "odd"  # noqa: E731
    ref = Reference(data, ids, rows, keep, split_respond, can_answer=can)
    ref.check_oracle(oracle, data, ids, rows, split_respond, can_answer=can)
    assert [r[0] for r in ref.results] == [WAITS if j % 2 else SOLVED for j in range(n)]
    node = acvm_amd.Node(acvm_amd.Circuit(data), ids, keep=keep, devices=[0], tile=TILE)
    handler = Handler(acvm_amd.SPACE_DEVICE, split_respond, decline=lambda r: r.function == "odd")
    handler.install(node)
    for form in ("host", "device"):
        del handler.seen[:]
        assert_equals_reference(run_node(node, form, rows, keep, [n]), ref)
        # a declined site is not asked about again in its tile: one call per tile and site
        assert sorted((s[1], s[3]) for s in handler.seen) == [(t, fn) for t in range(3) for fn in ("even", "odd")]
        st = node.foreign_stats(0)
        assert (st["rows_answered"], st["rows_declined"], st["rows_left_waiting"]) == ((n + 1) // 2, n // 2, 0)
    node.free()


@pytest.mark.parametrize("space", sorted(SPACES))
def test_rows_declined_through_the_answered_column(oracle, space):
    circ, ids = fd.relevel_circuit(4)
    data, keep, n = circ.to_bytes(), [5, 6, 9], 165
    rows = fd.relevel_rows(n)
    can = lambda j, fn, rnd: not (fn == "invert" and j % 5 == 2) and not (fn == "double" and j % 64 == 63)  # noqa: E731
    ref = Reference(data, ids, rows, keep, fd.relevel_respond, can_answer=can)
    ref.check_oracle(oracle, data, ids, rows, fd.relevel_respond, can_answer=can)
    left = [j for j in range(n) if j % 5 == 2 or j % 64 == 63]
    assert [j for j, r in enumerate(ref.results) if r[0] == WAITS] == left and all(r[0] in (WAITS, SOLVED) for r in ref.results)
    node = acvm_amd.Node(acvm_amd.Circuit(data), ids, keep=keep, devices=[0, 0], tile=TILE)
    for form in ("host", "device"):
        lanes_n = lane_split(form, n, 2)
        handler = Handler(SPACES[space], fd.relevel_respond, answers=can, offsets=offsets_of(form, lanes_n))
        handler.install(node)
        assert_equals_reference(run_node(node, form, rows, keep, lanes_n), ref)
        stats = [node.foreign_stats(d) for d in range(2)]
        assert sum(s["rows_left_waiting"] for s in stats) == 0 and sum(s["rows_declined"] for s in stats) >= len(left)
    node.free()


def test_an_answer_of_no_values(oracle):
    circ, ids = println_circuit()
    data, keep, n = circ.to_bytes(), [2, 3], 70
    rows = [[5 + j] for j in range(n)]
    respond = lambda j, fn, inputs: []  # noqa: E731
    ref = Reference(data, ids, rows, keep, respond)
    ref.check_oracle(oracle, data, ids, rows, respond)
    node = acvm_amd.Node(acvm_amd.Circuit(data), ids, keep=keep, devices=[0], tile=TILE)
    for space in sorted(SPACES):
        handler = Handler(SPACES[space], respond)
        handler.install(node)
        assert_equals_reference(run_node(node, "host", rows, keep, [n]), ref)
        assert [(s[1], s[3], len(s[4])) for s in handler.seen] == [(0, "println", 64), (1, "println", 6)]
    node.free()


def test_the_round_cap_leaves_rows_waiting_and_says_so(oracle):
    circ, ids = fd.relevel_circuit(4)
    data, keep, n = circ.to_bytes(), [5, 6, 9], 165
    rows = fd.relevel_rows(n)
    ref = Reference(data, ids, rows, keep, fd.relevel_respond, max_rounds=1)
    ref.check_oracle(oracle, data, ids, rows, fd.relevel_respond, max_rounds=1)
    assert all(r[0] == WAITS and r[2] == 2 for r in ref.results)  # every row waits at 'double'
    node = acvm_amd.Node(acvm_amd.Circuit(data), ids, keep=keep, devices=[0], tile=TILE)
    handler = Handler(acvm_amd.SPACE_HOST, fd.relevel_respond)
    handler.install(node, max_rounds=1)
    for form in ("host", "device"):
        del handler.seen[:]
        assert_equals_reference(run_node(node, form, rows, keep, [n]), ref)
        st = node.foreign_stats(0)
        assert (st["rounds"], st["handler_calls"], st["rows_answered"], st["rows_left_waiting"]) == (3, 3, n, n)
        assert {s[3] for s in handler.seen} == {"invert"}
    node.free()


def test_a_failing_handler_fails_the_call_and_leaves_the_node_usable(oracle):
    circ, ids = fd.relevel_circuit(4)
    data, keep, n = circ.to_bytes(), [5, 6, 9], 165
    rows = fd.relevel_rows(n)
    ref = Reference(data, ids, rows, keep, fd.relevel_respond)
    node = acvm_amd.Node(acvm_amd.Circuit(data), ids, keep=keep, devices=[0], tile=TILE)
    for form in ("host", "device"):
        for space in sorted(SPACES):
            bad = Handler(SPACES[space], fd.relevel_respond, returns=lambda r: -7 if r.tile == 1 and r.function == "double" else None)
            bad.install(node)
            with pytest.raises(acvm_amd.AcvmError, match=r"returned -7 for lane 0, tile 1, round 1, site \(opcode 2, brillig index 0, 'double'\)") as e:
                run_node(node, form, rows, keep, [n])
            assert fd.code_of(e) == -7
            # any value but 0, 1 and a negative one is ACVM_E_INVALID
            bad = Handler(SPACES[space], fd.relevel_respond, returns=lambda r: 5 if r.tile == 2 else None)
            bad.install(node)
            with pytest.raises(acvm_amd.AcvmError, match="returned 5 for lane 0, tile 2, round 0") as e:
                run_node(node, form, rows, keep, [n])
            assert fd.code_of(e) == -1

            def raising(r):
                raise ZeroDivisionError("the oracle is down")
            node.set_foreign_call_handler(raising, space=SPACES[space])
            with pytest.raises(ZeroDivisionError, match="the oracle is down"):
                run_node(node, form, rows, keep, [n])
            good = Handler(SPACES[space], fd.relevel_respond)
            good.install(node)
            assert_equals_reference(run_node(node, form, rows, keep, [n]), ref)
    node.free()


def test_without_a_handler_the_node_returns_what_it_returned_before(oracle):
    """uses nothing this handler adds: the rows come back in RequiresForeignCall, exactly as one plain batch leaves them after its first solve"""
    circ, ids = fd.relevel_circuit(4)
    data, keep, n = circ.to_bytes(), [5, 6, 9], 165
    rows = fd.relevel_rows(n)
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), n, ids)
    batch.set_initial_witness(values_from_rows(rows))
    assert batch.solve() == n
    want = [r.as_tuple() for r in batch.results()]
    assert all(r[0] == WAITS and r[2] == 0 for r in want)
    kept = np.zeros((n, len(keep), 32), dtype=np.uint8)
    asg = np.zeros((n, len(keep)), dtype=np.uint8)
    for k, w in enumerate(keep):
        kept[:, k], asg[:, k] = batch.witness(w)
    for devices in ([0], [0, 0]):
        node = acvm_amd.Node(acvm_amd.Circuit(data), ids, keep=keep, devices=devices, tile=TILE)
        not_solved, res, got_kept, got_asg, dig = node.solve(values_from_rows(rows), n)
        assert not_solved == n and [r.as_tuple() for r in res] == want
        assert got_kept.tobytes() == kept.tobytes() and got_asg.tobytes() == asg.tobytes() and dig.tobytes() == batch.digest().tobytes()
        got = run_node(node, "device", rows, keep, lane_split("device", n, len(devices)))
        assert got[0] == [r[:3] for r in want] and got[1].tobytes() == kept.tobytes() and got[2].tobytes() == asg.tobytes() and got[3].tobytes() == dig.tobytes()
        node.free()


def test_refused_handlers():
    circ, ids = fd.relevel_circuit(4)
    gc = acvm_amd.Circuit(circ.to_bytes())
    with_solver = acvm_amd.Node(gc, ids, keep=[5], devices=[0], tile=TILE, solver=acvm_amd.bb_stubbed())
    with pytest.raises(acvm_amd.AcvmError, match="BlackBoxFunctionSolver") as e:
        with_solver.set_foreign_call_handler(lambda r: False)
    assert fd.code_of(e) == -3
    with_solver.set_foreign_call_handler(None)  # no handler is fine
    with_solver.free()
    node = acvm_amd.Node(gc, ids, keep=[5], devices=[0], tile=TILE)
    for kw, text in ((dict(space=2), "unknown space 2"), (dict(in_encoding=9), "unknown encoding 9"), (dict(in_layout=16), "unknown layout 16")):
        with pytest.raises(acvm_amd.AcvmError, match=text) as e:
            node.set_foreign_call_handler(lambda r: False, **kw)
        assert fd.code_of(e) == -1
    # while a node call runs the handler cannot be changed: tried from inside the handler
    refusals = []

    def meddling(r):
        try:
            node.set_foreign_call_handler(None)
        except acvm_amd.AcvmError as err:
            refusals.append(str(err))
        return False
    node.set_foreign_call_handler(meddling, space=acvm_amd.SPACE_HOST)
    n = 3
    not_solved, res, _, _, _ = node.solve(values_from_rows(fd.relevel_rows(n)), n)
    assert not_solved == n and all(r.status == WAITS for r in res)
    assert len(refusals) == 1 and "error -5" in refusals[0] and "a node call is running" in refusals[0]
    node.set_foreign_call_handler(None)  # between calls it can
    node.free()


def test_the_round_trip_moves_eight_bytes_per_waiting_row_and_round_and_no_value():
    """Device space: io_bytes and foreign_stats grow by the 8 bytes per waiting row and round of the batch-wide calls (lane and instance number) plus the
    mask bytes when `answered` is given, and a few words per handler call (shape words, the sizing launches' results, the store's table after it grew:
    below 256 bytes) -- and by nothing per value: a wider encoding of inputs and answers moves the same bytes."""
    circ, ids = fd.relevel_circuit(4)
    data, keep, n = circ.to_bytes(), [5, 6, 9], 165
    rows = fd.relevel_rows(n)
    moved = []
    for masked in (False, True):
        for io in (dict(in_enc=acvm_amd.ENC_U64, out_enc=BE32), dict(in_enc=MONT, in_layout=WM, out_enc=LE32, out_layout=WM)):
            node = acvm_amd.Node(acvm_amd.Circuit(data), ids, keep=keep, devices=[0], tile=TILE)
            handler = Handler(acvm_amd.SPACE_DEVICE, fd.relevel_respond, answers=(lambda j, fn, rnd: True) if masked else None, **io)
            handler.install(node)
            before = node.io_bytes(0)
            not_solved = node.solve(values_from_rows(rows), n)[0]
            assert not_solved == 0
            after, st = node.io_bytes(0), node.foreign_stats(0)
            assert (after[0] - before[0], after[1] - before[1]) == (st["h2d_bytes"], st["d2h_bytes"])
            row_rounds, calls = 2 * n, 6  # two rounds, three tiles, one site each
            assert (st["rows_answered"], st["handler_calls"]) == (row_rounds, calls)
            assert 8 * row_rounds <= st["h2d_bytes"] <= 8 * row_rounds + 256 * calls
            mask_bytes = row_rounds if masked else 0
            assert mask_bytes <= st["d2h_bytes"] <= mask_bytes + 64 * calls
            moved.append((st["h2d_bytes"], st["d2h_bytes"]))
            node.free()
    assert moved[0] == moved[1] and moved[2] == moved[3]
    assert moved[2][1] - moved[0][1] == 2 * n and moved[2][0] == moved[0][0]
