"""Per-row answers of the batch-wide foreign-call round trip (acvm_batch_resolve_foreign_calls_device_rows): the lengths of a HeapVector output as a
device column (d_lens) and the rows that are answered as a device column (d_answered). Two handles run in lockstep as in
tests/test_gpu_foreign_device.py: `dev` is answered by the per-row call, `ref` by the per-instance call, and every result, assigned set and witness
map must be equal and equal the CPU oracle's, driven through ACVM::resolve_pending_foreign_call (acvm/src/pwg/mod.rs:203-228). The columns of rows
that are left out hold garbage (values, and lengths beyond any buffer): nothing of them may be read into a result or into the sizing."""
import pytest

import acvm_amd
from acvm_amd import ENC_BE32 as BE32, ENC_LE32 as LE32, ENC_MONT256_LE as MONT, LAYOUT_INSTANCE_MAJOR as IM, LAYOUT_WITNESS_MAJOR as WM
from acvm_amd.acir import P, Brillig, Circuit, Expression as E

import test_gpu_foreign_device as fd

pytestmark = pytest.mark.gpu
W = E.from_witness
WAITS, SOLVED = acvm_amd.STATUS_REQUIRES_FOREIGN_CALL, acvm_amd.STATUS_SOLVED
PAD = fd.PAD
GARBAGE_LEN = 0xFFFFFFF0


def vec_circuit(n_tail=6):
    """[w3, w4, w5] = the slice an oracle returns for w1, zero filled; w6 = its length; w7 = the single value behind it; then gates over them"""
    code = [("Const", 2, 20), ("Const", 5, 0)]
    for k in range(3):  # memory 20 .. 22 = 0: defined whatever the slice's length
        code += [("Const", 6, 20 + k), ("Store", 6, 5)]
    code += [("ForeignCall", "vec", [("HeapVector", 2, 3), ("Register", 4)], [("Register", 0)]), ("Mov", 0, 2), ("Mov", 1, 3), ("Mov", 2, 4), ("Stop",)]
    ops = [Brillig(inputs=[W(1)], outputs=[[3, 4, 5], 6, 7], bytecode=code), E([(1, 3, 7)], [(1, 6), (1, 5), (P - 1, 8)], 0)]
    nw = 8
    for _ in range(n_tail):
        ops.append(E([(1, nw, nw - 1)], [(1, 4), (P - 1, nw + 1)], 0))
        nw += 1
    return Circuit(nw, ops), [1]


def vec_respond(j, fn, inputs):
    assert fn == "vec"
    x = inputs[0][0]
    return [[(x * (k + 2) + j) % P for k in range((j * 7 + 3) % 4 if j else 0)], (x * 3 + 1) % P]


def vec_rows(B):
    return [[11 + 5 * j] for j in range(B)]


def resolve_per_row(dev, site, answers, first_row=0, enc=BE32, layout=IM, pad=0, n_columns=None, with_lens=True, with_mask=True):
    """answers: per row of the range a ForeignCallResult of the Python view, or None for a row that is left out. Arrays may differ in length from row
    to row (with_lens). Returns the device maximum: the largest total among the answered rows."""
    given = [a for a in answers if a is not None]
    kinds = tuple(isinstance(v, list) for v in (given[0] if given else []))
    assert all(tuple(isinstance(v, list) for v in a) == kinds for a in given)
    n, n_values = len(answers), len(kinds)
    totals = [len(fd.flat(a)[1]) for a in given]
    longest = max(totals, default=0)
    n_columns = longest if n_columns is None else n_columns
    size = fd.size_of(enc)
    stride = (n if layout == WM else n_columns) + pad
    buf = bytearray([PAD]) * (fd.extent(layout, stride, n, max(n_columns, 1)) * size + 64)
    lens = []
    for i, a in enumerate(answers):
        if a is None:
            lens += [GARBAGE_LEN] * n_values
            continue
        lens += [len(v) if isinstance(v, list) else GARBAGE_LEN for v in a]  # (ignored for a single value)
        for k, v in enumerate(fd.flat(a)[1]):
            at = fd.index(layout, stride, i, k)
            buf[at * size:(at + 1) * size] = fd.answer_bytes(v, enc)
    if with_lens:
        shape = [1 if is_arr else None for is_arr in kinds]
    else:
        assert all(fd.flat(a)[0] == fd.flat(given[0])[0] for a in given)
        shape = list(fd.flat(given[0])[0]) if given else []
    d = acvm_amd.DeviceBuffer(data=bytes(buf))
    d_lens = acvm_amd.DeviceBuffer(data=b"".join(x.to_bytes(4, "little") for x in lens) + bytes([PAD]) * 16)
    d_mask = acvm_amd.DeviceBuffer(data=bytes(0 if a is None else 1 + i % 250 for i, a in enumerate(answers)) + bytes([PAD]) * 16)
    assert with_mask or len(given) == n
    dev.resolve_foreign_calls_device_rows(site["opcode_index"], site["brillig_index"], shape, d.ptr, first_row=first_row, n_rows=n, encoding=enc, layout=layout,
                                          n_columns=n_columns, stride=stride if pad else 0, d_lens=d_lens.ptr if with_lens else None,
                                          d_answered=d_mask.ptr if with_mask else None)
    return longest


def site_of(dev, fn):
    (site,) = [s for s in dev.foreign_call_sites() if s["function"] == fn]
    return site


def finish(oracle, data, ids, rows, respond, dev, ref):
    assert fd.snapshot(dev) == fd.snapshot(ref)
    fd.check_against_oracle(oracle, data, ids, rows, respond, dev)


@pytest.mark.parametrize("relevel", [0, 1])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_a_vector_output_of_zero_to_three_values_per_row(oracle, B, relevel):
    circ, ids = vec_circuit()
    rows = vec_rows(B)
    with acvm_amd.tuning(fc_relevel=relevel):
        data, dev, ref = fd.two_handles(circ, ids, rows)
        dev.solve()
        ref.solve()
        site = site_of(dev, "vec")
        inst, pend = fd.waiting_at(dev, ref, site)
        assert inst == list(range(B))
        answers = [vec_respond(j, "vec", pend[j][1]) for j in inst]
        if B >= 63:
            assert {len(a[0]) for a in answers} == {0, 1, 2, 3}
        layout, enc = (WM, MONT) if B % 2 else (IM, BE32)
        resolve_per_row(dev, site, answers, enc=enc, layout=layout, pad=B % 3, with_mask=False)
        for j, a in zip(inst, answers):
            ref.resolve_pending_foreign_call(j, a)
        assert site_of(dev, "vec")["n_resolved"] == B
        assert dev.solve() == ref.solve()
    assert all(r[0] == SOLVED for r in fd.snapshot(dev)[0])
    finish(oracle, data, ids, rows, vec_respond, dev, ref)


MASKS = {"none": lambda i, n: False, "all": lambda i, n: True, "alternating": lambda i, n: i % 2 == 0, "last": lambda i, n: i == n - 1}


MASK_CIRCUITS = {"relevel": (lambda: fd.relevel_circuit(4), fd.relevel_rows, fd.relevel_respond, ("invert", "double"), False),
                 "vec": (vec_circuit, vec_rows, vec_respond, ("vec",), True)}


@pytest.mark.parametrize("circuit", sorted(MASK_CIRCUITS))
@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_masks_and_a_second_call_for_the_rows_left_out(oracle, B, mask, circuit):
    """every round of the circuit: a first call answers the rows of the mask, a second one of the same round the others. At B = 63 and 257 the last wave
    of both kernels is partial; the vec circuit adds the length column, so that the sizing launch sees the mask too. fc_relevel alternates with B."""
    make, make_rows, respond, fns, with_lens = MASK_CIRCUITS[circuit]
    circ, ids = make()
    rows = make_rows(B)
    with acvm_amd.tuning(fc_relevel=(B + len(mask)) % 2):
        data, dev, ref = fd.two_handles(circ, ids, rows)
        for fn in fns:
            dev.solve()
            ref.solve()
            site = site_of(dev, fn)
            inst, pend = fd.waiting_at(dev, ref, site)
            answers = [respond(j, fn, pend[j][1]) for j in inst]
            first = [a if MASKS[mask](i, B) else None for i, a in enumerate(answers)]
            store = dev.foreign_call_stats()["store_bytes"]
            resolve_per_row(dev, site, first, with_lens=with_lens, layout=WM)
            n_first = sum(a is not None for a in first)
            assert site_of(dev, fn)["n_resolved"] == n_first
            if not n_first:
                assert dev.foreign_call_stats()["store_bytes"] == store  # nothing was appended, nothing reserved
            if n_first < B:
                resolve_per_row(dev, site, [None if a is not None else answers[i] for i, a in enumerate(first)], with_lens=with_lens, enc=LE32)
            assert site_of(dev, fn)["n_resolved"] == B
            for j, a in zip(inst, answers):
                ref.resolve_pending_foreign_call(j, a)
        assert dev.solve() == ref.solve()
    assert all(r[0] == SOLVED for r in fd.snapshot(dev)[0])
    finish(oracle, data, ids, rows, respond, dev, ref)


def test_a_row_left_out_of_every_call_still_waits(oracle):
    circ, ids = vec_circuit()
    B = 70
    rows = vec_rows(B)
    left_out = 37
    data, dev, ref = fd.two_handles(circ, ids, rows)
    dev.solve()
    ref.solve()
    site = site_of(dev, "vec")
    inst, pend = fd.waiting_at(dev, ref, site)
    answers = [vec_respond(j, "vec", pend[j][1]) for j in inst]
    resolve_per_row(dev, site, [a if j % 2 and j != left_out else None for j, a in zip(inst, answers)])
    resolve_per_row(dev, site, [a if j % 2 == 0 and j != left_out else None for j, a in zip(inst, answers)], layout=WM)
    assert site_of(dev, "vec")["n_resolved"] == B - 1
    for j, a in zip(inst, answers):
        if j != left_out:
            ref.resolve_pending_foreign_call(j, a)
    assert dev.solve() == ref.solve()
    status = [r[0] for r in fd.snapshot(dev)[0]]
    assert status == [WAITS if j == left_out else SOLVED for j in range(B)]
    assert fd.snapshot(dev) == fd.snapshot(ref)
    (site,) = dev.foreign_call_sites()
    assert (site["n_waiting"], site["n_resolved"]) == (1, 0)
    # the row that waited is answered in the next round, alone
    resolve_per_row(dev, site, [answers[left_out]])
    ref.resolve_pending_foreign_call(left_out, answers[left_out])
    assert dev.solve() == ref.solve() == 0
    finish(oracle, data, ids, rows, vec_respond, dev, ref)


def test_a_buffer_one_column_below_the_device_maximum_is_refused_and_nothing_written(oracle):
    circ, ids = vec_circuit()
    B = 66
    rows = vec_rows(B)
    data, dev, ref = fd.two_handles(circ, ids, rows)
    dev.solve()
    ref.solve()
    site = site_of(dev, "vec")
    inst, pend = fd.waiting_at(dev, ref, site)
    answers = [vec_respond(j, "vec", pend[j][1]) for j in inst]
    longest = max(len(a[0]) + 1 for a in answers)
    assert longest == 4
    before = fd.snapshot(dev), dev.foreign_call_stats()["store_bytes"]
    with pytest.raises(acvm_amd.AcvmError, match="n_columns 3 is below the 4 values of the longest answered row") as e:
        resolve_per_row(dev, site, answers, n_columns=longest - 1)
    assert fd.code_of(e) == -1
    # only the rows that are answered count: with the long rows left out the same width is enough
    short = [a if len(a[0]) < 3 else None for a in answers]
    assert site_of(dev, "vec")["n_resolved"] == 0 and (fd.snapshot(dev), dev.foreign_call_stats()["store_bytes"]) == before
    resolve_per_row(dev, site, short, n_columns=longest - 1)
    assert site_of(dev, "vec")["n_resolved"] == sum(a is not None for a in short)
    resolve_per_row(dev, site, [a if s is None else None for a, s in zip(answers, short)], n_columns=longest + 2, layout=WM, pad=1)
    for j, a in zip(inst, answers):
        ref.resolve_pending_foreign_call(j, a)
    assert dev.solve() == ref.solve() == 0
    finish(oracle, data, ids, rows, vec_respond, dev, ref)


def test_mixed_with_the_range_call_and_the_per_instance_call(oracle):
    circ, ids = fd.relevel_circuit(4)
    B = 66
    rows = fd.relevel_rows(B)
    data, dev, ref = fd.two_handles(circ, ids, rows)
    for rnd, fn in enumerate(("invert", "double")):
        dev.solve()
        ref.solve()
        site = site_of(dev, fn)
        inst, pend = fd.waiting_at(dev, ref, site)
        answers = [fd.relevel_respond(j, fn, pend[j][1]) for j in inst]
        parts = [(0, 20), (20, 45), (45, B)]
        order = parts if rnd == 0 else parts[::-1]
        for lo, hi in order:
            if (lo, hi) == parts[0]:
                fd.resolve_rows(dev, site, fd.IO(), answers[lo:hi], first_row=lo)
            elif (lo, hi) == parts[1]:
                resolve_per_row(dev, site, [a if (lo + i) % 3 else None for i, a in enumerate(answers[lo:hi])], first_row=lo, with_lens=False)
            else:
                for j, a in zip(inst[lo:hi], answers[lo:hi]):
                    dev.resolve_pending_foreign_call(j, a)
        # a row that was answered and is marked answered again: refused as a whole; the same row left out: fine
        resolved = site_of(dev, fn)["n_resolved"]
        with pytest.raises(acvm_amd.AcvmError, match="was already answered since the last solve") as e:
            resolve_per_row(dev, site, answers[19:22], first_row=19, with_lens=False)
        assert fd.code_of(e) == -5 and site_of(dev, fn)["n_resolved"] == resolved
        rest = [a if i % 3 == 0 else None for i, a in enumerate(answers)]
        rest = [a if 20 <= i < 45 else None for i, a in enumerate(rest)]
        resolve_per_row(dev, site, rest, with_lens=False, layout=WM)  # the whole list, answered rows masked out
        assert site_of(dev, fn)["n_resolved"] == B
        for j, a in zip(inst, answers):
            ref.resolve_pending_foreign_call(j, a)
    assert dev.solve() == ref.solve() == 0
    finish(oracle, data, ids, rows, fd.relevel_respond, dev, ref)


def test_a_result_of_no_values_and_an_empty_range(oracle):
    """the println shape: a ForeignCall without destinations is answered by a result of no values, for the rows of a mask"""
    circ = Circuit(3, [Brillig(inputs=[W(1)], outputs=[2], bytecode=[("ForeignCall", "println", [], [("Register", 0)]), ("Stop",)]),
                       E([(1, 1, 2)], [(P - 1, 3)], 0)])
    B = 65
    rows = [[5 + j] for j in range(B)]
    respond = lambda j, fn, inputs: []  # noqa: E731
    data, dev, ref = fd.two_handles(circ, [1], rows)
    dev.solve()
    ref.solve()
    site = site_of(dev, "println")
    dev.resolve_foreign_calls_device_rows(site["opcode_index"], site["brillig_index"], [], None, first_row=3, n_rows=0)
    assert site_of(dev, "println")["n_resolved"] == 0
    mask = acvm_amd.DeviceBuffer(data=bytes(j % 2 for j in range(B)))
    dev.resolve_foreign_calls_device_rows(site["opcode_index"], site["brillig_index"], [], None, d_answered=mask.ptr)
    assert site_of(dev, "println")["n_resolved"] == B // 2
    for j in range(1, B, 2):
        ref.resolve_pending_foreign_call(j, [])
    assert dev.solve() == ref.solve()
    assert [r[0] for r in fd.snapshot(dev)[0]] == [SOLVED if j % 2 else WAITS for j in range(B)]
    assert fd.snapshot(dev) == fd.snapshot(ref)
    mask = acvm_amd.DeviceBuffer(data=bytes([1]) * (B - B // 2))
    dev.resolve_foreign_calls_device_rows(site["opcode_index"], site["brillig_index"], [], None, d_answered=mask.ptr)
    for j in range(0, B, 2):
        ref.resolve_pending_foreign_call(j, [])
    assert dev.solve() == ref.solve() == 0
    finish(oracle, data, [1], rows, respond, dev, ref)
