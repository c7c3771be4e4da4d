"""The checks and the list layout of every device import (acvm_amd/csrc/import_plan.cpp) without a device and without a handle: the module is
compiled as plain C++ (tools/import_plan_host_test.cpp) and its answers -- the plan, or the refusal with its code and text -- are judged by the
Python restatement below. The refusals are those the GPU tests assert (tests/test_gpu_import_device.py test_refusals_leave_the_handle_usable,
tests/test_gpu_typed_io.py test_parts_refusals_leave_the_previous_import_in_place), with the same texts."""
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE32, LE32, MONT, U8, U16, U32, U64, U128 = 0, 1, 2, 16, 17, 18, 19, 20
ENCODINGS = (BE32, LE32, MONT, U8, U16, U32, U64, U128)
IM, WM, BC = 0, 1, 16
NONE = 0xFFFFFFFF
PTR = 1 << 20  # a device address aligned to everything


def size_of(encoding):
    return 1 << (encoding - U8) if U8 <= encoding <= U128 else 32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    """the tool compiled as it is, and the second binary of `make asan` (AddressSanitizer + UndefinedBehaviorSanitizer): a stand-alone program on
    the CPU, given the same command streams -- a report ends it with a non-zero status"""
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("import_plan") / "import_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "import_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "import_plan.cpp"),
                               "-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "import_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/import_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith(("view", "noview")) for c in commands)
        return lines
    return run


# ---- the command stream
def fmt(lst):
    return "null" if lst is None else "e" if not len(lst) else ",".join(str(x) for x in lst)


class View:
    """what the checks see of a handle: B, per position the id, the row (the id, or a slot under slot reuse) and the byte plane"""

    def __init__(self, B, ids, rows=None, planes=None):
        self.B, self.ids, self.rows, self.planes = B, list(ids), list(ids if rows is None else rows), None if planes is None else list(planes)
        self.n_in = len(self.ids)

    def command(self):
        return "view %d %d %s %s %s" % (self.B, self.n_in, fmt(self.ids), fmt(self.rows), fmt(self.planes))


def desc(encoding=BE32, layout=IM, columns=None, n_columns=0, stride=0, ptr=PTR):
    return dict(encoding=encoding, layout=layout, columns=columns, n_columns=n_columns, stride=stride, ptr=ptr)


def part(positions, encoding=U8, layout=WM, columns=None, n_columns=0, stride=0, ptr=PTR, n=None):
    return dict(desc(encoding, layout, columns, n_columns, stride, ptr), positions=positions, n=len(positions) if n is None else n)


def desc_command(d):
    return "desc null" if d is None else "desc %d %d %d %d %d %s" % (d["encoding"], d["layout"], d["n_columns"], d["stride"], d["ptr"], fmt(d["columns"]))


def parts_command(parts):
    return "parts %d " % len(parts) + " ".join("%d %d %d %d %d %d %s %s" % (p["ptr"], p["encoding"], p["layout"], p["n"], p["n_columns"], p["stride"], fmt(p["positions"]),
                                                                           fmt(p["columns"])) for p in parts)


# ---- the restatement: ("err", text) or ("ok", plain, [part tuples], lists)
def model_buffer(view, d, n, is_part):
    """the checks of one described buffer in their order; returns (error text or None, part tuple without the list offsets, plain)"""
    e, layout = d["encoding"], d["layout"]
    if not (e < 3 or U8 <= e <= U128):
        return "unknown encoding %d" % e, None, False
    if not (layout in (IM, WM) or (is_part and layout == BC)):
        return "unknown layout %d" % layout, None, False
    if view is None:
        return "null batch", None, False
    if n and not d["ptr"]:
        return "null values", None, False
    n_columns = n if d["columns"] is None else d["n_columns"]
    for k, c in enumerate((d["columns"] or [])[:n]):
        if c >= n_columns:
            return "column %d of initial witness %d is not below n_columns %d" % (c, k, n_columns), None, False
    if layout == BC:
        stride = 1
    else:
        dense = view.B if layout == WM else n_columns
        stride = d["stride"] or dense
        if stride < dense:
            return "stride %d is below the dense stride %d of the layout" % (stride, dense), None, False
        if (n_columns if layout == WM else view.B) * stride > 1 << 57:
            return "stride %d is beyond any device buffer" % stride, None, False
    plain = not is_part and e == BE32 and layout == IM and d["columns"] is None and stride == view.n_in
    size = size_of(e)
    if not plain and d["ptr"] % min(size, 16):
        return ("d_values must be 16-byte aligned" if size == 32 else "d_values must be aligned to the element size, %d bytes" % size), None, False
    return None, (e, layout, size, stride, n, d["ptr"]), plain


def model_desc(view, d):
    if d is None:
        return ("err", "null argument")
    err, shape, plain = model_buffer(view, d, view.n_in if view else 0, False)
    if err:
        return ("err", err)
    has = d["columns"] is not None
    return ("ok", plain, [shape + (1, -1, -1, 0 if has else -1)], list(d["columns"][:view.n_in]) if has else [])


def model_parts(view, parts):
    shapes = []
    for q, p in enumerate(parts):
        err, shape, _ = model_buffer(view, p, p["n"], True)
        if not err and p["n"] and p["positions"] is None:
            err = "null positions"
        if err:
            return ("err", "part %d: %s" % (q, err))
        shapes.append(shape)
    if view is None:
        return ("err", "null batch")
    owner = {}
    for q, p in enumerate(parts):
        for pos in (p["positions"] or [])[:p["n"]]:
            if pos >= view.n_in:
                return ("err", "part %d: position %d is not below n_initial %d" % (q, pos, view.n_in))
            if pos in owner:
                return ("err", "position %d is supplied twice (parts %d and %d)" % (pos, owner[pos], q))
            owner[pos] = q
    for pos in range(view.n_in):
        if pos not in owner:
            return ("err", "position %d (initial witness %d) is supplied by no part" % (pos, view.ids[pos]))
    lists, out = [], []
    for p, shape in zip(parts, shapes):
        positions = (p["positions"] or [])[:p["n"]]
        rows_at = len(lists)
        lists += [view.rows[pos] for pos in positions]
        planes_at = -1
        if view.planes is not None:
            planes_at = len(lists)
            lists += [view.planes[pos] for pos in positions]
        columns_at = -1
        if p["columns"] is not None:
            columns_at = len(lists)
            lists += list(p["columns"][:p["n"]])
        out.append(shape + (0, rows_at, planes_at, columns_at))
    return ("ok", False, out, lists)


def parse(line):
    if line.startswith("err "):
        code, text = line[4:].split(" ", 1)
        assert int(code) == -1, line  # ACVM_E_INVALID
        return ("err", text)
    tok = line.split()
    assert tok[0] == "ok", line
    n_parts = int(tok[2])
    parts = [tuple(int(x) for x in tok[3 + 10 * q:13 + 10 * q]) for q in range(n_parts)]
    lists = [] if tok[3 + 10 * n_parts] == "e" else [int(x) for x in tok[3 + 10 * n_parts].split(",")]
    return ("ok", bool(int(tok[1])), parts, lists)


def ask(tool, calls):
    """calls: (view or None, "desc" / "parts", argument). Returns [(parsed answer, restated answer)]."""
    commands = []
    for view, kind, arg in calls:
        commands.append(view.command() if view else "noview")
        commands.append(desc_command(arg) if kind == "desc" else parts_command(arg))
    got = [parse(g) for g in tool(commands)]
    want = [model_desc(v, a) if kind == "desc" else model_parts(v, a) for v, kind, a in calls]
    return list(zip(got, want))


def assert_agree(tool, calls):
    answers = ask(tool, calls)
    for (got, want), call in zip(answers, calls):
        assert got == want, call[1:]
    return [g for g, _ in answers]


# ---- 1. the refusals of the GPU tests
def test_refusals_of_the_descriptor_tests(tool):
    n_in, B = 5, 65
    v = View(B, range(1, n_in + 1))
    calls = [
        (desc(stride=n_in - 1), "stride 4 is below the dense stride 5 of the layout"),
        (desc(layout=WM, stride=B - 1), "stride 64 is below the dense stride 65 of the layout"),
        (desc(columns=[0, 1, 2, 3, 4], n_columns=7, stride=6), "stride 6 is below the dense stride 7 of the layout"),
        (desc(columns=[0, 1, 2, 3, 7], n_columns=7), "column 7 of initial witness 4 is not below n_columns 7"),
        (desc(encoding=3), "unknown encoding 3"),
        (desc(encoding=15), "unknown encoding 15"),
        (desc(encoding=21), "unknown encoding 21"),
        (desc(layout=2), "unknown layout 2"),
        (desc(layout=BC), "unknown layout 16"),  # (the broadcast layout belongs to parts)
        (desc(encoding=LE32, ptr=PTR + 8), "d_values must be 16-byte aligned"),
        (desc(encoding=BE32, stride=n_in + 1, ptr=PTR + 8), "d_values must be 16-byte aligned"),  # (not the plain shape: a stride above dense)
        (desc(ptr=0), "null values"),
        (desc(encoding=U8, layout=WM, stride=B - 1), "stride 64 is below the dense stride 65 of the layout"),
        (None, "null argument"),
    ] + [(desc(encoding=e, layout=WM, ptr=PTR + lead), "d_values must be aligned to the element size, %d bytes" % size_of(e)) for e, lead in ((U16, 1), (U32, 2), (U64, 4), (U128, 8))]
    got = assert_agree(tool, [(v, "desc", d) for d, _ in calls])
    assert got == [("err", text) for _, text in calls]
    # encoding and layout are judged before the null batch, everything else behind it
    got = assert_agree(tool, [(None, "desc", desc(encoding=21)), (None, "desc", desc(layout=2)), (None, "desc", desc(encoding=U8, layout=WM, ptr=16)), (None, "desc", None)])
    assert got == [("err", "unknown encoding 21"), ("err", "unknown layout 2"), ("err", "null batch"), ("err", "null argument")]


def test_refusals_of_the_parts_test(tool):
    n_in, B = 4, 65
    v = View(B, range(1, n_in + 1))
    calls = [
        ([part([0, 1]), part([3])], "position 2 (initial witness 3) is supplied by no part"),
        ([part([0, 1, 2]), part([2, 3])], "position 2 is supplied twice (parts 0 and 1)"),
        ([part([0, 1, 1, 2, 3])], "position 1 is supplied twice (parts 0 and 0)"),
        ([part([0, 1, 2]), part([4])], "part 1: position 4 is not below n_initial 4"),
        ([part([0, 1]), part([2, 3], ptr=PTR + 8, encoding=U128)], "part 1: d_values must be aligned to the element size, 16 bytes"),
        ([part([0, 1]), part([2, 3], ptr=PTR + 8, encoding=LE32)], "part 1: d_values must be 16-byte aligned"),
        ([part([0, 1]), part([2, 3], encoding=21)], "part 1: unknown encoding 21"),
        ([part([0, 1]), part([2, 3], layout=2)], "part 1: unknown layout 2"),
        ([part([0, 1]), part([2, 3], stride=B - 1)], "part 1: stride 64 is below the dense stride 65 of the layout"),
        ([part([0, 1]), part([2, 3], columns=[0, 2], n_columns=2)], "part 1: column 2 of initial witness 1 is not below n_columns 2"),
        ([part([0, 1]), part([2, 3], ptr=0)], "part 1: null values"),
        ([part([0, 1]), part(None, n=2)], "part 1: null positions"),
        ([], "position 0 (initial witness 1) is supplied by no part"),
    ]
    got = assert_agree(tool, [(v, "parts", p) for p, _ in calls])
    assert got == [("err", text) for _, text in calls]
    # the texts match what tests/test_gpu_typed_io.py looks for
    for (_, text), pattern in zip(calls, ("position 2 .*no part", "position 2 .*twice", "position 1 .*twice", "position 4 ", "part 1: .*aligned", "part 1: .*aligned", "part 1: .*encoding",
                                          "part 1: .*layout", "part 1: .*stride", "part 1: .*column", "part 1: .*null")):
        assert re.search(pattern, text)
    # a part's shape is judged before the null batch, and the first refusal of the first refused part wins
    got = assert_agree(tool, [(None, "parts", [part([0], encoding=U8, layout=BC)]), (None, "parts", [part([0], layout=2)]), (None, "parts", [part([0], encoding=21, layout=BC)]),
                              (None, "parts", []), (v, "parts", [part([9], layout=3), part([0], encoding=5)])])
    assert got == [("err", "part 0: null batch"), ("err", "part 0: unknown layout 2"), ("err", "part 0: unknown encoding 21"), ("err", "null batch"), ("err", "part 0: unknown layout 3")]
    assert tool([v.command(), "parts null 2", "noview", "parts null 0"]) == ["err -1 null argument", "err -1 null batch"]


# ---- 2. strides
def test_stride_edges(tool):
    B, n_in, n_columns = 70, 5, 9
    v = View(B, range(1, n_in + 1))
    cols = [8, 0, 3, 3, 1]
    calls = []
    for layout, dense in ((IM, n_columns), (WM, B)):
        calls += [(v, "desc", desc(LE32, layout, cols, n_columns, s)) for s in (dense - 1, dense, 0, dense + 1)]
        calls += [(v, "parts", [part(range(n_in), LE32, layout, cols, n_columns, s)]) for s in (dense - 1, dense, 0, dense + 1)]
    got = assert_agree(tool, calls)
    for base, dense in ((0, n_columns), (8, B)):
        for at in (base, base + 4):
            assert got[at][0] == "err" and "below the dense stride %d" % dense in got[at][1]
            assert [g[2][0][3] for g in got[at + 1:at + 4]] == [dense, dense, dense + 1]  # (0 means dense; the stride comes back as launched)
    # rows * stride == 2^57 is accepted, one more is refused; rows is the column count witness-major and B instance-major
    B2, nc2 = 1 << 10, 1 << 5
    v2 = View(B2, [1])
    calls = []
    for layout, rows in ((WM, nc2), (IM, B2)):
        top = (1 << 57) // rows
        calls += [(v2, "desc", desc(U8, layout, [nc2 - 1], nc2, top)), (v2, "desc", desc(U8, layout, [nc2 - 1], nc2, top + 1)),
                  (v2, "parts", [part([0], U8, layout, [nc2 - 1], nc2, top)]), (v2, "parts", [part([0], U8, layout, [nc2 - 1], nc2, top + 1)])]
    got = assert_agree(tool, calls)
    assert [g[0] for g in got] == ["ok", "err"] * 4
    assert all("is beyond any device buffer" in g[1] for g in got[1::2])
    # broadcast ignores the stride: any value, launched as 1
    got = assert_agree(tool, [(v, "parts", [part(range(n_in), U16, BC, cols, n_columns, s)]) for s in (0, 1, 3, 1 << 63)])
    assert all(g[0] == "ok" and g[2][0][3] == 1 for g in got)


# ---- 3. alignment
def test_alignment_of_every_element_size(tool):
    v = View(3, [1, 2])
    calls, want = [], []
    for e in ENCODINGS:
        align = min(size_of(e), 16)
        for ptr in (PTR + align, PTR + align - 1):
            for layout in (IM, WM):
                calls += [(v, "desc", desc(e, layout, ptr=ptr, stride=7)), (v, "parts", [part([0, 1], e, layout, ptr=ptr, stride=7)])]
                want += ["ok" if ptr % align == 0 else "err"] * 2
            calls.append((v, "parts", [part([1, 0], e, BC, ptr=ptr)]))
            want.append("ok" if ptr % align == 0 else "err")
    got = assert_agree(tool, calls)
    assert [g[0] for g in got] == want and want.count("err") == 5 * 7  # (U8 takes any pointer)
    # the plain descriptor reads any pointer; the same shape as a part does not
    calls = [(v, "desc", desc(ptr=PTR + 1)), (v, "desc", desc(ptr=PTR + 1, stride=2)), (v, "parts", [part([0, 1], BE32, IM, ptr=PTR + 1)]), (v, "parts", [part([0, 1], BE32, IM, ptr=PTR + 16)])]
    got = assert_agree(tool, calls)
    assert [g[0] for g in got] == ["ok", "ok", "err", "ok"] and got[0][1] and got[1][1] and not got[3][1]


# ---- 4. degenerate shapes
def test_degenerate_shapes(tool):
    none = View(3, [])
    one = View(1, [7, 9, 8], planes=[NONE, 0, 1])
    calls = [
        (none, "desc", desc()), (none, "desc", desc(ptr=0)), (none, "desc", desc(U8, WM, [], 0, ptr=0)), (none, "desc", desc(stride=4)),   # n_in == 0
        (none, "parts", []), (none, "parts", [part([], ptr=0)]), (none, "parts", [part([0])]),
        (one, "parts", []),                                                                                                             # n_parts == 0, n_in > 0
        (one, "parts", [part([2, 0]), part([], U64, IM, ptr=0), part([1], BE32, BC)]),                                                   # a part with n == 0
        (one, "parts", [part([], U64, IM, ptr=0, columns=[], n_columns=0), part([2, 1, 0], U32, IM, columns=[0, 0, 0], n_columns=1)]),
        (one, "desc", desc(U16, WM)), (one, "desc", desc(MONT, IM, [2, 2, 0], 3)),                                                       # B == 1
    ]
    got = assert_agree(tool, calls)
    assert [g[0] for g in got] == ["ok", "ok", "ok", "ok", "ok", "ok", "err", "err", "ok", "ok", "ok", "ok"]
    assert got[0][1] and got[1][1] and not got[2][1] and not got[3][1]  # (without initial witnesses the dense stride is 0)
    assert got[4] == ("ok", False, [], []) and got[5][3] == []
    assert got[8][3] == [8, 7, 1, NONE, 9, 0] and [p[7:] for p in got[8][2]] == [(0, 2, -1), (4, 4, -1), (4, 5, -1)]
    assert got[10][2][0][3] == 1  # (the dense witness-major stride is B)


# ---- 5. the list layout
@pytest.mark.parametrize("with_planes", [False, True])
@pytest.mark.parametrize("slot_reuse", [False, True])
def test_list_layout(tool, with_planes, slot_reuse):
    ids = [4, 9, 2, 11, 5, 30, 6]
    v = View(130, ids, rows=[40 + 3 * k for k in range(len(ids))] if slot_reuse else None, planes=[0, NONE, 1, 2, NONE, NONE, 3] if with_planes else None)
    parts = [part([6, 0, 3], U8, WM), part([], U32, IM, ptr=0), part([5, 1], MONT, IM, columns=[4, 0], n_columns=6), part([2, 4], LE32, BC, columns=[1, 1], n_columns=2)]
    (got,) = assert_agree(tool, [(v, "parts", parts)])
    assert got[0] == "ok" and not got[1]
    lists, at = got[3], 0
    for p, g in zip(parts, got[2]):
        pos, resident, rows_at, planes_at, columns_at = p["positions"], g[6], g[7], g[8], g[9]
        assert not resident and rows_at == at and lists[at:at + len(pos)] == [v.rows[x] for x in pos]
        at += len(pos)
        if with_planes:
            assert planes_at == at and lists[at:at + len(pos)] == [v.planes[x] for x in pos]
            at += len(pos)
        else:
            assert planes_at == -1
        if p["columns"] is not None:
            assert columns_at == at and lists[at:at + len(pos)] == p["columns"]
            at += len(pos)
        else:
            assert columns_at == -1
    assert at == len(lists) == (3 + 2 + 2) * (2 if with_planes else 1) + 4
    assert (v.rows == ids) != slot_reuse


# ---- 6. a descriptor and its one-part twin
def test_descriptor_and_one_part_agree(tool):
    ids = [3, 1, 8, 5, 2]
    c = [6, 0, 3, 3, 1]
    calls = []
    for v in (View(65, ids), View(65, ids, rows=[9, 8, 7, 6, 5], planes=[NONE, 0, 1, NONE, 2])):
        for e in ENCODINGS:
            for layout in (IM, WM):
                for stride in (0, 77):
                    calls += [(v, "desc", desc(e, layout, c, 7, stride)), (v, "parts", [part(range(5), e, layout, c, 7, stride)])]
    got = assert_agree(tool, calls)
    for (view, _, _), d, p in zip(calls[::2], got[::2], got[1::2]):
        assert d[0] == p[0] == "ok" and not d[1] and not p[1]
        assert d[2][0][:6] == p[2][0][:6]  # encoding, layout, element size, stride, n, pointer
        # the descriptor refers to the handle's resident rows and planes and ships its columns only; the part ships all three
        assert d[2][0][6:] == (1, -1, -1, 0) and d[3] == c
        assert p[2][0][6:] == (0, 0, 5 if view.planes else -1, 10 if view.planes else 5) and p[3] == view.rows + (view.planes or []) + c
    # `plain` for exactly one shape
    v = View(65, ids)
    shapes = [desc(), desc(stride=5), desc(stride=6), desc(layout=WM), desc(encoding=LE32), desc(columns=[0, 1, 2, 3, 4], n_columns=5), desc(encoding=U8)]
    got = assert_agree(tool, [(v, "desc", d) for d in shapes] + [(v, "parts", [part(range(5), BE32, IM)])])
    assert [g[1] for g in got] == [True, True, False, False, False, False, False, False]
    lines = tool([v.command(), "plain %d" % PTR, desc_command(desc()), "eq", desc_command(desc(stride=6)), "eq", parts_command([part(range(5), BE32, IM)]), "plain %d" % (PTR + 4), "eq"])
    assert lines[0] == lines[1] and lines[2] == "eq 1" and lines[4] == "eq 0" and lines[7] == "eq 0"


# ---- 7. random calls, and operator==
def _random_call(rng, v):
    n_in = v.n_in
    wrong = rng.random() < 0.5  # half of the calls carry one deliberate mistake (others go wrong by chance)
    mistake = rng.choice(("encoding", "layout", "ptr", "align", "column", "stride", "huge", "position", "twice", "missing", "nullpos")) if wrong else None
    e = rng.choice(ENCODINGS) if mistake != "encoding" else rng.choice((3, 7, 15, 21, 1 << 31))
    if rng.random() < 0.4:
        layout = rng.choice((IM, WM)) if mistake != "layout" else rng.choice((2, 15, 16, 17))
        has = rng.random() < 0.6
        n_columns = n_in + rng.randrange(4) if has else rng.randrange(3)
        cols = [rng.randrange(max(n_columns, 1)) for _ in range(n_in)] if has else None
        if mistake == "column" and has and n_in:
            cols[rng.randrange(n_in)] = n_columns + rng.randrange(2)
        dense = v.B if layout == WM else (n_columns if has else n_in)
        stride = rng.choice((0, dense, dense + rng.randrange(1, 9)))
        if mistake == "stride":
            stride = max(dense - 1, 0)
        if mistake == "huge":
            stride = (1 << 57) + rng.randrange(1 << 20)
        ptr = 0 if mistake == "ptr" else PTR + (rng.choice((1, 2, 4, 8)) if mistake == "align" else 0)
        return (v, "desc", desc(e, layout, cols, n_columns, stride, ptr))
    order = list(range(n_in))
    rng.shuffle(order)
    if mistake == "missing" and order:
        order.pop()
    if mistake == "twice" and order:
        order.append(rng.choice(order))
    if mistake == "position" and order:
        order[rng.randrange(len(order))] = n_in + rng.randrange(3)
    n_parts = rng.randrange(1, 4)
    cuts = sorted(rng.randrange(len(order) + 1) for _ in range(n_parts - 1))
    parts, bad = [], rng.randrange(n_parts)
    for q, (a, b) in enumerate(zip([0] + cuts, cuts + [len(order)])):
        pos, mine = order[a:b], mistake if q == bad else None
        layout = rng.choice((IM, WM, BC)) if mine != "layout" else rng.choice((2, 15, 17))
        has = rng.random() < 0.5
        n_columns = len(pos) + rng.randrange(4) if has else rng.randrange(3)
        cols = [rng.randrange(max(n_columns, 1)) for _ in pos] if has else None
        if mine == "column" and has and pos:
            cols[rng.randrange(len(pos))] = n_columns
        dense = v.B if layout == WM else (n_columns if has else len(pos))
        stride = rng.choice((0, dense, dense + rng.randrange(1, 9)))
        if mine == "stride":
            stride = max(dense - 1, 0)
        if mine == "huge":
            stride = (1 << 57) + rng.randrange(1 << 20)
        ptr = 0 if mine == "ptr" else PTR + (rng.choice((1, 2, 4, 8)) if mine == "align" else 0)
        parts.append(part(None if mine == "nullpos" else pos, e if q == bad or mistake != "encoding" else U8, layout, cols, n_columns, stride, ptr, n=len(pos)))
    return (v, "parts", parts)


def test_random_calls_against_the_restatement(tool):
    rng = random.Random(0x1A907)
    views = [View(1, [5]), View(65, [1, 2, 3, 4, 5]), View(130, [9, 3, 7, 1], rows=[0, 5, 2, 6]), View(300, [2, 4, 6, 8, 10, 12, 14], planes=[0, 1, NONE, 2, NONE, 3, 4]),
             View(64, [8, 1, 6], rows=[2, 1, 0], planes=[NONE, NONE, 0]), View(7, [])]
    calls = [_random_call(rng, rng.choice(views)) for _ in range(600)]
    got = assert_agree(tool, calls)
    n_ok = sum(g[0] == "ok" for g in got)
    assert 150 < n_ok < 450, n_ok
    kinds = {re.sub(r"\d+", "N", g[1]) for g in got if g[0] == "err"}
    assert len(kinds) >= 14, kinds  # every kind of refusal occurred, with and without the part prefix


def _mutations(view, kind, arg):
    """calls that differ from (view, kind, arg) in one field or one list entry and are still valid"""
    out = []
    items = [arg] if kind == "desc" else arg
    for q, it in enumerate(items):
        def changed(**kw):
            new = dict(it, **kw)
            return (view, kind, new if kind == "desc" else arg[:q] + [new] + arg[q + 1:])
        out.append(changed(encoding=LE32 if it["encoding"] != LE32 else MONT))            # same size, another encoding
        out.append(changed(encoding=U128))                                                # another size
        out.append(changed(layout=WM if it["layout"] != WM else IM))
        out.append(changed(stride=it["stride"] + 5))
        if it["columns"]:
            cols = list(it["columns"])
            cols[-1] = cols[-1] - 1 if cols[-1] else cols[-1] + 1
            out.append(changed(columns=cols))
            out.append(changed(columns=None))
    return out


def test_plan_equality(tool):
    rows, planes = [12, 3, 9, 4, 7, 1], [NONE, 0, NONE, 1, 2, NONE]
    v = View(130, [1, 2, 3, 4, 5, 6], rows=rows, planes=planes)
    bases = [(v, "desc", desc(LE32, IM, [5, 4, 3, 2, 1, 0], 8, 140)), (v, "desc", desc(MONT, WM, None, 0, 140)),
             (v, "parts", [part([5, 0, 2], U8, WM, [1, 0, 2], 4, 135), part([4, 3, 1], MONT, IM, [0, 2, 2], 3, 131)])]  # (strides that are valid in both layouts)
    for base in bases:
        variants = _mutations(*base)
        if base[1] == "parts":  # the position lists, and what the handle's tables say about them
            swapped = [dict(base[2][0], positions=[0, 5, 2])] + base[2][1:]
            moved = [dict(base[2][0], positions=[5, 0], columns=[1, 0], n=2), dict(base[2][1], positions=[2, 4, 3, 1], columns=[0, 0, 2, 2], n=4)]
            variants += [(v, "parts", swapped), (v, "parts", moved), (View(130, v.ids, rows=rows[:-1] + [2], planes=planes), "parts", base[2]),
                         (View(130, v.ids, rows=rows, planes=[0] + planes[1:]), "parts", base[2]), (View(130, v.ids, rows=rows), "parts", base[2])]
        else:
            variants.append((v, "parts", [part(range(6), base[2]["encoding"], base[2]["layout"], base[2]["columns"], base[2]["n_columns"], base[2]["stride"])]))
        commands = []
        for view, kind, arg in [base, base] + [x for var in variants for x in (var, base)]:
            commands += [view.command(), desc_command(arg) if kind == "desc" else parts_command(arg), "eq"]
        lines = tool(commands)
        assert all(l.startswith("ok ") for l in lines[0::2]), [l for l in lines[0::2] if not l.startswith("ok ")]
        # the repeated call is equal (the callers' pointers are not compared: below); every variant differs from the base, in both orders
        assert lines[3] == "eq 1" and set(lines[5::2]) == {"eq 0"}, (base[1], lines[3::2])
    moved_ptr = [dict(p, ptr=p["ptr"] + 64) for p in bases[2][2]]
    lines = tool([v.command(), parts_command(bases[2][2]), parts_command(moved_ptr), "eq", desc_command(bases[0][2]), desc_command(dict(bases[0][2], ptr=PTR + 64)), "eq"])
    assert lines[2] == "eq 1" and lines[5] == "eq 1" and lines[0] != lines[1]
