"""The batch-wide foreign-call round trip before it touches a device (acvm_amd/csrc/foreign_plan.cpp): the site list and a site's waiting list derived
from hand-written lane records, every refusal of acvm_batch_foreign_call_inputs_device / acvm_batch_resolve_foreign_calls_device with its code and text,
the shape words of a ForeignCallResult and the capacity rule of a device-owned slot. The module is compiled as plain C++
(tools/foreign_plan_host_test.cpp), once as it is and once through `make asan`, and judged by the Python restatement below. The refusals are those
tests/test_gpu_foreign_device.py asserts on a real handle."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE32, LE32, MONT, U8, U16, U32, U64, U128 = 0, 1, 2, 16, 17, 18, 19, 20
ENCODINGS = (BE32, LE32, MONT, U8, U16, U32, U64, U128)
IM, WM = 0, 1
SOLVED, IN_PROGRESS, FAILURE, WAITS = 0, 1, 2, 3
E_INVALID, E_UNSUPPORTED, E_STATE = -1, -3, -5
PTR = 1 << 30  # a device address aligned to everything
SOURCES = [os.path.join(ROOT, "tools", "foreign_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "foreign_plan.cpp"),
           os.path.join(ROOT, "acvm_amd", "csrc", "import_plan.cpp")]
SILENT = ("clear", "decl", "lane", "view", "slot")


def size_of(encoding):
    return 1 << (encoding - U8) if U8 <= encoding <= U128 else 32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    """the tool compiled as it is, and the second binary of `make asan` (AddressSanitizer + UndefinedBehaviorSanitizer): a stand-alone program on
    the CPU, given the same command streams -- a report ends it with a non-zero status"""
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("foreign_plan") / "foreign_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + SOURCES + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "foreign_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/foreign_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith(SILENT) for c in commands)
        return lines
    return run


def fmt(lst):
    return "null" if lst is None else "e" if not len(lst) else ",".join(str(int(x)) for x in lst)


def lane(instance, status, opcode=0, brillig=0, resolved=0):
    return "lane %d %d %d %d %d" % (instance, status, opcode, brillig, resolved)


def inputs(opcode=2, brillig=0, first=0, n=4, encoding=BE32, layout=IM, n_columns=3, stride=0, values=PTR, mask=2 * PTR):
    return "inputs %d %d %d %d %d %d %d %d %d %d" % (opcode, brillig, first, n, encoding, layout, n_columns, stride, values, mask)


def answers(opcode=2, brillig=0, first=0, n=4, shape=(None, 2), encoding=BE32, layout=IM, n_columns=3, stride=0, values=PTR, is_array="auto", lens="auto"):
    ia = [0 if s is None else 1 for s in shape] if is_array == "auto" else is_array
    ln = [7 if s is None else s for s in shape] if lens == "auto" else lens  # (the length of a single value is ignored)
    return "answers %d %d %d %d %d %s %s %d %d %d %d %d" % (opcode, brillig, first, n, len(shape), fmt(ia), fmt(ln), encoding, layout, n_columns, stride, values)


def refusal(line, code=E_INVALID):
    assert line.startswith("err "), line
    got, text = line[4:].split(" ", 1)
    assert int(got) == code, line
    return text


# four instances wait at (2, 0); instance 6 was answered
FOUR = ["clear", "decl 2 0 2 0 f", lane(1, WAITS, 2, 0), lane(4, WAITS, 2, 0), lane(6, WAITS, 2, 0, 1), lane(9, WAITS, 2, 0), "view 1 0 0"]


# ---- 1. every refusal, with its code and text
def test_refusals_of_the_inputs_call(tool):
    cases = [
        (inputs(encoding=3), E_INVALID, "unknown encoding 3"),
        (inputs(encoding=21), E_INVALID, "unknown encoding 21"),
        (inputs(layout=2), E_INVALID, "unknown layout 2"),
        (inputs(layout=16), E_INVALID, "unknown layout 16"),
        (inputs(first=1, n=4), E_INVALID, "rows [1, 5) are outside the 4 rows waiting at opcode 2, brillig index 0"),
        (inputs(first=5, n=0), E_INVALID, "rows [5, 5) are outside the 4 rows waiting at opcode 2, brillig index 0"),
        (inputs(first=(1 << 32) - 1, n=(1 << 32) - 1), E_INVALID, "rows [4294967295, 8589934590) are outside the 4 rows waiting at opcode 2, brillig index 0"),
        (inputs(opcode=3, n=1), E_INVALID, "rows [0, 1) are outside the 0 rows waiting at opcode 3, brillig index 0"),
        (inputs(brillig=1, n=1), E_INVALID, "rows [0, 1) are outside the 0 rows waiting at opcode 2, brillig index 1"),
        (inputs(stride=2), E_INVALID, "stride 2 is below the dense stride 3 of the layout"),
        (inputs(layout=WM, stride=3), E_INVALID, "stride 3 is below the dense stride 4 of the layout"),
        (inputs(first=1, n=2, layout=WM, stride=1), E_INVALID, "stride 1 is below the dense stride 2 of the layout"),  # (against n_rows, not the list)
        (inputs(stride=(1 << 57) // 4 + 1), E_INVALID, "stride %d is beyond any device buffer" % ((1 << 57) // 4 + 1)),
        (inputs(values=PTR + 8), E_INVALID, "d_values must be 16-byte aligned"),
        (inputs(encoding=MONT, layout=WM, values=PTR + 4), E_INVALID, "d_values must be 16-byte aligned"),
        (inputs(encoding=U64, values=PTR + 4), E_INVALID, "d_values must be aligned to the element size, 8 bytes"),
    ]
    lines = tool(FOUR + [c for c, _, _ in cases])
    for line, (_, code, text) in zip(lines, cases):
        assert refusal(line, code) == text
    # the state of the handle is judged behind encoding and layout, in front of the range
    lines = tool(FOUR + ["view 0 0 0", inputs(), inputs(encoding=9), inputs(first=9), "view 1 0 1", inputs()])
    assert refusal(lines[0], E_STATE) == "batch not solved"
    assert refusal(lines[1]) == "unknown encoding 9"
    assert refusal(lines[2], E_STATE) == "batch not solved"
    assert refusal(lines[3]) == "the calls of this site are answered by the library (the caller's BlackBoxFunctionSolver)"
    # the width, once the device has said how long the longest row is
    lines = tool(["width 3 4 %d 0" % PTR, "width 3 4 0 %d" % PTR, "width 0 1 %d 0" % PTR, "width 3 4 0 0", "width 4 4 %d %d" % (PTR, PTR), "width 0 0 %d 0" % PTR])
    assert refusal(lines[0]) == "n_columns 3 is below the 4 values of the longest row"
    assert refusal(lines[1]) == "n_columns 3 is below the 4 values of the longest row"
    assert refusal(lines[2]) == "n_columns 0 is below the 1 values of the longest row"
    assert lines[3:] == ["ok", "ok", "ok"]  # the sizing call has no width; a buffer as wide as the longest row; nothing to write


def test_what_the_inputs_call_accepts(tool):
    lines = tool(FOUR + [inputs(), inputs(stride=5), inputs(layout=WM), inputs(first=1, n=2, layout=WM), inputs(first=4, n=0), inputs(values=0, mask=0, n_columns=0),
                         inputs(encoding=U8, values=PTR + 1), inputs(encoding=U32, layout=WM, values=PTR + 4, stride=9), inputs(values=0, mask=PTR + 3),
                         "view 1 1 0", inputs()])  # (reading inputs is not refused for a handle with a solver)
    assert lines == ["ok 3", "ok 5", "ok 4", "ok 2", "ok 3", "ok 0", "ok 3", "ok 9", "ok 3", "ok 3"]


def test_refusals_of_the_answers_call(tool):
    cases = [
        (answers(encoding=5), E_INVALID, "unknown encoding 5"),
        (answers(layout=3), E_INVALID, "unknown layout 3"),
        (answers(first=3, n=2), E_INVALID, "rows [3, 5) are outside the 4 rows waiting at opcode 2, brillig index 0"),
        (answers(opcode=7, n=1), E_INVALID, "rows [0, 1) are outside the 0 rows waiting at opcode 7, brillig index 0"),
        (answers(is_array=None), E_INVALID, "null argument"),
        (answers(lens=None), E_INVALID, "null argument"),
        (answers(n_columns=2), E_INVALID, "n_columns 2 is below the 3 values of the result's shape"),
        (answers(shape=(5, None, 1), n_columns=6), E_INVALID, "n_columns 6 is below the 7 values of the result's shape"),
        (answers(shape=((1 << 31) - 1, 2), n_columns=3), E_INVALID, "the result's 2147483649 values are beyond any result"),
        (answers(values=0), E_INVALID, "null values"),
        (answers(stride=2), E_INVALID, "stride 2 is below the dense stride 3 of the layout"),
        (answers(layout=WM, stride=3), E_INVALID, "stride 3 is below the dense stride 4 of the layout"),
        (answers(n_columns=8, stride=(1 << 57) // 4 + 1), E_INVALID, "stride %d is beyond any device buffer" % ((1 << 57) // 4 + 1)),
        (answers(values=PTR + 8), E_INVALID, "d_values must be 16-byte aligned"),
        (answers(encoding=U16, values=PTR + 1), E_INVALID, "d_values must be aligned to the element size, 2 bytes"),
        (answers(), E_STATE, "row 2 (instance 6) was already answered since the last solve; call acvm_batch_solve"),
        (answers(first=2, n=1), E_STATE, "row 2 (instance 6) was already answered since the last solve; call acvm_batch_solve"),
    ]
    lines = tool(FOUR + [c for c, _, _ in cases])
    for line, (_, code, text) in zip(lines, cases):
        assert refusal(line, code) == text
    lines = tool(FOUR + ["view 0 0 0", answers(first=0, n=2), "view 0 1 0", answers(first=0, n=2), "view 1 1 0", answers(first=0, n=2), answers(first=0, n=2, layout=9),
                         answers(first=0, n=9)])
    assert refusal(lines[0], E_STATE) == "batch not solved"
    assert refusal(lines[1], E_STATE) == "batch not solved"
    solver = "a handle with a caller's BlackBoxFunctionSolver keeps its foreign-call results on the host: resolve per instance (acvm_batch_resolve_foreign_call)"
    assert refusal(lines[2], E_UNSUPPORTED) == solver
    assert refusal(lines[3]) == "unknown layout 9"
    assert refusal(lines[4], E_UNSUPPORTED) == solver  # (judged in front of the range)


def test_what_the_answers_call_accepts(tool):
    lines = tool(FOUR + [answers(first=0, n=2), answers(first=3, n=1), answers(first=2, n=0), answers(first=4, n=0), answers(first=0, n=2, layout=WM),
                         answers(first=0, n=2, n_columns=9, stride=12), answers(first=0, n=2, shape=(), n_columns=0, values=0, is_array=None, lens=None),
                         answers(first=0, n=2, shape=(0,), n_columns=0, values=0), answers(first=0, n=0, values=0), answers(first=0, n=2, encoding=U8, values=PTR + 3)])
    assert lines == ["ok 3 3 2 0 1 1 2", "ok 3 3 2 0 1 1 2", "ok 3 3 2 0 1 1 2", "ok 3 3 2 0 1 1 2", "ok 2 3 2 0 1 1 2", "ok 12 3 2 0 1 1 2", "ok 0 0 0", "ok 0 0 1 1 0",
                     "ok 3 3 2 0 1 1 2", "ok 3 3 2 0 1 1 2"]


# ---- 2. sites and lists from hand-written lane records
def test_sites_and_lists_from_lane_records(tool):
    world = ["clear", "decl 5 0 1 0 invert", "decl 5 3 2 0 " + "x" * 70, "decl 9 1 4 1 \x01bb:pedersen", "decl 2 0 3 0 first",
             lane(0, WAITS, 5, 3), lane(1, WAITS, 5, 0), lane(2, FAILURE, 5, 0), lane(3, WAITS, 5, 3, 1), lane(4, SOLVED, 5, 3), lane(5, WAITS, 5, 0, 1),
             lane(6, IN_PROGRESS, 5, 0), lane(7, WAITS, 9, 1), lane(8, WAITS, 5, 3), lane(10, WAITS, 7, 2), lane(11, WAITS, 5, 0)]
    lines = tool(world + ["sites", "list 5 0", "list 5 3", "list 9 1", "list 7 2", "list 2 0", "list 5 1"])
    # two sites in one opcode, lanes interleaved between them; failed, solved and running lanes ignored; answered rows still listed and counted;
    # the internal site is not listed; a site the plan does not declare has no name; a declared site nobody waits at is not listed; names are cut at 63
    assert lines[0] == "ok 3 5 0 1 3 1 invert 5 3 2 3 1 %s 7 2 0 1 0 -" % ("x" * 63)
    assert lines[1] == "ok 3 1 1 0 5 5 1 10 11 0"   # (lane, instance, resolved): lane index != row
    assert lines[2] == "ok 3 0 0 0 3 3 1 8 8 0"
    assert lines[3] == "ok 1 7 7 0"                  # (the list of an internal site exists: the checks refuse it by the handle's view)
    assert lines[4] == "ok 1 9 10 0"
    assert lines[5] == "ok 0" and lines[6] == "ok 0"
    # lanes that do not come in ascending instance order: the list is ascending all the same
    lines = tool(["clear", lane(9, WAITS, 1, 0), lane(2, WAITS, 1, 0, 1), lane(5, WAITS, 1, 0), "list 1 0", "sites"])
    assert lines == ["ok 3 1 2 1 2 5 0 0 9 0", "ok 1 1 0 0 3 1 -"]
    assert tool(["clear", "sites", "list 0 0"]) == ["ok 0", "ok 0"]


# ---- 3. shape arithmetic and the capacity bound
def shape_words(shape):
    words = [len(shape)]
    for s in shape:
        words += [0, 1] if s is None else [1, s]
    return words, sum(1 if s is None else s for s in shape)


def test_shape_words_and_capacity(tool):
    shapes = [(), (None,), (3,), (None, 2), (0,), (0, 0, None), (5, None, 1, None, 7)]
    lines = tool(["shape %d %s %s" % (len(s), fmt([0 if x is None else 1 for x in s]), fmt([99 if x is None else x for x in s])) for s in shapes] +
                 ["shape 0 null null", "shape 1 null 1", "shape 2 1,1 %d,%d" % ((1 << 31), 1)])
    for line, s in zip(lines, shapes):
        words, total = shape_words(s)
        assert line == " ".join(str(x) for x in ["ok", total] + words)
    assert lines[len(shapes)] == "ok 0 0"
    assert refusal(lines[len(shapes) + 1]) == "null argument"
    assert refusal(lines[len(shapes) + 2]) == "the result's 2147483649 values are beyond any result"

    def want(bw, bv, rw, rv, aw, av, hw, hv):
        """(bounds, the round's largest result so far, this result, the capacities held) -> (grow, capacities to hold)"""
        nw, nv = bw + max(rw, aw), bv + max(rv, av)
        if nw > 1 << 31 or nv > 1 << 31:
            return None
        grow = nw > hw or nv > hv or hv == 0
        return (1, max(hw, nw + nw // 2 + 8), max(hv, nv + nv // 2 + 8)) if grow else (0, hw, hv)
    cases = [(1, 0, 0, 0, 3, 1, 0, 0), (1, 0, 0, 0, 3, 1, 4, 1), (1, 0, 0, 0, 3, 1, 3, 1), (1, 0, 0, 0, 3, 1, 4, 0), (1, 0, 0, 0, 1, 0, 2, 0), (1, 0, 0, 0, 1, 0, 2, 1),
             (10, 7, 0, 0, 5, 2, 15, 9), (10, 7, 0, 0, 5, 2, 15, 8), (10, 7, 0, 0, 5, 2, 14, 9), (1 << 31, 0, 0, 0, 1, 0, 0, 0), (1, 1 << 31, 0, 0, 1, 1, 9, 9),
             ((1 << 31) - 3, 5, 0, 0, 3, 5, 100, 100), ((1 << 32) - 1, 0, 0, 0, (1 << 32) - 1, 0, 8, 8),
             # a result of the round's size or less needs nothing new; a larger one needs its excess over the round's largest, each maximum on its own
             (10, 7, 5, 2, 5, 2, 15, 9), (10, 7, 5, 2, 3, 1, 15, 9), (10, 7, 5, 2, 7, 1, 15, 9), (10, 7, 5, 2, 3, 4, 15, 9), (10, 7, 5, 2, 7, 4, 17, 11),
             ((1 << 31) - 3, 5, 3, 5, 3, 5, 1 << 31, 100), ((1 << 31) - 3, 5, 3, 5, 4, 5, 1 << 31, 100), (1, 0, (1 << 32) - 1, 0, 1, 0, 8, 8)]
    lines = tool(["capacity %d %d %d %d %d %d %d %d" % c for c in cases])
    for line, c in zip(lines, cases):
        w = want(*c)
        if w is None:
            assert refusal(line) == "the results of one opcode would exceed 2^31 descriptor words or values per instance"
        else:
            assert line == "ok %d %d %d" % w, c
            assert w[1] >= c[0] + c[4] and w[2] >= c[1] + c[5] and w[2] >= 1  # the tables hold the result; a value table always exists
    assert [l.split()[1] for l in lines[13:18]] == ["0", "0", "1", "1", "0"]


def test_many_calls_in_one_round_cost_one_result_per_column(tool):
    """A row is answered once between two solves, so a column gains at most one result per round: 10 000 resolve calls in a round (partial ranges, the
    per-instance call on a device-owned slot) must leave the capacities where ONE call of the round's largest result leaves them, and the bounds grow
    by that one result when the solve consumes the round -- not by the number of calls."""
    one = tool(["slot 1 0 0 0", "call 3 1", "fold"])
    many = tool(["slot 1 0 0 0"] + ["call 3 1"] * 10000 + ["fold"])
    assert one == ["ok 1 14 9", "ok 4 1"]
    assert many[0] == one[0] and set(many[1:-1]) == {"ok 0 14 9"} and many[-1] == one[-1]
    # shapes of different sizes in one round: the capacities follow the largest words and the largest values seen, whatever the order and the count
    rng = random.Random(0xB07D)
    shapes = [(1 + 2 * n, v) for n, v in ((0, 0), (1, 1), (2, 7), (4, 4), (1, 30))]
    for _ in range(20):
        calls = [rng.choice(shapes) for _ in range(rng.randrange(1, 400))]
        bw, bv, hw, hv = rng.randrange(1, 50), rng.randrange(0, 50), rng.randrange(0, 80), rng.randrange(0, 80)
        lines = tool(["slot %d %d %d %d" % (bw, bv, hw, hv)] + ["call %d %d" % c for c in calls] + ["fold", "call 9 30", "fold"])
        mw, mv = max(c[0] for c in calls), max(c[1] for c in calls)
        cw, cv = hw, hv
        for line, c, k in zip(lines, calls, range(len(calls))):
            rw, rv = max([x[0] for x in calls[:k]] + [0]), max([x[1] for x in calls[:k]] + [0])
            nw, nv = bw + max(rw, c[0]), bv + max(rv, c[1])
            grow = nw > cw or nv > cv or cv == 0
            if grow:
                cw, cv = max(cw, nw + nw // 2 + 8), max(cv, nv + nv // 2 + 8)
            assert line == "ok %d %d %d" % (grow, cw, cv)
        assert cw >= bw + mw and cv >= bv + mv
        assert cw <= max(hw, (bw + mw) * 3 // 2 + 8) and cv <= max(hv, (bv + mv) * 3 // 2 + 8)  # never beyond what one call of the largest result asks for
        assert lines[len(calls)] == "ok %d %d" % (bw + mw, bv + mv)
        assert lines[-1] == "ok %d %d" % (bw + mw + 9, bv + mv + 30)  # the next round starts from the folded bounds


# ---- 4. seeded random calls: the Python restatement agrees, and the sanitizers have nothing to report
def test_random_calls(tool):
    rng = random.Random(0xF0CA11)
    commands, wants = [], []
    for _ in range(200):
        n_lanes = rng.randrange(0, 40)
        sites = [(rng.randrange(3), rng.randrange(2)) for _ in range(3)]
        recs = []
        instance = 0
        for _ in range(n_lanes):
            instance += rng.randrange(1, 4)
            op, bi = rng.choice(sites)
            recs.append((instance, rng.choice((SOLVED, FAILURE, WAITS, WAITS, WAITS)), op, bi, int(rng.random() < 0.3)))
        commands += ["clear", "view 1 0 0"] + [lane(*r) for r in recs]
        op, bi = rng.choice(sites)
        rows = [(t, r[0], r[4]) for t, r in enumerate(recs) if r[1] == WAITS and (r[2], r[3]) == (op, bi)]
        commands.append("list %d %d" % (op, bi))
        wants.append("ok %d" % len(rows) + "".join(" %d %d %d" % r for r in rows))
        first, n = rng.randrange(0, len(rows) + 2), rng.randrange(0, len(rows) + 2)
        shape = tuple(rng.choice((None, 0, 1, 2, 5)) for _ in range(rng.randrange(0, 4)))
        words, total = shape_words(shape)
        enc, layout = rng.choice(ENCODINGS), rng.choice((IM, WM))
        n_columns = max(total + rng.randrange(-1, 3), 0)
        dense = n if layout == WM else n_columns
        stride = rng.choice((0, dense, dense + 3, max(dense - 1, 0)))
        values = PTR + rng.choice((0, 0, 0, 16, size_of(enc), 1))
        commands.append(answers(op, bi, first, n, shape, enc, layout, n_columns, stride, values))
        if first + n > len(rows):
            w = (E_INVALID, "rows [%d, %d) are outside the %d rows waiting at opcode %d, brillig index %d" % (first, first + n, len(rows), op, bi))
        elif n_columns < total:
            w = (E_INVALID, "n_columns %d is below the %d values of the result's shape" % (n_columns, total))
        elif stride and stride < dense:
            w = (E_INVALID, "stride %d is below the dense stride %d of the layout" % (stride, dense))
        elif values % min(size_of(enc), 16):
            w = (E_INVALID, "d_values must be 16-byte aligned" if size_of(enc) == 32 else "d_values must be aligned to the element size, %d bytes" % size_of(enc))
        elif any(r[2] for r in rows[first:first + n]):
            r, row = next((i, row) for i, row in enumerate(rows) if i >= first and row[2])
            w = (E_STATE, "row %d (instance %d) was already answered since the last solve; call acvm_batch_solve" % (r, row[1]))
        else:
            w = "ok %d %d " % (stride or dense, total) + " ".join(str(x) for x in words)
        wants.append(w)
    lines = tool(commands)
    assert len(lines) == len(wants)
    for line, w in zip(lines, wants):
        if isinstance(w, tuple):
            assert refusal(line, w[0]) == w[1]
        else:
            assert line == w
