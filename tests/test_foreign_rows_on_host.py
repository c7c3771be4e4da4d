"""Per-row answers of the batch-wide foreign-call round trip without a device (acvm_batch_resolve_foreign_calls_device_rows): the per-row append of
acvm_amd/csrc/foreign_store.hpp compiled for the host (tools/foreign_rows_store_host_test.hip runs what a lane of fc_append_rows_kernel and of
fc_answers_max_kernel runs) and the host-only plan of acvm_amd/csrc/foreign_plan.cpp (tools/foreign_rows_plan_host_test.cpp): the lanes a mask resumes,
the refusals in their order with code and text, the bounds of the result store from a per-row maximum. Both tools are stand-alone programs, compiled
as they are and with AddressSanitizer + UndefinedBehaviorSanitizer, and judged by the Python restatement below."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BE32, LE32, MONT, U8, U64 = 0, 1, 2, 16, 19
IM, WM = 0, 1
SOLVED, WAITS = 0, 3
E_INVALID, E_UNSUPPORTED, E_STATE = -1, -3, -5
PTR = 1 << 30
GARBAGE = 0xFFFFFFF0
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def runner(exe, silent=()):
    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        if silent:
            assert len(lines) == sum(not c.startswith(silent) for c in commands)
        return lines
    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def store(request, tmp_path_factory):
    """the tables, the length and mask columns and the caller's buffer are heap arrays of exactly the stated size: under the sanitizers a load or a
    store past an edge ends the program with a report"""
    exe = str(tmp_path_factory.mktemp("foreign_rows_store") / "foreign_rows_store_host_test")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + [x for f in SANITIZE for x in ("-Xarch_host", f)]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17"] + flags + [os.path.join(ROOT, "tools", "foreign_rows_store_host_test.hip"), "-o", exe])
    return runner(exe)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("foreign_rows_plan") / "foreign_rows_plan_host_test")
    flags = ["-O1", "-Wall"] if request.param == "plain" else ["-O1", "-g", "-Wall", "-Wno-sign-compare"] + SANITIZE
    sources = [os.path.join(ROOT, "tools", "foreign_rows_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "foreign_plan.cpp"),
               os.path.join(ROOT, "acvm_amd", "csrc", "import_plan.cpp")]
    subprocess.check_call(["g++", "-std=c++17"] + flags + sources + ["-o", exe])
    return runner(exe, silent=("clear", "lane", "view", "slot"))


def fmt(lst):
    return "null" if lst is None else "e" if not len(lst) else ",".join(str(int(x)) for x in lst)


# ---- the store
def element(x, encoding):
    """the bytes of one element of the caller's buffer whose 256-bit string is x, and the field value the store must hold for it"""
    if encoding == BE32:
        return x.to_bytes(32, "big"), x % P
    if encoding == LE32:
        return x.to_bytes(32, "little"), x % P
    if encoding == MONT:
        return x.to_bytes(32, "little"), x * pow(1 << 256, -1, P) % P
    size = 1 << (encoding - U8)
    x %= 1 << (8 * size)
    return x.to_bytes(size, "little"), x


def size_of(encoding):
    return 1 << (encoding - U8) if encoding >= U8 else 32


class Column:
    """what upload_fc_tables writes for the results of one instance; a result: (kinds, per output its values)"""

    def __init__(self):
        self.results = []

    def words(self):
        out = [len(self.results)]
        for kinds, outputs in self.results:
            out.append(len(kinds))
            for is_array, vals in zip(kinds, outputs):
                out += [1 if is_array else 0, len(vals)]
        return out

    def values(self):
        return [v for _, outputs in self.results for vals in outputs for v in vals]


def rows_command(rng, encoding, n_columns, kinds, js, answers, use_lens=True, use_mask=True, shape_lens=None):
    """answers: per row None (left out) or per output a list of integers. Rows that are left out carry garbage lengths and values."""
    n_values = len(kinds)
    size = size_of(encoding)
    lens, cells, stored = [], [], []
    for a in answers:
        row = []
        if a is None:
            lens += [GARBAGE] * n_values
            stored.append(None)
        else:
            lens += [len(v) if is_array else GARBAGE for is_array, v in zip(kinds, a)]  # (the length of a single value is ignored)
            els = [[element(x, encoding) for x in v] for v in a]
            row = [b for v in els for b, _ in v]
            stored.append([[val for _, val in v] for v in els])
        assert len(row) <= n_columns
        row += [bytes(rng.randrange(256) for _ in range(size)) for _ in range(n_columns - len(row))]
        cells += row
    cmd = "rows %d %d %s %s %s %s %s %s" % (encoding, n_columns, fmt([1 if k else 0 for k in kinds]), fmt(shape_lens if shape_lens is not None else [7] * n_values), fmt(js),
                                            fmt(lens) if use_lens else "null", fmt([0 if a is None else rng.randrange(1, 256) for a in answers]) if use_mask else "null",
                                            ",".join(b.hex() for b in cells) or "e")
    return cmd, stored


@pytest.mark.parametrize("Bp", [1, 64, 65])
def test_per_row_appends_build_the_layout_of_the_host_store(store, Bp):
    rng = random.Random(0xF0E1 + Bp)
    desc_words, vals_cap = 64, 40
    columns = [Column() for _ in range(Bp)]
    commands, expect = ["new %d %d %d" % (Bp, desc_words, vals_cap)], []
    shapes = [(True,), (True, False), (False, True, True), (), (False,)]  # n_values = 0: the println shape
    for call in range(8):
        kinds = shapes[call % len(shapes)]
        js = sorted(rng.sample(range(Bp), min(Bp, rng.choice((1, 3, Bp)))))
        answers = []
        for j in js:
            if call != 5 and rng.random() < 0.35:  # (call 5 has no mask: every row is answered)
                answers.append(None)
                continue
            answers.append([[rng.choice((rng.randrange(1 << 256), P, (1 << 256) - 1, 0, rng.randrange(300))) for _ in range(rng.randrange(0, 4) if is_array else 1)] for is_array in kinds])
        if call == 0:
            answers[0] = [[]]  # a zero-length array in every run
        if call == 2:
            answers = [None] * len(js)  # a call that leaves every row out
        totals = [sum(len(v) for v in a) for a in answers if a is not None]
        n_columns = max(totals, default=0) + call % 2
        enc = (BE32, LE32, MONT, U8, U64)[call % 5]
        cmd, stored = rows_command(rng, enc, n_columns, kinds, js, answers, use_mask=call != 5)
        commands.append(cmd)
        expect.append("max %d" % max(totals, default=0))
        for j, a, s in zip(js, answers, stored):
            col = columns[j]
            fits = a is not None and len(col.words()) + 1 + 2 * len(kinds) <= desc_words and len(col.values()) + sum(len(v) for v in a) <= vals_cap
            expect.append("%s %d %d %d" % ("left_out" if a is None else "appended" if fits else "refused", len(col.words()), len(col.values()), len(col.results)))
            if fits:
                col.results.append((kinds, s))
    for j in range(Bp):
        commands += ["walk %d" % j, "column %d" % j, "values %d %d" % (j, vals_cap)]
    lines = store(commands)
    assert lines[:len(expect)] == expect
    assert any("appended" in e for e in expect) and any("left_out" in e for e in expect)
    assert any(len(c.results) >= 2 for c in columns) and any(0 in [len(v) for _, o in c.results for v in o] for c in columns)  # zero-length arrays
    at = len(expect)
    for j, col in enumerate(columns):  # every column word for word: a row that was left out and the neighbours of an appended one are untouched
        assert lines[at] == "%d %d %d" % (len(col.words()), len(col.values()), len(col.results))
        assert [int(x) for x in lines[at + 1].split()] == col.words() + [0] * (desc_words - len(col.words())), j
        want = [v * (1 << 261) % P for v in col.values()]
        assert [int(x, 16) for x in lines[at + 2].split()] == want + [0] * (vals_cap - len(want)), j
        at += 3


def test_host_lengths_hold_without_a_length_column_and_a_mask_alone(store):
    rng = random.Random(5)
    cmd, _ = rows_command(rng, BE32, 3, (True, False), [0, 1, 2], [[[1, 2], [3]], None, [[4, 5], [6]]], use_lens=False, shape_lens=[2, 9])
    lines = store(["new 3 8 4", cmd, "column 0", "column 1", "column 2", "values 0 3", "values 1 3", "values 2 3"])
    assert lines[:4] == ["max 3", "appended 1 0 0", "left_out 1 0 0", "appended 1 0 0"]
    assert lines[4] == lines[6] == "1 2 1 2 0 1 0 0" and lines[5] == "0 0 0 0 0 0 0 0"
    assert [int(x, 16) for x in lines[7].split()] == [v * (1 << 261) % P for v in (1, 2, 3)]
    assert [int(x, 16) for x in lines[8].split()] == [0, 0, 0]
    assert [int(x, 16) for x in lines[9].split()] == [v * (1 << 261) % P for v in (4, 5, 6)]


def test_a_row_whose_lengths_pass_an_edge_is_refused_not_written(store):
    rng = random.Random(9)
    one = lambda j, a, n_columns, **kw: rows_command(rng, BE32, n_columns, (True, False), [j], [a], **kw)[0]  # noqa: E731
    commands = ["new 65 8 3", one(64, [[7], [8]], 2), "column 64", "values 64 3"]
    before = len(commands)
    # the caller's columns: a row of 3 values in a buffer of 2 per row (the lengths changed behind the sizing launch); lengths whose sum passes 2^32
    long_row = "rows 0 2 1,0 7,7 64 3,%d null %s" % (GARBAGE, ",".join(bytes(32).hex() for _ in range(2)))
    huge = "rows 0 2 1,1 7,7 64 %d,%d null %s" % (GARBAGE, GARBAGE, ",".join(bytes(32).hex() for _ in range(2)))
    commands += [long_row, huge]
    commands.append(one(64, [[1, 2], [3]], 3))   # the slot's values: 2 + 3 > 3
    commands.append(one(64, [[], [9]], 1))       # words [count] + 5 + 5 > 8: the descriptor edge
    commands += ["column 64", "values 64 3", "walk 64", "column 63", "column 0"]
    commands += ["new 2 11 3", one(1, [[7], [8]], 2), one(1, [[], [9]], 1), one(1, [[], [5]], 1, use_lens=False, shape_lens=[0, 0]), "column 1", "values 1 3", "column 0"]
    lines = store(commands)
    assert lines[:2] == ["max 2", "appended 1 0 0"]
    filled, vals = lines[2], lines[3]
    assert filled == "1 2 1 1 0 1 0 0"
    assert lines[before:before + 8] == ["max 4", "refused 6 2 1", "max %d" % 0xFFFFFFFF, "refused 6 2 1", "max 3", "refused 6 2 1", "max 1", "refused 6 2 1"]
    assert lines[before + 8] == filled and lines[before + 9] == vals and lines[before + 10] == "6 2 1"
    assert lines[before + 11] == lines[before + 12] == "0 0 0 0 0 0 0 0"
    rest = lines[before + 13:]
    assert rest[:6] == ["max 2", "appended 1 0 0", "max 1", "appended 6 2 1", "max 1", "refused 11 3 2"]  # 10 + 1 words fill the 11 exactly; the next has no room
    assert rest[6] == "2 2 1 1 0 1 2 1 0 0 1" and [int(x, 16) for x in rest[7].split()] == [v * (1 << 261) % P for v in (7, 8, 9)]
    assert rest[8] == " ".join(["0"] * 11)


# ---- the host plan
def lane(instance, status, opcode=0, brillig=0, resolved=0):
    return "lane %d %d %d %d %d" % (instance, status, opcode, brillig, resolved)


def answers(first=0, n=4, n_values=2, is_array=(1, 0), lens=(2, 1), encoding=BE32, layout=IM, n_columns=3, stride=0, values=PTR, d_lens=0, d_answered=0, opcode=2):
    return "answers %d 0 %d %d %d %s %s %d %d %d %d %d %d %d" % (opcode, first, n, n_values, fmt(is_array), fmt(lens), encoding, layout, n_columns, stride, values, d_lens,
                                                              d_answered)


# instances 3, 5, 8, 9, 12 wait at opcode 2 (lanes 1, 2, 4, 5, 7); 5 and 9 were answered since the last solve
LANES = [lane(1, SOLVED), lane(3, WAITS, 2), lane(5, WAITS, 2, 0, 1), lane(7, WAITS, 4), lane(8, WAITS, 2), lane(9, WAITS, 2, 0, 1), lane(10, WAITS, 2, 1), lane(12, WAITS, 2)]
LIST = [(1, 3, 0), (2, 5, 1), (4, 8, 0), (5, 9, 1), (7, 12, 0)]
ALREADY = "row %d (instance %d) was already answered since the last solve; call acvm_batch_solve"


def test_the_lanes_a_mask_resumes(plan):
    cases = [(0, 5, [1, 0, 1, 0, 7]), (0, 5, [0, 0, 0, 0, 0]), (2, 1, None), (2, 3, [255, 0, 1]), (0, 0, None), (1, 1, [0]), (0, 5, None), (0, 2, [1, 1]), (3, 2, [1, 0]),
             (4, 1, [1])]
    lines = plan(["clear"] + LANES + ["resumes 2 0 %d %d %s" % (f, n, fmt(m)) for f, n, m in cases])
    for line, (first, n, mask) in zip(lines, cases):
        rows = [first + i for i in range(n) if mask is None or mask[i]]
        bad = [r for r in rows if LIST[r][2]]
        if bad:  # an answered row that is marked answered again: the first one, ACVM_E_STATE; one that is left out is fine
            assert line == "err %d %s" % (E_STATE, ALREADY % (bad[0], LIST[bad[0]][1]))
        else:
            assert line == "ok %d" % len(rows) + "".join(" %d %d" % LIST[r][:2] for r in rows)
    assert sum(line.startswith("err") for line in lines) == 3


def test_the_refusals_in_their_order_with_code_and_text(plan):
    L, A = 3 * PTR, 5 * PTR
    cases = [
        # (the command, the view, what it answers); each case adds the next refusal to a descriptor that still has all the later ones
        (answers(encoding=7, first=4, n=3, n_columns=0, values=PTR + 8), "view 0 1 0", "err %d unknown encoding 7" % E_INVALID),
        (answers(first=4, n=3, n_columns=0, values=PTR + 8), "view 0 1 0", "err %d batch not solved" % E_STATE),
        (answers(first=4, n=3, n_columns=0, values=PTR + 8), "view 1 1 0", "err %d a handle with a caller's BlackBoxFunctionSolver keeps its foreign-call results on the host: "
                                                                         "resolve per instance (acvm_batch_resolve_foreign_call)" % E_UNSUPPORTED),
        (answers(first=4, n=3, n_columns=0, values=PTR + 8), "view 1 0 0", "err %d rows [4, 7) are outside the 5 rows waiting at opcode 2, brillig index 0" % E_INVALID),
        (answers(n=5, is_array=None, n_columns=0, values=PTR + 8, d_lens=L), "view 1 0 0", "err %d null argument" % E_INVALID),
        (answers(n=5, n_columns=2, values=PTR + 8), "view 1 0 0", "err %d n_columns 2 is below the 3 values of the result's shape" % E_INVALID),
        (answers(n=5, values=0), "view 1 0 0", "err %d null values" % E_INVALID),
        (answers(n=5, values=PTR + 8), "view 1 0 0", "err %d d_values must be 16-byte aligned" % E_INVALID),
        (answers(n=5, stride=2), "view 1 0 0", "err %d stride 2 is below the dense stride 3 of the layout" % E_INVALID),
        (answers(n=5), "view 1 0 0", "err %d %s" % (E_STATE, ALREADY % (1, 5))),          # no mask: an answered row in the range is refused here
        (answers(n=5, d_answered=A), "view 1 0 0", "ok 3 3 2 1 2 0 1"),                      # with a mask: judged once it is on the host
        (answers(n=1), "view 1 0 0", "ok 3 3 2 1 2 0 1"),
        # with a length column the host lengths are not read (null is fine), an array's word is 0, and the width waits for the sizing launch
        (answers(n=1, lens=None, n_columns=0, values=0, d_lens=L), "view 1 0 0", "ok 0 1 2 1 0 0 1"),  # (stride 0: the dense stride of a row-major buffer of no columns)
        (answers(n=1, lens=None, n_columns=0, values=PTR + 8, d_lens=L), "view 1 0 0", "err %d d_values must be 16-byte aligned" % E_INVALID),
        (answers(n=1, n_values=0, is_array=None, lens=None, n_columns=0, values=0), "view 1 0 0", "ok 0 0 0"),  # the println shape
        (answers(n=0, first=5, n_values=0, is_array=None, lens=None, n_columns=0, values=0, d_answered=A), "view 1 0 0", "ok 0 0 0"),
    ]
    commands = ["clear"] + LANES
    for cmd, view, _ in cases:
        commands += [view, cmd]
    commands += ["width 3 4 1", "width 4 4 1", "width 4 4 0", "width 0 0 0", "width 4000000000 %d 1" % 0xFFFFFFFF, "width 4000000000 %d 1" % (1 << 31),
                 "width 4000000000 %d 1" % ((1 << 31) - 1)]
    lines = plan(commands)
    for line, (_, _, want) in zip(lines, cases):  # (the texts of the shared buffer checks may go on behind what is stated here)
        assert line == want or (want.startswith("err") and line.startswith(want)), (line, want)
    assert lines[len(cases):] == ["err %d n_columns 3 is below the 4 values of the longest answered row" % E_INVALID, "ok 4", "err %d null values" % E_INVALID, "ok 0",
                                  "err %d a row's lengths sum to 2^31 values or more: beyond any result" % E_INVALID,
                                  "err %d a row's lengths sum to 2^31 values or more: beyond any result" % E_INVALID, "ok %d" % ((1 << 31) - 1)]


def test_bounds_after_masked_calls_equal_those_of_one_unmasked_call(plan):
    """A round answered by several masked calls -- each with the largest total of ITS answered rows -- leaves the bounds, and after the same rounds the
    capacities' need, of one call with the round's largest total: a column gains one result per round."""
    rng = random.Random(77)
    rounds = [[rng.randrange(0, 9) for _ in range(rng.randrange(1, 6))] for _ in range(6)]  # per round: the maxima of its calls
    words = [1 + 2 * rng.randrange(0, 4) for _ in rounds]
    many, one = ["slot 1 0 0 0"], ["slot 1 0 0 0"]
    for w, maxima in zip(words, rounds):
        many += ["call %d %d" % (w, m) for m in maxima] + ["fold"]
        one += ["call %d %d" % (w, max(maxima)), "fold"]
    got_many, got_one = plan(many), plan(one)
    folds_many = [line for line, c in zip(got_many, [c for c in many if c != "slot 1 0 0 0"]) if c == "fold"]
    folds_one = [line for line, c in zip(got_one, [c for c in one if c != "slot 1 0 0 0"]) if c == "fold"]
    assert folds_many == folds_one
    bw, bv = 1, 0
    for line, w, maxima in zip(folds_one, words, rounds):
        bw, bv = bw + w, bv + max(maxima)
        assert line == "ok %d %d %d %d" % (bw, bv, w, max(maxima))
    # the tables hold every column's results at every moment: what a call reserves is never below the bounds plus the round's largest result so far
    bw, bv, at = 1, 0, 0
    for w, maxima in zip(words, rounds):
        for i in range(len(maxima)):
            _, _, have_w, have_v = got_many[at].split()
            assert int(have_w) >= bw + w and int(have_v) >= bv + max(maxima[:i + 1])
            at += 1
        at += 1
        bw, bv = bw + w, bv + max(maxima)


# ---- the node's foreign-call loop: acvm_amd/csrc/node_foreign_plan.cpp
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def node_plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("node_foreign_plan") / "node_foreign_plan_host_test")
    flags = ["-O1", "-Wall"] if request.param == "plain" else ["-O1", "-g", "-Wall", "-Wno-sign-compare"] + SANITIZE
    sources = [os.path.join(ROOT, "tools", "node_foreign_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "node_foreign_plan.cpp"),
               os.path.join(ROOT, "acvm_amd", "csrc", "import_plan.cpp")]
    subprocess.check_call(["g++", "-std=c++17"] + flags + sources + ["-o", exe])
    return runner(exe)


def align256(x):
    return (x + 255) // 256 * 256


def test_row_base_of_first_middle_and_partial_last_tiles_of_both_node_forms(node_plan):
    """acvm_node_solve numbers a row by its global instance -- the lane's first instance plus the tile's offset --, acvm_node_solve_device by the row of
    the lane's own buffers, whatever the lane's place in the node. n = 165 in tiles of 64: tiles 0, 1 and the partial tile 2 (37 rows)."""
    tile, n = 64, 165
    tiles = range((n + tile - 1) // tile)
    cases = [(form, first, k) for form in (0, 1) for first in (0, 192, (1 << 33) + 64) for k in tiles]
    lines = node_plan(["row_base %d %d %d %d" % (form, first, k, tile) for form, first, k in cases])
    assert [int(x) for x in lines] == [(0 if form else first) + k * tile for form, first, k in cases]
    # the last row of the partial tile: row_base + 36 is the lane's last row, n - 1
    assert int(node_plan(["row_base 1 0 2 64"])[0]) + (n - 2 * tile) - 1 == n - 1
    # no 32-bit product: tile 2^17 at tile index 2^15 is 2^32
    assert node_plan(["row_base 0 5 32768 131072", "row_base 1 5 32768 131072"]) == [str((1 << 32) + 5), str(1 << 32)]


def test_scratch_sizes(node_plan):
    """inputs: rows | lens | values | mask, each part on a 256-byte boundary and as long as its elements; an uploaded answer: values from the first to the
    last described element | row_lens | answered"""
    cases = [(1, 1, 1, 32), (64, 2, 3, 32), (65, 0, 0, 32), (37, 3, 5, 1), (131072, 2, 2, 8), (0, 1, 0, 32)]
    lines = node_plan(["inputs %d %d %d %d" % c for c in cases])
    for line, (n_rows, n_inputs, longest, size) in zip(lines, cases):
        o_lens = align256(4 * n_rows)
        o_values = o_lens + align256(4 * n_rows * n_inputs)
        o_mask = o_values + align256(n_rows * longest * size)
        assert line == "ok 0 %d %d %d %d" % (o_lens, o_values, o_mask, o_mask + align256(n_rows * longest))
    assert node_plan(["inputs 4294967295 1 4294967295 32"]) == ["too-large"]
    # encoding layout n_columns stride n_rows n_values values row_lens answered
    answers = [((BE32, IM, 3, 0, 10, 2, 1, 0, 0), 10 * 3 * 32, 0, 0), ((BE32, IM, 3, 5, 10, 2, 1, 1, 1), (9 * 5 + 3) * 32, 10 * 2 * 4, 10),
               ((MONT, WM, 2, 0, 37, 2, 1, 0, 1), 2 * 37 * 32, 0, 37), ((U8, WM, 2, 64, 37, 1, 1, 1, 0), 64 + 37, 37 * 4, 0),
               ((BE32, IM, 0, 0, 65, 0, 0, 0, 1), 0, 0, 65), ((U64, IM, 1, 0, 1, 1, 1, 0, 0), 8, 0, 0)]
    lines = node_plan(["answer " + " ".join(str(x) for x in a) for a, _, _, _ in answers])
    for line, (_, values, lens, answered) in zip(lines, answers):
        o_lens = align256(values)
        o_answered = o_lens + align256(lens)
        assert line == "0 0 %d %d %d %d" % (o_lens, o_answered, o_answered + align256(answered), values)
    refused = node_plan(["answer 7 0 1 0 4 1 1 0 0", "answer 0 2 1 0 4 1 1 0 0", "answer 0 0 3 2 4 1 1 0 0", "answer 0 1 3 3 4 1 1 0 0", "answer 0 0 1 0 4 1 0 0 0"])
    assert refused[0] == "%d unknown encoding 7" % E_INVALID and refused[1] == "%d unknown layout 2" % E_INVALID
    assert refused[2].startswith("%d stride 2 is below the dense stride 3" % E_INVALID) and refused[3].startswith("%d stride 3 is below the dense stride 4" % E_INVALID)
    assert refused[4] == "%d null values" % E_INVALID
    # grow-only, with a quarter of slack
    assert node_plan(["grow 4096 4096", "grow 4096 100", "grow 0 0"]) == ["0", "0", "0"]
    (grown,) = node_plan(["grow 4096 8000"])
    assert int(grown) == align256(8000 + 2000 + 256)


def test_round_cap_handler_checks_and_return_values(node_plan):
    assert node_plan(["rounds 0", "rounds 1", "rounds 256", "rounds 4000000000"]) == ["256", "1", "256", "4000000000"]
    assert node_plan(["verdict 0", "verdict 1", "verdict -7", "verdict -1", "verdict 2", "verdict 1000"]) == [
        "answered 0", "declined 0", "abort -7", "abort -1", "abort %d" % E_INVALID, "abort %d" % E_INVALID]
    # handler <null|set> fn space encoding layout has_solver running: the refusals in their order
    lines = node_plan(["handler set 1 0 0 0 0 0", "handler set 1 1 2 1 0 0", "handler set 1 1 19 0 0 0", "handler null 0 0 0 0 0 0", "handler null 0 0 0 0 1 0",
                       "handler set 1 2 0 0 0 0", "handler set 1 0 3 0 0 0", "handler set 1 0 0 16 0 0", "handler set 0 0 0 0 0 0",
                       "handler set 1 2 0 0 1 0", "handler set 1 2 0 0 1 1", "handler null 0 0 0 0 0 1"])
    assert lines[:5] == ["0 "] * 5
    assert lines[5] == "%d unknown space 2" % E_INVALID and lines[6] == "%d unknown encoding 3" % E_INVALID and lines[7] == "%d unknown layout 16" % E_INVALID
    assert lines[8] == "%d null handler function" % E_INVALID
    assert lines[9].startswith("%d a node with a caller's BlackBoxFunctionSolver" % E_UNSUPPORTED)
    assert lines[10].startswith("%d a node call is running" % E_STATE) and lines[11].startswith("%d a node call is running" % E_STATE)
