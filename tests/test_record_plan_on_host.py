"""The checks, the field table and the window cut of the record import (acvm_amd/csrc/record_plan.cpp) without a device and without a handle:
the module is compiled as plain C++ (tools/record_plan_host_test.cpp) -- once as it is, once with AddressSanitizer and
UndefinedBehaviorSanitizer as `make asan` builds it, a stand-alone program either way -- and its answers are judged by the Python restatement
below. The refusals are those tests/test_gpu_records.py asserts on the device, with the same texts."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE32, LE32, MONT, U8, U16, U32, U64, U128 = 0, 1, 2, 16, 17, 18, 19, 20
ENCODINGS = (BE32, LE32, MONT, U8, U16, U32, U64, U128)
NONE = 0xFFFFFFFF
PTR = (1 << 20) + 3  # a device address of no alignment at all
CAP = 256


def size_of(encoding):
    return 1 << (encoding - U8) if U8 <= encoding <= U128 else 32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    sources = [os.path.join(ROOT, "tools", "record_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "record_plan.cpp"),
               os.path.join(ROOT, "acvm_amd", "csrc", "import_plan.cpp")]
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("record_plan") / "record_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sources + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "record_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/record_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith(("view", "noview")) for c in commands)
        return lines
    return run


def fmt(lst):
    return "null" if lst is None else "e" if not len(lst) else ",".join(str(x) for x in lst)


class View:
    def __init__(self, B, ids, rows=None, planes=None):
        self.B, self.ids, self.rows, self.planes = B, list(ids), list(ids if rows is None else rows), None if planes is None else list(planes)
        self.n_in = len(self.ids)

    def command(self):
        return "view %d %d %s %s %s" % (self.B, self.n_in, fmt(self.ids), fmt(self.rows), fmt(self.planes))


def records_command(pitch, fields, ptr=PTR, null_fields=None):
    if null_fields is not None:
        return "records %d %d null%d" % (pitch, ptr, null_fields)
    return "records %d %d %d" % (pitch, ptr, len(fields)) + "".join(" %d %d %d" % f for f in fields)


# ---- the restatement: ("err", text) or ("ok", pitch, windows [(offset, length, first, n)], table [(row, plane, encoding, byte)])
def model(view, pitch, fields, ptr=PTR):
    if view is None:
        return ("err", "null batch")
    owner = {}
    for f, (position, encoding, offset) in enumerate(fields):
        who = "field %d (position %d): " % (f, position)
        if encoding not in ENCODINGS:
            return ("err", who + "unknown encoding %d" % encoding)
        if position >= view.n_in:
            return ("err", who + "position %d is not below n_initial %d" % (position, view.n_in))
        if offset + size_of(encoding) > pitch:  # (Python integers: no wrap)
            return ("err", who + "offset %d + size %d is beyond the pitch %d" % (offset, size_of(encoding), pitch))
        if position in owner:
            return ("err", "position %d is supplied twice (fields %d and %d)" % (position, owner[position], f))
        owner[position] = f
    for position in range(view.n_in):
        if position not in owner:
            return ("err", "position %d (initial witness %d) is supplied by no field" % (position, view.ids[position]))
    if fields and view.B and not ptr:
        return ("err", "null records")
    if fields and view.B * pitch > (1 << 57):
        return ("err", "pitch %d is beyond any device buffer" % pitch)
    cuts = []
    if fields and pitch <= CAP:
        cuts = [[0, pitch, list(range(len(fields)))]]
    elif fields:
        for f in sorted(range(len(fields)), key=lambda f: (fields[f][2], f)):
            begin, end = fields[f][2], fields[f][2] + size_of(fields[f][1])
            if not cuts or end - cuts[-1][0] > CAP:
                cuts.append([begin, 0, []])
            cuts[-1][1] = max(cuts[-1][1], end - cuts[-1][0])
            cuts[-1][2].append(f)
    windows, table, first = [], [], 0
    for offset, length, members in cuts:
        windows.append((offset, length, first, len(members)))
        first += len(members)
        for f in members:
            position, encoding, at = fields[f]
            table.append((view.rows[position], view.planes[position] if view.planes is not None else NONE, encoding, at - offset))
    return ("ok", pitch, windows, table)


def parse(line):
    if line.startswith("err "):
        code, text = line[4:].split(" ", 1)
        assert code == "-1"
        return ("err", text)
    tok = [int(t) for t in line.split()[1:]]
    records, pitch, n_windows, n_parts = tok[:4]
    assert records == 1 and n_parts == 0
    windows = [tuple(tok[4 + 4 * w:8 + 4 * w]) for w in range(n_windows)]
    rest = tok[4 + 4 * n_windows:]
    assert len(rest) % 4 == 0
    return ("ok", pitch, windows, [tuple(rest[i:i + 4]) for i in range(0, len(rest), 4)])


def check(tool, view, cases):
    """cases: (pitch, fields) or (pitch, fields, ptr); the answers against the model, returned parsed"""
    commands = ["noview" if view is None else view.command()] + [records_command(c[0], c[1], *c[2:]) for c in cases]
    got = [parse(g) for g in tool(commands)]
    for c, g in zip(cases, got):
        assert g == model(view, *c), c
    return got


def assert_windows_hold_whole_fields(answer, fields, pitch):
    """every field lies whole in exactly one window, no window is above the cap, every window lies inside the record"""
    _, _, windows, table = answer
    assert sum(w[3] for w in windows) == len(fields) == len(table)
    placed = []
    for offset, length, first, n in windows:
        assert 0 < length <= CAP and offset + length <= pitch
        for row, plane, encoding, byte in table[first:first + n]:
            assert byte + size_of(encoding) <= length
            placed.append((row, encoding, offset + byte))
    assert sorted(placed) == sorted((p + 100, e, o) for p, e, o in fields)  # (rows = position + 100 below)


VIEW3 = View(130, [5, 6, 9], rows=[105, 106, 109], planes=[2, NONE, 0])
VIEW_ROWS = View(65, [1, 2, 3, 4, 5, 6, 7, 8, 9], rows=[100, 101, 102, 103, 104, 105, 106, 107, 108])
MIXED108 = [(0, U8, 0), (1, U16, 1), (2, U32, 3), (3, U64, 7), (4, U128, 15), (5, BE32, 31), (6, LE32, 64), (7, U8, 107), (8, U32, 100)]


def test_the_cap_is_the_kernels(tool):
    assert tool(["cap"]) == ["cap %d" % CAP]
    text = open(os.path.join(ROOT, "acvm_amd", "csrc", "record_decode.hpp")).read()
    assert "RECORD_WINDOW_CAP = %du" % CAP in text


def test_refusals_name_the_field_or_the_position(tool):
    good = [(0, U8, 0), (1, BE32, 1), (2, U32, 40)]
    cases = [
        (44, good[:2]),                                   # position 2 never
        (44, good[1:]),                                   # position 0 never
        (44, good + [(1, BE32, 1)]),                      # twice, at the same offset
        (44, good + [(1, U8, 43)]),                       # twice, at DIFFERENT offsets
        (44, [(3, U8, 0)] + good),                        # a position >= n_initial
        (44, [(NONE, U8, 0)] + good),
        (44, [(0, 3, 0)] + good[1:]),                     # unknown encodings
        (44, [(0, 15, 0)] + good[1:]),
        (44, [(0, 21, 0)] + good[1:]),
        (43, good),                                       # offset + size > pitch by one byte
        (44, good[:2] + [(2, U32, 41)]),
        (44, good[:2] + [(2, U32, (1 << 64) - 1)]),       # offset + size wraps 2^64
        (44, good[:2] + [(2, BE32, (1 << 64) - 32)]),     # ... to exactly 0
        (44, good[:2] + [(2, U8, (1 << 64) - 1)]),
        (0, good),                                        # pitch 0
        (44, good, 0),                                    # null records while there are fields and live instances
        ((1 << 57) // 130 + 1, good),                     # B * pitch beyond any buffer
        (44, []),                                         # no fields for a circuit with initial witnesses
    ]
    got = check(tool, VIEW3, cases)
    assert all(g[0] == "err" for g in got)
    texts = [g[1] for g in got]
    assert texts[0].startswith("position 2 (initial witness 9)") and texts[1].startswith("position 0 (initial witness 5)")
    assert texts[2] == texts[3] == "position 1 is supplied twice (fields 1 and 3)"
    assert texts[4].startswith("field 0 (position 3)") and texts[11].startswith("field 2 (position 2)") and "beyond the pitch" in texts[11]
    assert texts[14].startswith("field 0 (position 0)") and texts[15] == "null records" and texts[17].startswith("position 0 ")
    # the null descriptor, null fields with n_fields > 0, the null batch
    lines = tool([VIEW3.command(), "records null", records_command(44, None, null_fields=3), "noview", records_command(44, good)])
    assert lines == ["err -1 null argument", "err -1 null fields", "err -1 null batch"]


def test_accepted_overlaps_any_order_and_no_fields(tool):
    cases = [
        (44, [(0, U8, 0), (1, BE32, 1), (2, U32, 40)]),
        (44, [(2, U32, 40), (1, BE32, 1), (0, U8, 0)]),                    # descending order
        (44, [(0, U32, 4), (1, U32, 4), (2, U16, 5)]),                     # the same and overlapping bytes
        (32, [(0, BE32, 0), (1, LE32, 0), (2, MONT, 0)]),
        (1 << 40, [(0, U8, 0), (1, BE32, (1 << 40) - 32), (2, U32, 40)]),  # a pitch beyond 32 bits
    ]
    got = check(tool, VIEW3, cases)
    assert all(g[0] == "ok" for g in got)
    assert got[0][3] == [(105, 2, U8, 0), (106, NONE, BE32, 1), (109, 0, U32, 40)]  # rows and planes are the handle's, per position
    assert got[1][3] == got[0][3][::-1]
    # null records are fine without live instances; n_fields == 0 for n_initial == 0 reads nothing (any pitch, any pointer)
    check(tool, View(0, [5, 6, 9]), [(44, cases[0][1], 0)])
    none = check(tool, View(130, []), [(0, []), (7, [], 0)])
    assert none[0] == ("ok", 0, [], []) and none[1] == ("ok", 7, [], [])
    lines = tool([View(130, []).command(), records_command(0, None, null_fields=0)])
    assert lines[0].startswith("ok 1 0 0 0")


@pytest.mark.parametrize("pitch", [1, 33, 108, CAP - 1, CAP, CAP + 1])
def test_window_cut_at_the_pitches_around_the_cap(tool, pitch):
    if pitch == 1:
        fields = [(0, U8, 0)]
    elif pitch == 33:
        fields = [(0, BE32, 1)]
    elif pitch == 108:
        fields = MIXED108
    else:
        fields = [(0, BE32, 0), (1, U8, pitch - 1), (2, U128, pitch - 17), (3, U16, 100), (4, LE32, pitch - 33)]
    view = View(65, list(range(1, len(fields) + 1)), rows=[100 + k for k in range(len(fields))])
    got = check(tool, view, [(pitch, fields)])[0]
    assert_windows_hold_whole_fields(got, fields, pitch)
    if pitch <= CAP:
        assert got[2] == [(0, pitch, 0, len(fields))]  # the record is the window: contiguous records, the fields in the caller's order
        assert [t[0] - 100 for t in got[3]] == [f[0] for f in fields]
    else:
        assert got[2] == [(0, CAP, 0, 4), (CAP, 1, 4, 1)]  # the last byte of the record no longer fits the window that begins at byte 0


def test_window_cut_of_long_records(tool):
    # a 1 500-byte record with fields at both ends: two windows, nothing in between is covered
    fields = [(0, BE32, 2), (1, U8, 0), (2, LE32, 1468), (3, U16, 1465)]
    view = View(65, [1, 2, 3, 4], rows=[100, 101, 102, 103])
    got = check(tool, view, [(1500, fields)])[0]
    assert got[2] == [(0, 34, 0, 2), (1465, 35, 2, 2)]
    assert_windows_hold_whole_fields(got, fields, 1500)
    # random long records: whole fields, the cap, and the model's cut
    rng = random.Random(0x4EC04D)
    cases = []
    for _ in range(40):
        pitch = rng.choice([257, 300, 777, 1500, 4096, 70000])
        n = rng.randrange(1, 10)
        order = list(range(9))
        rng.shuffle(order)
        fl = []
        for position in sorted(order[:n]) + order[n:]:
            encoding = rng.choice(ENCODINGS)
            fl.append((position, encoding, rng.randrange(0, pitch - size_of(encoding) + 1)))
        rng.shuffle(fl)
        cases.append((pitch, fl))
    for c, g in zip(cases, check(tool, VIEW_ROWS, cases)):
        assert g[0] == "ok"
        assert_windows_hold_whole_fields(g, c[1], c[0])
    # a field of exactly the cap's reach: 32 bytes ending at byte 256 of the window stay, one byte further opens a window
    a = check(tool, View(1, [1, 2], rows=[100, 101]), [(600, [(0, U8, 10), (1, BE32, 10 + CAP - 32)]), (600, [(0, U8, 10), (1, BE32, 10 + CAP - 31)])])
    assert len(a[0][2]) == 1 and a[0][2][0][1] == CAP and len(a[1][2]) == 2


def test_plan_equality(tool):
    """a record plan equals a record plan of the same pitch and tables (whatever the pointer), and never a plan of another kind"""
    fields = [(0, U8, 0), (1, BE32, 1), (2, U32, 40)]
    lines = tool([VIEW3.command(), records_command(44, fields), records_command(44, fields, PTR + 64), "eq", records_command(45, fields), "eq",
                  records_command(44, fields[::-1]), "eq", "plain 4096", "eq", records_command(44, fields), "eq"])
    assert [l for l in lines if l.startswith("eq")] == ["eq 1", "eq 0", "eq 0", "eq 0", "eq 0"]
