"""The assigned set every host read rests on (acvm_amd/csrc/assigned_view.hpp) without a device and without a handle: the header is compiled as
plain C++ (tools/assigned_view_host_test.cpp) and its answers are judged by the Python restatement below, written from the rule's words:

  * witness w is assigned for instance j: producer[w] is set, if the level kernels solved j; bit w of j's column of the bitmap (row w >> 5 of
    n_slow words, word = j's lane, bit w & 31), if j took the exact path; never for w at or beyond n_witnesses;
  * an unassigned witness reads as 32 zero bytes, an assigned one is left as it was read;
  * the witness an extraction names: the lowest instance that lacks a listed witness, then that instance's first missing witness in the list's order;
  * a row of the bitmap is copied at most once per view, only rows of listed witnesses, and none when no exact lane is looked at."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    """the tool compiled as it is, and the second binary of `make asan` (AddressSanitizer + UndefinedBehaviorSanitizer): a stand-alone program on
    the CPU, given the same command streams -- a report ends it with a non-zero status"""
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("assigned_view") / "assigned_view_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tools", "assigned_view_host_test.cpp"), "-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "assigned_view_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/assigned_view_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith("batch") for c in commands)
        return lines
    return run


def fmt(lst):
    return "null" if lst is None else "e" if not len(lst) else ",".join(str(x) for x in lst)


class Model:
    """a solved batch as the rule sees it: producer[], the lane of every instance (-1: level kernels), per lane the set of assigned witnesses"""

    def __init__(self, nw, producer, slow_index, lane_sets):
        self.nw, self.producer, self.slow_index, self.lane_sets = nw, list(producer), list(slow_index), [set(s) for s in lane_sets]  # (slow_index None: instance j is lane j)
        self.n_slow = len(self.lane_sets)
        assert len(self.producer) == nw and all(-1 <= t < self.n_slow for t in self.slow_index)

    def command(self):
        words = [0] * (((self.nw + 31) // 32) * self.n_slow)
        for t, have in enumerate(self.lane_sets):
            for w in have:
                words[(w // 32) * self.n_slow + t] |= 1 << (w % 32)
        return "batch %d %d %s %s %s" % (self.nw, self.n_slow, fmt(self.producer), fmt(self.slow_index), fmt(words))

    def assigned(self, j, w):
        if w >= self.nw:
            return False
        t = self.lane(j)
        return self.producer[w] != NONE if t < 0 else w in self.lane_sets[t]

    def lane(self, j):
        return j if self.slow_index is None else self.slow_index[j]

    def fill(self, first, n, lanes, sel):
        sel = list(range(self.nw)) if sel is None else sel
        flags, values = "", ""
        for j in range(first, first + n):
            for w in sel:
                if lanes == "LEVEL" and self.lane(j) >= 0:
                    flags, values = flags + ".", values + "k"
                else:
                    a = self.assigned(j, w)
                    flags, values = flags + "01"[a], values + "zk"[a]
        return flags or "e", values or "e"

    def first_missing(self, first, n, listed):
        for j in range(first, first + n):          # the lowest instance ...
            for w in listed:                       # ... and its first missing witness in the caller's order
                if not self.assigned(j, w):
                    return "missing %d %d" % (j, w)
        return "missing none"

    def rows_allowed(self, instances, witnesses):
        """the rows a view may copy for these instances and witnesses"""
        if not any(self.lane(j) >= 0 for j in instances):
            return set()
        return {w // 32 for w in witnesses if w < self.nw}


def split(line):
    answer, rows = line.split(" | ")
    return answer, [] if rows == "-" else [int(x) for x in rows.split(",")]


def check(tool, model, calls):
    """calls: ("assigned", [(j, w)]) / ("fill", first, n, lanes, whole, sel) / ("missing", first, n, list); every answer against the model"""
    commands = [model.command()]
    for c in calls:
        if c[0] == "assigned":
            commands.append("assigned " + " ".join("%d %d" % p for p in c[1]))
        elif c[0] == "fill":
            commands.append("fill %d %d %s %d %s" % (c[1], c[2], c[3], c[4], fmt(c[5])))
        else:
            commands.append("missing %d %d %s" % (c[1], c[2], fmt(c[3])))
    answers = []
    for c, line in zip(calls, tool(commands)):
        got, rows = split(line)
        if c[0] == "assigned":
            want = "assigned " + " ".join("01"[model.assigned(j, w)] for j, w in c[1])
            allowed = {w // 32 for j, w in c[1] if model.lane(j) >= 0 and w < model.nw}
        elif c[0] == "fill":
            want = "fill %s %s" % model.fill(c[1], c[2], c[3], c[5])
            sel = range(model.nw) if c[5] is None else c[5]
            allowed = set() if c[3] == "LEVEL" or c[4] else model.rows_allowed(range(c[1], c[1] + c[2]), sel)
        else:
            want = model.first_missing(c[1], c[2], c[3])
            allowed = model.rows_allowed(range(c[1], c[1] + c[2]), c[3])
        assert got == want, (c, model.command())
        assert len(rows) == len(set(rows)) and set(rows) <= allowed, (c, rows, allowed)
        answers.append((got, rows))
    return answers


# 33 witnesses: two words of the bitmap. Witnesses 3 and 32 have no producer; lane 0 lacks 0 and 31, lane 1 lacks 32 only, lane 2 has nothing
NW = 33
PRODUCER = [NONE if w in (3, 32) else w + 100 for w in range(NW)]


def _mixed():
    return Model(NW, PRODUCER, [-1, 0, 1, -1, -1, 2, -1], [set(range(NW)) - {0, 31}, set(range(NW)) - {32}, set()])


def test_every_pair_of_a_mixed_batch(tool):
    m = _mixed()
    pairs = [(j, w) for j in range(7) for w in list(range(NW)) + [NW, NW + 31, 64, 1 << 20]]
    (got, rows), = check(tool, m, [("assigned", pairs)])
    assert sorted(rows) == [0, 1]  # both words were needed, each copied once for all 3 x 37 questions about exact lanes
    # bit 31 and bit 32 lie in different words: lane 0 lacks 31 and has 32, lane 1 the other way round
    flags = dict(zip(pairs, got.split()[1:]))
    assert (flags[(1, 31)], flags[(1, 32)], flags[(2, 31)], flags[(2, 32)]) == ("0", "1", "1", "0")
    assert flags[(0, 32)] == "0" and flags[(0, 31)] == "1"  # the level kernels' lanes follow producer[] whatever the bitmap says


def test_no_exact_lanes_and_one(tool):
    none = Model(NW, PRODUCER, [-1] * 5, [])
    calls = [("assigned", [(j, w) for j in range(5) for w in (0, 3, 31, 32, 33)]), ("fill", 0, 5, "ALL", 0, None), ("fill", 1, 3, "ALL", 1, [32, 0, 40]),
             ("fill", 0, 0, "ALL", 0, [1]), ("fill", 2, 2, "ALL", 0, []), ("missing", 0, 5, [0, 1, 2]), ("missing", 0, 5, [0, 32, 3]), ("missing", 4, 1, [3]), ("missing", 0, 0, [3]),
             ("missing", 0, 5, [])]
    got = check(tool, none, calls)
    assert all(rows == [] for _, rows in got)
    assert [g for g, _ in got[5:]] == ["missing none", "missing 0 32", "missing 4 3", "missing none", "missing none"]
    one = Model(NW, PRODUCER, [-1, -1, 0, -1], [{1, 2, 32}])
    got = check(tool, one, [("assigned", [(2, w) for w in range(40)]), ("fill", 0, 4, "ALL", 0, None), ("fill", 2, 1, "ALL", 0, None), ("fill", 0, 2, "ALL", 0, None),
                            ("missing", 0, 4, [1, 2]), ("missing", 2, 1, [32, 2, 1]), ("missing", 2, 1, [32, 2, 0, 1]), ("missing", 0, 4, [32])])
    assert got[3][1] == []  # (a range of level lanes only copies nothing)
    assert [g for g, _ in got[4:]] == ["missing none", "missing none", "missing 2 0", "missing 0 32"]


@pytest.mark.parametrize("first,n,kind", [(3, 2, "level"), (1, 2, "exact"), (0, 7, "mixed"), (2, 4, "mixed"), (5, 1, "exact"), (6, 1, "level")])
def test_ranges_of_level_lanes_exact_lanes_and_both(tool, first, n, kind):
    m = _mixed()
    exact = [m.slow_index[j] >= 0 for j in range(first, first + n)]
    assert {"level": not any(exact), "exact": all(exact), "mixed": any(exact) and not all(exact)}[kind]
    lists = [None, [0], [31, 32], [32, 31], [5, 5, 3, 5], [33, 0, 1 << 31, 31], list(range(NW - 1, -1, -1))]  # repeated witnesses, w >= n_witnesses
    calls = [("fill", first, n, lanes, whole, sel) for sel in lists for lanes in ("ALL", "LEVEL") for whole in (0, 1)]
    calls += [("missing", first, n, sel) for sel in lists[1:]]
    got = check(tool, m, calls)
    if kind == "level":
        assert all(rows == [] for _, rows in got)
    else:
        by_call = dict(zip([c[:5] + (tuple(c[5]) if c[5] else None,) for c in calls if c[0] == "fill"], got))
        assert by_call[("fill", first, n, "ALL", 0, None)][1] in ([0, 1], [1, 0])
        assert by_call[("fill", first, n, "ALL", 0, (5, 5, 3, 5))][1] == [0]  # one row for four entries of one word
        assert by_call[("fill", first, n, "ALL", 0, (31, 32))][1] == [0, 1]


def test_the_witness_an_extraction_names(tool):
    """the lowest failing instance's first missing witness, in list order, is not what a scan by witness finds first"""
    # lane 0 = instance 1 lacks 9 only; lane 1 = instance 4 lacks 2 and 9; the level lanes lack 3
    m = Model(NW, PRODUCER, [-1, 0, -1, -1, 1], [set(range(NW)) - {9}, set(range(NW)) - {2, 9}])
    calls = [
        ("missing", 1, 4, [2, 9]),      # witness 2 is missing first in the list, but only for instance 4; instance 1 is lower and lacks 9
        ("missing", 1, 4, [9, 2]),
        ("missing", 4, 1, [9, 2]),      # for instance 4 alone the order of the list decides
        ("missing", 4, 1, [2, 9]),
        ("missing", 0, 5, [2, 9, 3]),   # a level lane in front: instance 0 lacks 3, the last entry
        ("missing", 1, 1, [2, 3, 9]),   # an exact lane has what its bitmap says, not producer[]: 3 is there
        ("missing", 2, 3, [9, 2, 3]),   # instances 2 and 3 are level lanes (lack 3); 4 comes later
        ("missing", 1, 4, [2, 2, 9, 9]),
        ("missing", 1, 1, [2, 5]),
    ]
    got = [g for g, _ in check(tool, m, calls)]
    assert got == ["missing 1 9", "missing 1 9", "missing 4 9", "missing 4 2", "missing 0 3", "missing 1 9", "missing 2 3", "missing 1 9", "missing none"]


def test_lanes_as_instances(tool):
    """a null slow_index: the view is over the lanes themselves, instance j is lane j (the outcome of an exact job)"""
    m = Model(NW, PRODUCER, [0, 1, 2], [set(range(NW)) - {0, 31}, set(range(NW)) - {32}, {3}])
    want = check(tool, m, [("fill", 0, 3, "ALL", 1, [31, 32, 3, 40]), ("fill", 1, 2, "ALL", 0, None), ("missing", 0, 3, [3, 31]), ("assigned", [(2, 3), (2, 4), (0, 32)])])
    m.slow_index = None
    got = check(tool, m, [("fill", 0, 3, "ALL", 1, [31, 32, 3, 40]), ("fill", 1, 2, "ALL", 0, None), ("missing", 0, 3, [3, 31]), ("assigned", [(2, 3), (2, 4), (0, 32)])])
    assert [g for g, _ in got] == [g for g, _ in want] and got[2][0] == "missing 0 31"


def _random_model(rng):
    nw = rng.choice((1, 5, 31, 32, 33, 64, 65, 100))
    B = rng.randrange(1, 12)
    producer = [NONE if rng.random() < 0.15 else rng.randrange(1000) for _ in range(nw)]
    style = rng.choice(("level", "exact", "mixed", "mixed"))
    flagged = [style == "exact" or (style == "mixed" and rng.random() < 0.4) for _ in range(B)]
    slow_index, lanes = [], []
    for f in flagged:
        slow_index.append(len(lanes) if f else -1)
        if f:
            p = rng.choice((0.0, 0.5, 0.9, 0.97, 1.0))
            lanes.append({w for w in range(nw) if rng.random() < p})
    return Model(nw, producer, slow_index, lanes), B


def test_random_batches_against_the_restatement(tool):
    rng = random.Random(0xA551)
    n_calls, named = 0, set()
    for _ in range(60):
        m, B = _random_model(rng)
        calls = []
        for _ in range(6):
            first = rng.randrange(B)
            n = rng.randrange(0, B - first + 1)
            k = rng.randrange(0, 7)
            sel = [rng.randrange(m.nw + 3) if rng.random() < 0.2 else rng.randrange(m.nw) for _ in range(k)]
            calls.append(("fill", first, n, rng.choice(("ALL", "ALL", "LEVEL")), rng.randrange(2), rng.choice((None, sel))))
            inside = [w for w in sel if w < m.nw]  # (the extraction refuses a witness beyond n_witnesses before it asks)
            calls.append(("missing", first, n, inside))
            calls.append(("assigned", [(rng.randrange(B), rng.randrange(m.nw + 2)) for _ in range(5)]))
        got = check(tool, m, calls)
        n_calls += len(calls)
        named |= {g.split()[1] != "none" for (g, _), c in zip(got, calls) if c[0] == "missing"}
    assert n_calls >= 1000 and named == {True, False}
