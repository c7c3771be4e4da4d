"""The checks, the window cut, the cover bitmaps and the field table of the record export (acvm_amd/csrc/record_out_plan.cpp) without a device
and without a handle: the module is compiled as plain C++ (tools/record_out_plan_host_test.cpp) -- once as it is, once with AddressSanitizer and
UndefinedBehaviorSanitizer as `make asan` builds it, a stand-alone program either way -- and its answers are judged byte-wise in Python. The
refusals are those tests/test_gpu_records_out.py asserts on the device."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE32, LE32, MONT, U8, U16, U32, U64, U128 = 0, 1, 2, 16, 17, 18, 19, 20
ENCODINGS = (BE32, LE32, MONT, U8, U16, U32, U64, U128)
PTR = (1 << 20) + 3  # a device address of no alignment at all
CAP = 256
VALUE, MASK, BOTH = 1, 2, 3


def size_of(encoding):
    return 1 << (encoding - U8) if U8 <= encoding <= U128 else 32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    sources = [os.path.join(ROOT, "tools", "record_out_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "record_out_plan.cpp"),
               os.path.join(ROOT, "acvm_amd", "csrc", "import_plan.cpp")]
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("record_out_plan") / "record_out_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sources + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "record_out_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/record_out_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith(("live", "nolive")) for c in commands)
        return lines
    return run


def out_command(pitch, fields, first=0, n=65, ptr=PTR, lst=0, null_fields=None):
    """fields: (witness, encoding, offset, mask offset or None)"""
    head = "out %d %d %d %d %d " % (pitch, ptr, first, n, lst)
    if null_fields is not None:
        return head + "null%d" % null_fields
    return head + "%d" % len(fields) + "".join(" %d %d %d %s" % (w, e, o, "-" if m is None else str(m)) for w, e, o, m in fields)


def parse(line):
    """("err", text) or ("ok", pitch, first, n, mont, plain, witnesses, windows [(offset, length, first, n, bitmap int)], entries [(w, e, byte, kind, mask byte)])"""
    if line.startswith("err "):
        code, text = line[4:].split(" ", 1)
        assert code == "-1"
        return ("err", text)
    tok = [int(t) for t in line.split()[1:]]
    pitch, first, n, n_windows, n_entries, mont, plain, n_distinct = tok[:8]
    witnesses = tok[8:8 + n_distinct]
    at = 8 + n_distinct
    windows = []
    for _ in range(n_windows):
        bitmap = sum(word << (32 * k) for k, word in enumerate(tok[at + 4:at + 12]))
        windows.append(tuple(tok[at:at + 4]) + (bitmap,))
        at += 12
    rest = tok[at:]
    assert len(rest) == 4 * n_entries
    entries = [(rest[i], rest[i + 1], rest[i + 2], rest[i + 3] & 3, rest[i + 3] >> 8) for i in range(0, len(rest), 4)]
    assert all(e[3] in (VALUE, MASK, BOTH) and e[4] < CAP and (e[3] & MASK or e[4] == 0) for e in entries)
    return ("ok", pitch, first, n, bool(mont), bool(plain), witnesses, windows, entries)


def covered_ranges(fields):
    """every covered range of the record: (begin, end, field index, is the mask byte)"""
    out = []
    for f, (w, e, o, m) in enumerate(fields):
        out.append((o, o + size_of(e), f, False))
        if m is not None:
            out.append((m, m + 1, f, True))
    return out


def assert_plan_covers_exactly(answer, pitch, fields):
    """Byte-wise: the windows lie inside the record, hold at most the cap, do not overlap; the entries write every covered byte of the record
    exactly once and nothing else; each window's bitmap is exactly the bytes its entries write; element and mask byte of a field that fall into
    one window are one fused entry."""
    _, _, _, _, mont, plain, witnesses, windows, entries = answer
    assert witnesses == sorted({f[0] for f in fields})
    assert mont == any(f[1] == MONT for f in fields) and plain == any(f[1] != MONT for f in fields)
    want = {}  # byte of the record -> (field, is mask)
    for begin, end, f, is_mask in covered_ranges(fields):
        for b in range(begin, end):
            assert b not in want
            want[b] = (f, is_mask)
    got = {}
    by_field = {}
    last_end = 0
    assert sum(w[3] for w in windows) == len(entries)
    for offset, length, first, n, bitmap in windows:
        assert 0 < length <= CAP and offset + length <= pitch and offset >= last_end
        last_end = offset + length
        assert first == sum(w[3] for w in windows if w[0] < offset)
        written = set()
        for w, e, byte, kind, mask_byte in entries[first:first + n]:
            spans = ([(byte, byte + size_of(e), False)] if kind & VALUE else []) + ([(mask_byte, mask_byte + 1, True)] if kind & MASK else [])
            for begin, end, is_mask in spans:
                assert end <= length
                for b in range(begin, end):
                    assert offset + b not in got, "a byte written twice"
                    got[offset + b] = (w, e, is_mask, b - begin)
                    written.add(b)
            by_field.setdefault((w, e), []).append((offset, kind))
        assert bitmap == sum(1 << b for b in written), "the bitmap is the bytes the window's entries write"
        assert bitmap >> length == 0
    assert set(got) == set(want)
    for b, (f, is_mask) in want.items():
        w, e, o, m = fields[f]
        assert got[b] == (w, e, is_mask, b - (m if is_mask else o))
    if pitch <= CAP:
        assert len(windows) <= 1 and all(w[0] == 0 and w[1] == pitch for w in windows)
        assert [(e[0], e[1]) for e in entries] == [(f[0], f[1]) for f in fields] and all(e[3] == (BOTH if f[3] is not None else VALUE) for e, f in zip(entries, fields))
    # fused where one window holds both, split where not
    n_expected = 0
    for w, e, o, m in fields:
        window_of = lambda b: [k for k, win in enumerate(windows) if win[0] <= b < win[0] + win[1]][0]
        n_expected += 1 if m is None or window_of(o) == window_of(m) else 2
    assert len(entries) == n_expected


GOOD = [(1, U8, 0, 41), (2, BE32, 1, None), (3, U32, 36, 40)]


def test_the_cap_is_the_kernels(tool):
    assert tool(["cap"]) == ["cap %d" % CAP]


# ---- the refusals, one by one
@pytest.mark.parametrize("case", [
    ("an unknown encoding", dict(pitch=44, fields=[(1, 3, 0, None)] + GOOD[1:]), "field 0 (witness 1): unknown encoding 3"),
    ("an unknown encoding", dict(pitch=44, fields=GOOD[:2] + [(3, 21, 36, None)]), "field 2 (witness 3): unknown encoding 21"),
    ("offset + size > pitch by one byte", dict(pitch=39, fields=[(1, U8, 0, None), GOOD[1], (3, U32, 36, None)]), "field 2 (witness 3): offset 36 + size 4 is beyond the pitch 39"),
    ("offset + size wraps 2^64", dict(pitch=44, fields=GOOD[:2] + [(3, U32, (1 << 64) - 2, None)]), "field 2 (witness 3): offset"),
    ("offset + size wraps to exactly 0", dict(pitch=44, fields=GOOD[:2] + [(3, BE32, (1 << 64) - 32, None)]), "field 2 (witness 3): offset"),
    ("pitch 0", dict(pitch=0, fields=GOOD), "field 0 (witness 1): offset 0 + size 1 is beyond the pitch 0"),
    ("mask_offset == pitch", dict(pitch=44, fields=GOOD[:2] + [(3, U32, 36, 44)]), "field 2 (witness 3): mask offset 44 is beyond the pitch 44"),
    ("mask_offset huge", dict(pitch=44, fields=GOOD[:2] + [(3, U32, 36, (1 << 64) - 2)]), "field 2 (witness 3): mask offset"),
    ("two elements overlap", dict(pitch=44, fields=GOOD + [(4, U16, 32, None)]), "the element of field 3 (witness 4) at offset 32 overlaps the element of field 1 (witness 2) at [1, 33)"),
    ("the same witness twice on the same bytes", dict(pitch=44, fields=GOOD + [(3, U32, 36, None)]), "overlaps"),
    ("a mask byte inside an element", dict(pitch=44, fields=GOOD[:2] + [(3, U32, 36, 20)]), "the mask byte of field 2 (witness 3) at offset 20 overlaps the element of field 1 (witness 2)"),
    ("two mask bytes on one byte", dict(pitch=44, fields=[(1, U8, 0, 41), (2, BE32, 1, 41)]), "the mask byte of field 1 (witness 2) at offset 41 overlaps the mask byte of field 0 (witness 1)"),
    ("a field's mask byte inside its own element", dict(pitch=44, fields=[(2, BE32, 1, 32)]), "overlaps"),
    ("a range beyond the live instances", dict(pitch=44, fields=GOOD, first=60, n=6), "instances [60, 66) are beyond the 65 live instances"),
    ("first beyond the live instances", dict(pitch=44, fields=GOOD, first=66, n=0), "are beyond the 65 live instances"),
    ("first + n wraps 2^32", dict(pitch=44, fields=GOOD, first=2, n=(1 << 32) - 1), "are beyond the 65 live instances"),
    ("first != 0 with a list", dict(pitch=44, fields=GOOD, first=1, n=3, lst=1), "first must be 0 for a list export"),
    ("a null buffer while there is something to write", dict(pitch=44, fields=GOOD, ptr=0), "null records"),
    ("n * pitch beyond any buffer", dict(pitch=(1 << 57) // 65 + 1, fields=GOOD), "is beyond any device buffer"),
], ids=lambda c: c[0])
def test_refusal(tool, case):
    _, args, text = case
    answer = parse(tool(["live 65", out_command(**args)])[0])
    assert answer[0] == "err" and text in answer[1], answer


def test_refusals_of_the_arguments_themselves(tool):
    lines = tool(["live 65", "out null", out_command(44, None, null_fields=3), "nolive", out_command(44, GOOD)])
    assert lines == ["err -1 null argument", "err -1 null fields", "err -1 null batch"]


def test_what_is_accepted(tool):
    cases = [
        dict(pitch=44, fields=GOOD),
        dict(pitch=44, fields=GOOD[::-1]),                                                    # any order
        dict(pitch=44, fields=[(7, U8, 0, 1), (7, BE32, 2, 34)]),                                # one witness in two encodings
        dict(pitch=44, fields=GOOD, first=60, n=5),                                           # first > 0, up to the last live instance
        dict(pitch=44, fields=GOOD, first=65, n=0),
        dict(pitch=44, fields=GOOD, first=0, n=1000, lst=1),                                  # a list is as long as it likes
        dict(pitch=44, fields=GOOD, n=0, ptr=0),                                              # nothing to write: a null buffer is fine
        dict(pitch=44, fields=[], ptr=0),
        dict(pitch=0, fields=[], ptr=0),
        dict(pitch=1 << 40, fields=[(1, U8, 0, (1 << 40) - 1), (2, BE32, (1 << 40) - 33, None)]),  # a pitch beyond 32 bits
        dict(pitch=44, fields=[(1 << 31, U8, 0, None), (0xFFFFFFFF, U8, 1, 2)]),               # a witness beyond any circuit is the device's to judge
    ]
    for c, line in zip(cases, tool(["live 65"] + [out_command(**c) for c in cases])):
        answer = parse(line)
        assert answer[0] == "ok", (c, answer)
        assert answer[1:4] == (c["pitch"], c.get("first", 0), c.get("n", 65))
        assert_plan_covers_exactly(answer, c["pitch"], c["fields"])
    fused = parse(tool(["live 65", out_command(44, GOOD)])[0])
    assert fused[8] == [(1, U8, 0, BOTH, 41), (2, BE32, 1, VALUE, 0), (3, U32, 36, BOTH, 40)]
    lines = tool(["live 65", out_command(0, None, null_fields=0)])
    assert lines[0].startswith("ok 0 0 65 0 0")


def test_a_mask_byte_in_another_window_than_its_element(tool):
    # a 1 500-byte record: the element at the front, its mask byte at the very end; a second field fused at the end
    fields = [(1, BE32, 2, 1499), (2, U16, 1465, 1467), (3, U8, 0, None)]
    answer = parse(tool(["live 65", out_command(1500, fields)])[0])
    assert answer[0] == "ok"
    assert [w[:4] for w in answer[7]] == [(0, 34, 0, 2), (1465, 35, 2, 2)]
    assert answer[8] == [(3, U8, 0, VALUE, 0), (1, BE32, 2, VALUE, 0), (2, U16, 0, BOTH, 2), (1, BE32, 0, MASK, 34)]
    assert_plan_covers_exactly(answer, 1500, fields)
    # exactly the cap's reach stays one window, one byte further opens another
    a = [parse(l) for l in tool(["live 1", out_command(600, [(1, U8, 10, None), (2, BE32, 10 + CAP - 32, None)], n=1), out_command(600, [(1, U8, 10, None), (2, BE32, 10 + CAP - 31, None)], n=1),
                                 out_command(600, [(1, U8, 10, 10 + CAP - 1)], n=1), out_command(600, [(1, U8, 10, 10 + CAP)], n=1)])]
    assert [len(x[7]) for x in a] == [1, 2, 1, 2] and a[0][7][0][1] == CAP and a[2][8] == [(1, U8, 0, BOTH, CAP - 1)]


def _random_fields(rng, pitch, n_fields):
    """fields whose covered ranges do not overlap, placed at random"""
    taken = set()
    fields = []
    for _ in range(n_fields):
        for _attempt in range(50):
            e = rng.choice(ENCODINGS)
            o = rng.randrange(0, pitch - size_of(e) + 1) if pitch >= size_of(e) else None
            if o is None or any(b in taken for b in range(o, o + size_of(e))):
                continue
            m = None
            if rng.random() < 0.6:
                m = rng.randrange(0, pitch) if rng.random() < 0.5 else min(pitch - 1, o + size_of(e))
                if m in taken or o <= m < o + size_of(e):
                    m = None
            taken.update(range(o, o + size_of(e)))
            if m is not None:
                taken.add(m)
            fields.append((rng.randrange(0, 40), e, o, m))
            break
    rng.shuffle(fields)
    return fields


def test_seeded_random_descriptors(tool):
    rng = random.Random(0x4EC04D07)
    cases = []
    for _ in range(120):
        pitch = rng.choice([1, 2, 3, 7, 33, 44, 108, 128, CAP - 1, CAP, CAP + 1, 300, 777, 1500, 4096, 70000])
        cases.append((pitch, _random_fields(rng, pitch, rng.randrange(1, 12))))
    assert sum(len(c[1]) for c in cases) > 400 and any(any(f[3] is not None for f in c[1]) and c[0] > CAP for c in cases)
    split = 0
    for (pitch, fields), line in zip(cases, tool(["live 65"] + [out_command(p, f) for p, f in cases])):
        answer = parse(line)
        assert answer[0] == "ok", (pitch, fields, answer)
        assert_plan_covers_exactly(answer, pitch, fields)
        split += sum(e[3] == MASK for e in answer[8])
    assert split > 10  # mask bytes that lie in another window than their elements were among them
    # and the same descriptors with one more range laid over a covered byte are refused
    bad = []
    for pitch, fields in cases:
        if not fields:
            continue
        w, e, o, m = fields[0]
        bad.append((pitch, fields + [(99, U8, o + size_of(e) - 1, None)]))
    for line in tool(["live 65"] + [out_command(p, f) for p, f in bad]):
        answer = parse(line)
        assert answer[0] == "err" and "overlaps" in answer[1]
