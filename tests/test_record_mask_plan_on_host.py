"""The checks, the unit placement and the tables of the masked record import (acvm_amd/csrc/record_plan.cpp import_plan_records_masked) without a
device and without a handle: the module is compiled as plain C++ (tools/record_mask_plan_host_test.cpp) -- once as it is, once with
AddressSanitizer and UndefinedBehaviorSanitizer as `make asan` builds it, a stand-alone program either way -- and its answers are judged by the
Python restatement below, which sits on the unmasked plan's restatement of tests/test_record_plan_on_host.py."""
import importlib.util
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unmasked_module():
    spec = importlib.util.spec_from_file_location("_record_plan_for_masks", os.path.join(ROOT, "tests", "test_record_plan_on_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_RP = _unmasked_module()
View, size_of, fmt, records_command, unmasked_model = _RP.View, _RP.size_of, _RP.fmt, _RP.records_command, _RP.model
BE32, LE32, MONT, U8, U16, U32, U64, U128, ENCODINGS = _RP.BE32, _RP.LE32, _RP.MONT, _RP.U8, _RP.U16, _RP.U32, _RP.U64, _RP.U128, _RP.ENCODINGS
NONE, PTR, CAP = _RP.NONE, _RP.PTR, _RP.CAP
MASK_NONE, MASK_FAR = 0xFFFFFFFF, 0xFFFFFFFE
WINDOW_WORDS, FIELD_WORDS = 6, 8  # the masked tables; the unmasked ones keep 5 and 4


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    sources = [os.path.join(ROOT, "tools", "record_mask_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "record_plan.cpp"),
               os.path.join(ROOT, "acvm_amd", "csrc", "import_plan.cpp")]
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("record_mask_plan") / "record_mask_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sources + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "record_mask_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/record_mask_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith(("view", "noview")) for c in commands)
        return lines
    return run


def masked_command(pitch, fields, ptr=PTR, null_fields=None):
    """fields: (position, encoding, offset, mask_offset or None)"""
    if null_fields is not None:
        return "masked %d %d null%d" % (pitch, ptr, null_fields)
    return "masked %d %d %d" % (pitch, ptr, len(fields)) + "".join(" %d %d %d %s" % (p, e, o, "n" if m is None else str(m)) for p, e, o, m in fields)


# ---- the restatement: ("err", text), or ("unmasked", pitch, windows, table) exactly as the unmasked model answers, or
# ("masked", pitch, windows [(offset, length, first, n, miss_base)], table [(row, plane, encoding, byte, position, mask, far_offset)])
def model(view, pitch, fields, ptr=PTR):
    plain = unmasked_model(view, pitch, [f[:3] for f in fields], ptr)
    if plain[0] == "err":
        return plain
    for f, (position, encoding, offset, mask) in enumerate(fields):
        if mask is not None and mask >= pitch:
            return ("err", "field %d (position %d): mask_offset %d is not below the pitch %d" % (f, position, mask, pitch))
    if all(f[3] is None for f in fields):
        return ("unmasked",) + plain[1:]
    units = []
    for position, encoding, offset, mask in fields:
        begin, end, far = offset, offset + size_of(encoding), False
        if mask is not None:
            b, e = min(begin, mask), max(end, mask + 1)
            if e - b <= CAP:
                begin, end = b, e
            else:
                far = True
        units.append((begin, end, far))
    if pitch <= CAP:
        cuts = [[0, pitch, list(range(len(fields)))]]
    else:
        cuts = []
        for f in sorted(range(len(fields)), key=lambda f: (units[f][0], f)):
            if not cuts or units[f][1] - cuts[-1][0] > CAP:
                cuts.append([units[f][0], 0, []])
            cuts[-1][1] = max(cuts[-1][1], units[f][1] - cuts[-1][0])
            cuts[-1][2].append(f)
    windows, table, first = [], [], 0
    for offset, length, members in cuts:
        windows.append((offset, length, first, len(members), min(fields[f][0] >> 5 for f in members)))
        first += len(members)
        for f in members:
            position, encoding, at, mask = fields[f]
            word = MASK_NONE if mask is None else MASK_FAR if units[f][2] else mask - offset
            table.append((view.rows[position], view.planes[position] if view.planes is not None else NONE, encoding, at - offset, position, word,
                          mask if units[f][2] else 0))
    return ("masked", pitch, windows, table)


def parse(line):
    if line.startswith("err "):
        code, text = line[4:].split(" ", 1)
        assert code == "-1"
        return ("err", text)
    tok = [int(t) for t in line.split()[1:]]
    records, masks, pitch, n_windows, n_parts = tok[:5]
    assert records == 1 and n_parts == 0
    words = tok[5:]
    if not masks:
        head = 5 * n_windows
        windows = [(words[w] | words[w + 1] << 32, words[w + 2], words[w + 3], words[w + 4]) for w in range(0, head, 5)]
        assert (len(words) - head) % 4 == 0
        return ("unmasked", pitch, windows, [tuple(words[i:i + 4]) for i in range(head, len(words), 4)])
    head = WINDOW_WORDS * n_windows
    windows = [(words[w] | words[w + 1] << 32, words[w + 2], words[w + 3], words[w + 4], words[w + 5]) for w in range(0, head, WINDOW_WORDS)]
    assert (len(words) - head) % FIELD_WORDS == 0
    table = [tuple(words[i:i + 6]) + (words[i + 6] | words[i + 7] << 32,) for i in range(head, len(words), FIELD_WORDS)]
    return ("masked", pitch, windows, table)


def check(tool, view, cases):
    commands = ["noview" if view is None else view.command()] + [masked_command(c[0], c[1], *c[2:]) for c in cases]
    got = [parse(g) for g in tool(commands)]
    for c, g in zip(cases, got):
        assert g == model(view, *c), c
    return got


def assert_units_placed(answer, fields, pitch):
    """every field in exactly one window; a near unit -- element and mask byte -- whole inside it; the far form exactly where the span is above the
    cap; no window above the cap or outside the record"""
    _, _, windows, table = answer
    assert sum(w[3] for w in windows) == len(fields) == len(table)
    by_position = {f[0]: f for f in fields}
    seen = []
    for offset, length, first, n, base in windows:
        assert 0 < length <= CAP and offset + length <= pitch
        assert base == min(t[4] >> 5 for t in table[first:first + n])
        for row, plane, encoding, byte, position, word, far_offset in table[first:first + n]:
            _, enc, at, mask = by_position[position]
            assert (row, encoding, offset + byte) == (position + 100, enc, at) and byte + size_of(enc) <= length
            seen.append(position)
            if mask is None:
                assert word == MASK_NONE and far_offset == 0
                continue
            span = max(at + size_of(enc), mask + 1) - min(at, mask)
            if span <= CAP:
                assert word < length and offset + word == mask and far_offset == 0  # the kernel reads it from the LDS image
            else:
                assert word == MASK_FAR and far_offset == mask                      # ... or with a byte load at this offset of the record
    assert sorted(seen) == sorted(by_position)


VIEW3 = View(130, [5, 6, 9], rows=[105, 106, 109], planes=[2, NONE, 0])
VIEW_ROWS = View(65, list(range(1, 41)), rows=[100 + k for k in range(40)])


def test_strides_and_special_words(tool):
    assert tool(["strides"]) == ["strides %d %d %d %d" % (WINDOW_WORDS, FIELD_WORDS, MASK_NONE, MASK_FAR)]


def test_mask_offset_refusals_and_every_unmasked_refusal_in_its_order(tool):
    good = [(0, U8, 0, 40), (1, BE32, 1, None), (2, U32, 36, 43)]
    cases = [
        (44, good[:2] + [(2, U32, 36, 44)]),                      # mask_offset == pitch
        (44, [(0, U8, 0, 1 << 63)] + good[1:]),
        (44, [(0, U8, 0, (1 << 64) - 2)] + good[1:]),            # just below ACVM_RECORD_NO_MASK: no wrap, refused
        (0, []),                                                  # (n_initial == 3: position 0 never -- the unmasked refusal)
        # every refusal of the unmasked plan, each together with a bad mask offset that must NOT be what is reported
        (44, [(0, U8, 0, 99), (1, BE32, 1, None)]),               # position 2 never
        (44, good + [(1, U8, 43, 99)]),                           # twice
        (44, [(3, U8, 0, 99)] + good),                            # a position >= n_initial
        (44, [(0, 3, 0, 99)] + good[1:]),                         # unknown encoding
        (43, [(0, U8, 0, 99), (1, BE32, 1, None), (2, U32, 40, None)]),   # offset + size > pitch
        (44, good[:2] + [(2, U32, (1 << 64) - 1, 99)]),           # offset + size wraps
        (44, [(0, U8, 0, 99)] + good[1:], 0),                     # null records
        ((1 << 57) // 130 + 1, [(0, U8, 0, 1 << 60)] + good[1:]),  # B * pitch beyond any buffer
    ]
    got = check(tool, VIEW3, cases)
    assert all(g[0] == "err" for g in got)
    texts = [g[1] for g in got]
    assert texts[0] == "field 2 (position 2): mask_offset 44 is not below the pitch 44"
    assert texts[1].startswith("field 0 (position 0): mask_offset %d" % (1 << 63)) and texts[2].startswith("field 0 (position 0): mask_offset")
    assert all("mask_offset" not in t for t in texts[3:])
    # ... and word for word what the unmasked plan says to the same fields without their masks
    lines = tool([VIEW3.command()] + [records_command(c[0], [f[:3] for f in c[1]], *c[2:]) for c in cases[3:]])
    assert [l.split(" ", 2)[2] for l in lines] == texts[3:]
    # the null descriptor, null fields with n_fields > 0, the null batch
    lines = tool([VIEW3.command(), "masked null", masked_command(44, None, null_fields=3), "noview", masked_command(44, good)])
    assert lines == ["err -1 null argument", "err -1 null fields", "err -1 null batch"]


def _random_descriptors(rng, n_cases, with_masks):
    """the seeded descriptors of tests/test_record_plan_on_host.py's kind: nine positions, any encodings, any offsets, short and long records"""
    cases = []
    for _ in range(n_cases):
        pitch = rng.choice([44, 108, 256, 257, 300, 777, 1500, 4096, 70000])
        fl = []
        for position in rng.sample(range(9), 9):
            encoding = rng.choice(ENCODINGS if pitch >= 32 else ENCODINGS[3:])
            offset = rng.randrange(0, pitch - size_of(encoding) + 1)
            mask = None
            if with_masks and rng.random() < 0.7:
                mask = rng.choice([rng.randrange(pitch), max(0, offset - 1), min(pitch - 1, offset + size_of(encoding)), 0, pitch - 1])
            fl.append((position, encoding, offset, mask))
        cases.append((pitch, fl))
    return cases


VIEW9 = View(65, [1, 2, 3, 4, 5, 6, 7, 8, 9], rows=[100, 101, 102, 103, 104, 105, 106, 107, 108])


def test_no_mask_is_the_unmasked_plan_word_for_word(tool):
    rng = random.Random(0x4EC04D)
    cases = _random_descriptors(rng, 40, with_masks=False)
    commands = [VIEW9.command()]
    for pitch, fl in cases:
        commands += [records_command(pitch, [f[:3] for f in fl]), masked_command(pitch, fl), "eq"]
    lines = tool(commands)
    for q in range(len(cases)):
        plain, masked, eq = lines[3 * q:3 * q + 3]
        assert plain.startswith("ok 1 0 ") and masked == plain and eq == "eq 1"  # flags, pitch, windows and every word of lists
    # one mask byte and the plan is another kind: never equal to the unmasked one, equal to itself whatever the pointer
    pitch, fl = cases[0]
    one = [fl[0][:3] + (0,)] + fl[1:]
    lines = tool([VIEW9.command(), records_command(pitch, [f[:3] for f in fl]), masked_command(pitch, one), "eq", masked_command(pitch, one, PTR + 64), "eq"])
    assert lines[1].startswith("ok 1 1 ") and lines[2] == "eq 0" and lines[4] == "eq 1"


def test_random_descriptors_with_masks(tool):
    rng = random.Random(0x4EC04E)
    cases = _random_descriptors(rng, 60, with_masks=True)
    n_far = 0
    for c, g in zip(cases, check(tool, VIEW9, cases)):
        if g[0] == "masked":
            assert_units_placed(g, c[1], c[0])
            n_far += sum(t[5] == MASK_FAR for t in g[3])
    assert n_far > 0


def test_near_and_far_at_the_cap(tool):
    """a field and its mask byte span exactly the cap: near, one window; one byte more: far, and the window holds the element alone"""
    view = View(1, [1, 2], rows=[100, 101])
    near = (600, [(0, U8, 599, None), (1, BE32, 10 + CAP - 32, 10)])
    far = (600, [(0, U8, 599, None), (1, BE32, 10 + CAP - 31, 10)])
    behind = (600, [(0, U8, 599, None), (1, BE32, 40, 40 + CAP - 1)])    # the mask byte BEHIND its element, the last byte of the span
    behind_far = (600, [(0, U8, 599, None), (1, BE32, 40, 40 + CAP)])
    got = check(tool, view, [near, far, behind, behind_far])
    assert got[0][2][0][:2] == (10, CAP) and got[0][3][0][3:] == (CAP - 32, 1, 0, 0)
    assert got[1][3][0][5:] == (MASK_FAR, 10) and got[1][2][0][:2] == (10 + CAP - 31, 32)
    assert got[2][2][0][:2] == (40, CAP) and got[2][3][0][5:] == (CAP - 1, 0)
    assert got[3][3][0][5:] == (MASK_FAR, 40 + CAP) and got[3][2][0][:2] == (40, 32)
    for c, g in zip((near, far, behind, behind_far), got):
        assert_units_placed(g, c[1], c[0])


def test_shared_mask_bytes_the_record_edges_and_a_mask_inside_a_field(tool):
    n = 40
    view = VIEW_ROWS
    # (a) one `valid` byte at record byte 0 for a struct of eight fields, one at pitch - 1 for another eight, the rest unmasked; short record
    pitch = 255
    fields = [(k, U8, 1 + k, 0) for k in range(8)] + [(8 + k, U16, 20 + 2 * k, pitch - 1) for k in range(8)] + [(16 + k, U32, 60 + 4 * k, None) for k in range(24)]
    a = check(tool, view, [(pitch, fields)])[0]
    assert a[2] == [(0, pitch, 0, n, 0)]
    assert [t[5] for t in a[3][:16]] == [0] * 8 + [pitch - 1] * 8 and all(t[5] == MASK_NONE for t in a[3][16:])
    assert_units_placed(a, fields, pitch)
    # (b) the same in a long record: the head byte is near for the first fields and far for those beyond a window's reach; pitch - 1 likewise
    pitch = 2000
    fields = [(k, BE32, 1 + 48 * k, 0) for k in range(20)] + [(20 + k, U64, 1000 + 48 * k, pitch - 1) for k in range(20)]
    b = check(tool, view, [(pitch, fields)])[0]
    assert_units_placed(b, fields, pitch)
    words = {t[4]: t[5] for t in b[3]}
    assert words[0] == 0 and words[4] == 0 and words[5] == MASK_FAR and words[19] == MASK_FAR  # 1 + 48 * 4 + 32 = 225 <= 256 < 1 + 48 * 5 + 32
    assert words[39] != MASK_FAR and words[20] == MASK_FAR
    assert len(b[2]) >= 3 and {w[4] for w in b[2]} == {0, 1} | {w[4] for w in b[2]}  # windows of positions >= 32 begin at missing word 1
    # (c) a mask byte inside another field's bytes, and inside its own field's
    pitch = 300
    fields = [(0, BE32, 0, 40), (1, LE32, 33, 10), (2, U32, 100, 101)] + [(k, U8, 200 + k, None) for k in range(3, n)]
    c = check(tool, view, [(pitch, fields)])[0]
    assert_units_placed(c, fields, pitch)
    assert {t[4]: t[5] for t in c[3]}[2] == 101 - c[2][0][0]
