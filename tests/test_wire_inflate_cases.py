"""The case lists of the gzip import (tests/wire_inflate_cases.py) and their model (tests/wire_inflate_ref.py), pinned without a device: the model
accepts a row exactly when zlib's own gzip reader does and gives the same bytes; every branch and every class-and-cause is reached at least
twice; each of the model's six wrong variants is caught by the rows meant for it."""
import struct
import zlib

import pytest

import wire_in_cases as wc
import wire_inflate_cases as cases
import wire_inflate_ref as ref
import wire_ref

BRANCHES = ("block.stored", "block.fixed", "block.dynamic", "blocks.many", "head.fextra", "head.fname", "head.fcomment", "head.fhcrc", "repeat.16", "repeat.17",
            "repeat.18", "repeat.cross", "copy.overlap", "copy.far", "dist.32768", "dist.all_written", "len.258", "code.15bit", "dist.onecode", "dist.none",
            "lit.onecode", "codes.hlit29", "codes.hdist29", "stored.empty", "stored.some", "stored.full", "trailing")
CAUSES = {ref.HEAD: ("head.magic", "head.method", "head.reserved", "head.fhcrc"), ref.BLOCK: ("block.type3",), ref.STORED: ("stored.nlen",),
          ref.CODES: ("codes.hlit", "codes.hdist", "codes.clc_over", "codes.clc_incomplete", "codes.repeat_first", "codes.repeat_past", "codes.no_eob", "codes.lit_over",
                      "codes.lit_incomplete", "codes.dist_over", "codes.dist_incomplete"),
          ref.SYMBOL: ("symbol.nocode_lit", "symbol.nocode_dist", "symbol.lit286", "symbol.dist30"), ref.DISTANCE: ("distance",),
          ref.INPUT: ("input.head", "input.block", "input.trailer"), ref.OUTPUT: ("output",), ref.CRC: ("crc",), ref.ISIZE: ("isize",)}


def _cap(c):
    return cases.CAP if c.cap is None else c.cap


def _judged(c):
    return cases.judged(c.row, _cap(c))


def test_names_are_unique_and_caps_fit_the_probe():
    names = [c.name for c in cases.everything()]
    assert len(set(names)) == len(names)
    assert all(_cap(c) % 4 == 0 for c in cases.everything())


def test_the_model_accepts_exactly_what_zlib_accepts():
    """every row of the three lists, and 4 000 mutations: accepted by both with the same bytes, or refused by both. (A row that is about the
    bound is judged without it here: the bound is this project's, not zlib's.)"""
    rows = [c.row for c in cases.everything()] + cases.mutations(4000, seed=0x1F8B0001)
    n_accepted = 0
    for row in rows:
        m = ref.inflate(row) if len(row) > 400 else cases.judged(row, None)
        accepted, out = ref.zlib_accepts(row)
        assert accepted == (m.cls == 0), (row[:40].hex(), m.cls, m.cause)
        if accepted:
            n_accepted += 1
            assert out == m.out and m.crc == zlib.crc32(out)
    assert 300 < n_accepted < len(rows) - 2000  # the mutations are mostly refused, and not all of them


def test_list_a_and_b_pass_and_list_c_names_its_class():
    for c in cases.list_a() + cases.list_b():
        m = _judged(c)
        assert m.cls == 0 and m.cause is None, (c.name, m.cause)
    for c in cases.list_c():
        m = _judged(c)
        word = c.name.split()[1]
        want = {"head": ref.HEAD, "block": ref.BLOCK, "stored": ref.STORED, "codes": ref.CODES, "symbol": ref.SYMBOL, "distance": ref.DISTANCE, "input": ref.INPUT,
                "output": ref.OUTPUT, "crc": ref.CRC, "isize": ref.ISIZE}[word]
        if "passes" in c.name or "exactly the cap" in c.name or "is the same" in c.name:
            assert m.cls == 0, c.name
        else:
            assert m.cls == want and m.cause in CAUSES[want], (c.name, m.cls, m.cause)
    # list A's bodies are maps: what the rows hold is what their names say
    for c in cases.list_a():
        if c.name.startswith("A 440"):
            assert len(_judged(c).out) == 8 + 76 * 440
    member, witness_map = cases.pinned()
    assert len(member) == 106 and len(witness_map) == 6 and ref.inflate(member).out == wire_ref.body(witness_map)


def test_every_branch_and_every_cause_is_reached_at_least_twice():
    labels, causes = {}, {}
    for c in cases.everything():
        m = _judged(c)
        for l in m.labels:
            labels[l] = labels.get(l, 0) + 1
        if m.cls:
            causes[(m.cls, m.cause)] = causes.get((m.cls, m.cause), 0) + 1
    for b in BRANCHES:
        assert labels.get(b, 0) >= 2, b
    for cls, names in CAUSES.items():
        for cause in names:
            assert causes.get((cls, cause), 0) >= 2, cause
    assert set(causes) == {(cls, cause) for cls, names in CAUSES.items() for cause in names}  # and nothing the table does not know


def test_the_440_entry_rows_hold_a_distance_above_16384():
    far = [c for c in cases.list_a() if c.name.startswith("A 440 repeat250") and "copy.far" in _judged(c).labels]
    assert len(far) >= 2, [c.name for c in far]
    assert any("level9" in c.name for c in far)


def test_the_termination_tripwire():
    """a slot of empty stored blocks to its very end: class 7, after (pitch - 10) / 5 block headers and not one output byte"""
    for c in cases.list_c():
        if "empty stored blocks" in c.name:
            m = _judged(c)
            pitch = len(c.row)
            assert (m.cls, len(m.out)) == (ref.INPUT, 0) and m.block in ((pitch - 10) // 5, (pitch - 10) // 5 + 1), (c.name, m.block)
    # a truncation at every byte of one small member
    cut = [c for c in cases.list_c() if c.name.startswith("C input truncated at ")]
    total = int(cut[0].name.split()[-1])
    assert sorted(len(c.row) for c in cut) == list(range(1, total))


MEANT_FOR = {"repeat_may_not_cross": "B a ", "distance_limit_off_by_one": "B distance", "one_bit_incomplete_refused": "B a one-code", "isize_before_crc": "C crc",
             "fhcrc_skipped": "C head FHCRC", "stored_len_big_endian": "B "}  # (a LEN of 65 535 or 0 reads the same either way: the other stored rows tell)


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_each_wrong_variant_is_caught_by_the_rows_meant_for_it(variant):
    meant = [c for c in cases.everything() if c.name.startswith(MEANT_FOR[variant])]
    assert len(meant) >= 2
    caught = []
    for c in meant:
        right, wrong = _judged(c), ref.inflate(c.row, _cap(c), variant)
        if (right.cls, right.block, right.out) != (wrong.cls, wrong.block, wrong.out):
            caught.append(c.name)
    assert len(caught) >= 2, (variant, caught)


def test_list_d_inflates_cleanly_to_bodies_the_body_import_refuses():
    ids = list(range(1, 13))
    values = [(0x1234567890 << (8 * k)) + k for k in range(12)]
    rows = cases.list_d(ids, values, 8)
    assert {b.cls for b, _ in rows} == {1, 2, 3, 4, 5}
    for b, row in rows:
        m = ref.inflate(row, 8 + 76 * len(ids) if b.cls != 1 else None)
        assert m.cls == 0 and m.out == b.row, b
        slot = m.out + bytes(-len(m.out) % 16)
        assert (b.cls, b.rank) in wc.findings(slot + bytes(16), wire_ref.BINCODE, ids, len(m.out)), b


def test_the_token_writer_against_zlibs_own_output():
    """the writer's fixed block of literals is zlib's Z_FIXED stream of a short text, bit for bit"""
    text = b"gzip"
    w = cases.Bits()
    cases.fixed(w, list(text), 1)
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    assert w.bytes() == c.compress(text) + c.flush()
    assert struct.unpack("<I", cases.member(w.bytes(), text)[-8:-4])[0] == zlib.crc32(text)
