"""tests/wire_deflate_ref.py -- the Python restatement of ACVM_WIRE_GZIP_DEFLATE -- against zlib: every fixture's member inflates through
zlib's gzip reader (which checks CRC-32 and ISIZE) to exactly tests/wire_ref.py's body, ends where the member ends, and is no longer than the
bound; six wrong variants of the model are each caught; and the members are about as small as zlib's level 1 makes them."""
import functools
import random
import zlib

import pytest

import wire_deflate_cases as cases
import wire_deflate_ref as ref

P = cases.P


@functools.lru_cache(maxsize=None)
def big_fixtures():
    """maps of 1 000 entries and more: what a circuit's witnesses look like"""
    rng = random.Random(0xDEF1A7E1)
    widths = [1, 8, 32, 64, 254]
    return {
        "random": {w: rng.randrange(P) for w in range(1000)},
        "bits": {w: rng.randrange(2) for w in range(1000)},
        "bytes": {w: rng.randrange(256) for w in range(1000)},
        "u32": {w: rng.randrange(1 << 32) for w in range(1000)},
        "u64 keys 7k+3": {7 * w + 3: rng.randrange(1 << 64) for w in range(1000)},
        "mixed": {w: rng.randrange(1 << rng.choice(widths)) % P for w in range(3000)},
    }


@functools.lru_cache(maxsize=None)
def fixtures():
    out = dict(big_fixtures())
    out.update({"case row %d" % j: m for j, m in enumerate(cases.rows())})
    out.update({"keyed row %d" % j: m for j, m in enumerate(cases.keyed_rows())})
    out.update({"count row %d" % len(m): m for m in cases.count_rows()})
    out["empty"] = {}
    return out


def test_every_member_inflates_to_the_body_and_respects_the_bound():
    for name, m in fixtures().items():
        body = ref.body(m)
        member = ref.member(body)
        d = zlib.decompressobj(31)
        assert d.decompress(member) == body and d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", name
        assert len(member) <= ref.bound(ref.GZIP_DEFLATE, len(m)) and ref.bound(ref.GZIP_DEFLATE, len(m)) % 16 == 0, name
        block, bits = ref.MODEL.block(body)
        assert bits <= ref.bound_bits(len(m)) and len(member) == 11 + (bits + 7) // 8 + 8, name
        with pytest.raises((zlib.error, AssertionError)):
            ref.inflate(member[:-1])  # and not a byte less
    assert ref.inflate(ref.encode({})) == bytes(8) and len(ref.encode({})) == 63


def test_the_format_is_the_one_the_header_comment_states():
    lengths = ref.litlen_lengths()
    assert [lengths[c] for c in b"0123456789abcdef"] == [5] * 16 and lengths[257:] == [7] * 21 and len(lengths) == 278
    others = [lengths[s] for s in range(257) if s not in list(b"0123456789abcdef")]
    assert others == [9] * 103 + [10] * 138
    assert 16 * 2 ** 10 + 21 * 2 ** 8 + 103 * 2 ** 6 + 138 * 2 ** 5 == 2 ** 15  # Kraft: 16/32 + 21/128 + 103/512 + 138/1024 = 1
    assert ref.dist_lengths() == [1] + [0] * 11 + [1]
    assert [ref.length_symbol(n)[0] for n in (3, 10, 11, 12, 66, 67, 76, 82)] == [257, 264, 265, 265, 276, 277, 277, 277]
    assert ref.bound(ref.GZIP_DEFLATE, 1000) < 0.73 * ref.bound(ref.wire_ref.GZIP_STORED, 1000)
    # the match-versus-literals inequality the bound rests on: a match never costs more than its literals at 5 bits each
    for n in range(3, 77):
        for distance in (1, 76):
            b = ref.Bits()
            ref.MODEL.token_bits(b, ("match", n, distance))
            assert b.n <= 5 * n and b.n <= 17


WRONG = {
    "a tie taken the other way": dict(tie_to_distance_1=True),
    "matches of length 2": dict(min_match=2),
    "distance 76 at rank 0": dict(distance_76_at_rank_0=True),
    "a wrong extra-bit count at one length base": dict(wrong_extra_at=19),
    "a header one bit short": dict(header_short=True),
    "ISIZE off by one": dict(isize_off=1),
}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_variants_are_caught(name):
    """by a fixture whose member zlib rejects or inflates to something else -- or, for a variant that is still a valid stream of the same
    body (the tie), whose bytes are not the format's"""
    wrong = ref.Model(**WRONG[name])
    caught = []
    for fixture, m in fixtures().items():
        body = ref.body(m)
        member = wrong.member(body)
        try:
            ok = ref.inflate(member) == body
        except (zlib.error, AssertionError):
            ok = False
        if not ok or member != ref.member(body):
            caught.append((fixture, ok))
            if not ok or name == "a tie taken the other way":
                break
    assert caught, name
    if name != "a tie taken the other way":
        assert any(not ok for _, ok in caught), name  # zlib itself objects


@pytest.mark.parametrize("name", ["random", "bits", "bytes", "u32", "mixed"])
def test_size_against_zlib_level_1(name):
    m = big_fixtures()[name]
    assert len(m) >= 1000
    body = ref.body(m)
    ours, theirs = len(ref.member(body)), len(zlib.compress(body, 1))
    print("%s: body %d, the format %d, zlib level 1 %d, ratio %.3f" % (name, len(body), ours, theirs, ours / theirs))
    assert ours <= 1.5 * theirs
