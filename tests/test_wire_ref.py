"""tests/wire_ref.py -- the expected bytes of the batch-wide wire format -- pinned against the library's own WitnessMap codec (which the oracle
pins) and Python's inflaters: the body is the inflated compress_witness, a member reads back through decompress_witness, gzip.decompress and
zlib, the lengths follow the formula, and a flipped byte does not pass."""
import gzip
import random
import zlib

import pytest

import acvm_amd
import wire_ref

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SIZES = [0, 1, 862, 863, 1724, 1725]  # 8 + 76 * 862 = 65 520 fits one stored block, 863 needs two, 1 725 three


def _map(n, seed=0):
    rng = random.Random(0x31BE2000 + n + seed)
    ws = sorted(rng.sample(range(0, 3 * n + 5), n))
    edge = [0, 1, P - 1, 15, 16, 0xabcdef, (1 << 253) + 5]
    return {w: edge[k] if k < len(edge) else rng.randrange(P) for k, w in enumerate(ws)}


@pytest.mark.parametrize("n", SIZES)
def test_body_is_the_inflated_compress_witness(n):
    m = _map(n)
    assert wire_ref.body(m) == gzip.decompress(acvm_amd.compress_witness(m))
    assert len(wire_ref.body(m)) == 8 + 76 * n


@pytest.mark.parametrize("n", SIZES)
def test_member_reads_back(n):
    m = _map(n)
    member = wire_ref.encode(m, wire_ref.GZIP_STORED)
    assert gzip.decompress(member) == wire_ref.body(m)
    assert zlib.decompress(member, 31) == wire_ref.body(m)
    assert acvm_amd.decompress_witness(member) == m
    assert acvm_amd.decompress_witness(wire_ref.encode(m, wire_ref.BINCODE)) == m
    assert member[:11] == bytes.fromhex("1f8b08080000000000ff00")


@pytest.mark.parametrize("n", SIZES)
def test_lengths_formula(n):
    m = _map(n)
    L = 8 + 76 * n
    assert len(wire_ref.encode(m, wire_ref.BINCODE)) == wire_ref.length(wire_ref.BINCODE, n) == L
    assert len(wire_ref.encode(m, wire_ref.GZIP_STORED)) == wire_ref.length(wire_ref.GZIP_STORED, n) == 16 + L + 20 * (-(-L // 65532) - 1) + 8
    assert wire_ref.bound(wire_ref.GZIP_STORED, n) % 16 == 0 and 0 <= wire_ref.bound(wire_ref.GZIP_STORED, n) - wire_ref.length(wire_ref.GZIP_STORED, n) < 16
    assert wire_ref.length(wire_ref.GZIP_STORED, n) % 4 == 0
    # the first body byte at 16, every block's data at a multiple of 4
    assert all(wire_ref.body_offset(wire_ref.GZIP_STORED, b * 65532) % 4 == 0 for b in range(4)) and wire_ref.body_offset(wire_ref.GZIP_STORED, 0) == 16


def test_block_structure():
    m = _map(1725)
    member = wire_ref.encode(m, wire_ref.GZIP_STORED)
    body = wire_ref.body(m)
    at = 11
    for k in range(3):
        if k:
            assert member[at:at + 15] == bytes.fromhex("000000ffff") * 3
            at += 15
        final, length, nlength = member[at], int.from_bytes(member[at + 1:at + 3], "little"), int.from_bytes(member[at + 3:at + 5], "little")
        assert final == (1 if k == 2 else 0) and length == min(65532, len(body) - 65532 * k) and nlength == length ^ 0xFFFF
        assert member[at + 5:at + 5 + length] == body[65532 * k:65532 * k + length]
        at += 5 + length
    assert member[at:] == zlib.crc32(body).to_bytes(4, "little") + len(body).to_bytes(4, "little")


def test_slots_at_a_pitch():
    maps = [_map(3), {}, _map(1)]
    pitch = wire_ref.bound(wire_ref.GZIP_STORED, 3) + 48
    buf, lengths = wire_ref.slots(maps, wire_ref.GZIP_STORED, pitch, tail=16)
    assert len(buf) == 3 * pitch + 16 and lengths == [wire_ref.length(wire_ref.GZIP_STORED, len(m)) for m in maps]
    for i, m in enumerate(maps):
        assert buf[i * pitch:i * pitch + lengths[i]] == wire_ref.encode(m, wire_ref.GZIP_STORED)
        assert set(buf[i * pitch + lengths[i]:(i + 1) * pitch]) == {0xA5}
    assert set(buf[3 * pitch:]) == {0xA5}
    assert wire_ref.restrict({1: 5, 4: 6, 9: 7}, [0, 4, 9, 50]) == {4: 6, 9: 7}


@pytest.mark.parametrize("n", [1, 863])
def test_a_flipped_byte_does_not_pass(n):
    """the test bites: the inflater checks the CRC"""
    member = bytearray(wire_ref.encode(_map(n), wire_ref.GZIP_STORED))
    for at in (16 + 8 + 20, len(member) - 9, len(member) - 8):  # a hex character, the last body byte, the CRC itself
        bad = bytearray(member)
        bad[at] ^= 1
        with pytest.raises(Exception):
            gzip.decompress(bytes(bad))
        with pytest.raises(zlib.error):
            zlib.decompress(bytes(bad), 31)
