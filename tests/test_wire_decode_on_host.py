"""The wire-import kernels' arithmetic without a device: acvm_amd/csrc/wire_decode.hpp compiled for the host (tools/wire_decode_host_test.hip).
The hex decoding is judged by bytes.fromhex, the value by int, the CRC accumulated entry by entry by zlib.crc32, the framing offsets by
tests/wire_ref.py's member around its body; then the argument checks that need no GPU and the Python view."""
import ctypes as C
import os
import random
import struct
import subprocess
import zlib

import pytest

import wire_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
HEX = b"0123456789abcdefABCDEF"
BINCODE, GZIP = 0, 1


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wire_decode") / "wire_decode_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tools", "wire_decode_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _limbs(tokens):
    return sum(int(t, 16) << (32 * k) for k, t in enumerate(tokens))


def test_every_byte_value_at_every_place_of_a_dword(tool):
    """all 256 byte values: the 22 digits of either case give their nibble, the other 234 are flagged -- in each of the four bytes, the other
    three holding digits, and the flag names exactly that byte"""
    cases = [(place, byte) for place in range(4) for byte in range(256)]
    others = b"7aF0"
    commands = []
    for place, byte in cases:
        chars = bytearray(others)
        chars[place] = byte
        commands.append("unhex4 %d" % struct.unpack("<I", bytes(chars))[0])
    n_digits = 0
    for (place, byte), got in zip(cases, tool(commands)):
        nibbles, bad = (int(x) for x in got.split())
        want = [int(chr(c), 16) for c in others]
        if byte in HEX:
            n_digits += 1
            want[place] = int(chr(byte), 16)
            assert bad == 0 and list(struct.pack("<I", nibbles)) == want, (place, byte)
        else:
            assert bad == 0x80 << (8 * place), (place, byte, bad)
            got_nibbles = list(struct.pack("<I", nibbles))
            assert [got_nibbles[k] for k in range(4) if k != place] == [want[k] for k in range(4) if k != place], (place, byte)
    assert n_digits == 4 * 22


def test_each_of_the_64_positions(tool):
    """a digit of either case and a bad character at each of the 64 places of a string: the bytes are bytes.fromhex's, the flag falls"""
    rng = random.Random(0x31BE2001)
    base = bytes(rng.choice(HEX) for _ in range(64))
    strings = [base]
    for at in range(64):
        for c in (b"f", b"F", b"0", b"9", b"a", b"A"):
            strings.append(base[:at] + c + base[at + 1:])
    for s, got in zip(strings, tool(["unhex " + s.hex() for s in strings])):
        valid, raw = got.split()
        assert valid == "1" and bytes.fromhex(raw) == bytes.fromhex(s.decode()), s
    bad = [base[:at] + c + base[at + 1:] for at in range(64) for c in (b"g", b"G", b"x", b"/", b":", b"@", b"`", b" ", b"\x00", b"\xb1", b"\xe6")]
    for s, got in zip(bad, tool(["unhex " + s.hex() for s in bad])):
        assert got.split()[0] == "0", s
    # a 0x prefix is a finding, not a 31-byte value
    assert tool(["unhex " + (b"0x" + base[2:]).hex()])[0].split()[0] == "0"


def test_value_row_and_plane_are_ints(tool):
    """the 64 characters to the element import_decode makes of them: reduced mod p like from_be_bytes_reduce, a string >= p included"""
    rng = random.Random(0x31BE2002)
    values = [0, 1, 255, 256, P - 1, P, P + 1, 2 * P, 5 * P, (1 << 256) - 1, (1 << 255), 0xa9, (1 << 29) - 1, 1 << 29] + [rng.randrange(1 << 256) for _ in range(100)]
    strings = []
    for v in values:
        s = b"%064x" % v
        strings += [s, s.upper(), bytes(rng.choice((c, ord(chr(c).upper()))) for c in s)]
    for k, got in enumerate(tool(["value " + s.hex() for s in strings])):
        tok = got.split()
        v = values[k // 3] % P
        assert tok[0] == "1"
        assert _limbs(tok[1:9]) == v, strings[k]
        assert _limbs(tok[9:17]) == v * (1 << 261) % P, strings[k]
        assert int(tok[17], 16) == (v & 0x1FFFFFFF) | (0x80000000 if v < 256 else 0), strings[k]


def test_the_count_word(tool):
    n_initial = 40
    cases = []
    for c in (BINCODE, GZIP):
        bound = wire_ref.bound(c, n_initial)
        for pitch in (16, 32, bound - 16, bound, bound + 48):
            for n in (0, 1, 39, 40, 41, 1 << 31, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - 1):
                for have, length in ((0, 0), (1, wire_ref.length(c, min(n, 1 << 40))), (1, wire_ref.length(c, min(n, 1 << 40)) + 1), (1, 0)):
                    cases.append((c, pitch, n, have, length))
    commands = ["count %d %d %d %d %d %d" % (c, pitch, n_initial, n, have, length) for c, pitch, n, have, length in cases]
    for (c, pitch, n, have, length), got in zip(cases, tool(commands)):
        readable, ok = (int(x) for x in got.split())
        assert readable == (wire_ref.body_offset(c, 0) + 8 <= pitch)
        want = n <= n_initial and wire_ref.length(c, n) <= pitch and (not have or length == wire_ref.length(c, n))
        assert ok == want, (c, pitch, n, have, length)
        assert not ok or readable


def _body(n, rng):
    return wire_ref.body({3 * w + 1: rng.randrange(P) for w in range(n)})


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 100, 862, 863, 870])
def test_crc_entry_by_entry_is_zlibs(tool, n):
    body = _body(n, random.Random(0x31BE2003 + n))
    assert int(tool(["crc " + body.hex()])[0]) == zlib.crc32(body)
    # uppercase characters are other bytes with another CRC: the reader takes the bytes as they are
    upper = body[:8] + b"".join(body[8 + 76 * r:8 + 76 * r + 12] + body[8 + 76 * r + 12:8 + 76 * (r + 1)].upper() for r in range(n))
    assert int(tool(["crc " + upper.hex()])[0]) == zlib.crc32(upper)


def test_framing_offsets_of_a_body_straddling_a_block_joint(tool):
    """870 entries are 66 128 body bytes, two stored blocks: entry 862 spans the joint at 65 532. The joint, the trailer and ISIZE lie where
    wire_ref's member has them."""
    for n in (0, 1, 862, 863, 870, 1725):
        body = _body(n, random.Random(0x31BE2004))
        member = wire_ref.member(body)
        tok = [int(x) for x in tool(["frame %d" % n])[0].split()]
        trailer, isize, joints = tok[0], tok[1], tok[2:]
        assert trailer == len(member) - 8 and struct.unpack("<II", member[trailer:]) == (zlib.crc32(body), isize)
        assert len(joints) == wire_ref.n_blocks(len(body)) - 1
        for block, at in enumerate(joints, 1):
            assert member[at:at + 15] == wire_ref.EMPTY_BLOCK * 3 and at + 20 == wire_ref.body_offset(GZIP, block * wire_ref.BLOCK)
            assert member[at + 20:at + 24] == body[block * wire_ref.BLOCK:block * wire_ref.BLOCK + 4]
    assert wire_ref.n_blocks(8 + 76 * 870) == 2 and 8 + 76 * 862 == 65520 < wire_ref.BLOCK < 8 + 76 * 863


def test_the_finding_key_orders_instance_class_rank(tool):
    triples = [(0, 1, 0), (0, 2, 0), (0, 2, 39), (0, 7, 0), (1, 1, 0), (64, 5, 8), (64, 6, 0), (65, 2, 3), (130000, 7, 39), ((1 << 17) - 1, 3, 63)]
    lines = tool(["key %d %d %d 6" % t for t in triples])
    keys = []
    for t, got in zip(triples, lines):
        key, j, cls, rank = (int(x) for x in got.split())
        assert (j, cls, rank) == t and key != 0
        keys.append(key)
    assert keys == sorted(keys, reverse=True)  # atomicMax keeps the smallest triple
    # the widest fields the plan admits: 28 + 3 + 32 = 63 bits
    key, j, cls, rank = (int(x) for x in tool(["key %d 7 %d 32" % ((1 << 28) - 1, (1 << 32) - 1)])[0].split())
    assert (j, cls, rank) == ((1 << 28) - 1, 7, (1 << 32) - 1) and key != 0


def test_the_key_lookup(tool):
    rng = random.Random(0x31BE2005)
    for ids in ([], [5], [1, 2, 3], [9, 4, 7, 1], rng.sample(range(5000), 870)):
        probes = sorted(set(ids[:20] + [0, 1, 6, 4999, 5000, (1 << 32) - 1] + [w + 1 for w in ids[:20]]))
        lines = tool(["position %d %d %s" % (k, len(ids), " ".join(map(str, ids))) for k in probes])
        for k, got in zip(probes, lines):
            assert int(got) == (ids.index(k) if k in ids else 0xFFFFFFFF), (ids[:8], k)


def test_argument_checks_without_a_device():
    import acvm_amd
    L = acvm_amd.lib()
    for name in ("acvm_batch_import_device_wire", "acvm_batch_set_initial_witness_maps_wire"):
        assert name in acvm_amd.ABI_SYMBOLS
    desc = acvm_amd.WireInDesc(container=acvm_amd.WIRE_GZIP_STORED, pitch=64)
    assert L.acvm_batch_import_device_wire(None, C.byref(desc), 16, None) == -1 and b"null batch" in L.acvm_last_error()
    lengths = (C.c_uint64 * 1)(8)
    assert L.acvm_batch_set_initial_witness_maps_wire(None, bytes(8), 8, lengths) == -1 and b"null batch" in L.acvm_last_error()
    assert L.acvm_abi_version() == 6


def test_python_view():
    import inspect
    import acvm_amd
    # acvm_wire_in_desc_t as the C compiler lays it out
    assert C.sizeof(acvm_amd.WireInDesc) == 16 and acvm_amd.WireInDesc.pitch.offset == 8
    assert list(inspect.signature(acvm_amd.Batch.import_device_wire).parameters)[1:] == ["d_ptr", "container", "pitch", "d_lengths"]
    assert list(inspect.signature(acvm_amd.Batch.set_initial_witness_maps_wire).parameters)[1:] == ["maps"]
