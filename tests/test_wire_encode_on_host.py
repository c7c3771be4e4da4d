"""The wire-format kernels' arithmetic without a device: acvm_amd/csrc/wire_encode.hpp compiled for the host (tools/wire_encode_host_test.hip).
The hex expansion is judged by binascii.hexlify, the entry and the framing by tests/wire_ref.py, the CRC pieces -- the raw CRC, the product
mod P, the powers of x and the combination rule -- by zlib.crc32; then the argument checks that need no GPU and the Python view."""
import binascii
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
EDGES = [0, 1, 9, 10, 15, 16, 0xa9, 0x9a, P - 1, P // 2, (1 << 253) + 0xabcdef, 0x0123456789abcdef, int("f" * 62, 16), int("9" * 63, 16) % P, int("a0" * 31, 16)]


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wire_encode") / "wire_encode_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tools", "wire_encode_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _raw(data):
    """the register after `data` from a zero register, no final xor: zlib's crc with both xors taken off"""
    return zlib.crc32(data) ^ zlib.crc32(bytes(len(data)))


def _values(rng, n):
    return [rng.choice(EDGES) if rng.random() < 0.3 else rng.randrange(P) for _ in range(n)]


def test_constants(tool):
    entry, block, window, pitch, rows = (int(x) for x in tool(["const"])[0].split())
    assert (entry, block) == (wire_ref.ENTRY, wire_ref.BLOCK) and block % 4 == 0 and rows == 64
    assert pitch == window * entry // 4 + 1 and pitch % 2 == 1  # lane = row: 64 rows at an odd pitch fall on 64 banks
    assert 64 * pitch * 4 <= 48 * 1024


def test_hex_is_hexlify(tool):
    rng = random.Random(0x31BE0001)
    values = EDGES + [rng.randrange(1 << 256) for _ in range(200)]  # (the expansion is byte arithmetic: any 32 bytes)
    raws = [v.to_bytes(32, "big") for v in values]
    for raw, got in zip(raws, tool(["hex " + r.hex() for r in raws])):
        assert bytes.fromhex(got) == binascii.hexlify(raw)


def test_entry_is_the_references(tool):
    rng = random.Random(0x31BE0002)
    cases = [(w, v) for w in (0, 1, 255, 256, 10016, (1 << 32) - 1) for v in _values(rng, 4)]
    for (w, v), got in zip(cases, tool(["entry %d %s" % (w, v.to_bytes(32, "big").hex()) for w, v in cases])):
        assert bytes.fromhex(got) == wire_ref.body({w: v})[8:]
        assert len(got) == 2 * wire_ref.ENTRY


def test_raw_crc_product_and_powers(tool):
    rng = random.Random(0x31BE0003)
    datas = [bytes(rng.randrange(256) for _ in range(n)) for n in (4, 8, 12, 76, 76, 152, 1024)] + [bytes(8), struct.pack("<Q", 863)]
    for d, got in zip(datas, tool(["raw " + d.hex() for d in datas])):
        assert int(got) == _raw(d)
    for d, got in zip(datas, tool(["raw4 " + d.hex() for d in datas])):  # sliced by 4: what the kernel runs
        assert int(got) == _raw(d)
    # x^(8 m) * c is c advanced over m zero bytes: raw(d + zeros) = raw(d) * x^(8 m)
    cases = [(d, m) for d in datas[:5] for m in (0, 1, 3, 76, 76 * 862, 65532, (1 << 32) + 5)]
    pows = [int(x) for x in tool(["xpow %d" % m for _, m in cases])]
    small = [(d, m, p) for (d, m), p in zip(cases, pows) if m <= 1 << 20]
    for (d, m, p), got in zip(small, tool(["mul %d %d" % (p, _raw(d)) for d, m, p in small])):
        assert int(got) == _raw(d + bytes(m)), (len(d), m)
    # the product is commutative, x^0 is its unit, powers add
    one = int(tool(["xpow 0"])[0])
    assert one == 0x80000000
    a, b = _raw(datas[3]), _raw(datas[4])
    ab, ba, a1 = (int(x) for x in tool(["mul %d %d" % (a, b), "mul %d %d" % (b, a), "mul %d %d" % (a, one)]))
    assert ab == ba and a1 == a
    big = dict(((m, p) for (_, m), p in zip(cases, pows)))
    assert int(tool(["mul %d %d" % (big[76], big[3])])[0]) == int(tool(["xpow 79"])[0])
    assert int(tool(["mul %d %d" % (big[(1 << 32) + 5], big[76])])[0]) == int(tool(["xpow %d" % ((1 << 32) + 81)])[0])


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 100, 863])
def test_combination_rule_is_zlib_crc32(tool, n):
    rng = random.Random(0x31BE0004 + n)
    ws = sorted(rng.sample(range(0, 4 * n + 10), n))
    m = dict(zip(ws, _values(rng, n)))
    got = int(tool(["crc %d " % n + " ".join("%d %s" % (w, m[w].to_bytes(32, "big").hex()) for w in ws)])[0])
    assert got == zlib.crc32(wire_ref.body(m))


def test_lengths_offsets_and_framing(tool):
    ns = [0, 1, 2, 861, 862, 863, 864, 1724, 1725, 5000, 10017, 1 << 26]
    commands = ["length %d %d" % (c, n) for c in (0, 1) for n in ns]
    for cmd, got in zip(commands, tool(commands)):
        _, c, n = cmd.split()
        assert int(got) == wire_ref.length(int(c), int(n)), cmd
    ks = [0, 7, 8, 65531, 65532, 65533, 131063, 131064, 3 * 65532 - 1, 3 * 65532, 1 << 33]
    commands = ["offset %d %d" % (c, k) for c in (0, 1) for k in ks]
    for cmd, got in zip(commands, tool(commands)):
        _, c, k = cmd.split()
        assert int(got) == wire_ref.body_offset(int(c), int(k)), cmd
    # the head and the joints are the bytes of wire_ref's member around the body's blocks
    for n in (0, 1, 862, 863, 1724, 1725):
        body = wire_ref.body({w: (w * 0x9e3779b97f4a7c15) % P for w in range(n)})
        member = wire_ref.member(body)
        L = len(body)
        assert bytes.fromhex(tool(["head %d" % L])[0]) == member[:16]
        for block in range(1, wire_ref.n_blocks(L)):
            at = wire_ref.body_offset(1, block * wire_ref.BLOCK)
            assert bytes.fromhex(tool(["joint %d %d" % (L, block)])[0]) == member[at - 20:at]
            assert member[at:at + 4] == body[block * wire_ref.BLOCK:block * wire_ref.BLOCK + 4]


def test_argument_checks_without_a_device():
    import acvm_amd
    L = acvm_amd.lib()
    for name in ("acvm_batch_wire_bound", "acvm_batch_witness_maps_wire_device", "acvm_batch_witness_maps_wire"):
        assert name in acvm_amd.ABI_SYMBOLS
    desc, _keep = acvm_amd.wire_desc(acvm_amd.WIRE_GZIP_STORED, 0, 4)
    assert L.acvm_batch_witness_maps_wire_device(None, C.byref(desc), None, 16, None) == -1 and b"null batch" in L.acvm_last_error()
    assert L.acvm_batch_witness_maps_wire_device(None, None, None, 16, None) == -1 and b"null argument" in L.acvm_last_error()
    assert L.acvm_batch_witness_maps_wire(None, C.byref(desc), None, None) == -1
    assert L.acvm_batch_wire_bound(None, C.byref(desc)) == -1 and b"null batch" in L.acvm_last_error()
    assert L.acvm_abi_version() == 6


def test_python_view():
    import inspect
    import acvm_amd
    # acvm_wire_desc_t as the C compiler lays it out
    assert C.sizeof(acvm_amd.WireDesc) == 40 and acvm_amd.WireDesc.witnesses.offset == 16 and acvm_amd.WireDesc.n_witnesses.offset == 24 and acvm_amd.WireDesc.pitch.offset == 32
    assert (acvm_amd.WIRE_BINCODE, acvm_amd.WIRE_GZIP_STORED) == (0, 1)
    assert list(inspect.signature(acvm_amd.Batch.wire_bound).parameters)[1:] == ["container", "witnesses"]
    assert list(inspect.signature(acvm_amd.Batch.witness_maps_wire_device).parameters)[1:] == ["d_ptr", "container", "witnesses", "first", "n", "pitch", "d_instances", "d_lengths"]
    assert list(inspect.signature(acvm_amd.Batch.witness_maps_wire).parameters)[1:] == ["container", "witnesses", "first", "n"]
    desc, arr = acvm_amd.wire_desc(1, 5, 7, [1, 4, 9], 4096)
    assert (desc.container, desc.first, desc.n, desc.n_witnesses, desc.pitch) == (1, 5, 7, 3, 4096) and list(arr) == [1, 4, 9]
