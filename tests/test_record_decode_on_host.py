"""The record import without a device: the element assembly and the staging image's address map of acvm_amd/csrc/record_decode.hpp compiled
for the host (tools/record_decode_host_test.hip). The assembly is judged by Python integers for every element size, at byte offsets across dword
and 16-byte joints, in all eight encodings, on the value edges; the address map by the bank condition the kernel's LDS layout is chosen for; then
the argument checks that need no GPU and the Python view."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BE32, LE32, MONT, U8, U16, U32, U64, U128 = 0, 1, 2, 16, 17, 18, 19, 20
ENCODINGS = (BE32, LE32, MONT, U8, U16, U32, U64, U128)
OFFSETS = list(range(0, 8)) + list(range(29, 36))
SIZES = (1, 2, 4, 8, 16, 32)


def size_of(encoding):
    return 1 << (encoding - U8) if U8 <= encoding <= U128 else 32


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("record_decode") / "record_decode_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tools", "record_decode_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        return out.stdout.split("\n")[:-1]
    return run


def _edges(size):
    """0, 1, 255, 256, 2^29 - 1, 2^29 + 1, the top bit, all ones -- those the width holds -- and p - 1, p, 2^256 - 1 for 32 bytes"""
    bits = 8 * size
    vals = [v for v in (0, 1, 255, 256, (1 << 29) - 1, (1 << 29) + 1, 1 << (bits - 1), (1 << bits) - 1) if v < (1 << bits)]
    if size == 32:
        vals += [P - 1, P, (1 << 256) - 1]
    return sorted(set(vals))


def _image(raw, offset, rng):
    """the aligned dwords from byte 0 to the element's last byte, the element at `offset`, noise everywhere else"""
    n = (offset + len(raw) + 3) // 4 * 4
    b = bytearray(rng.randrange(1, 256) for _ in range(n))
    b[offset:offset + len(raw)] = raw
    return bytes(b).hex()


def test_constants(tool):
    cap, image_words, lds_pitch, lds_words = (int(x) for x in tool(["const"])[0].split())
    assert cap == 256 and image_words == (cap + 3 + 3) // 4 and lds_pitch >= image_words and lds_words == 64 * lds_pitch
    assert 4 * 4 * lds_words <= 160 * 1024  # four blocks per CU, at least


def test_assembly_of_every_size_at_every_offset(tool):
    rng = random.Random(0x4EC0DE)
    commands, want = [], []
    for size in SIZES:
        for offset in OFFSETS:
            for v in _edges(size) + [rng.getrandbits(8 * size) for _ in range(3)]:
                raw = v.to_bytes(size, "little")
                commands.append("asm %d %d %s" % (offset, size, _image(raw, offset, rng)))
                want.append(raw + bytes(32 - size))  # zero-extended, in memory order
    got = tool(commands)
    assert len(got) == len(want)
    for c, g, w in zip(commands, got, want):
        assert g == w.hex(), c


def _value(raw, encoding):
    if encoding == BE32:
        return int.from_bytes(raw, "big") % P
    if encoding == MONT:
        return int.from_bytes(raw, "little") * pow(1 << 256, -1, P) % P
    return int.from_bytes(raw, "little") % P


def test_decode_of_all_encodings_at_every_offset(tool):
    """canonical value, row and plane word: what acvm_batch_import_device's decoding gives for the same bytes"""
    rng = random.Random(0x4EC0DF)
    commands, want = [], []
    for encoding in ENCODINGS:
        size = size_of(encoding)
        for offset in OFFSETS:
            for s in _edges(size):
                raw = s.to_bytes(size, "big" if encoding == BE32 else "little")  # (the string s as the encoding reads it)
                commands.append("dec %d %d %s" % (offset, encoding, _image(raw, offset, rng)))
                want.append(_value(raw, encoding))
    got = tool(commands)
    assert len(got) == len(want)
    for c, g, x in zip(commands, got, want):
        canonical, row, plane = (int(h, 16) for h in g.split())
        assert canonical == x and row == x * (1 << 261) % P and plane == (x & 0x1FFFFFFF) | (int(x < 256) << 31), c


def test_address_map_keeps_each_records_phase(tool):
    lds_pitch = int(tool(["const"])[0].split()[2])
    for pitch, base, offset, byte in [(7, 1, 0, 5), (108, 3, 64, 31), (1500, 2, 1465, 34), (1, 0, 0, 0)]:
        got = [int(x) for x in tool(["lds %d %d %d %d" % (pitch, base, offset, byte)])[0].split()]
        assert got == [i * lds_pitch + ((base + i * pitch + offset) % 4 + byte) // 4 for i in range(64)]


@pytest.mark.parametrize("pitch", [4, 64, 108, 128, 256, 1024])
def test_phase_2_reads_fall_on_at_least_32_banks(tool, pitch):
    """A condition, not a measurement: 64 banks of 4 bytes. The 64 lanes of one word read of phase 2 -- lane = instance, every lane on the same
    byte of its window -- fall on at least 32 distinct banks, at most 2 lanes per bank: the floor under the 32-bank modulus of a dword read.
    Every base alignment, window offset and byte, each word of a 32-byte element included."""
    cap = 256
    commands = []
    for base in range(4):
        for offset in ([0] if pitch <= cap else [0, 1, 2, 3, pitch - cap]):
            length = pitch if pitch <= cap else cap
            for byte in sorted({0, 1, 2, 3, 4, 31, 32, 33, length // 2, length - 1}):
                if byte < length:
                    commands.append("lds %d %d %d %d" % (pitch, base, offset, byte))
    for c, line in zip(commands, tool(commands)):
        words = [int(x) for x in line.split()]
        assert len(words) == 64
        lanes_per_bank = {}
        for w in words:
            lanes_per_bank[w % 64] = lanes_per_bank.get(w % 64, 0) + 1
        assert len(lanes_per_bank) >= 32 and max(lanes_per_bank.values()) <= 2, c


def test_argument_checks_without_a_device():
    import acvm_amd
    L = acvm_amd.lib()
    for name in ("acvm_batch_import_device_records", "acvm_batch_set_initial_witness_records", "acvm_node_solve_records"):
        assert name in acvm_amd.ABI_SYMBOLS
    desc, _keep = acvm_amd.record_desc(33, [(0, BE32, 1)])
    assert L.acvm_batch_import_device_records(None, C.byref(desc), 16) == -1 and b"null batch" in L.acvm_last_error()
    assert L.acvm_batch_import_device_records(None, None, 16) == -1 and b"null argument" in L.acvm_last_error()
    assert L.acvm_batch_set_initial_witness_records(None, C.byref(desc), None) == -1
    assert L.acvm_node_solve_records(None, 1, C.byref(desc), None, None, None, None, None) == -1
    assert L.acvm_abi_version() == 6


def test_python_view():
    import inspect
    import numpy as np
    import acvm_amd
    # acvm_record_field_t / acvm_record_desc_t as the C compiler lays them out
    assert C.sizeof(acvm_amd.RecordField) == 16 and acvm_amd.RecordField.offset.offset == 8
    assert C.sizeof(acvm_amd.RecordDesc) == 24 and acvm_amd.RecordDesc.fields.offset == 8 and acvm_amd.RecordDesc.n_fields.offset == 16
    assert list(inspect.signature(acvm_amd.Batch.import_device_records).parameters)[1:] == ["d_ptr", "pitch", "fields"]
    assert list(inspect.signature(acvm_amd.Batch.set_initial_witness_records).parameters)[1:] == ["records", "pitch", "fields"]
    assert list(inspect.signature(acvm_amd.Node.solve_records).parameters)[1:5] == ["records", "n_instances", "pitch", "fields"]
    # { msg: [u8; 64], root: Field, idx: u32, flags: [bool; 8] }, packed
    dt = np.dtype([("msg", np.uint8, 64), ("root", "V32"), ("idx", "<u4"), ("flags", np.bool_, 8)])
    pitch, fields = acvm_amd.record_fields_from_dtype(dt, {"msg": range(64), "root": 64, "idx": 65, "flags": range(66, 74)})
    assert pitch == 108
    assert fields == [(k, U8, k) for k in range(64)] + [(64, BE32, 64), (65, U32, 96)] + [(66 + k, U8, 100 + k) for k in range(8)]
    # an aligned struct: the padding is no field; an encoding of the caller's choice
    al = np.dtype([("flag", "u1"), ("x", "<u8"), ("m", "V32")], align=True)
    pitch, fields = acvm_amd.record_fields_from_dtype(al, {"x": 1, "flag": 0, "m": (2, MONT)})
    assert pitch == 48 and fields == [(1, U64, 8), (0, U8, 0), (2, MONT, 16)]
    with pytest.raises(ValueError):
        acvm_amd.record_fields_from_dtype(dt, {"msg": range(5)})
    with pytest.raises(ValueError):
        acvm_amd.record_fields_from_dtype(dt, {"idx": (0, U8)})
