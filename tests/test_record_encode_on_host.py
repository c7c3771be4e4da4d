"""The record export without a device: the element scatter and the cover nibble of acvm_amd/csrc/record_encode.hpp compiled for the host
(tools/record_encode_host_test.hip). The scatter is judged by a byte-wise restatement for every element size at every byte phase, at offsets on
both edges of a window and across dword and 16-byte joints, alone and beside a neighbour in the same word; the nibble by a byte-wise restatement
for every phase; the address map by the bank condition the kernel's LDS layout is chosen for; then the argument checks that need no GPU and the
Python view."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE32, LE32, MONT, U8, U16, U32, U64, U128 = 0, 1, 2, 16, 17, 18, 19, 20
SIZES = (1, 2, 4, 8, 16, 32)
CAP = 256


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("record_encode") / "record_encode_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tools", "record_encode_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _offsets(size):
    """byte phases 0 .. 3 at the window's lower edge, across a dword and a 16-byte joint, and ending on the last bytes of a full window behind
    the largest phase: image bytes [0, 3 + 256)"""
    top = 3 + CAP - size
    return sorted(set(list(range(0, 8)) + list(range(13, 19)) + list(range(top - 4, top + 1))))


def _element(rng, size):
    return bytes(rng.randrange(1, 256) for _ in range(size))  # (no zero byte: a byte that is missing shows)


def _want_ops(byte, size):
    """a word the element owns whole is a plain store, a word it shares is an OR"""
    ops = []
    for w in range(byte // 4, (byte + size - 1) // 4 + 1):
        ops.append(("s" if 4 * w >= byte and 4 * w + 4 <= byte + size else "o") + str(w))
    return ",".join(ops)


def test_constants(tool):
    cap, image_words, lds_pitch, lds_words = (int(x) for x in tool(["const"])[0].split())
    assert cap == CAP and image_words == (cap + 3 + 3) // 4 and lds_pitch == 65 and lds_pitch >= image_words and lds_words == 64 * lds_pitch


def test_scatter_then_assemble_is_the_identity(tool):
    rng = random.Random(0x5CA77E4)
    commands, want = [], []
    for size in SIZES:
        for byte in _offsets(size):
            for _ in range(2):
                raw = _element(rng, size)
                commands.append("round %d %d %s" % (byte, size, raw.hex()))
                want.append(raw + bytes(32 - size))
    for c, g, w in zip(commands, tool(commands), want):
        assert g == w.hex(), c


def test_scatter_places_the_bytes_and_nothing_else(tool):
    """the image of one element: its bytes at its offset, zero everywhere else, whole words stored and shared words ORed"""
    rng = random.Random(0x5CA77E5)
    commands, want = [], []
    for size in SIZES:
        for byte in _offsets(size):
            raw = _element(rng, size)
            n_words = (byte + size + 3) // 4
            commands.append("put %d %d %d %s" % (n_words, byte, size, raw.hex()))
            image = bytearray(4 * n_words)
            image[byte:byte + size] = raw
            want.append("%s %s" % (bytes(image).hex(), _want_ops(byte, size)))
    for c, g, w in zip(commands, tool(commands), want):
        assert g == w, c


def test_two_fields_that_share_a_word_do_not_disturb_each_other(tool):
    """neighbours that meet inside a dword, in either order of arrival, and a one-byte mask squeezed between two elements"""
    rng = random.Random(0x5CA77E6)
    commands, want = [], []
    for size_a in SIZES:
        for size_b in SIZES:
            for byte in (1, 2, 3, 5, 14):
                a, b = _element(rng, size_a), _element(rng, size_b)
                m = _element(rng, 1)
                at_m, at_b = byte + size_a, byte + size_a + 1
                n_words = (at_b + size_b + 3) // 4
                image = bytearray(4 * n_words)
                image[byte:byte + size_a], image[at_m:at_m + 1], image[at_b:at_b + size_b] = a, m, b
                puts = [(byte, size_a, a), (at_m, 1, m), (at_b, size_b, b)]
                for order in (puts, puts[::-1]):
                    commands.append("put %d " % n_words + " ".join("%d %d %s" % (at, s, r.hex()) for at, s, r in order))
                    want.append(bytes(image).hex())
    for c, g, w in zip(commands, tool(commands), want):
        assert g.split()[0] == w, c


def _nibble(bitmap_bits, length, phase, k):
    """byte-wise: byte b of aligned dword k is byte 4 k + b - phase of the window"""
    out = 0
    for b in range(4):
        at = 4 * k + b - phase
        if 0 <= at < length and at in bitmap_bits:
            out |= 1 << b
    return out


def _bitmap_words(bits):
    return " ".join(str(sum(1 << (b - 32 * w) for b in bits if 32 * w <= b < 32 * w + 32)) for w in range(CAP // 32))


def test_cover_nibble_against_a_byte_wise_restatement(tool):
    rng = random.Random(0x5CA77E7)
    commands, want = [], []
    for length in (1, 2, 3, 4, 5, 7, 31, 32, 33, 108, 255, 256):
        patterns = [set(range(length)), {0}, {length - 1}, {b for b in range(length) if rng.random() < 0.5}, {b for b in range(length) if rng.random() < 0.9},
                    set(range(CAP))]  # (the last: bits at and above the length are set, and must not show)
        for bits in patterns:
            words = _bitmap_words(bits)
            for phase in range(4):
                n_dwords = (phase + length + 3) // 4
                for k in sorted(set(list(range(min(n_dwords, 10))) + list(range(max(0, n_dwords - 3), n_dwords + 1)))):
                    commands.append("nib %d %d %d %s" % (phase, length, k, words))
                    want.append(_nibble(bits, length, phase, k))
    assert len(commands) > 2000
    for c, g, w in zip(commands, tool(commands), want):
        assert int(g) == w, c


@pytest.mark.parametrize("pitch", [3, 4, 7, 64, 108, 128, 256, 1024])
def test_phase_1_writes_fall_on_at_least_32_banks(tool, pitch):
    """A condition, not a measurement: 64 banks of 4 bytes. The 64 lanes of one word write of the scatter -- lane = row, every lane on the same
    byte of its window -- fall on at least 32 distinct banks, at most 2 lanes per bank. Every base alignment, window offset and byte."""
    commands = []
    for base in range(4):
        for offset in ([0] if pitch <= CAP else [0, 1, 2, 3, pitch - CAP]):
            length = pitch if pitch <= CAP else CAP
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
    for name in ("acvm_batch_export_device_records", "acvm_batch_witness_records"):
        assert name in acvm_amd.ABI_SYMBOLS
    desc, _keep = acvm_amd.record_out_desc(40, [(1, BE32, 1, 33), (2, U8, 0)], 0, 4)
    assert L.acvm_batch_export_device_records(None, C.byref(desc), None, 16) == -1 and b"null batch" in L.acvm_last_error()
    assert L.acvm_batch_export_device_records(None, None, None, 16) == -1 and b"null argument" in L.acvm_last_error()
    assert L.acvm_batch_witness_records(None, C.byref(desc), None) == -1
    assert L.acvm_abi_version() == 6


def test_python_view():
    import inspect
    import acvm_amd
    # acvm_record_out_field_t / acvm_record_out_desc_t as the C compiler lays them out
    assert C.sizeof(acvm_amd.RecordOutField) == 24 and acvm_amd.RecordOutField.offset.offset == 8 and acvm_amd.RecordOutField.mask_offset.offset == 16
    assert C.sizeof(acvm_amd.RecordOutDesc) == 32 and acvm_amd.RecordOutDesc.fields.offset == 8 and acvm_amd.RecordOutDesc.n_fields.offset == 16
    assert acvm_amd.RecordOutDesc.first.offset == 20 and acvm_amd.RecordOutDesc.n.offset == 24
    assert list(inspect.signature(acvm_amd.Batch.export_device_records).parameters)[1:] == ["d_ptr", "pitch", "fields", "first", "n", "d_instances"]
    assert list(inspect.signature(acvm_amd.Batch.witness_records).parameters)[1:] == ["pitch", "fields", "first", "n"]
    desc, arr = acvm_amd.record_out_desc(40, [(1, BE32, 1, 33), (2, U8, 0), (3, U8, 34, None)], 5, 7)
    assert (desc.pitch, desc.n_fields, desc.first, desc.n) == (40, 3, 5, 7)
    assert [(f.witness, f.encoding, f.offset, f.mask_offset) for f in arr] == [(1, BE32, 1, 33), (2, U8, 0, acvm_amd.RECORD_NO_MASK), (3, U8, 34, acvm_amd.RECORD_NO_MASK)]
    assert acvm_amd.RECORD_NO_MASK == (1 << 64) - 1
