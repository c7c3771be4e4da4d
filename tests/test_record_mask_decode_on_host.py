"""The masked record import's addressing without a device: the presence byte in a record's word image, the word and bit of the missing set, and
the block's OR of those bits in LDS, of acvm_amd/csrc/record_decode.hpp and import_mask.hpp compiled for the host
(tools/record_mask_decode_host_test.hip) and judged by Python integers."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SLOT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("record_mask_decode") / "record_mask_decode_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tools", "record_mask_decode_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        return out.stdout.split("\n")[:-1]
    return run


def test_constants(tool):
    slots, miss_words, image_words = (int(x) for x in tool(["const"])[0].split())
    assert slots >= 2 and miss_words == 64 * slots
    assert 8 * 4 * (miss_words + image_words) <= 160 * 1024  # eight blocks of 256 threads -- every wave slot of a CU -- still fit its LDS


def test_presence_byte_at_every_phase(tool):
    """the mask byte at offset m of a window whose record begins at phase 0 .. 3 of its first dword: byte phase + m of the image, whatever
    surrounds it (the values 0, 1, 2, 255 and noise around them)"""
    rng = random.Random(0x3A5CD)
    commands, want = [], []
    for phase in range(4):
        for m in (0, 1, 2, 3, 4, 7, 63, 255):
            for value in (0, 1, 2, 255):
                byte = phase + m
                image = bytearray(rng.randrange(3, 255) for _ in range((byte // 4 + 1) * 4))
                image[byte] = value
                commands.append("presence %d %s" % (byte, bytes(image).hex()))
                want.append(str(value))
    assert tool(commands) == want


def test_word_and_bit_of_the_missing_set(tool):
    bp, j = 320, 77
    got = tool(["bit %d %d %d" % (k, bp, j) for k in (0, 31, 32, 36)])
    assert got == ["%d %d" % (j, 1), "%d %d" % (j, 1 << 31), "%d %d" % (bp + j, 1), "%d %d" % (bp + j, 1 << 4)]
    # beyond 32 bits of word index: position 2^20, a stride of 2^27
    assert tool(["bit %d %d %d" % (1 << 20, 1 << 27, 5)]) == ["%d 1" % ((1 << 15) * (1 << 27) + 5)]


def test_slots(tool):
    slots = int(tool(["const"])[0].split()[0])
    cases = [(0, 0, 0), (31, 0, 0), (32, 0, 1), (36, 1, 0), (32 * slots - 1, 0, slots - 1), (32 * slots, 0, NO_SLOT), (32 * (slots + 3) + 5, 3, NO_SLOT), (32 * (slots + 2) + 31, 3, slots - 1)]
    assert tool(["slot %d %d" % (k, base) for k, base, _ in cases]) == [str(s) for _, _, s in cases]


def test_the_blocks_or(tool):
    """absent (instance, position) pairs of one window, as several waves would bring them: one LDS word per (missing word, instance) holds the OR
    of its bits; a position beyond the slots goes to global memory directly; nothing else is nonzero"""
    slots = int(tool(["const"])[0].split()[0])
    pairs = [(0, 0), (0, 31), (0, 32), (0, 36), (63, 36), (63, 37), (5, 0), (5, 0 + 32 * slots), (17, 32 * (slots - 1) + 9)]
    line = tool(["or 0 %d " % len(pairs) + " ".join("%d %d" % p for p in pairs)])[0]
    words, direct = line.split("direct")
    want = {}
    for inst, k in pairs:
        if k >> 5 < slots:
            want[(k >> 5, inst)] = want.get((k >> 5, inst), 0) | 1 << (k & 31)
    assert words.split() == ["%d:%d:%d" % (w, i, bits) for (w, i), bits in sorted(want.items())]
    assert want[(0, 0)] == 1 | 1 << 31 and want[(1, 0)] == 1 | 1 << 4 and want[(1, 63)] == 3 << 4
    assert direct.split() == ["5:%d" % (32 * slots)]
    # a window whose lowest word is 1: position 36 falls into slot 0 and is reported as word 1
    assert tool(["or 1 2 7 36 7 %d" % (32 * (slots + 1) - 1)])[0] == "1:7:16 %d:7:%d direct" % (slots, 1 << 31)
    assert tool(["or 0 0"])[0] == "direct"
