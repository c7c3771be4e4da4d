"""The packed wire buffers' device code without a device: acvm_amd/csrc/wire_repitch.hpp compiled for the host with the host side under
AddressSanitizer and UndefinedBehaviorSanitizer (tools/wire_repitch_host_test.hip, a stand-alone program: source, destination and columns in
heap blocks of exactly the stated sizes). The per-lane body of the repitch kernel at all 16 x 16 source and destination alignments and the
lengths around every unit and tile edge, every output byte against a plain Python slice and every byte outside the row against the 0xA5
fill; the three classes of the offsets judgement, and that a row with a finding copies nothing; the scan's block arithmetic against running
sums; then the argument checks that need no GPU and the Python view."""
import ctypes as C
import inspect
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = list(range(0, 41)) + [63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
FILL = 0xA5


def source(n):
    return bytes((k * 131 + 7) % 251 for k in range(n))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wire_repitch") / "wire_repitch_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "wire_repitch_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def unhex(text):
    return b"" if text == "-" else bytes.fromhex(text)


def copy_command(src_align, dst_align, src_bytes, dst_bytes, rows):
    return "copy %d %d %d %d %d" % (src_align, dst_align, src_bytes, dst_bytes, len(rows)) + "".join(" %d %d %d" % r for r in rows)


def copy_model(src_bytes, dst_bytes, rows):
    src, dst = source(src_bytes), bytearray([FILL]) * dst_bytes
    for s, d, n in rows:
        dst[d:d + n] = src[s:s + n]
    return bytes(dst)


def test_every_alignment_and_length_in_blocks_of_exactly_the_row(tool):
    """the row IS the source and IS the destination: a load or store one byte outside either is one the sanitizer reports"""
    asked = [(sa, da, n, n, [(0, 0, n)]) for sa in range(16) for da in range(16) for n in LENGTHS]
    got = tool([copy_command(*a) for a in asked])
    for (sa, da, src_bytes, dst_bytes, rows), line in zip(asked, got):
        assert unhex(line) == copy_model(src_bytes, dst_bytes, rows), (sa, da, rows)


def test_every_alignment_and_length_with_fill_around_the_row(tool):
    """the row inside larger buffers, at offsets that move its ends through a unit: the fill before and behind it stays"""
    asked = []
    for sa in range(16):
        for da in range(16):
            for n in LENGTHS:
                s, d = (3 * sa + n) % 19, (5 * da + n) % 23
                asked.append((sa, da, s + n + (sa + da) % 3, d + n + 17, [(s, d, n)]))
    got = tool([copy_command(*a) for a in asked])
    for (sa, da, src_bytes, dst_bytes, rows), line in zip(asked, got):
        want = copy_model(src_bytes, dst_bytes, rows)
        assert unhex(line) == want, (sa, da, rows)
        s, d, n = rows[0]
        assert want[:d] == bytes([FILL]) * d and want[d + n:] == bytes([FILL]) * (dst_bytes - d - n)


def test_rows_that_share_a_dword_each_store_their_own_bytes(tool):
    rng = random.Random(7)
    asked = []
    for _ in range(300):
        lens = [rng.choice([0, 1, 2, 3, 5, 15, 16, 17, 31, 33, 63, 64, 65, 100]) for _ in range(rng.randrange(2, 9))]
        rows, s, d = [], 0, 0
        for n in lens:  # back to back on both sides: no byte between rows
            rows.append((s, d, n))
            s, d = s + n, d + n
        asked.append((rng.randrange(16), rng.randrange(16), s, d, rows))
    got = tool([copy_command(*a) for a in asked])
    for (sa, da, src_bytes, dst_bytes, rows), line in zip(asked, got):
        assert unhex(line) == copy_model(src_bytes, dst_bytes, rows), (sa, da, rows)


def test_pack_pitched_rows_at_a_capacity(tool):
    rng = random.Random(11)
    asked = []
    for _ in range(200):
        pitch = rng.choice([16, 48, 80, 272])
        lens = [rng.choice([0, 1, 15, 16, min(17, pitch), pitch - 1, pitch]) for _ in range(rng.randrange(1, 8))]  # (a slot holds at most its pitch)
        total = sum(lens)
        capacity = rng.choice([0, total, max(total - 1, 0), total // 2])
        asked.append((rng.randrange(16), rng.randrange(16), pitch, capacity, total + 5, lens))
    got = tool(["pack %d %d %d %d %d %d" % (sa, da, pitch, cap, dst_bytes, len(lens)) + "".join(" %d" % n for n in lens) for sa, da, pitch, cap, dst_bytes, lens in asked])
    for (sa, da, pitch, cap, dst_bytes, lens), line in zip(asked, got):
        src, want, at = source(len(lens) * pitch), bytearray([FILL]) * dst_bytes, 0
        for i, n in enumerate(lens):
            if at + n <= cap:  # (the leading rows that end at or in front of the capacity: offsets only grow)
                want[at:at + n] = src[i * pitch:i * pitch + n]
            at += n
        assert unhex(line) == bytes(want), (sa, da, pitch, cap, lens)


def unpack(tool, cases):
    got = tool(["unpack %d %d %d %d %d" % (sa, da, n_bytes, pitch, len(offsets) - 1) + "".join(" %d" % o for o in offsets) for sa, da, n_bytes, pitch, offsets in cases])
    out = []
    for (sa, da, n_bytes, pitch, offsets), line in zip(cases, got):
        tok = line.split()
        out.append(([int(t) for t in tok[:-1]], unhex(tok[-1])))
    return out


def unpack_model(n_bytes, pitch, offsets):
    src, n = source(n_bytes), len(offsets) - 1
    classes, dst = [], bytearray([FILL]) * (n * pitch)
    for j in range(n):
        lo, hi = offsets[j], offsets[j + 1]
        cls = 1 if hi < lo else 2 if hi > n_bytes else 3 if hi - lo > pitch else 0
        classes.append(cls)
        if not cls:
            dst[j * pitch:j * pitch + hi - lo] = src[lo:hi]
    return classes, bytes(dst)


def test_the_three_offsets_classes_and_a_row_with_a_finding_copies_nothing(tool):
    cases = [
        (0, 0, 100, 32, [0, 10, 5, 40, 72, 100]),         # class 1 at row 1; row 2 (5 .. 40) is 35 bytes: class 3
        (5, 9, 100, 32, [0, 10, 101, 101, 100]),           # class 2 at rows 1 and 2 (an empty row beyond the end too), class 1 at row 3
        (0, 0, 100, 32, [0, 33, 65, 97, 100]),             # class 3 at row 0; exactly the pitch passes
        (3, 0, 61, 16, [0, 16, 32, 48, 61]),               # a buffer that ends in mid-dword
        (0, 0, 0, 16, [0, 0, 0]),                          # nothing at all
        (0, 0, 50, 16, [1 << 63, 1 << 62, (1 << 64) - 1, 3, 10]),
        (0, 7, 40, 64, [60, 70, 20, 40]),                  # a start beyond the buffer: class 2, then class 1, then a row that passes
    ]
    got = unpack(tool, cases)
    seen = set()
    for (sa, da, n_bytes, pitch, offsets), g in zip(cases, got):
        assert g == unpack_model(n_bytes, pitch, offsets), (n_bytes, pitch, offsets, g[0])
        seen |= set(g[0])
    assert seen == {0, 1, 2, 3}
    assert got[0][0] == [0, 1, 3, 0, 0] and got[1][0] == [0, 2, 2, 1] and got[2][0] == [3, 0, 0, 0]


def test_unpack_a_seeded_sweep_at_every_alignment(tool):
    rng = random.Random(3)
    cases = []
    for k in range(512):
        pitch = rng.choice([16, 32, 80])
        lens = [rng.choice([0, 1, 7, 15, 16, 17, pitch, pitch + 1]) for _ in range(rng.randrange(1, 7))]
        offsets = [0]
        for n in lens:
            offsets.append(offsets[-1] + n)
        n_bytes = offsets[-1] - rng.choice([0, 0, 0, 1])
        if rng.random() < 0.2:
            offsets[rng.randrange(len(offsets))] = rng.randrange(0, n_bytes + 40)
        cases.append((k % 16, (k // 16) % 16, max(n_bytes, 0), pitch, offsets))
    for case, g in zip(cases, unpack(tool, cases)):
        assert g == unpack_model(*case[2:]), case


def test_the_scan_block_arithmetic(tool):
    rng = random.Random(5)
    asked = []
    for m, chunk in ((0, 64), (1, 64), (3, 1), (63, 64), (64, 64), (65, 64), (130, 64), (1023, 2000), (1024, 2000), (1025, 2000), (2500, 960), (4100, 4100)):
        lens = [rng.choice([0, 1, 63, 760000, (1 << 33) + 5]) for _ in range(m)]
        base = rng.choice([0, 12345, 1 << 40])
        total = base + sum(lens)
        for capacity in (0, total, total - 1 if total else 0, (base + total) // 2, (1 << 64) - 1):
            asked.append((base, capacity, chunk, lens))
    got = tool(["scan %d %d %d %d" % (base, cap, chunk, len(lens)) + "".join(" %d" % n for n in lens) for base, cap, chunk, lens in asked])
    for (base, cap, chunk, lens), line in zip(asked, got):
        tok = [int(t) for t in line.split()]
        want = [base]
        for n in lens:
            want.append(want[-1] + n)
        assert tok[:-2] == want and tok[-2] == want[-1], (base, cap, chunk, len(lens))
        assert tok[-1] == sum(1 for o in want[1:] if o <= cap), (base, cap, chunk, len(lens))


def test_the_finding_key_orders_instance_and_class(tool):
    pairs = [(0, 1), (0, 2), (0, 3), (1, 1), (63, 3), (64, 1), ((1 << 32) - 1, 3)]
    keys = []
    for p, got in zip(pairs, tool(["key %d %d" % p for p in pairs])):
        key, j, cls = (int(x) for x in got.split())
        assert (j, cls) == p and 0 < key < 1 << 64
        keys.append(key)
    assert keys == sorted(keys, reverse=True)  # atomicMax keeps the smallest pair


def test_argument_checks_without_a_device():
    import acvm_amd
    L = acvm_amd.lib()
    for name in ("acvm_batch_witness_maps_wire_packed_device", "acvm_batch_witness_maps_wire_packed", "acvm_batch_import_device_wire_packed", "acvm_debug_wire_repitch"):
        assert name in acvm_amd.ABI_SYMBOLS
    desc, _keep = acvm_amd.wire_desc(acvm_amd.WIRE_BINCODE, 0, 1)
    total, fit, offsets = C.c_uint64(), C.c_uint32(), (C.c_uint64 * 2)()
    assert L.acvm_batch_witness_maps_wire_packed_device(None, C.byref(desc), None, 16, 64, 32, C.byref(total), C.byref(fit)) == -1 and b"null batch" in L.acvm_last_error()
    assert L.acvm_batch_witness_maps_wire_packed(None, C.byref(desc), None, 0, offsets, C.byref(total), C.byref(fit)) == -1 and b"null batch" in L.acvm_last_error()
    in_desc = acvm_amd.WireInDesc(container=acvm_amd.WIRE_GZIP_DEFLATE, pitch=64)
    assert L.acvm_batch_import_device_wire_packed(None, C.byref(in_desc), 16, 0, 32) == -1 and b"null batch" in L.acvm_last_error()
    result = (C.c_uint64 * 2)()
    assert L.acvm_debug_wire_repitch(0, 1, 8, None, offsets, None, 0, 0, offsets, 0, 0, None, result) == -1 and b"null argument" in L.acvm_last_error()
    assert L.acvm_debug_wire_repitch(0, 0, 8, None, None, None, 0, 16, offsets, 0, 0, None, result) == -1 and b"displacement" in L.acvm_last_error()
    assert L.acvm_abi_version() == 6


def test_python_view():
    import acvm_amd
    assert list(inspect.signature(acvm_amd.Batch.witness_maps_wire_packed_device).parameters)[1:] == ["d_ptr", "capacity", "d_offsets", "container", "witnesses", "first", "n", "d_instances"]
    assert list(inspect.signature(acvm_amd.Batch.witness_maps_wire_packed).parameters)[1:] == ["container", "witnesses", "first", "n", "capacity"]
    assert list(inspect.signature(acvm_amd.Batch.import_device_wire_packed).parameters)[1:] == ["d_ptr", "n_bytes", "d_offsets", "container", "pitch"]
    assert list(inspect.signature(acvm_amd.debug_wire_repitch).parameters) == ["rows", "packed", "offsets", "pitch", "displacement", "capacity", "scan_chunk", "fill", "lengths"]
