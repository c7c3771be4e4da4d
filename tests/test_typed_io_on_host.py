"""The narrow encodings of the device I/O (ACVM_ENC_U8 .. ACVM_ENC_U128) and acvm_batch_import_device_parts without a device: the per-element
decoding and encoding of acvm_amd/csrc/import_decode.hpp / export_encode.hpp compiled for the host (tools/typed_io_host_test.hip) and judged by
Python integers; the byte addressing of every element size; the argument checks that need no GPU; the Python view."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
U8, U16, U32, U64, U128 = 16, 17, 18, 19, 20
NARROW = (U8, U16, U32, U64, U128)
SIZE = {U8: 1, U16: 2, U32: 4, U64: 8, U128: 16}
INSTANCE_MAJOR, WITNESS_MAJOR, BROADCAST = 0, 1, 16
N_RANDOM = 500


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("typed_io") / "typed_io_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tools", "typed_io_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        return out.stdout.split("\n")[:-1]
    return run


def _decode_values(encoding):
    """what the issue lists: 0, 1, the byte and plane-word boundaries, the top bit, all ones, alternating bits, seeded random values -- those that
    the width holds"""
    bits = 8 * SIZE[encoding]
    alternating = [int("55" * SIZE[encoding], 16), int("aa" * SIZE[encoding], 16)]
    vals = [0, 1, 255, 256, (1 << 29) - 1, 1 << 29, 1 << (bits - 1), (1 << bits) - 1] + alternating
    rng = random.Random(0x7E10 + encoding)
    vals = [v for v in vals if v < (1 << bits)] + [rng.getrandbits(bits) for _ in range(N_RANDOM)]
    if encoding == U8:
        vals += list(range(256))  # every byte: the closed form fr_mont_of_byte stands for this row on the device
    return vals


def test_sizes_and_validity(tool):
    got = [tuple(int(x) for x in line.split()) for line in tool(["size %d" % e for e in range(0, 24)])]
    for e, (valid, narrow, size) in enumerate(got):
        assert valid == (e < 3 or 16 <= e <= 20), e
        assert narrow == (16 <= e <= 20), e
        assert size == (SIZE[e] if e in SIZE else 32), e


@pytest.mark.parametrize("encoding", NARROW)
def test_decode_against_python_integers(tool, encoding):
    """the value is the integer, the row is the fully reduced x * 2^261 mod p, the plane word is low 29 bits | is-byte << 31"""
    vals = _decode_values(encoding)
    got = tool(["dec %d %s" % (encoding, x.to_bytes(SIZE[encoding], "little").hex()) for x in vals])
    assert len(got) == len(vals)
    for x, g in zip(vals, got):
        canonical, row, plane = (int(h, 16) for h in g.split())
        assert canonical == x, (encoding, hex(x))
        assert row < P and row == x * (1 << 261) % P, (encoding, hex(x))
        assert plane == (x & 0x1FFFFFFF) | (int(x < 256) << 31), (encoding, hex(x))


def _representatives(x, rng, scaled):
    """(row, factor) pairs that mean x: the row as stored -- x * 2^261 * scale mod p -- and its unreduced representatives below 2^256 (relaxed
    rows), the factor 1 or 1 / scale as a canonical integer, as tests/test_export_device_on_host.py feeds the 32-byte encodings"""
    scale = rng.randrange(1, P) if scaled else 1
    stored = x * (1 << 261) * scale % P
    reps = [stored] + [stored + k * P for k in range(1, 6) if stored + k * P < (1 << 256)]
    return [(row, pow(scale, -1, P)) for row in reps]


@pytest.mark.parametrize("encoding", NARROW)
def test_encode_against_python_integers(tool, encoding):
    """low bytes and the fits flag from canonical values below, at and above 2^w (p - 1 among them), from relaxed and unreduced rows, from scaled
    rows; an unassigned element is zero bytes and mask 0; export followed by import reproduces x whenever it fits"""
    size, bits = SIZE[encoding], 8 * SIZE[encoding]
    rng = random.Random(0xE4C0 + encoding)
    values = [0, 1, 255, 256, (1 << bits) - 1, 1 << bits, (1 << bits) + 1, (1 << bits) + 255, (1 << (bits - 1)), 1 << 128, (1 << 128) - 1, (1 << 253) + 7, P - 1, P - 256]
    values += [rng.getrandbits(bits) for _ in range(100)] + [rng.randrange(P) for _ in range(100)] + [rng.getrandbits(bits) | (1 << rng.randrange(bits, 253)) for _ in range(50)]
    commands, want = [], []
    for n, x in enumerate(values):
        for scaled in (False, True):
            reps = _representatives(x, rng, scaled)
            for row, factor in (reps if n < 14 else [reps[0], rng.choice(reps)]):
                commands.append("enc %d 1 %064x %064x" % (encoding, row, factor))
                want.append(((x % (1 << bits)).to_bytes(size, "little"), 1 if x < (1 << bits) else 2, x))
    commands.append("enc %d 0 %064x %064x" % (encoding, rng.randrange(1 << 256), 1))
    want.append((bytes(size), 0, None))
    got = tool(commands)
    assert len(got) == len(want)
    again = []
    for c, g, (low, mask, x) in zip(commands, got, want):
        b, m = g.split()
        assert (bytes.fromhex(b), int(m)) == (low, mask), c
        if mask == 1:
            again.append((x, "dec %d %s" % (encoding, b)))
    assert len(again) > 200
    for (x, c), g in zip(again, tool([c for _, c in again])):
        assert int(g.split()[0], 16) == x, c


def test_byte_addressing(tool):
    """element (i, c) lies at index x size with the index rule of the 32-byte encodings; a broadcast column holds one element"""
    cases = []
    for size in (1, 2, 4, 8, 16, 32):
        cases += [(INSTANCE_MAJOR, 7, 5, 3, size), (INSTANCE_MAJOR, 9, 129, 8, size), (WITNESS_MAJOR, 130, 129, 8, size), (WITNESS_MAJOR, 137, 0, 41, size),
                  (WITNESS_MAJOR, (1 << 33) + 1, 5, 9, size), (INSTANCE_MAJOR, (1 << 32) + 3, (1 << 20) + 1, 2, size),
                  (BROADCAST, 0, 129, 8, size), (BROADCAST, 777, 5, 0, size), (BROADCAST, 1 << 33, 1 << 20, 41, size)]
    got = [int(g) for g in tool(["at %d %d %d %d %d" % c for c in cases])]
    want = [(c if layout == BROADCAST else c * s + i if layout == WITNESS_MAJOR else i * s + c) * size for layout, s, i, c, size in cases]
    assert got == want


def test_argument_checks_without_a_device():
    import acvm_amd
    L = acvm_amd.lib()
    for name in ("acvm_batch_import_device_parts", "acvm_debug_import_list_copies"):
        assert name in acvm_amd.ABI_SYMBOLS
    E_INVALID = -1
    for encoding in NARROW:  # valid encodings: the refusal is the null batch's, not the encoding's
        d = acvm_amd.ImportDesc(encoding=encoding, layout=WITNESS_MAJOR, n_columns=0, stride=0)
        for fn in (L.acvm_batch_import_device, L.acvm_batch_solve_then_import_ex):
            assert fn(None, C.byref(d), 16) == E_INVALID
            assert b"encoding" not in L.acvm_last_error()
        x = acvm_amd.ExportDesc(encoding=encoding, layout=INSTANCE_MAJOR, first=0, n=1, stride=0)
        assert L.acvm_batch_export_device(None, C.byref(x), 16, None) == E_INVALID
        assert b"encoding" not in L.acvm_last_error()
    for encoding in (3, 15, 21):
        d = acvm_amd.ImportDesc(encoding=encoding, layout=0, n_columns=0, stride=0)
        assert L.acvm_batch_import_device(None, C.byref(d), 16) == E_INVALID
        assert b"encoding" in L.acvm_last_error()
        x = acvm_amd.ExportDesc(encoding=encoding, layout=0, first=0, n=1, stride=0)
        assert L.acvm_batch_export_device(None, C.byref(x), 16, None) == E_INVALID
        assert b"encoding" in L.acvm_last_error()
    # the broadcast layout belongs to parts alone
    d = acvm_amd.ImportDesc(encoding=U8, layout=BROADCAST, n_columns=0, stride=0)
    assert L.acvm_batch_import_device(None, C.byref(d), 16) == E_INVALID
    assert b"layout" in L.acvm_last_error()
    # the parts entry point
    assert L.acvm_batch_import_device_parts(None, None, 1) == E_INVALID
    assert L.acvm_batch_import_device_parts(None, None, 0) == E_INVALID  # (the null batch)
    parts = (acvm_amd.ImportPart * 2)()
    parts[0].encoding, parts[0].layout, parts[0].d_values = U8, BROADCAST, 16
    parts[1].encoding, parts[1].layout, parts[1].d_values = U8, 2, 16
    assert L.acvm_batch_import_device_parts(None, parts, 1) == E_INVALID
    assert b"layout" not in L.acvm_last_error() and b"encoding" not in L.acvm_last_error()
    assert L.acvm_batch_import_device_parts(None, C.cast(C.byref(parts[1]), C.POINTER(acvm_amd.ImportPart)), 1) == E_INVALID
    assert b"layout" in L.acvm_last_error()
    parts[1].encoding, parts[1].layout = 21, BROADCAST
    assert L.acvm_batch_import_device_parts(None, C.cast(C.byref(parts[1]), C.POINTER(acvm_amd.ImportPart)), 1) == E_INVALID
    assert b"encoding" in L.acvm_last_error()
    assert L.acvm_debug_import_list_copies(None) == 0


def test_python_view(tool):
    import acvm_amd
    import inspect
    assert (acvm_amd.ENC_U8, acvm_amd.ENC_U16, acvm_amd.ENC_U32, acvm_amd.ENC_U64, acvm_amd.ENC_U128) == NARROW
    assert acvm_amd.LAYOUT_BROADCAST == BROADCAST
    assert [acvm_amd.element_size(e) for e in (0, 1, 2) + NARROW] == [32, 32, 32, 1, 2, 4, 8, 16]
    assert callable(acvm_amd.Batch.import_device_parts)
    # the signatures the earlier interface pinned are as they were
    assert list(inspect.signature(acvm_amd.Batch.import_device).parameters)[1:] == ["d_ptr", "encoding", "layout", "columns", "n_columns", "stride"]
    assert C.sizeof(acvm_amd.ImportDesc) == 32 and acvm_amd.lib().acvm_abi_version() == 6  # (the change is additive)
    # acvm_import_part_t as the C compiler lays it out
    part = acvm_amd.ImportPart
    fields = (part.d_values, part.encoding, part.layout, part.positions, part.columns, part.n, part.n_columns, part.stride)
    assert [int(x) for x in tool(["part"])[0].split()] == [C.sizeof(part)] + [f.offset for f in fields]
