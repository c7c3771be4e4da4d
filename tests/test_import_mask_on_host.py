"""The masked device import without a device: the addressing arithmetic of acvm_amd/csrc/import_mask.hpp -- where a mask byte lies, the word and
bit of the missing set, the result word of a bad byte, the pieces an instance-major mask row is read in -- compiled for the host
(tools/import_mask_host_test.hip) and judged by Python index arithmetic; the masked plan's checks and its inequality to the unmasked plan; the
argument checks of the entry points that need no GPU; the Python view."""
import ctypes as C
import inspect
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE32, LE32, MONT, U8, U64 = 0, 1, 2, 16, 19
IM, WM = 0, 1
E_INVALID = -1


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("import_mask") / "import_mask_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "import_mask_host_test.hip"),
                           os.path.join(ROOT, "acvm_amd", "csrc", "import_plan.cpp"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        return out.stdout.split("\n")[:-1]
    return run


def test_mask_byte_addressing(tool):
    """element (instance i, column c) is byte i * stride + c instance-major and c * stride + i witness-major: dense, padded, beyond 2^32"""
    rng = random.Random(0x3A5C)
    cases = [(IM, 37, 0, 0), (IM, 37, 299, 36), (IM, 41, 299, 36), (WM, 300, 299, 36), (WM, 304, 0, 36), (WM, 192, 129, 0), (WM, 1 << 33, 5, 9), (IM, 1 << 33, 5, 9)]
    cases += [(rng.randrange(2), rng.randrange(1, 1 << 20), rng.randrange(1 << 20), rng.randrange(1 << 12)) for _ in range(200)]
    got = tool(["byte %d %d %d %d" % c for c in cases])
    assert [int(g) for g in got] == [c * s + i if layout == WM else i * s + c for layout, s, i, c in cases]


def test_missing_set_word_and_bit(tool):
    """position k of instance j: word (k >> 5) * Bp + j, bit k & 31 -- at the word edges 0, 31, 32, 36, 63, 64 and at random positions"""
    rng = random.Random(0x3A5D)
    cases = [(k, 320, j) for k in (0, 1, 31, 32, 36, 63, 64, 65, 1023, 1024) for j in (0, 63, 64, 299, 319)]
    cases += [(rng.randrange(1 << 16), 64 * rng.randrange(1, 1 << 12), rng.randrange(1 << 16)) for _ in range(200)]
    got = tool(["word %d %d %d" % c for c in cases])
    for (k, bp, j), g in zip(cases, got):
        words, index, bit = (int(x) for x in g.split())
        assert (words, index, bit) == ((k + 32) // 32, (k // 32) * bp + j, 1 << (k % 32)), (k, bp, j)


def test_bad_byte_key_orders_by_instance_then_position(tool):
    """the device keeps the LARGEST result word; that is the smallest (instance, position), and zero means none"""
    rng = random.Random(0x3A5E)
    pairs = [(0, 0), (0, 36), (1, 0), (299, 36), (63, 31), (64, 32), ((1 << 32) - 2, (1 << 32) - 2)] + [(rng.randrange(1 << 20), rng.randrange(1 << 12)) for _ in range(100)]
    got = tool(["key %d %d" % p for p in pairs])
    words = []
    for (i, k), g in zip(pairs, got):
        w, gi, gk = g.split()
        assert (int(gi), int(gk)) == (i, k)
        assert int(w, 16) == ((1 << 64) - 1) ^ (i << 32 | k) and int(w, 16) != 0
        words.append(int(w, 16))
    assert pairs[max(range(len(pairs)), key=lambda q: words[q])] == min(pairs)


def test_instance_major_row_pieces(tool):
    """a row of n bytes at any address: bytes up to the first 16-byte boundary, whole 16-byte units inside the row, the rest bytes"""
    cases = [(a, n) for a in (0, 1, 15, 16, 17, 37 * 7, 4096 + 5) for n in (0, 1, 15, 16, 17, 31, 32, 33, 36, 37, 64, 1000)]
    got = tool(["pieces %d %d" % c for c in cases])
    for (a, n), g in zip(cases, got):
        head, units, tail = (int(x) for x in g.split())
        assert head + 16 * units + tail == n, (a, n)
        assert head == min(n, -a % 16) and tail < 16, (a, n)
        assert units == 0 or (a + head) % 16 == 0, (a, n)


def test_masked_plan_checks_and_inequality(tool):
    """every check of the unmasked descriptor, unchanged; a mask makes the plan unequal to the unmasked one; a null mask IS the unmasked plan"""
    n_in, B = 37, 300
    cols = ",".join(str((5 * k + 3) % n_in) for k in range(n_in))
    got = tool(["view %d %d" % (B, n_in),
                "desc %d %d 0 0 4096 0 null" % (MONT, WM),          # 1 unmasked
                "desc %d %d 0 0 4096 7 null" % (MONT, WM),          # 2 masked, any alignment of the mask
                "eq",
                "desc %d %d 0 0 4096 0 null" % (MONT, WM),          # 4 a null mask: the unmasked plan again
                "eq",                                               #   (against the masked one)
                "desc %d %d 0 0 4096 0 null" % (MONT, WM),
                "eq",                                               # 7 unmasked == unmasked
                "desc %d %d 0 0 4097 9 null" % (BE32, IM),          # 8 the plain shape keeps its exemption from the alignment rule
                "desc %d %d 0 %d 4104 9 null" % (LE32, IM, n_in),   # 9 misaligned values
                "desc %d %d 0 %d 4096 9 null" % (LE32, IM, n_in - 1),
                "desc %d %d 0 %d 4096 9 null" % (LE32, WM, B - 1),
                "desc %d %d %d 0 4096 9 %s" % (U8, IM, n_in, cols),
                "desc %d %d %d 0 4100 9 %s" % (U64, WM, n_in, cols),
                "desc %d %d %d 0 4096 9 %s" % (LE32, IM, n_in - 1, cols),
                "desc 3 0 0 0 4096 9 null", "desc 0 2 0 0 4096 9 null", "desc 0 0 0 0 0 9 null"])
    assert got[0] == "ok 0 0 %d %d 32 %d %d -1 0" % (MONT, WM, B, n_in)
    assert got[1] == "ok 0 1 %d %d 32 %d %d -1 0" % (MONT, WM, B, n_in)
    assert got[2] == "eq 0"
    assert got[3] == got[0] and got[4] == "eq 0"
    assert got[6] == "eq 1"
    assert got[7] == "ok 1 1 %d %d 32 %d %d -1 0" % (BE32, IM, n_in, n_in)
    assert got[8].startswith("err -1 ") and "16-byte aligned" in got[8]
    assert got[9].startswith("err -1 ") and "stride" in got[9] and got[10].startswith("err -1 ") and "stride" in got[10]
    assert got[11] == "ok 0 1 %d %d 1 %d %d 0 %d" % (U8, IM, n_in, n_in, n_in)
    assert got[12].startswith("err -1 ") and "aligned to the element size, 8 bytes" in got[12]
    assert got[13].startswith("err -1 ") and "column" in got[13]
    assert "encoding" in got[14] and "layout" in got[15] and got[16] == "err -1 null values"


def test_argument_checks_without_a_device():
    import acvm_amd
    L = acvm_amd.lib()
    for name in ("acvm_batch_import_device_masked", "acvm_batch_set_initial_witness_masked", "acvm_debug_import_missing"):
        assert name in acvm_amd.ABI_SYMBOLS and hasattr(L, name)
    good = acvm_amd.ImportDesc(encoding=acvm_amd.ENC_LE32, layout=acvm_amd.LAYOUT_WITNESS_MAJOR, n_columns=0, stride=0)
    assert L.acvm_batch_import_device_masked(None, C.byref(good), 16, 16) == E_INVALID
    assert b"null batch" in L.acvm_last_error()
    assert L.acvm_batch_import_device_masked(None, None, 16, 16) == E_INVALID
    bad = acvm_amd.ImportDesc(encoding=3, layout=0, n_columns=0, stride=0)
    assert L.acvm_batch_import_device_masked(None, C.byref(bad), 16, 16) == E_INVALID
    assert b"encoding" in L.acvm_last_error()
    assert L.acvm_batch_set_initial_witness_masked(None, None, None) == E_INVALID
    assert L.acvm_debug_import_missing(None) == 0


def test_python_view():
    import acvm_amd
    for name in ("import_device_masked", "set_initial_witness_masked", "import_missing"):
        assert callable(getattr(acvm_amd.Batch, name))
    assert list(inspect.signature(acvm_amd.Batch.import_device_masked).parameters)[1:] == ["d_ptr", "d_assigned", "encoding", "layout", "columns", "n_columns", "stride"]

    class Recorder(acvm_amd.Batch):
        def __init__(self):
            self.calls = []

        def __del__(self):
            pass

        def import_device_masked(self, d_ptr, d_assigned, *args, **keywords):
            self.calls.append((d_ptr, d_assigned, args, keywords))

    r = Recorder()
    r.import_device(4096, acvm_amd.ENC_MONT256_LE, layout=acvm_amd.LAYOUT_WITNESS_MAJOR, d_assigned=8191)
    assert r.calls == [(4096, 8191, (acvm_amd.ENC_MONT256_LE,), {"layout": acvm_amd.LAYOUT_WITNESS_MAJOR})]
