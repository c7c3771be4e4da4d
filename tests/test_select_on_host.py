"""The ordered selection of acvm_batch_outcomes_device without a device: the block, slot and rank arithmetic of acvm_amd/csrc/select_scan.hpp
compiled for the host (tools/select_host_test.hip walks the three launches with it) against a plain loop; the refusals of
acvm_batch_outcomes_device and acvm_batch_export_device_list that need no GPU; the Python view."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("select") / "select_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tools", "select_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        return out.stdout.split("\n")[:-1]
    return run


def patterns(n, rng):
    """status arrays over {0, 2}: none, all, alternating, first only, last only, seeded random -- selected by mask 1 << 2"""
    yield "none", [0] * n
    yield "all", [2] * n
    yield "alternating", [2 * (i & 1) for i in range(n)]
    yield "first", [2 if i == 0 else 0 for i in range(n)]
    yield "last", [2 if i == n - 1 else 0 for i in range(n)]
    yield "random", [rng.choice((0, 2)) for _ in range(n)]


def sizes(span):
    return list(range(0, 301)) + [span - 1, span, span + 1, 3 * span + 1]


def test_offsets_against_a_plain_loop(tool):
    span, threads, rounds = (int(x) for x in tool(["span"])[0].split())
    assert span == threads * rounds and threads % 64 == 0
    rng = random.Random(0x5E1EC7)
    commands, want = [], []
    for n in sizes(span):
        for name, st in patterns(n, rng):
            first = rng.choice((0, 1, 64, 1 << 20))
            commands.append("sel %d %d %s" % (first, 1 << 2, bytes(st).hex() or "-"))
            want.append((n, name, [first + i for i, s in enumerate(st) if s == 2]))
    got = tool(commands)
    assert len(got) == len(want)
    for line, (n, name, w) in zip(got, want):
        assert not line.startswith("bad"), (n, name, line)
        head, _, rest = line.partition(":")
        assert int(head) == len(w), (n, name)
        assert [int(x) for x in rest.split()] == w, (n, name)


def test_masks_and_status_bytes_beyond_the_mask(tool):
    """every single-bit mask and a multi-bit one over status bytes 0 .. 3; a status byte of 32 or more is selected by nothing"""
    rng = random.Random(0x5E1EC8)
    st = [rng.randrange(4) for _ in range(700)] + [32, 33, 255, 3, 0]
    masks = [1, 2, 4, 8, 0b1101, 0, 0xFFFFFFFF]
    got = tool(["sel 0 %d %s" % (m, bytes(st).hex()) for m in masks])
    for line, m in zip(got, masks):
        w = [i for i, s in enumerate(st) if s < 32 and (m >> s) & 1]
        head, _, rest = line.partition(":")
        assert int(head) == len(w) and [int(x) for x in rest.split()] == w, m


def test_refusals_without_a_device():
    """null descriptor, nothing to write, first != 0 for the list export: refused before the handle is looked at"""
    import acvm_amd
    L = acvm_amd.lib()
    for name in ("acvm_batch_outcomes_device", "acvm_batch_export_device_list", "acvm_debug_export_h2d_bytes", "acvm_debug_select"):
        assert name in acvm_amd.ABI_SYMBOLS
    E_INVALID = -1
    got = C.c_uint32(7)
    assert L.acvm_batch_outcomes_device(None, None, C.byref(got)) == E_INVALID
    nothing = acvm_amd.OutcomesDesc(first=0, n=4, select_mask=1)
    assert L.acvm_batch_outcomes_device(None, C.byref(nothing), None) == E_INVALID
    assert b"nothing to write" in L.acvm_last_error()
    count_only = acvm_amd.OutcomesDesc(first=0, n=4, select_mask=1)
    assert L.acvm_batch_outcomes_device(None, C.byref(count_only), C.byref(got)) == E_INVALID  # (a null handle)
    assert b"nothing to write" not in L.acvm_last_error()
    assert got.value == 7
    good = acvm_amd.ExportDesc(encoding=acvm_amd.ENC_LE32, layout=acvm_amd.LAYOUT_WITNESS_MAJOR, first=0, n=1, stride=0)
    assert L.acvm_batch_export_device_list(None, None, 16, 16, None) == E_INVALID
    assert L.acvm_batch_export_device_list(None, C.byref(good), 16, 16, None) == E_INVALID
    shifted = acvm_amd.ExportDesc(encoding=acvm_amd.ENC_LE32, layout=acvm_amd.LAYOUT_WITNESS_MAJOR, first=1, n=1, stride=0)
    assert L.acvm_batch_export_device_list(None, C.byref(shifted), 16, 16, None) == E_INVALID
    assert b"first must be 0" in L.acvm_last_error()
    bad = acvm_amd.ExportDesc(encoding=3, layout=0, first=0, n=1, stride=0)
    assert L.acvm_batch_export_device_list(None, C.byref(bad), 16, 16, None) == E_INVALID
    assert b"encoding" in L.acvm_last_error()
    assert L.acvm_debug_export_h2d_bytes(None) == 0
    assert L.acvm_debug_select(None, 0, 1, None, None) == E_INVALID


def test_python_view():
    import acvm_amd
    assert callable(acvm_amd.Batch.outcomes_device) and callable(acvm_amd.Batch.export_device_list) and callable(acvm_amd.debug_select)
    assert callable(acvm_amd.Batch.export_h2d_bytes)
    # acvm_outcomes_desc_t as the C compiler lays it out: 2 x u32, three pointers, a u32 (+ padding), a pointer
    D = acvm_amd.OutcomesDesc
    assert C.sizeof(D) == 48 and D.d_status.offset == 8 and D.select_mask.offset == 32 and D.d_selected.offset == 40
