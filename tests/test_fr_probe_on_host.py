"""The per-item switch of the acvm_debug_fr probe (acvm_amd/csrc/fr_probe.hpp is __host__ __device__) executed on the HOST over the cases of
tests/fr_ref.py, every output word compared with Python integers: the C forms of the column scans, the reductions, the lazy arithmetic, both
inversions. It proves the reference and the case generator here, before tests/test_gpu_fr_probe.py runs the same cases on a GPU (where the
scans are the asm blocks and the multiply-adds the device's own). No GPU is needed: hipcc builds the host side of tools/fr_probe_host_test.hip."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_NAMES = [n for n in fr_ref.WHATS if n not in fr_ref.DEVICE_ONLY]


def write_sections(path, names):
    """the tool's input (tools/fr_probe_host_test.hip): per launch what, n, the 18 uniform words, the items"""
    with open(path, "wb") as f:
        for name in names:
            for u, items in fr_ref.sections(name):
                np.array([fr_ref.WHATS[name][0], len(items)] + list(u or [0] * 18), dtype=np.uint32).tofile(f)
                np.array(items, dtype=np.uint32).tofile(f)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = str(tmp_path_factory.mktemp("fr_probe_host") / "fr_probe_host_test")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-x", "hip", os.path.join(ROOT, "tools", "fr_probe_host_test.hip"),
                    "-o", out], check=True, timeout=900)
    return out


def test_reference_stays_inside_the_documented_bounds():
    """every generated case of every routine: the reference's own result obeys the routine's documented output bound (fr_ref.check_bound) -- a
    wrong remark in a contract comment fails here, on integers alone"""
    for name in fr_ref.WHATS:
        fr_ref.expected(name)
        assert fr_ref.n_cases(name) >= 250, name


def test_table_of_routines_matches_the_package():
    import acvm_amd
    assert [(wi, wo) for _, wi, wo in sorted(fr_ref.WHATS.values())] == list(acvm_amd.FR_PROBE_WORDS)
    assert [w for w, _, _ in sorted(fr_ref.WHATS.values())] == list(range(len(fr_ref.WHATS)))


def test_table_of_routines_matches_the_header(exe):
    """the words in / out of every routine as acvm_amd/csrc/fr_probe.hpp has them (the tool prints its table) against the reference's"""
    r = subprocess.run([exe, "--words"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert got == sorted(fr_ref.WHATS.values())


def test_every_routine_on_host(exe, tmp_path):
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    write_sections(fin, HOST_NAMES)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    raw = np.fromfile(fout, dtype=np.uint32)
    pos = 0
    for name in HOST_NAMES:
        wo = fr_ref.WHATS[name][2]
        for k, (_, items) in enumerate(fr_ref.sections(name)):
            got = raw[pos:pos + len(items) * wo].reshape(len(items), wo)
            pos += len(items) * wo
            fr_ref.compare(name, got, k)
    assert pos == raw.size


def test_host_pass_refuses_the_table_routines(exe, tmp_path):
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    write_sections(fin, ["fr_from_byte"])
    assert subprocess.run([exe, fin, fout], capture_output=True, timeout=60).returncode == 2
