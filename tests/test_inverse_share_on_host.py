"""inverse_batch_kernel_shared<G>'s body (acvm_amd/csrc/inverse_batch.hpp is __host__ __device__) executed on the HOST: a workgroup of G waves as three
loops over its waves (every wave's prefix pass; the share step, one field inversion per lane for the G waves, through the word-major table the
kernel keeps in LDS; every wave's back-substitution), lanes and whole waves past B predicated off as in the kernel
(tools/inverse_share_host_test.hip). The cases and the assertions are those of the one-wave body (tests/inverse_batch_ref.py, Python integers),
and the table must equal the one-wave tool's (tools/inverse_batch_host_test.hip) byte for byte in every lane without a zero denominator: wave w
starts its way back from the canonical 1 / T_w either way. No GPU is needed: hipcc builds the host side of both tools."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from inverse_batch_ref import run_case, spread, zero_placements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARES = (2, 4, 8)


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    d = tmp_path_factory.mktemp("inverse_share_host")
    exe = {}
    for name in ("inverse_batch_host_test", "inverse_share_host_test"):
        exe[name] = str(d / name)
        subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-x", "hip",
                        os.path.join(ROOT, "tools", name + ".hip"), "-o", exe[name]], check=True, timeout=900)

    def backend(G):
        """G = 1: the one-wave tool"""
        def run(den, inv_chunk, slot):
            n_jobs, B = den.shape[0], den.shape[1]
            fin, fout = str(d / "in.bin"), str(d / f"out{G}.bin")
            with open(fin, "wb") as f:
                np.array([n_jobs, B, spread(n_jobs, inv_chunk)] + list(slot if slot is not None else range(n_jobs)), dtype=np.uint32).tofile(f)
                np.ascontiguousarray(den, dtype=np.uint32).tofile(f)
            cmd = [exe["inverse_batch_host_test"], fin, fout] if G == 1 else [exe["inverse_share_host_test"], fin, fout, str(G)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-1000:] + r.stderr[-1000:]
            raw = np.fromfile(fout, dtype=np.uint32)
            assert raw.size == n_jobs * B * 8 + B + 1
            return raw[:n_jobs * B * 8].reshape(n_jobs, B, 8), raw[n_jobs * B * 8:-1], (int(raw[-1]),)
        return run
    return backend


def both(tools, G):
    """a backend that runs the case through the G-wave tool and through the one-wave tool, compares the two tables in the lanes nobody flagged
    and hands the G-wave tool's result to run_case's assertions"""
    shared, single = tools(G), tools(1)

    def run(den, inv_chunk, slot):
        inv, ev, counters = shared(den, inv_chunk, slot)
        inv1, ev1, counters1 = single(den, inv_chunk, slot)
        assert (ev == ev1).all() and counters == counters1
        clean = ev == 0xFFFFFFFF
        assert clean.any()
        assert inv[:, clean].tobytes() == inv1[:, clean].tobytes()
        return inv, ev, counters
    return run


@pytest.mark.parametrize("G", SHARES)
def test_inverses(tools, G):
    backend = both(tools, G)
    for B in (1, 64, 65, 64 * G - 1, 64 * G, 64 * G + 1, 64 * G + 65):
        for inv_chunk, n_jobs in ((1, 1), (1, 3), (3, 2), (3, 7), (128, 5)):
            run_case(backend, n_jobs, B, inv_chunk, n_jobs % 2 == 1)
    run_case(backend, 129, 64 * G + 1, 128, True)


@pytest.mark.parametrize("G", SHARES)
def test_shorter_chunks_and_zero_denominators(tools, G):
    backend = both(tools, G)
    for n_jobs, inv_chunk in ((4, 3), (129, 128), (9, 4)):
        c = spread(n_jobs, inv_chunk)
        assert c < inv_chunk
        run_case(backend, n_jobs, 5, inv_chunk, True, zeros=((c, 0), (c - 1, 1), (n_jobs - 1, 2)), seed=2)
    for inv_chunk, n_jobs in ((3, 7), (128, 257), (1, 3), (3, 2)):
        for permuted in (False, True):
            run_case(backend, n_jobs, 64 * 4 + 2, inv_chunk, permuted, zeros=zero_placements(n_jobs, inv_chunk), seed=3)
    # a whole wave of zeros in one job (its total is the product of the other jobs), a lane that is zero in every job (its wave's total there is 1),
    # a zero in the only live lane of a last partial wave
    B = 64 * G + 1
    for inv_chunk, n_jobs in ((3, 7), (128, 5)):
        zeros = [(n_jobs // 2, 64 + lane) for lane in range(64)] + [(k, 7) for k in range(n_jobs)] + [(n_jobs - 1, B - 1)]
        run_case(backend, n_jobs, B, inv_chunk, True, zeros=tuple(zeros), seed=5)
