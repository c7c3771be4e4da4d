"""inverse_batch_kernel's body (acvm_amd/csrc/inverse_batch.hpp is __host__ __device__) executed on the HOST over tables laid out like the
device's, with the cases and the assertions of tests/test_gpu_inverse_batch.py (tests/inverse_batch_ref.py): the prefix-product pass, the
prefixes parked in the jobs' own inverse slots, the back-substitution, the last, shorter chunk, zero denominators. The launcher's spreading is
mirrored by inverse_batch_ref.spread; the launcher itself and its second launch run on the GPU only. No GPU is needed: hipcc builds the host
side of tools/inverse_batch_host_test.hip."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from inverse_batch_ref import job_counts, run_case, spread, zero_placements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    d = tmp_path_factory.mktemp("inverse_batch_host")
    exe = str(d / "inverse_batch_host_test")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-x", "hip",
                    os.path.join(ROOT, "tools", "inverse_batch_host_test.hip"), "-o", exe], check=True, timeout=900)

    def backend(den, inv_chunk, slot):
        n_jobs, B = den.shape[0], den.shape[1]
        fin, fout = str(d / "in.bin"), str(d / "out.bin")
        with open(fin, "wb") as f:
            np.array([n_jobs, B, spread(n_jobs, inv_chunk)] + list(slot if slot is not None else range(n_jobs)), dtype=np.uint32).tofile(f)
            np.ascontiguousarray(den, dtype=np.uint32).tofile(f)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-1000:] + r.stderr[-1000:]
        raw = np.fromfile(fout, dtype=np.uint32)
        assert raw.size == n_jobs * B * 8 + B + 1
        return raw[:n_jobs * B * 8].reshape(n_jobs, B, 8), raw[n_jobs * B * 8:-1], (int(raw[-1]),)
    return backend


@pytest.mark.parametrize("inv_chunk", [1, 3, 128])
def test_inverses(host, inv_chunk):
    for B in (1, 65):
        for n_jobs in job_counts(inv_chunk):
            run_case(host, n_jobs, B, inv_chunk, n_jobs % 2 == 1)


def test_shorter_chunks_and_zero_denominators(host):
    for n_jobs, inv_chunk in ((4, 3), (129, 128), (9, 4)):
        c = spread(n_jobs, inv_chunk)
        assert c < inv_chunk
        run_case(host, n_jobs, 5, inv_chunk, True, zeros=((c, 0), (c - 1, 1), (n_jobs - 1, 2)), seed=2)
    for inv_chunk, n_jobs in ((3, 7), (128, 257), (1, 3), (3, 2)):
        for permuted in (False, True):
            run_case(host, n_jobs, 64 * 4 + 2, inv_chunk, permuted, zeros=zero_placements(n_jobs, inv_chunk), seed=3)
