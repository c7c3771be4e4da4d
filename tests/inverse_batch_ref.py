"""Cases and assertions for the inversion batch (inverse_batch_kernel's body, acvm_amd/csrc/inverse_batch.hpp), shared by the run on the device
(tests/test_gpu_inverse_batch.py, through launch_inverse_batch) and the run of the same body on the host (tests/test_inverse_batch_on_host.py).
Python integers are the spec. A lane without a zero denominator: every row v of the inverse table has v den = R^2 (mod p) -- 1 / den in the
storage form's Montgomery sense --, v < 2^256 by its eight words, and 256 v < GATE_K_INVERSE p, the bound plan.cpp feeds into the gate that
reads the row (gate_record.hpp). A lane with a zero: its event word is the smallest opcode among its zero jobs and it is counted exactly once, in
every counter; its inverse rows are unspecified (the exact path owns the lane). Every other event word stays 0xFFFFFFFF. Test infrastructure only."""
import random

import numpy as np

from fr_ref import P, R1, R2, GATE_K_INVERSE

RNG = random.Random(0x1BA7C4)
POOL = [1, P - 1, R1, 2, P - 2, (1 << 253), (1 << 232) - 1] + [RNG.randrange(1, P) for _ in range(300)]  # canonical, non-zero
NONE = 0xFFFFFFFF


def spread(n_jobs, inv_chunk):
    """jobs per chunk after the launcher's even spreading (kernels.hip launch_inverse_batch)"""
    n_chunks = -(-n_jobs // inv_chunk)
    return -(-n_jobs // n_chunks)


def job_counts(chunk):
    return sorted({n for n in (1, 2, chunk - 1, chunk, chunk + 1, 2 * chunk + 1) if n >= 1})


def zero_placements(n_jobs, inv_chunk):
    """(job, lane) pairs for a batch of 64 * 4 + 2 lanes: zeros at the first / a middle / the last job of a chunk, in every job of one lane, in every
    lane of one wave, in one lane of each of several waves, and twice in one lane"""
    c = spread(n_jobs, inv_chunk)
    mid, last_of_chunk = min(c // 2, n_jobs - 1), min(c - 1, n_jobs - 1)
    second = min(c, n_jobs - 1)  # the first job of the second chunk (where there is one)
    zeros = [(0, 3), (second, 4), (mid, 5), (last_of_chunk, 6), (n_jobs - 1, 7)]
    zeros += [(k, 9) for k in range(n_jobs)]
    zeros += [((5 * j) % n_jobs, 64 + j) for j in range(64)]
    zeros += [(n_jobs - 1, 128 + 17), (0, 192 + 63), (mid, 256 + 1)]
    zeros += [(n_jobs - 1, 11), (0, 11)] if n_jobs > 1 else []  # two zeros: the smaller opcode wins whichever is met first
    return tuple(zeros)


def run_case(backend, n_jobs, B, inv_chunk, permuted, zeros=(), seed=0):
    """backend(den uint32 [n_jobs][B][8], inv_chunk, slot list or None) -> (rows [n_jobs][B][8], event words [B], the counters, a tuple);
    zeros: (job, lane) pairs whose denominator is 0"""
    rng = random.Random(seed * 1000003 + n_jobs * 131 + B * 7 + inv_chunk)
    den = [[POOL[(3 * k + 5 * j + rng.randrange(4)) % len(POOL)] for j in range(B)] for k in range(n_jobs)]
    if n_jobs * B >= 3:  # the named denominators wherever the pool's walk does not reach them
        den[0][0], den[-1][-1], den[n_jobs // 2][B // 2] = 1, P - 1, R1
    for k, j in zeros:
        den[k][j] = 0
    arr = np.frombuffer(b"".join(v.to_bytes(32, "little") for row in den for v in row), dtype="<u4").reshape(n_jobs, B, 8)
    slot = None
    if permuted:
        slot = list(range(n_jobs))
        rng.shuffle(slot)
    inv, ev, counters = backend(arr, inv_chunk, slot)
    raw = np.ascontiguousarray(inv).astype("<u4").tobytes()
    first_zero = {}
    for k, j in sorted(zeros):
        first_zero.setdefault(j, k)
    want_ev = np.full(B, NONE, dtype=np.uint32)
    for j, k in first_zero.items():
        want_ev[j] = k
    assert (ev == want_ev).all(), (np.nonzero(ev != want_ev)[0][:8], ev[ev != want_ev][:8])
    assert all(c == len(first_zero) for c in counters), (counters, len(first_zero))
    for k in range(n_jobs):
        row = slot[k] if slot else k
        for j in range(B):
            if j in first_zero:
                continue
            off = 32 * (row * B + j)
            v = int.from_bytes(raw[off:off + 32], "little")
            assert (v * den[k][j] - R2) % P == 0, (k, j, hex(den[k][j]), hex(v))
            assert 256 * v < GATE_K_INVERSE * P, (k, j, hex(v))
