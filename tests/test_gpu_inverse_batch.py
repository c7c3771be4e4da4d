"""The inversion batch of the level schedule (inverse_batch_kernel through launch_inverse_batch, exactly as a solve starts it) run directly, through
the acvm_debug_inverse_batch probe, against Python integers: the prefix-product pass, the packed prefixes parked in the jobs' own inverse slots,
the last, shorter chunk, the launcher's even spreading of jobs over chunks, the second launch past grid.y's 65 535 chunks, and the flagging of
instances with a zero denominator, counted on the device and in the host's counter. The cases and what is asserted: tests/inverse_batch_ref.py
(the same run on the host: tests/test_inverse_batch_on_host.py)."""
import pytest

from inverse_batch_ref import job_counts, run_case, spread, zero_placements

pytestmark = pytest.mark.gpu


def device(den, inv_chunk, slot):
    import acvm_amd
    inv, ev, dcount, hcount = acvm_amd.debug_inverse_batch(den, inv_chunk, slot)
    return inv, ev, (dcount, hcount)


@pytest.mark.parametrize("inv_chunk", [1, 3, 128])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_inverses(B, inv_chunk):
    for n_jobs in job_counts(inv_chunk):
        for permuted in (False, True):
            run_case(device, n_jobs, B, inv_chunk, permuted)


@pytest.mark.parametrize("B", [1, 65, 130])
def test_even_spread_makes_chunks_shorter_than_inv_chunk(B):
    for n_jobs, inv_chunk in ((4, 3), (129, 128), (9, 4)):
        assert spread(n_jobs, inv_chunk) < inv_chunk
        run_case(device, n_jobs, B, inv_chunk, True, seed=1)
        # a zero in the first and in the last job of the shorter chunks: the chunk boundaries are where the launcher put them
        c = spread(n_jobs, inv_chunk)
        if B >= 3:
            run_case(device, n_jobs, B, inv_chunk, False, zeros=((c, 0), (c - 1, 1), (n_jobs - 1, 2)), seed=2)


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("inv_chunk,n_jobs", [(3, 7), (128, 257), (1, 3), (3, 2)])
def test_zero_denominators_flag_their_instances(inv_chunk, n_jobs, permuted):
    run_case(device, n_jobs, 64 * 4 + 2, inv_chunk, permuted, zeros=zero_placements(n_jobs, inv_chunk), seed=3)  # five waves, the last one two lanes wide


def test_second_launch_past_the_grid_limit():
    """inv_chunk = 1 and 65 536 + 3 jobs: the only thing that executes the launcher's second launch (about 2 x 135 MB of device memory)"""
    run_case(device, 65536 + 3, 1, 1, False, seed=4)
