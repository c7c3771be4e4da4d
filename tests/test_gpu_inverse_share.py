"""The inversion batch with ONE field inversion for the corresponding lanes of G waves (inverse_batch_kernel_shared<G> through launch_inverse_batch,
tuning key inv_share), run directly through the acvm_debug_inverse_batch_shared probe against Python integers (tests/inverse_batch_ref.py): batch
sizes around the wave and the workgroup of G waves (lanes and whole waves of the last block predicated off, never returning before the barriers),
chunks of one job, short last chunks, zero denominators that make a wave's total 1 or sit in the only live lane of a wave; the table against the
one-wave kernel's, byte for byte in every lane without a zero; and whole solves of an inversion-heavy circuit with every inv_share against the
oracle. The same body on the host: tests/test_inverse_share_on_host.py."""
import numpy as np
import pytest

from inverse_batch_ref import NONE, POOL, run_case, zero_placements

pytestmark = pytest.mark.gpu

SHARES = (2, 4, 8)
JOBS = ((1, 1), (1, 3), (3, 2), (3, 7), (128, 5), (128, 129))  # (inv_chunk, n_jobs)


def device(G):
    def backend(den, inv_chunk, slot):
        import acvm_amd
        inv, ev, dcount, hcount = acvm_amd.debug_inverse_batch(den, inv_chunk, slot, inv_share=G)
        return inv, ev, (dcount, hcount)
    return backend


def sizes(G):
    return sorted({1, 64, 65, 64 * G - 1, 64 * G, 64 * G + 1, 64 * G + 65})


@pytest.mark.parametrize("G,B", [(G, B) for G in SHARES for B in sizes(G)])
def test_inverses(G, B):
    for inv_chunk, n_jobs in JOBS:
        for permuted in (False, True):
            run_case(device(G), n_jobs, B, inv_chunk, permuted)


@pytest.mark.parametrize("G", SHARES)
def test_zero_denominators_flag_their_instances(G):
    for inv_chunk, n_jobs in ((3, 7), (128, 257), (1, 3), (3, 2)):
        for permuted in (False, True):
            run_case(device(G), n_jobs, 64 * 4 + 2, inv_chunk, permuted, zeros=zero_placements(n_jobs, inv_chunk), seed=3)
    # every lane of one whole wave zero in some job; one lane zero in every job (its wave's total there is 1); a zero in the only live lane of the
    # last, partial wave (B = 64 G + 1: the second block is that lane and G - 1 waves without any)
    B = 64 * G + 1
    for inv_chunk, n_jobs in ((3, 7), (128, 5), (1, 3)):
        zeros = [(n_jobs // 2, 64 + lane) for lane in range(64)] + [(k, 7) for k in range(n_jobs)] + [(n_jobs - 1, B - 1)]
        run_case(device(G), n_jobs, B, inv_chunk, True, zeros=tuple(zeros), seed=5)


@pytest.mark.parametrize("G", SHARES + (0, 3, 5, 100))
def test_table_equals_the_one_wave_kernels(G):
    """inv_share = G against inv_share = 1 on the same inputs: the same bytes in every lane without a zero (values other than 1, 2, 4, 8 are the
    next lower of those)"""
    import acvm_amd
    g = max(G, 2)
    for (inv_chunk, n_jobs), B in zip(JOBS, (64 * g + 65, 65, 64 * g - 1, 64 * g + 1, 130, 64 * g)):
        den = [[POOL[(7 * k + 3 * j) % len(POOL)] for j in range(B)] for k in range(n_jobs)]
        for k, j in ((0, 0), (n_jobs - 1, B - 1), (n_jobs // 2, 70)):
            if j < B:
                den[k][j] = 0
        arr = np.frombuffer(b"".join(v.to_bytes(32, "little") for row in den for v in row), dtype="<u4").reshape(n_jobs, B, 8)
        slot = [(k * 5 + 1) % n_jobs for k in range(n_jobs)] if n_jobs % 5 else None
        inv, ev, dc, hc = acvm_amd.debug_inverse_batch(arr, inv_chunk, slot, inv_share=G)
        inv1, ev1, dc1, hc1 = acvm_amd.debug_inverse_batch(arr, inv_chunk, slot, inv_share=1)
        assert (ev == ev1).all() and (dc, hc) == (dc1, hc1)
        clean = ev == NONE
        assert clean.sum() >= B - 3 and (clean.any() or B == 1)
        assert inv[:, clean].tobytes() == inv1[:, clean].tobytes()


def test_the_plain_probe_follows_the_process_wide_inv_share():
    import acvm_amd
    for G in (1, 4):
        with acvm_amd.tuning(inv_share=G):
            def backend(den, inv_chunk, slot):
                inv, ev, dcount, hcount = acvm_amd.debug_inverse_batch(den, inv_chunk, slot)
                return inv, ev, (dcount, hcount)
            run_case(backend, 7, 64 * 4 + 65, 3, True, zeros=((2, 1), (6, 300)), seed=6)


# ---- whole solves: an inversion-heavy arithmetic circuit, every inv_share, against the oracle
N_IN = 16


@pytest.fixture(scope="module")
def heavy(oracle):
    """the circuit, and per batch size the inputs (one planted zero denominator, in the last instance) and the oracle's answer"""
    from acvm_amd import synth
    circ, ids = synth.arithmetic_circuit(300, mix=(20, 20, 20, 40))
    # the first gate whose unknown is multiplied by an INPUT witness: that input = 0 makes its denominator vanish
    at, partner = next((i, t[1]) for i, e in enumerate(circ.opcodes) for t in e.mul_terms if t[2] == N_IN + 1 + i and t[1] <= N_IN)
    data = circ.to_bytes()
    cases = {}
    for B in (130, 300):
        values = bytearray(synth.witness_batch(B, edge_cases=False))
        off = ((B - 1) * N_IN + partner - 1) * 32
        values[off:off + 32] = bytes(32)
        values = bytes(values)
        cases[B] = (values, oracle.solve_batch(oracle.Circuit(data), ids, values, B))
    return data, ids, cases


@pytest.mark.parametrize("inv_chunk", [3, 128])
@pytest.mark.parametrize("inv_share", [1, 2, 4, 8])
def test_whole_solve_parity(heavy, inv_share, inv_chunk):
    import acvm_amd
    data, ids, cases = heavy
    with acvm_amd.tuning(inv_share=inv_share, inv_chunk=inv_chunk):
        for B, (values, (ores, oasg, ovals)) in cases.items():
            batch = acvm_amd.Batch(acvm_amd.Circuit(data), B, ids)
            batch.set_initial_witness(values)
            batch.solve()
            gres = batch.results()
            gasg, gvals = batch.witness_map()
            st = batch.stats()
            batch.free()
            for j in range(B):
                assert gres[j].as_tuple() == ores[j].as_tuple(), (B, j, gres[j].as_tuple(), ores[j].as_tuple())
            nw = min(oasg.shape[1], gasg.shape[1])
            assert np.array_equal(oasg[:, :nw], gasg[:, :nw]), "assigned sets differ"
            assert np.array_equal(ovals[:, :nw], gvals[:, :nw]), "witness values differ"
            assert st["n_dyn_gates"] >= 60 and st["n_slow_instances"] == 1  # the planted zero denominator, and nothing else, took the exact path
