"""The import kernel (kernels.hip import_witness_kernel: from_be_bytes_reduce of the caller's 256-bit strings, Montgomery rows, byte planes) pinned
directly, against Python integers -- int.from_bytes(x, "big") % P -- and, where a circuit reads what the import wrote, against the CPU oracle.

Read-back circuit: n_in initial witnesses and one gate per input, w[n_in + k] = 3 w[k] + 1. The initial witnesses read back check the round trip,
the gate outputs check that the row really is x R mod p (a row that is x' R for some x' = x mod 2^29, or a non-canonical one, gives another
product). Covered: the quotient-estimate reduction at the multiples of p and at the thresholds of its top-limb comparison, the wave-uniform byte
shortcut with one lane that is no byte, the byte-plane word of values whose low 29 bits look like a byte, and caller pointers that are not 16-byte
aligned (import_witness_kernel<false>), as acvm_batch_set_initial_witness_device and as acvm_batch_solve_then_import's next buffer."""
import functools

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import Circuit, Expression as E, P

pytestmark = pytest.mark.gpu


def _edge_values():
    """the reduction's edges: around every multiple of p below 2^256, and the top limb on / beside each threshold k * p7 of the quotient estimate
    (p7 = p's top limb + 1), once with the 224 bits below it all zero and once all one; then the powers of two and the byte / plane-word boundaries"""
    p7 = (P >> 224) + 1
    vals = [k * P + d for k in range(6) for d in (-2, -1, 0, 1, 2)]
    low = (1 << 224) - 1
    vals += [((k * p7 + d) << 224) | fill for k in range(6) for d in (-1, 0, 1) if k * p7 + d >= 0 for fill in (0, low)]
    vals += [(1 << 256) - 1, 1 << 255, 1 << 254, 1 << 253, 255, 256, 257, (1 << 29) - 1, 1 << 29, (1 << 32) - 1, 1 << 32]
    out = []
    for v in vals:
        if 0 <= v < (1 << 256) and v not in out:
            out.append(v)
    return out


EDGE = _edge_values()


def _edge_rows(B, n_in, rot=0):
    """cell (instance j, input k) = EDGE[(j + k + rot) % 72]"""
    return [[EDGE[(j + k + rot) % len(EDGE)] for k in range(n_in)] for j in range(B)]


@functools.lru_cache(maxsize=None)
def _readback_circuit(n_in):
    ops = [E([], [(3, k), (P - 1, n_in + k)], 1) for k in range(1, n_in + 1)]
    return acvm_amd.Circuit(Circuit(2 * n_in, ops).to_bytes())


def _be(rows):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for r in rows for v in r), dtype=np.uint8).reshape(len(rows), -1, 32)


def _assert_read_back(batch, rows, what=""):
    """every initial witness reads back as x mod p and every gate output as 3 (x mod p) + 1 mod p, for every instance"""
    B, n_in = len(rows), len(rows[0])
    res = batch.results()
    assert all(r.status == acvm_amd.STATUS_SOLVED for r in res), what
    want_in = _be([[x % P for x in r] for r in rows])
    want_out = _be([[(3 * (x % P) + 1) % P for x in r] for r in rows])
    for k in range(n_in):
        for w, want, name in ((1 + k, want_in, "initial witness"), (1 + n_in + k, want_out, "gate output")):
            vals, asg = batch.witness(w)
            assert asg.all(), (what, w)
            bad = np.nonzero((vals != want[:, k]).any(axis=1))[0]
            assert bad.size == 0, (f"{what}: {name} {w} of instance {bad[0]} (input {rows[bad[0]][k]:#x}) is {vals[bad[0]].tobytes().hex()}, "
                                   f"expected {want[bad[0], k].tobytes().hex()} ({bad.size} instances differ)")


def _solve_rows(rows, what=""):
    B, n_in = len(rows), len(rows[0])
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    batch.set_initial_witness(synth.values_from_rows(rows))
    assert batch.solve() == 0, what
    _assert_read_back(batch, rows, what)
    return batch


def test_edge_value_set():
    """the set the issue describes: 72 values; and (host arithmetic only) the claim the kernel's single conditional subtraction rests on"""
    assert len(EDGE) == 72 and len(set(EDGE)) == 72
    p7 = (P >> 224) + 1
    for v in EDGE:
        q = sum(1 for k in range(1, 6) if (v >> 224) >= k * p7)
        assert v // P - q in (0, 1), hex(v)


# each n_in (a full group of four inputs, ragged last groups, more than two groups) and each B (one instance, below / on / above one block, three
# blocks with a ragged last one) at least once
@pytest.mark.parametrize("n_in,B", [(1, 130), (2, 63), (3, 64), (4, 65), (5, 1), (9, 130), (4, 1), (5, 63)])
def test_reduction_edges_shapes(n_in, B):
    _solve_rows(_edge_rows(B, n_in), f"n_in {n_in} B {B}").free()


def test_every_edge_value_in_every_place():
    """every edge value at input position 0, at a position k with k % 4 != 0 and in the last instance of a ragged batch (65 = one block and one
    instance): eight rotations of the layout through one handle"""
    n_in, B = 9, 65
    at0, off4, last = set(), set(), set()
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    for rot in range(0, 72, 9):
        rows = _edge_rows(B, n_in, rot)
        at0 |= {r[0] for r in rows}
        off4 |= {r[k] for r in rows for k in range(n_in) if k % 4}
        last |= set(rows[-1])
        batch.set_initial_witness(synth.values_from_rows(rows))
        assert batch.solve() == 0
        _assert_read_back(batch, rows, f"rotation {rot}")
    batch.free()
    assert at0 == off4 == last == set(EDGE)


def _random_values(rng, n):
    return [int.from_bytes(rng.bytes(32), "big") for _ in range(n)]


@pytest.mark.parametrize("odd_one", [None, 256, P + 200, (1 << 256) - 1])
def test_byte_shortcut_is_decided_per_wave(odd_one):
    """A wave converts 16 consecutive instances x 4 inputs and takes the closed form for bytes only when every value it converts is one AFTER the
    reduction. Waves of bytes (0 and 255 among them): instances [0, 16), [112, 128) and the two live instances of the ragged last wave; beside each
    a wave of random values. Then the same with exactly one value of each byte wave replaced: 256 and 2^256 - 1 (no bytes: the whole wave takes the
    product), p + 200 (a byte once reduced: the wave still takes the closed form, with the reduced value)."""
    B, n_in = 130, 4
    rng = np.random.default_rng(0xB17E)
    rows = [_random_values(rng, n_in) for _ in range(B)]
    byte_waves = (range(0, 16), range(112, 128), range(128, 130))
    for wave in byte_waves:
        for j in wave:
            rows[j] = [int(b) for b in rng.integers(0, 256, n_in)]
        rows[wave[0]][:2] = [0, 255]
        rows[wave[-1]][2:] = [255, 0]
    if odd_one is not None:
        for wave, (j, k) in zip(byte_waves, ((5, 2), (127, 0), (129, 3))):
            assert j in wave
            rows[j][k] = odd_one
    _solve_rows(rows, f"odd one {odd_one}").free()


def _assert_oracle_parity(oracle, data, ids, values, B, want_planes):
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values, B)
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), B, ids)
    if want_planes is not None:
        assert batch.stats()["n_byte_planes"] == want_planes
    batch.set_initial_witness(values)
    batch.solve()
    res = batch.results()
    for j in range(B):
        assert res[j].as_tuple() == ores[j].as_tuple(), f"instance {j}: {res[j].as_tuple()}, the oracle's {ores[j].as_tuple()}"
    asg, vals = batch.witness_map()
    nw = min(oasg.shape[1], asg.shape[1])
    assert np.array_equal(asg[:, :nw], oasg[:, :nw]), "assigned sets differ"
    bad = np.argwhere((vals[:, :nw] != ovals[:, :nw]).any(axis=2))
    assert bad.size == 0, f"witness {bad[0][1]} of instance {bad[0][0]} differs from the oracle's ({len(bad)} differ)"
    batch.free()
    return ores


@pytest.mark.parametrize("with_range", [True, False])
def test_byte_plane_words_of_values_that_look_like_bytes(oracle, with_range):
    """SHA256 and Keccak256 over initial witnesses read the 4-byte plane word the import writes (low 29 bits | is-byte << 31) instead of the row.
    p + b is the byte b once reduced and is hashed as b; 256 is no byte; 2^29 + 7, 2^32 + 7 and 2^253 + 7 are no bytes although their low 29 bits
    are the byte 7 -- they must not be hashed as 7. With the RANGE checks they fail there; without, the hash opcode sees them."""
    n_msg, B = 5, 70
    circ, ids = synth.hash_circuit(n_msg=n_msg, with_range=with_range)
    n_in = len(ids)
    data = circ.to_bytes()
    values = np.frombuffer(synth.byte_batch(B, n_in), dtype=np.uint8).reshape(B, n_in, 32).copy()

    def put(j, k, v):
        values[j, k] = np.frombuffer(int(v).to_bytes(32, "big"), dtype=np.uint8)

    sent = int(values[3, 2, 31])
    put(3, 2, P + sent)                           # a message byte sent unreduced
    put(5, n_msg + 4, 256)                        # one of the Keccak inputs
    put(7, 1, (1 << 29) + 7)
    put(9, 4, (1 << 32) + 7)
    put(11, 0, (1 << 253) + 7)
    raw = values.tobytes()
    ores = _assert_oracle_parity(oracle, data, ids, raw, B, want_planes=n_in)
    assert ores[3].status == 0 and all(ores[j].status == 0 for j in range(B) if j not in (3, 5, 7, 9, 11))
    # the reference hashes instance 3 as if the byte itself had been sent
    plain = values.copy()
    plain[3, 2] = 0
    plain[3, 2, 31] = sent
    pres, pasg, pvals = oracle.solve_batch(oracle.Circuit(data), ids, plain[3:4].tobytes(), 1)
    _, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values[3:4].tobytes(), 1)
    assert pres[0].status == 0 and np.array_equal(pvals, ovals)
    with acvm_amd.tuning(byte_plane=0):
        _assert_oracle_parity(oracle, data, ids, raw, B, want_planes=0)


def _whole_state(batch):
    asg, vals = batch.witness_map()
    return [r.as_tuple() for r in batch.results()], asg, vals


@pytest.mark.parametrize("off", [1, 4, 8])
def test_unaligned_device_pointer(off):
    """a caller's device pointer that is not 16-byte aligned takes import_witness_kernel<false> (byte loads): results and the whole map equal the
    aligned run's bit for bit, on the reduction-edge inputs; the same pointer as acvm_batch_solve_then_import's next buffer"""
    n_in, B = 5, 65
    rows = _edge_rows(B, n_in)
    values = synth.values_from_rows(rows)
    aligned = _solve_rows(rows, "aligned")
    want = _whole_state(aligned)
    aligned.free()
    buf = acvm_amd.DeviceBuffer(size=len(values) + 16)
    buf.upload(values, offset=off)
    assert buf.ptr % 16 == 0 and (buf.ptr + off) % 16 == off
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    batch.set_initial_witness_device(buf.ptr + off)
    assert batch.solve() == 0
    _assert_read_back(batch, rows, f"offset {off}")
    got = _whole_state(batch)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    batch.free()
    # behind a solve of other (clean) inputs, as the next tile
    rng = np.random.default_rng(off)
    first = [_random_values(rng, n_in) for _ in range(B)]
    batch = acvm_amd.Batch(_readback_circuit(n_in), B, list(range(1, n_in + 1)))
    batch.set_initial_witness(synth.values_from_rows(first))
    assert batch.solve(then_import=buf.ptr + off) == 0
    batch.set_initial_witness_device(buf.ptr + off)
    assert batch.solve() == 0
    _assert_read_back(batch, rows, f"offset {off}, imported behind a solve")
    got = _whole_state(batch)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    batch.free()
    buf.free()
