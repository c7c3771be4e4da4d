"""GPU parity of EcdsaSecp256k1 / EcdsaSecp256r1 (acvm/src/pwg/blackbox/signature/ecdsa.rs, blackbox_solver/src/lib.rs:66-210):
the reference's two vectors (lib.rs:216-284) on the device, and seeded batches of valid / tampered / high-S / panicking inputs
against the CPU oracle, through the level kernel and the exact kernel."""
import random

import pytest

from acvm_amd.acir import BlackBoxFuncCall as BB, Circuit, FunctionInput as FI
from ecdsa_ref import CURVES, public_key, sign
from test_gpu_opcodes import both_paths
from test_oracle_ecdsa import K1, R1

pytestmark = pytest.mark.gpu


def ecdsa_circuit(curve, n_x=32, n_y=32, n_sig=64, n_msg=32):
    ids = list(range(1, n_x + n_y + n_sig + n_msg + 1))
    x, y, sig, msg = ids[:n_x], ids[n_x:n_x + n_y], ids[n_x + n_y:n_x + n_y + n_sig], ids[n_x + n_y + n_sig:]
    op = BB("EcdsaSecp256k1" if curve == 0 else "EcdsaSecp256r1",
            {"public_key_x": [FI(w, 8) for w in x], "public_key_y": [FI(w, 8) for w in y], "signature": [FI(w, 8) for w in sig],
             "hashed_message": [FI(w, 8) for w in msg], "output": ids[-1] + 1})
    return Circuit(ids[-1] + 1, [op]), ids


def row(x, y, sig, z):
    return list(x) + list(y) + list(sig) + list(z)


@pytest.mark.parametrize("curve,v", [(0, K1), (1, R1)])
def test_reference_vectors_on_device(oracle, curve, v):
    circ, ids = ecdsa_circuit(curve)
    good = row(*[bytes.fromhex(v[k]) for k in ("x", "y", "sig", "z")])
    bad = list(good)
    bad[70] ^= 1
    ores, _ = both_paths(oracle, circ, ids, [good, bad])
    assert ores[0].status == 0 and ores[1].status == 0
    import acvm_amd
    from acvm_amd.synth import values_from_rows
    batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), 2, ids)
    batch.set_initial_witness(values_from_rows([good, bad]))
    assert batch.solve() == 0
    vals, asg = batch.witness(ids[-1] + 1)
    assert [int(vals[j, 31]) for j in range(2)] == [1, 0]


@pytest.mark.parametrize("curve", [0, 1])
def test_batch_against_oracle(oracle, curve):
    r = random.Random(40 + curve)
    c = CURVES[curve]
    be = lambda v: int(v).to_bytes(32, "big")  # noqa: E731
    rows = []
    for i in range(10):
        sk, k, z = r.randrange(1, c["n"]), r.randrange(1, c["n"]), r.randrange(c["n"])
        Q = public_key(curve, sk)
        rr, ss = sign(curve, sk, k, z, low_s=(i % 5 != 4))
        rows.append(row(be(Q[0]), be(Q[1]), be(rr) + be(ss), be(z)))
        rows.append(row(be(Q[0]), be(Q[1] ^ 2), be(rr) + be(ss), be(z)))       # only the parity of y matters
        rows.append(row(be(Q[0]), be(Q[1] ^ 1), be(rr) + be(ss), be(z)))
        rows.append(row(be(Q[0]), be(Q[1]), be(rr) + be(ss), be(z ^ 4)))
    Q = public_key(curve, 7)
    rows += [row(be(Q[0]), be(Q[1]), be(0) + be(1), be(5)), row(be(Q[0]), be(Q[1]), be(1) + be(c["n"]), be(5)),
             row(be(c["p"]), be(1), be(1) + be(1), be(5)), row(be(5 if curve == 0 else 0), be(1), be(1) + be(1), be(5)),
             row(be(Q[0]), be(Q[1]), be(1) + be(1), be(c["n"]))]
    rows.append([300 + b for b in rows[0]])  # witnesses above 255: only the last byte of each counts (to_u8_vec)
    circ, ids = ecdsa_circuit(curve)
    # the panic paths (rows 40..44): status, error kind and opcode are pinned by the call sites of blackbox_solver/src/lib.rs:120-129;
    # the message TEXT both sides report is UNPINNED (the reference's is k256 / p256's unwrap text)
    ores, _ = both_paths(oracle, circ, ids, rows)
    assert ores[0].status == 0 and ores[40].err == oracle.E_PANIC and ores[44].err == oracle.E_PANIC


@pytest.mark.parametrize("curve", [0, 1])
def test_batch_size_across_the_workgroup_boundary(oracle, curve):
    """the record kernel runs in workgroups of four waves (256 instances): 321 instances = one full workgroup, one full wave and a partly filled one"""
    from acvm_amd import synth
    import numpy as np
    v = (K1, R1)[curve]
    good = row(*[bytes.fromhex(v[k]) for k in ("x", "y", "sig", "z")])
    rows = []
    for i in range(321):
        r = list(good)
        if i % 5 == 3: r[128 + (i % 32)] ^= 1 << (i % 8)   # a flipped digest bit: invalid
        if i % 11 == 7: r[32 + 31] ^= 2                     # another y of the same parity: still the same key
        rows.append(r)
    circ, ids = ecdsa_circuit(curve)
    ores, _ = both_paths(oracle, circ, ids, rows)
    assert ores[0].status == 0


def test_wrong_lengths_and_short_digest(oracle):
    for kw in (dict(n_x=31), dict(n_y=33), dict(n_sig=63), dict(n_msg=31)):
        circ, ids = ecdsa_circuit(0, **kw)
        rows = [[1] * len(ids)] * 2
        ores, _ = both_paths(oracle, circ, ids, rows)
        assert ores[0].status == 2


# ---- the exceptional paths of secp_device.hpp as opcodes (tests/secp_cases.py, built for the device's 16-bit generator windows)
def case_row(x):
    r, s, qx, qy, z = x.sig
    be = lambda v: int(v).to_bytes(32, "big")  # noqa: E731
    return row(be(qx), be(qy), be(r) + be(s), be(z))


SPECIAL_AT = (0, 63, 64, 130, 1, 65, 127, 129)  # doubling, cancel + re-entry, final identity, z = 0: the first and last lanes of the waves; then the recodings


def rows_with_rare_lanes(curve, B=131):
    """B rows of ordinary valid signatures with the eight special cases in single lanes, and verify_model's outcome of every row"""
    import secp_cases as sc
    from test_secp_device_on_host import CURVES as CV, verify_model
    r = random.Random(70 + curve)
    c = CURVES[curve]
    be = lambda v: int(v).to_bytes(32, "big")  # noqa: E731
    ordinary = []
    for _ in range(6):
        sk, k, z = r.randrange(1, c["n"]), r.randrange(1, c["n"]), r.randrange(c["n"])
        Q = public_key(curve, sk)
        rr, ss = sign(curve, sk, k, z)
        ordinary.append((row(be(Q[0]), be(Q[1]), be(rr) + be(ss), be(z)), verify_model(CV[curve], rr, ss, Q[0], Q[1] & 1, 32, z)))
    special = sc.special_rows(curve, 16)
    at = dict(zip(SPECIAL_AT, special))
    rows, want = [], []
    for i in range(B):
        if i in at:
            rr, ss, qx, qy, z = at[i].sig
            rows.append(case_row(at[i]))
            want.append(verify_model(CV[curve], rr, ss, qx, qy & 1, 32, z))
        else:
            rows.append(ordinary[i % 6][0])
            want.append(ordinary[i % 6][1])
    return rows, want


@pytest.mark.parametrize("curve", [0, 1])
def test_rare_branches_in_single_lanes(oracle, curve):
    """131 rows = two full waves and three lanes. Rows 0, 63, 64 and 130 verify a signature whose generator window doubles inside the complete addition,
    one that cancels and re-enters from the identity, one whose sum IS the identity, and one with z = 0 (no generator addition); four more lanes take the
    extreme recodings of u2. Every other lane of those waves takes the common path. The oracle and the integer model are independent of each other and
    of the device: all three must agree."""
    from acvm_amd.synth import values_from_rows
    rows, want = rows_with_rare_lanes(curve)
    assert want[0] == want[63] == want[130] == (1, 0) and want[64] == (0, 5) and all(w == (1, 0) for i, w in enumerate(want) if i != 64)
    circ, ids = ecdsa_circuit(curve)
    out = ids[-1] + 1
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(circ.to_bytes()), ids, values_from_rows(rows), len(rows))
    for j, (res, panic) in enumerate(want):  # the oracle against the model, row by row
        if panic:
            assert ores[j].status == 2 and ores[j].err == oracle.E_PANIC and ores[j].aux1 == panic, (j, ores[j].as_tuple())
        else:
            assert ores[j].status == 0 and oasg[j, out] and int(ovals[j, out, 31]) == res and not ovals[j, out, :31].any(), (j, ores[j].as_tuple())
    assert ores[64].err == oracle.E_PANIC and ores[64].aux1 == 5 and b"identity" in ores[64].message
    assert all(ores[j].status == 0 and int(ovals[j, out, 31]) == 1 for j in (0, 63, 130))
    both_paths(oracle, circ, ids, rows)  # the device against the oracle, bit for bit: level kernel and exact kernel


@pytest.mark.parametrize("curve", [0, 1])
def test_output_conflict(oracle, curve):
    """the output witness is also an initial witness (insert_value, pwg/mod.rs:338-357): equal to the result -> Solved, different -> UnsatisfiedConstrain"""
    import secp_cases as sc
    circ, ids = ecdsa_circuit(curve)
    good = case_row(sc.special_rows(curve, 16)[0])  # (a valid signature: the doubling inside the addition)
    bad = list(good)
    bad[32 + 32 + 64 + 31] ^= 1                       # a flipped digest bit: invalid
    rows = [good + [1], good + [0], bad + [0], bad + [1], good + [2]]
    ores, _ = both_paths(oracle, circ, ids + [ids[-1] + 1], rows)
    assert [ores[j].status for j in range(5)] == [0, 2, 0, 2, 2]
    assert all(ores[j].err == oracle.E_UNSATISFIED for j in (1, 3, 4))
