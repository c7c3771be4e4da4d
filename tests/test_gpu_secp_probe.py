"""The curve arithmetic of the ECDSA kernels (acvm_amd/csrc/secp_device.hpp) run ON THE DEVICE against Python integers, through the
acvm_debug_secp probes: the same cases tests/test_secp_device_on_host.py runs through the host build of that header. The reference's
arithmetic is k256 0.11.6 / p256 0.11.1 behind blackbox_solver/src/lib.rs:66-210; integers modulo the two primes are the spec."""
import random

import pytest

from test_secp_device_on_host import CURVES, affine, ec_add, ec_mul, edge_values

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", [0, 1])
def test_field_arithmetic_on_device(c):
    import acvm_amd
    p = CURVES[c]["p"]
    rng = random.Random(4000 + c)
    ev = edge_values(p)
    pairs = [(a, b) for a in ev for b in ev] + [(rng.randrange(p), rng.randrange(p)) for _ in range(4000)]
    for _ in range(2000):  # long runs of ones / zeros drive the carries of the reductions
        a = rng.choice([0, 2**256 - 1]) ^ (((1 << rng.randrange(1, 256)) - 1) << rng.randrange(0, 256))
        b = rng.choice([0, 2**256 - 1]) ^ (((1 << rng.randrange(1, 256)) - 1) << rng.randrange(0, 256))
        pairs.append((a % 2**256 % p, b % 2**256 % p))
    for what, name, f in ((0, "mul", lambda a, b: a * b % p), (2, "add", lambda a, b: (a + b) % p), (3, "sub", lambda a, b: (a - b) % p)):
        got = acvm_amd.debug_secp(c, what, pairs)
        bad = [(name, hex(a), hex(b), hex(g[0]), hex(f(a, b))) for (a, b), g in zip(pairs, got) if g[0] != f(a, b)]
        assert not bad, bad[:3]
    for what, name, f in ((9, "(a+b)^2", lambda a, b: (a + b) ** 2 % p), (10, "a-4b", lambda a, b: (a - 4 * b) % p)):
        got = acvm_amd.debug_secp(c, what, pairs)
        bad = [(name, hex(a), hex(b), hex(g[0]), hex(f(a, b))) for (a, b), g in zip(pairs, got) if g[0] != f(a, b)]
        assert not bad, bad[:3]
    ones = [(a,) for a, _ in pairs]
    for what, e in ((8, 4), (11, 32)):
        got = acvm_amd.debug_secp(c, what, ones)
        bad = [(f"a^{e}", hex(a), hex(g[0]), hex(pow(a, e, p))) for (a,), g in zip(ones, got) if g[0] != pow(a, e, p)]
        assert not bad, bad[:3]
    got = acvm_amd.debug_secp(c, 1, ones)
    bad = [("sqr", hex(a), hex(g[0])) for (a,), g in zip(ones, got) if g[0] != a * a % p]
    assert not bad, bad[:3]
    got = acvm_amd.debug_secp(c, 4, ones[:600])
    bad = [("inv", hex(a), hex(g[0])) for (a,), g in zip(ones[:600], got) if g[0] != (pow(a, -1, p) if a else 0)]
    assert not bad, bad[:3]
    sq = [(a * a % p,) for a, _ in pairs[200:500]]
    got = acvm_amd.debug_secp(c, 5, sq)
    bad = [("sqrt", hex(a), hex(g[0])) for (a,), g in zip(sq, got) if g[0] != pow(a, (p + 1) // 4, p)]
    assert not bad, bad[:3]


@pytest.mark.parametrize("c", [0, 1])
def test_point_formulas_on_device(c):
    import acvm_amd
    cv = CURVES[c]
    p, n = cv["p"], cv["n"]
    rng = random.Random(5000 + c)
    dbl, add, want_d, want_a = [], [], [], []
    for it in range(300):
        P, Q = ec_mul(cv, rng.randrange(1, n), cv["g"]), ec_mul(cv, rng.randrange(1, n), cv["g"])
        z = rng.randrange(1, p)
        X, Y, Z = P[0] * z * z % p, P[1] * z * z * z % p, z
        dbl.append((X, Y, Z)); want_d.append(ec_add(cv, P, P))
        if it % 10 == 0: Q = P                      # the addition that is a doubling
        if it % 10 == 1: Q = (P[0], (p - P[1]) % p)  # ... and the one that cancels
        add.append((X, Y, Z, Q[0], Q[1])); want_a.append(ec_add(cv, P, Q))
    add.append((1, 1, 0, cv["g"][0], cv["g"][1])); want_a.append(cv["g"])  # identity + G
    dbl.append((1, 1, 0)); want_d.append(None)
    for what, items, want in ((6, dbl, want_d), (7, add, want_a)):
        got = acvm_amd.debug_secp(c, what, items)
        for it, g, w in zip(items, got, want):
            assert affine(cv, *g) == w, (what, it, g)


# ---- what a verification is made of above the base field (probes 12..16), at the cases of tests/secp_cases.py built for the device's 16-bit generator
# windows: the host run of the same header (tests/test_secp_device_on_host.py) uses 8-bit ones, so its digits, window count and table differ
@pytest.mark.parametrize("c", [0, 1])
def test_scalar_field_on_device(c):
    """sn_mul (two Montgomery products) and sn_inv (safegcd over n) against integers"""
    import acvm_amd
    n = CURVES[c]["n"]
    rng = random.Random(6000 + c)
    ev = edge_values(n)
    pairs = [(a, b) for a in ev for b in ev]
    for _ in range(1000):  # long runs of ones / zeros drive the carries
        a = rng.choice([0, 2**256 - 1]) ^ (((1 << rng.randrange(1, 256)) - 1) << rng.randrange(0, 256))
        b = rng.choice([0, 2**256 - 1]) ^ (((1 << rng.randrange(1, 256)) - 1) << rng.randrange(0, 256))
        pairs.append((a % 2**256 % n, b % 2**256 % n))
    pairs += [(rng.randrange(n), rng.randrange(n)) for _ in range(2000)]
    got = acvm_amd.debug_secp(c, 12, pairs)
    bad = [("nmul", hex(a), hex(b), hex(g[0])) for (a, b), g in zip(pairs, got) if g[0] != a * b % n]
    assert not bad, bad[:3]
    ones = [(a,) for a, _ in pairs[:300]] + [(a,) for a, _ in pairs[-300:]]
    got = acvm_amd.debug_secp(c, 13, ones)
    bad = [("ninv", hex(a), hex(g[0])) for (a,), g in zip(ones, got) if g[0] != (pow(a, -1, n) if a else 0)]
    assert not bad, bad[:3]


def test_endomorphism_split_on_device():
    """every output word of secp256k1_split_lambda against libsecp256k1's rounding in integers (secp_cases.split_lambda): the 2 000-sample, in which at
    least 40 / 20 scalars use digit 128 of k1 / k2 and 40 each sign combination, and the fixed shapes. The split is secp256k1's: curve 1 is refused."""
    import acvm_amd
    import secp_cases as sc
    ks = sc.split_shapes() + list(sc.split_sample()[0])
    got = acvm_amd.debug_secp(0, 14, [(k,) for k in ks])
    bad = [(hex(k), g, sc.split_lambda(k)) for k, g in zip(ks, got) if g != sc.split_lambda(k)]
    assert not bad, bad[:3]
    with pytest.raises(acvm_amd.AcvmError):
        acvm_amd.debug_secp(1, 14, [(1,)])


@pytest.mark.parametrize("c", [0, 1])
def test_exceptional_sums_on_device(c):
    """u1 G + u2 Q through secp_mul2 with the device's own generator tables, families A..E: the generator windows colliding with the accumulator (the
    doubling inside the complete addition, the cancellation and the re-entry from the identity, the identity as the result), the shapes of u1, the
    extreme recodings of u2 (digit 128 of both halves / the carry digit), the special keys. Z = 0 exactly when the sum is the identity."""
    import acvm_amd
    import secp_cases as sc
    cv = CURVES[c]
    n, G = cv["n"], cv["g"]
    cs = sc.cases(c, 16)
    extra = [(0, 0), (1, 0), (n - 1, 0), (0, 1), (n - 1, 1), (1, n - 1)]  # u2 = 0 makes no signature; with Q = G
    items = [(x.u1, x.Q[0], x.Q[1], x.u2) for x in cs] + [(u1, G[0], G[1], u2) for u1, u2 in extra]
    want = [x.R for x in cs] + [ec_mul(cv, (u1 + u2) % n, G) for u1, u2 in extra]
    labels = [x.label for x in cs] + [f"Q = G, u1 = {u1:#x}, u2 = {u2:#x}" for u1, u2 in extra]
    assert sum(w is None for w in want) >= 3
    items, want, labels = items * 3, want * 3, labels * 3  # (three waves and a part of a fourth: the same case in different lanes)
    for label, g, w in zip(labels, acvm_amd.debug_secp(c, 15, items), want):
        assert affine(cv, *g) == w and (g[2] == 0) == (w is None), (label, g, w)


@pytest.mark.parametrize("c", [0, 1])
def test_exceptional_verifications_on_device(c):
    """secp_verify as the opcodes call it (y given) against verify_model: the signatures of families A..E with the key's y as the true root, as an
    off-curve value and as an unreduced value of the same parity (the decompression shortcut and its two fall-backs), the high-S mirror of each, each with
    one flipped bit of the digest, and the panic shapes. Panics 1..5 are all met; panic 6 needs R.x in [n, p), a 2^-128 event nobody can construct, so
    no row claims it."""
    import acvm_amd
    import secp_cases as sc
    rows = sc.verification_rows(c, 16)
    got = acvm_amd.debug_secp(c, 16, [item for _, item, _ in rows])
    seen = set()
    for (label, item, want), g in zip(rows, got):
        assert g == want, (label, [hex(v) for v in item], g, want)
        seen.add(g)
    assert {(1, 0), (0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5)} <= seen
