"""The case builder of the exceptional ECDSA paths (tests/secp_cases.py) checks itself: every collision case meets, in the accumulation order
written down as walk(), the event it was built for; every family is there for both window widths (8: the host run, 16: the device); the sample
of the endomorphism split holds its minimum counts; split_lambda recombines. No GPU, no compiler."""
import pytest

import secp_cases as sc
from test_secp_device_on_host import CURVES, ec_mul


@pytest.mark.parametrize("W", [8, 16])
@pytest.mark.parametrize("c", [0, 1])
def test_families_and_event_coverage(c, W):
    cv = CURVES[c]
    cs = sc.cases(c, W)  # (asserts every family-A case against walk while it builds)
    assert {x.family for x in cs} == {"A", "B", "D" if c == 0 else "C", "E"}
    ev = [x.events for x in cs if x.family == "A"]
    nwin = 256 // W
    for j in (0, 1, nwin // 2 - 1, nwin - 1):
        assert sum(e == (("doubling", j),) for e in ev) == 4
        assert sum(e[0] == ("cancel", j) for e in ev) == 4
    assert any(len(e) == 2 and e[0][0] == "cancel" and e[1][0] == "from_identity" for e in ev)
    assert sum(x.R is None for x in cs) >= 2 and all(x.events[-1][0] == "cancel" for x in cs if x.R is None)
    for x in cs:  # the signature is one of (u1, u2) for the key d, low-S
        r, s, qx, qy, z = x.sig
        n = cv["n"]
        assert 0 < r < n and 0 < s <= n // 2 and z * pow(s, -1, n) % n == x.u1 and r * pow(s, -1, n) % n == x.u2
        assert (qx, qy) == x.Q and (x.R is None or x.R[0] % n == r)
    assert any(x.sig[4] == 0 for x in cs)
    rows = sc.special_rows(c, W)
    assert len(rows) == 8 and len({x.label for x in rows}) == 8


def test_walk_agrees_with_the_plain_sum():
    cv = CURVES[1]
    x = sc.cases(1, 16)[-1]
    got, ev = sc.walk(cv, 16, x.u1, x.u2, x.Q)
    assert got == x.R == ec_mul(cv, (x.u1 + x.u2 * x.d) % cv["n"], cv["g"]) and ev == []
    # ... and with the other width the same scalars meet no event either
    assert sc.walk(cv, 8, x.u1, x.u2, x.Q) == (x.R, [])


def test_split_sample_and_model():
    ks, cls = sc.split_sample()  # (asserts the minimum counts)
    assert len(ks) == 2000 and len(cls["k1_digit_128"]) >= 40 and len(cls["k2_digit_128"]) >= 20
    assert all(len(cls["signs", a, b]) >= 40 for a in (0, 1) for b in (0, 1))
    n = sc.N_K1
    for k in sc.split_shapes() + list(ks):
        a, s1, b, s2 = sc.split_lambda(k)
        assert a < 2**128 and b < 2**128 and ((-a if s1 else a) + (-b if s2 else b) * sc.LAMBDA) % n == k
    assert sc.signature_for(CURVES[0], 5, 0, 7) is None


@pytest.mark.parametrize("c", [0, 1])
def test_verification_rows_reach_every_constructible_outcome(c):
    rows = sc.verification_rows(c, 16)
    assert {(1, 0), (0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5)} <= {w for _, _, w in rows}
    assert all(w == (0, 0) for label, _, w in rows if label.endswith("high S"))
