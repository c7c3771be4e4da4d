"""One builder of the ECDSA cases that random signatures essentially never reach, in Python integers, for the host run of
acvm_amd/csrc/secp_device.hpp (tests/test_secp_device_on_host.py, 8-bit generator windows) and the device run (tests/test_gpu_secp_probe.py,
tests/test_gpu_ecdsa.py, tests/test_gpu_brillig.py, 16-bit windows). W is the width of a generator window.

A case is (u1, u2, d): the two scalars of R = u1 G + u2 Q and the secret key of Q = d G. Since Q is a known multiple of G, the accumulator of
secp_mul2 -- u2 Q first, then the nonzero W-bit windows of u1 from the lowest (walk() below is that order as a specification) -- can be steered
onto +-(the window it is about to add): the complete addition then doubles, or cancels and re-enters from the identity. A signature
(r, s, z) with u1 = z / s, u2 = r / s follows from R (signature_for), so every case also runs as a whole verification.
Every expected value is an exact integer: (u1 + u2 d) G for the sum, verify_model for the verification, split_lambda for the endomorphism split."""
import collections
import functools
import random

from test_secp_device_on_host import CURVES, ec_add, ec_mul, verify_model  # noqa: F401  (verify_model: re-exported for the users of the cases)

SEED = 20260                 # of every random draw below
SAMPLE_SEED, SAMPLE_SIZE = 1, 2000

# ---- the endomorphism split of secp256k1 as libsecp256k1 rounds it (scalar_split_lambda), in integers. The lattice basis is checked against lambda
# and the two multipliers are derived from it here, so nothing below is copied from the header under test.
N_K1 = CURVES[0]["n"]
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
A1, B1 = 0x3086D221A7D46BCDE86C90E49284EB15, -0xE4437ED6010E88286F547FA90ABFE4C3
A2, B2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8, 0x3086D221A7D46BCDE86C90E49284EB15
assert pow(LAMBDA, 3, N_K1) == 1 and LAMBDA != 1
assert (A1 + B1 * LAMBDA) % N_K1 == 0 and (A2 + B2 * LAMBDA) % N_K1 == 0
G1 = (B2 * 2**384 + N_K1 // 2) // N_K1       # round(2^384 b2 / n)
G2 = (-B1 * 2**384 + N_K1 // 2) // N_K1      # round(2^384 (-b1) / n)
EIGHTS128 = int("8" * 32, 16)


def split_lambda(k):
    """(|k1|, neg1, |k2|, neg2) with k = k1 + k2 lambda (mod n)"""
    n = N_K1
    c1, c2 = (k * G1 + 2**383) >> 384, (k * G2 + 2**383) >> 384
    k2 = (c1 * -B1 + c2 * -B2) % n
    k1 = (k - k2 * LAMBDA) % n
    neg1, neg2 = k1 > n // 2, k2 > n // 2
    return (n - k1 if neg1 else k1), int(neg1), (n - k2 if neg2 else k2), int(neg2)


def uses_digit_128(mag):
    """the 33rd signed digit of a half of the split: bit 128 of e = |k| + 0x88..8"""
    return mag + EIGHTS128 >= 2**128


@functools.lru_cache(maxsize=None)
def split_sample():
    """2 000 seeded scalars classified by what their split exercises: (list of u2, {class: indices}). The minimum counts are conditions on
    the sample (the measured shares are 13.9 % / 3.1 % / 25 %: expected 277 / 63 / 500)."""
    rng = random.Random(SAMPLE_SEED)
    ks = [rng.randrange(N_K1) for _ in range(SAMPLE_SIZE)]
    cls = collections.defaultdict(list)
    for i, k in enumerate(ks):
        a, s1, b, s2 = split_lambda(k)
        assert a < 2**128 and b < 2**128
        if uses_digit_128(a): cls["k1_digit_128"].append(i)
        if uses_digit_128(b): cls["k2_digit_128"].append(i)
        cls["signs", s1, s2].append(i)
    assert len(cls["k1_digit_128"]) >= 40 and len(cls["k2_digit_128"]) >= 20
    assert all(len(cls["signs", s1, s2]) >= 40 for s1 in (0, 1) for s2 in (0, 1))
    return ks, dict(cls)


def split_shapes():
    """fixed inputs of the split: the ends of the range, the halves alone, the extreme recodings of each half"""
    n = N_K1
    sevens, top = int("7" * 32, 16), int("7" * 31 + "8", 16)
    return [0, 1, 2, 3, n - 1, n - 2, n // 2, n // 2 + 1, LAMBDA, n - LAMBDA, 2**128, 2**128 - 1, 2**128 + 1, 2**255, (2**256 - 1) % n,
            sevens, top, sevens * LAMBDA % n, top * LAMBDA % n, (2**126 + sevens * LAMBDA) % n, (2**126 + top * LAMBDA) % n, (n - top) % n, (n - 2**126 - top * LAMBDA) % n, 2**127 - 1]


# ---- the accumulation order
def curve_index(cv):
    return 0 if cv["a"] == 0 else 1


@functools.lru_cache(maxsize=None)
def _window_bases(c, W):
    """2^(W j) G"""
    cv = CURVES[c]
    out = [cv["g"]]
    for _ in range(256 // W - 1):
        P = out[-1]
        for _ in range(W):
            P = ec_add(cv, P, P)
        out.append(P)
    return out


def windows(u1, W):
    return [(u1 >> (W * j)) & ((1 << W) - 1) for j in range(256 // W)]


def walk(cv, W, u1, u2, Q):
    """u2 Q, then + d_j 2^(W j) G for the nonzero W-bit windows d_j of u1 from the lowest: (result, [(event, j)]) with the events an
    addition of a finite point can meet: 'doubling' (acc = addend), 'cancel' (acc = -addend), 'from_identity' (acc is the identity)"""
    bases = _window_bases(curve_index(cv), W)
    acc, events = ec_mul(cv, u2, Q), []
    for j, d in enumerate(windows(u1, W)):
        if not d:
            continue
        T = ec_mul(cv, d, bases[j])
        if acc is None: events.append(("from_identity", j))
        elif acc == T: events.append(("doubling", j))
        elif acc[0] == T[0]: events.append(("cancel", j))
        acc = ec_add(cv, acc, T)
    return acc, events


# ---- signatures
def _signature(cv, u1, u2, d, Q):
    """(R, (r, s, x, y, z)) or None when s comes out high (or r = 0): R = (u1 + u2 d) G, r = R.x mod n, s = r / u2, z = u1 s"""
    n = cv["n"]
    if not u2 % n:
        return None
    R = ec_mul(cv, (u1 + u2 * d) % n, cv["g"])
    iu2 = pow(u2, -1, n)
    if R is None:  # any r in [1, n) will do: the first that gives a low s
        r = next(r for r in range(1, 64) if 0 < r * iu2 % n <= n // 2)
    else:
        r = R[0] % n
    s = r * iu2 % n
    if not r or not s or s > n // 2:
        return None
    return R, (r, s, Q[0], Q[1], u1 * s % n)


def signature_for(cv, u1, u2, d):
    """(r, s, x, y, z) of a low-S signature whose verification computes u1 G + u2 (d G), or None (draw again)"""
    made = _signature(cv, u1, u2, d, ec_mul(cv, d % cv["n"], cv["g"]))
    return made[1] if made else None


def y_forms(cv, y):
    """the three forms public_key_y arrives in: the root itself, an off-curve value of its parity, an unreduced value (>= p) of its parity"""
    off, big = (12345678 << 1) | (y & 1), (2**256 - 2) | (y & 1)
    assert off != y and big >= cv["p"]
    return [y, off, big]


def panic_rows(cv):
    """(r, s, x, y, n_msg, z) for the panics 1..4 of the reference's call site (5 is the final identity of family A; 6 needs R.x in [n, p))"""
    p, n = cv["p"], cv["n"]
    Q = ec_mul(cv, 5, cv["g"])
    x = 1
    while pow((x ** 3 + cv["a"] * x + cv["b"]) % p, (p - 1) // 2, p) == 1: x += 1
    return [(0, 1, Q[0], Q[1], 32, 5), (1, 0, Q[0], Q[1], 32, 5), (n, 1, Q[0], Q[1], 32, 5), (1, n, Q[0], Q[1], 32, 5), (2**256 - 1, 2**256 - 1, Q[0], Q[1], 32, 5),
            (1, 1, p, 0, 32, 5), (1, 1, 2**256 - 1, 1, 32, 5), (1, 1, x, 0, 32, 5),
            (1, 1, Q[0], Q[1], 31, 5), (1, 1, Q[0], Q[1], 33, 5), (1, 1, Q[0], Q[1], 0, 5),
            (1, 1, Q[0], Q[1], 32, n), (1, 1, Q[0], Q[1], 32, 2**256 - 1)]


# ---- the families
Case = collections.namedtuple("Case", "family label u1 u2 d Q R sig events")  # sig = (r, s, x, y, z); events: of walk (family A only)


@functools.lru_cache(maxsize=None)
def cases(c, W):
    """Families A..E for curve c and window width W, each with its key, its exact sum and a low-S signature. Built once per process."""
    cv = CURVES[c]
    n, nwin, mask = cv["n"], 256 // W, (1 << W) - 1
    rng = random.Random(SEED + 100 * c + W)
    keys = {}

    def key(d):
        if d not in keys:
            keys[d] = ec_mul(cv, d, cv["g"])
        return keys[d]

    pool = [rng.randrange(1, n) for _ in range(3)]  # the random keys of families B..D
    out = []

    def add(family, label, draw, check=None):
        for _ in range(64):
            u1, u2, d = draw()
            made = _signature(cv, u1, u2, d, key(d))
            if made:
                break
        else:
            raise AssertionError(f"no low-S signature for {family} {label}")
        events = check(u1, u2, d, made[0]) if check else None
        out.append(Case(family, label, u1, u2, d, key(d), made[0], made[1], events))

    # (A) collisions: after the windows below j the accumulator is +-d_j 2^(W j) G
    def collision(j, sign, d_of):
        def draw():
            d = d_of()
            while True:
                u1 = rng.randrange(1, n)
                if (u1 >> (W * j)) & mask:
                    break
            return u1, (sign * (u1 & (mask << (W * j))) - (u1 & ((1 << (W * j)) - 1))) * pow(d, -1, n) % n, d

        def check(u1, u2, d, R):
            got, ev = walk(cv, W, u1, u2, key(d))
            assert got == R
            if sign > 0:
                assert ev == [("doubling", j)] and R is not None, ev
            else:
                later = [i for i in range(j + 1, nwin) if (u1 >> (W * i)) & mask]
                assert ev == [("cancel", j)] + ([("from_identity", later[0])] if later else []) and (R is None) == (not later), ev
            return tuple(ev)
        return draw, check

    for j in (0, 1, nwin // 2 - 1, nwin - 1):
        for sign in (1, -1):
            for name, d_of in (("1", lambda: 1), ("2", lambda: 2), ("n-1", lambda: n - 1), ("random", lambda: rng.randrange(1, n))):
                add("A", f"window {j} sign {sign:+d} d {name}", *collision(j, sign, d_of))
    # ... and the colliding window as the last nonzero one, in the middle of the scalar: the sum is the identity
    jm = nwin // 2

    def lone_window():
        d = pool[0]
        u1 = (rng.randrange(1, mask + 1) << (W * jm)) | rng.randrange(1, 1 << (W * jm))
        return u1, -u1 * pow(d, -1, n) % n, d

    def lone_check(u1, u2, d, R):
        got, ev = walk(cv, W, u1, u2, key(d))
        assert got is None and R is None and ev == [("cancel", jm)], ev
        return tuple(ev)
    add("A", f"window {jm} is the last one: identity", lone_window, lone_check)

    # (B) shapes of u1
    def shape_u1(u1):
        assert 0 <= u1 < n
        return lambda: (u1, rng.randrange(1, n), rng.choice(pool))
    alternating = [sum(mask << (W * j) for j in range(ph, nwin, 2)) for ph in (0, 1)]
    for label, u1 in (("0", 0), ("1", 1), ("2^W - 1", mask), ("2^W", 1 << W), ("top window alone", mask << (256 - W)), ("n - 1", n - 1),
                      ("alternating windows, even", alternating[0]), ("alternating windows, odd", alternating[1]),
                      ("0x80.. in every window", sum(1 << (W * j + W - 1) for j in range(nwin)))):
        add("B", "u1 = " + label, shape_u1(u1))

    # (C) / (D) shapes of u2
    def shape_u2(u2):
        assert 0 < u2 < n
        return lambda: (rng.randrange(n), u2, rng.choice(pool))
    if c == 1:  # signed 4-bit digits of e = u2 + 0x88..8, digit 64 = the carry
        shapes = [("all digits -8, with the carry", int("7" * 63 + "8", 16)), ("all digits +7", int("7" * 64, 16))]
        shapes += [(str(v), v) for v in (1, 2, 8, 9, 15, 16)] + [(f"8 * 16^{i}", 8 * 16**i) for i in (31, 63)]
        # (u2 = n - 2: the last digit is -1 and the digits in front of it sum to n - 1 = -1 (mod n), so the LADDER's last addition, -Q onto -Q, is a
        # doubling inside the complete addition -- the one scalar for which the ladder itself meets acc = addend)
        shapes += [("n - 1", n - 1), ("n - 2", n - 2), ("2^128", 2**128)]
        for label, u2 in shapes:
            add("C", "u2 = " + label, shape_u2(u2))
    else:   # the two 128-bit halves of the split, 32 signed digits and bit 128 each
        sevens, top = int("7" * 32, 16), int("7" * 31 + "8", 16)
        for u2 in (3, sevens, top):
            assert split_lambda(u2) == (u2, 0, 0, 0)
        assert split_lambda(5 * LAMBDA % n) == (0, 0, 5, 0)
        for m in (sevens, top):  # (k1 = 0 is not what the rounding returns for a k2 this large: the lattice reduces it; beside k1 = 2^126 it is)
            assert split_lambda((2**126 + m * LAMBDA) % n) == (2**126, 0, m, 0)
        shapes = [("3 (k2 = 0)", 3), ("0x77..77 (k2 = 0, all digits +7)", sevens), ("0x77..78 (k2 = 0, all digits -8 and digit 128)", top),
                  ("5 lambda (k1 = 0)", 5 * LAMBDA % n), ("2^126 + 0x77..77 lambda (k2: all digits +7)", (2**126 + sevens * LAMBDA) % n),
                  ("2^126 + 0x77..78 lambda (k2: all digits -8 and digit 128)", (2**126 + top * LAMBDA) % n),
                  ("lambda", LAMBDA), ("n - lambda", n - LAMBDA), ("n - 1", n - 1), ("n // 2", n // 2), ("n // 2 + 1", n // 2 + 1), ("2^128 - 1", 2**128 - 1), ("2^128 + 1", 2**128 + 1)]
        ks, cls = split_sample()
        shapes += [(f"sample[{i}]: digit 128 of k1", ks[i]) for i in cls["k1_digit_128"][:2]] + [(f"sample[{i}]: digit 128 of k2", ks[i]) for i in cls["k2_digit_128"][:2]]
        shapes += [(f"sample[{cls['signs', s1, s2][0]}]: signs {s1} {s2}", ks[cls["signs", s1, s2][0]]) for s1 in (0, 1) for s2 in (0, 1)]
        for label, u2 in shapes:
            add("D", "u2 = " + label, shape_u2(u2))

    # (E) keys
    for label, d in (("1", 1), ("2", 2), ("n - 1", n - 1), ("n - 2", n - 2), ("2^16", 2**16), ("2^240", 2**240), ("(n + 1) / 2", (n + 1) // 2)):
        add("E", "d = " + label, lambda d=d: (rng.randrange(n), rng.randrange(1, n), d))
    return tuple(out)


def special_rows(c, W):
    """The eight cases the opcode tests place among ordinary signatures, one lane of a wave each: the three collisions of family A (doubling,
    cancel + re-entry, final identity), z = 0, the two extreme recodings of u2 (C or D), and two more shapes of u2."""
    by = {x.label: x for x in cases(c, W)}
    mid = 256 // W // 2 - 1
    ext = ("u2 = all digits -8, with the carry", "u2 = all digits +7") if c == 1 else \
          ("u2 = 0x77..78 (k2 = 0, all digits -8 and digit 128)", "u2 = 2^126 + 0x77..78 lambda (k2: all digits -8 and digit 128)")
    more = ("u2 = 8 * 16^63", "u2 = n - 1") if c == 1 else ("u2 = 2^126 + 0x77..77 lambda (k2: all digits +7)", "u2 = n - lambda")
    names = [f"window {mid} sign +1 d random", f"window {mid} sign -1 d random", f"window {mid + 1} is the last one: identity", "u1 = 0", *ext, *more]
    rows = [by[k] for k in names]
    assert rows[0].events == (("doubling", mid),) and rows[1].events[0] == ("cancel", mid) and rows[1].events[1][0] == "from_identity"
    assert rows[2].R is None and rows[3].sig[4] == 0 and all(x.R is not None for x in rows[:2] + rows[3:])
    return rows


@functools.lru_cache(maxsize=None)
def verification_rows(c, W):
    """What the verification tests run, as (label, (r, s, x, y, n_msg, z), (result, panic) of verify_model): every case of cases(c, W) with its
    key in the three forms of y, the high-S mirror of its signature, its digest with one bit flipped; then the panic shapes."""
    cv = CURVES[c]
    n, out = cv["n"], []
    for i, x in enumerate(cases(c, W)):
        r, s, qx, qy, z = x.sig
        want = verify_model(cv, r, s, qx, qy & 1, 32, z)
        assert want == ((1, 0) if x.R is not None else (0, 5)), x.label  # (what the construction promises)
        for form, y in zip(("root", "off-curve y", "unreduced y"), y_forms(cv, qy)):
            out.append((f"{x.family} {x.label}: {form}", (r, s, qx, y, 32, z), want))
        out.append((f"{x.family} {x.label}: high S", (r, n - s, qx, qy, 32, z), verify_model(cv, r, n - s, qx, qy & 1, 32, z)))
        zf = z ^ (1 << (37 * i % 256))
        out.append((f"{x.family} {x.label}: flipped digest bit", (r, s, qx, qy, 32, zf), verify_model(cv, r, s, qx, qy & 1, 32, zf)))
    for row in panic_rows(cv):
        out.append(("panic shape", row, verify_model(cv, row[0], row[1], row[2], row[3] & 1, row[4], row[5])))
    return tuple(out)
