"""Independent big-integer model of the BN254-Fr device library (acvm_amd/csrc/fr_device.hpp and the byte helpers of ops_common.hpp), used to
pin it routine by routine: through the host compiler (tests/test_fr_probe_on_host.py) and on the device (tests/test_gpu_fr_probe.py, the
acvm_debug_fr probe). Plain Python integers only; nothing of the project is imported. Test infrastructure only.

Every function gives the EXACT integer the routine returns, not only its residue: the column scan of a Montgomery reduction returns
(sum a_t b_t + m p) / 2^261 + h with m = -(sum a_t b_t) / p mod 2^261, and that integer is unique, so results are compared limb for limb.

The second half is the case generator: deterministic, seeded, and per routine only operands inside the routine's documented contract (the comment
above expect() quotes them). For the routines with a documented output bound the reference's own result is checked against that bound for every case
here, on the host, before anything reaches a GPU."""
import functools
import random

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
RBITS = 261
R = 1 << RBITS
M29 = (1 << 29) - 1
M32 = (1 << 32) - 1
T256 = 1 << 256
T261 = 1 << 261
PINV = pow(P, -1, R)
R1 = R % P            # the Montgomery one
R2 = R * R % P
RINV = pow(R, -1, P)

# GATE_H_MAX (gate_record.hpp) = 111 units of 2^25 per limb bounds the lazy sum h of a gate: at most 111 / 16 < 7 operands below 2^256 (top limb
# below 2^24) or 111 / 33 = 3 subtracted terms (8 p - x: top limb below 2^25) are in it, so its top limb stays below 7 * 2^24; the limbs below
# the top are 32-bit words as far as the scan is concerned (it adds them into a 64-bit column).
H_TOP_MAX = 7 * (1 << 24) - 1
GATE_K_INVERSE = 359  # gate_record.hpp: rows of the inverse table are below 359 p / 256

# ---------------------------------------------------------------------------------------------- forms


def s_words(v):
    """storage form: 8 x u32, little-endian"""
    assert 0 <= v < T256, hex(v)
    return [(v >> (32 * i)) & M32 for i in range(8)]


def s_value(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def w_words(v):
    """working form with normalised limbs: 8 limbs of 29 bits and the top limb with whatever is left"""
    assert 0 <= v < 1 << (232 + 32), hex(v)
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def w_value(w):
    """value of ANY nine limbs (lazy sums have limbs above 2^29)"""
    return sum(int(x) << (29 * i) for i, x in enumerate(w))


def is_normalised(w):
    return all(0 <= x <= M29 for x in w[:8]) and 0 <= w[8] <= M32


def mont(a):
    """canonical integer -> Montgomery representative"""
    return a * R % P


def kp_sub_words(klog2):
    """2^klog2 p with every limb below the top raised by 2^29 and the borrow taken from the next one (fr_kp29_sub)"""
    n = w_words((1 << klog2) * P)
    return [n[i] + (1 << 29 if i < 8 else 0) - (1 if i > 0 else 0) for i in range(9)]


# ---------------------------------------------------------------------------------------------- the routines


def scan(pairs, h=None):
    """the column scan: (sum a_t b_t + m p) / 2^261 + h, a_t, b_t, h integers"""
    s = sum(a * b for a, b in pairs)
    m = (-s * PINV) % R
    t, rem = divmod(s + m * P, R)
    assert rem == 0
    return t + (h or 0)


def cond_sub_p(v):
    return v - P if v >= P else v


def csub(v, klog2):
    k = (1 << klog2) * P
    return v - k if v >= k else v


def lt2p(v):
    return csub(csub(v, 2), 1)


def canon(v):
    return csub(lt2p(v), 0)


WEAK_MU = (1 << 268) // P
assert WEAK_MU == 21668


def weak(v):
    q = ((v >> 248) * WEAK_MU) >> 20
    r = v - q * P
    assert r >= 0
    return r


def norm(w):
    """carry propagation over raw limbs; the contract is that no limb overflows 32 bits on the way"""
    r = list(w)
    for i in range(8):
        r[i + 1] += r[i] >> 29
        assert r[i + 1] <= M32, "outside fr29_norm's contract"
        r[i] &= M29
    return r


def subl(a, b, klog2):
    c = kp_sub_words(klog2)
    return [(a[i] + c[i] - b[i]) & M32 for i in range(9)]


def addl(a, b):
    return [(a[i] + b[i]) & M32 for i in range(9)]


def dbll(a):
    return [(2 * a[i]) & M32 for i in range(9)]


def is_zero_mod_p(w):
    return int(all(x == 0 for x in w) or list(w) == w_words(P))


def fr_mul(a, b):
    return cond_sub_p(scan([(a, b)]))


def fr_add(a, b):
    return cond_sub_p(a + b)


def fr_sub(a, b):
    return a - b if a >= b else a - b + P


def fr_neg(a):
    return fr_sub(0, a)


def fr_inv(x):
    """x: the Montgomery representative a R; 1 / a in Montgomery form, 0 for 0"""
    return pow(x, -1, P) * R2 % P if x else 0


def fr_to_canonical(x):
    return fr_mul(x, 1)


def fr_low_limb(x):
    v = x * RINV % P
    return (v, 1) if v < 256 else (v & M29, 0)


def fr_is_byte(x):
    v = x * RINV % P
    return (1, v) if v < 256 else (0, 0)  # (the second word is unspecified when the first is 0)


def fr_from_byte(d):
    return mont(d & 0xff)


def fr29_redc_low(x):
    return (x * RINV % P) & M29


# ---------------------------------------------------------------------------------------------- the probe's routines
# name: (what, words in, words out). S = 8 words, W = 9 words.
WHATS = {
    "fr_mul": (0, 16, 8), "fr_mul_portable": (1, 16, 8), "fr_sqr": (2, 8, 8), "fr_add": (3, 16, 8), "fr_sub": (4, 16, 8), "fr_neg": (5, 8, 8),
    "fr_inv": (6, 8, 8), "fr_inv_eea": (7, 8, 8), "fr_to_canonical": (8, 8, 8), "fr_low_limb": (9, 8, 2), "fr_is_byte": (10, 8, 2),
    "fr_from_byte": (11, 1, 8), "fr29_from": (12, 8, 9), "fr29_pack": (13, 9, 8), "fr29_mul": (14, 18, 9), "fr29_mul_b": (15, 18, 9),
    "fr29_sqr": (16, 9, 9), "fr29_redc_low": (17, 9, 1), "fr29_cond_sub_p": (18, 9, 9), "fr29_csub": (19, 10, 9), "fr29_lt2p": (20, 9, 9),
    "fr29_weak": (21, 9, 9), "fr29_canon": (22, 9, 9), "fr29_norm": (23, 9, 9), "fr29_subl": (24, 19, 9), "fr29_addl": (25, 18, 9),
    "fr29_dbll": (26, 9, 9), "fr29_is_zero_mod_p": (27, 9, 1), "fr29_dot<1>": (28, 18, 9), "fr29_dot<2>": (29, 36, 9), "fr29_dot<3>": (30, 54, 9),
    "fr29_dot_add<1>": (31, 27, 9), "fr29_dot_add<2>": (32, 45, 9), "fr29_dot_add_b<1,0>": (33, 27, 9), "fr29_dot_add_b<2,0>": (34, 45, 9),
    "fr29_dot_add_b<1,1>": (35, 18, 9), "fr29_dot_add_b<2,2>": (36, 36, 9), "fr29_dot_add_b<2,3>": (37, 27, 9),
}
DEVICE_ONLY = ("fr_low_limb", "fr_is_byte", "fr_from_byte")  # the byte tables live in the device's constant memory
UNIFORM = ("fr29_dot_add_b<1,1>", "fr29_dot_add_b<2,2>", "fr29_dot_add_b<2,3>")

# The contract each routine's cases stay inside (fr_device.hpp, gate_eval.hpp "relaxed rows") and the output bound checked here.
#   "fr_mul": "any two rows below 2^256 (relaxed rows: the product reduces) -> canonical",
#   "fr_sqr": "any row below 2^256 -> canonical",
#   "fr_to_canonical": "any row below 2^256 -> canonical integer",
#   "fr_mul_portable": "a, b < p -> canonical (the 8 x 32 CIOS has no spare bits)",
#   "fr_add": "a, b < p", "fr_sub": "a, b < p", "fr_neg": "a < p", "fr_inv": "a < p; 0 -> 0", "fr_inv_eea": "a < p; 0 -> 0",
#   "fr_low_limb": "a < p", "fr_is_byte": "a < p", "fr_from_byte": "any word; the low byte counts",
#   "fr29_from": "any row below 2^256 -> limbs < 2^29, top limb < 2^24", "fr29_pack": "limbs < 2^29, value < 2^256",
#   "fr29_mul": "limbs < 2^29, values < 8 p -> normalised limbs, value < 1.4 p (< 1.1 p for inputs < 4 p)",
#   "fr29_mul_b": "as fr29_mul", "fr29_sqr": "as fr29_mul",
#   "fr29_redc_low": "fr29_from of a < p",
#   "fr29_cond_sub_p": "limbs < 2^29, value < 2 p -> canonical",
#   "fr29_csub": "normalised limbs, any value below 2^261, klog2 0..4",
#   "fr29_lt2p": "normalised, value < 8 p -> < 2 p", "fr29_canon": "normalised, value < 8 p -> canonical",
#   "fr29_weak": "normalised, any value below 2^261 -> same residue below 1.03 p",
#   "fr29_norm": "any limbs that do not overflow 32 bits with the carry of the limb below (<= 0xfffffff8)",
#   "fr29_subl": "a: limbs < 0xc0000000; b normalised, value <= 2^klog2 p; klog2 1..4",
#   "fr29_addl": "limb sums below 2^32", "fr29_dbll": "limbs below 2^31", "fr29_is_zero_mod_p": "normalised, value < 2 p",
#   "fr29_dot": "limbs < 2^29, the top one included; values enter through the bound p + sum a_t b_t / 2^261 only (two rows below 2^256: < 1.34 p)",
#   "fr29_dot_add": "as fr29_dot; h: limbs below 2^32, top limb <= H_TOP_MAX",


def expect(name, w, u=None):
    """the words the routine returns for the input words w of one item (u: the 18 words of the two uniform factors)"""
    S = lambda i: s_value(w[i:i + 8])  # noqa: E731
    W = lambda i: w_value(w[i:i + 9])  # noqa: E731
    if name == "fr_mul": return s_words(fr_mul(S(0), S(8)))
    if name == "fr_mul_portable": return s_words(S(0) * S(8) * RINV % P)
    if name == "fr_sqr": return s_words(fr_mul(S(0), S(0)))
    if name == "fr_add": return s_words(fr_add(S(0), S(8)))
    if name == "fr_sub": return s_words(fr_sub(S(0), S(8)))
    if name == "fr_neg": return s_words(fr_neg(S(0)))
    if name in ("fr_inv", "fr_inv_eea"): return s_words(fr_inv(S(0)))
    if name == "fr_to_canonical": return s_words(fr_to_canonical(S(0)))
    if name == "fr_low_limb": return list(fr_low_limb(S(0)))
    if name == "fr_is_byte": return list(fr_is_byte(S(0)))
    if name == "fr_from_byte": return s_words(fr_from_byte(w[0]))
    if name == "fr29_from": return w_words(S(0))
    if name == "fr29_pack": return s_words(W(0))
    if name in ("fr29_mul", "fr29_mul_b"): return w_words(scan([(W(0), W(9))]))
    if name == "fr29_sqr": return w_words(scan([(W(0), W(0))]))
    if name == "fr29_redc_low": return [fr29_redc_low(W(0))]
    if name == "fr29_cond_sub_p": return w_words(cond_sub_p(W(0)))
    if name == "fr29_csub": return w_words(csub(W(0), w[9]))
    if name == "fr29_lt2p": return w_words(lt2p(W(0)))
    if name == "fr29_weak": return w_words(weak(W(0)))
    if name == "fr29_canon": return w_words(canon(W(0)))
    if name == "fr29_norm": return norm(w[0:9])
    if name == "fr29_subl": return subl(w[0:9], w[9:18], w[18])
    if name == "fr29_addl": return addl(w[0:9], w[9:18])
    if name == "fr29_dbll": return dbll(w[0:9])
    if name == "fr29_is_zero_mod_p": return [is_zero_mod_p(w[0:9])]
    if name.startswith("fr29_dot<"):
        n = int(name[9])
        return w_words(scan([(W(18 * t), W(18 * t + 9)) for t in range(n)]))
    if name in ("fr29_dot_add<1>", "fr29_dot_add_b<1,0>"): return w_words(scan([(W(0), W(9))], W(18)))
    if name in ("fr29_dot_add<2>", "fr29_dot_add_b<2,0>"): return w_words(scan([(W(0), W(9)), (W(18), W(27))], W(36)))
    u0, u1 = w_value(u[0:9]), w_value(u[9:18])
    if name == "fr29_dot_add_b<1,1>": return w_words(scan([(W(0), u0)], W(9)))
    if name == "fr29_dot_add_b<2,2>": return w_words(scan([(W(0), W(9)), (W(18), u0)], W(27)))
    if name == "fr29_dot_add_b<2,3>": return w_words(scan([(W(0), u0), (W(9), u1)], W(18)))
    raise KeyError(name)


def check_bound(name, w, out, u=None):
    """the documented output bound of a bounded-output routine, on the reference's own result (and what the result must be congruent to)"""
    W = lambda i: w_value(w[i:i + 9])  # noqa: E731
    if name in ("fr_mul", "fr_sqr", "fr_to_canonical", "fr_mul_portable", "fr_add", "fr_sub", "fr_neg", "fr_inv", "fr_inv_eea"):
        assert s_value(out) < P, (name, w)
    elif name in ("fr29_mul", "fr29_mul_b", "fr29_sqr"):
        a, b = W(0), W(0 if name == "fr29_sqr" else 9)
        v = w_value(out)
        assert is_normalised(out) and out[8] <= M29 and (v * R - a * b) % P == 0, (name, w)
        assert 10 * v < 14 * P, (name, w)                      # < 1.4 p for inputs < 8 p
        if a < 4 * P and b < 4 * P: assert 10 * v < 11 * P, (name, w)  # < 1.1 p for inputs < 4 p (1 + 16 p / 2^261 = 1.0945)
    elif name == "fr29_from":
        assert all(x <= M29 for x in out[:8]) and out[8] < 1 << 24
    elif name == "fr29_cond_sub_p":
        assert w_value(out) < P and (w_value(out) - W(0)) % P == 0
    elif name == "fr29_lt2p":
        assert w_value(out) < 2 * P and (w_value(out) - W(0)) % P == 0
    elif name == "fr29_canon":
        assert w_value(out) < P and (w_value(out) - W(0)) % P == 0
    elif name == "fr29_weak":
        assert is_normalised(out) and 100 * w_value(out) < 103 * P and (w_value(out) - W(0)) % P == 0, (name, w)
    elif name == "fr29_norm":
        assert all(x <= M29 for x in out[:8]) and w_value(out) == W(0)
    elif name == "fr29_subl":
        assert (w_value(out) - (W(0) + (P << w[18]) - W(9))) % (1 << 264) == 0  # (the top limb may wrap: it cancels in fr29_norm)
    elif name == "fr29_is_zero_mod_p":
        assert out[0] == int(W(0) % P == 0)
    elif name.startswith("fr29_dot"):
        assert is_normalised(out)
        if name.startswith("fr29_dot<2>") and all(W(9 * t) < T256 for t in range(4)):
            assert 100 * w_value(out) < 134 * P, (name, w)     # two products of any two rows of the witness table


# ---------------------------------------------------------------------------------------------- the case generator


def runs(rng, bits):
    """a long run of ones in zeros or of zeros in ones (the secp probe's form): what drives the carries"""
    return (rng.choice([0, (1 << bits) - 1]) ^ (((1 << rng.randrange(1, bits)) - 1) << rng.randrange(0, bits))) & ((1 << bits) - 1)


def edge_values(limit, bits):
    """the named edges below `limit` (< 2^bits): 0, 1, every k p and its neighbours, powers of two across the limb boundaries of both forms and their
    predecessors, every limb at its maximum, every limb zero except one"""
    vals = {0, 1, 2, limit - 1, limit - 2}
    for k in range(1, limit // P + 2):  # every k the limit admits (2^261 is 169 p)
        vals.update((k * P - 1, k * P, k * P + 1))
    for step in (29, 32):
        for i in range(0, bits // step + 1):
            for d in (-1, 0, 1):
                vals.update(((1 << (step * i)) + d, (1 << (step * i)) - 1 + d))
            vals.add(((1 << step) - 1) << (step * i))            # one limb at its maximum, the others zero
            vals.add(((1 << bits) - 1) ^ (((1 << step) - 1) << (step * i)))  # one limb zero, the others at their maximum
    vals.add((1 << bits) - 1)                                    # every limb at its maximum
    vals.add(sum(M29 << (29 * i) for i in range(0, 9, 2)))       # alternate limbs
    vals.add(sum(M32 << (32 * i) for i in range(1, 8, 2)))
    return sorted(v for v in vals if 0 <= v < limit)


SMALL_EDGE_K = (0, 1, 2, 4, 5, 8)


def small_edges(limit):
    """the short list that is paired with itself"""
    vals = {0, 1, limit - 1, M29, 1 << 29, M32, 1 << 32, (1 << 232) - 1, 1 << 232}
    for k in SMALL_EDGE_K:
        vals.update((k * P - 1, k * P, k * P + 1))
    b = limit.bit_length()
    vals.update(((1 << (b - 1)) - 1, 1 << (b - 1)))
    return sorted(v for v in vals if 0 <= v < limit)


def values(rng, limit, n_random, n_runs):
    bits = (limit - 1).bit_length()
    out = edge_values(limit, bits)
    out += [rng.randrange(limit) for _ in range(n_random)]
    out += [rng.randrange(limit - (limit >> 6), limit) for _ in range(n_random // 8)]  # just below the contract's edge
    out += [runs(rng, bits) % limit for _ in range(n_runs)]
    return out


def pairs(rng, limit, n_random, n_runs):
    se = small_edges(limit)
    out = [(a, b) for a in se for b in se]
    vs = values(rng, limit, n_random, n_runs)
    out += [(a, vs[rng.randrange(len(vs))]) for a in vs]
    out += [(vs[rng.randrange(len(vs))], b) for b in vs[::3]]
    return out


def h_words(rng, n):
    """lazy sums h: raw 32-bit limbs, the top one at most H_TOP_MAX"""
    fixed = [[0] * 9, [M32] * 8 + [H_TOP_MAX], [M32] * 8 + [0], [0] * 8 + [H_TOP_MAX], [M29] * 9, [1 << 29] * 8 + [1],
             [M32, 0] * 4 + [H_TOP_MAX], [0, M32] * 4 + [0]]
    out = []
    for i in range(n):
        if i < len(fixed): out.append(fixed[i])
        elif i % 4 == 0: out.append([rng.choice((0, M32, M29, 1 << 29, 1 << 31)) for _ in range(8)] + [rng.choice((0, H_TOP_MAX, 0xffff))])
        else: out.append([rng.randrange(1 << 32) for _ in range(8)] + [rng.randrange(H_TOP_MAX + 1)])
    return out


def raw_limbs(rng, n, limb_max, top_max):
    picks = (0, 1, M29, 1 << 29, limb_max, limb_max - 1)
    out = [[0] * 9, [limb_max] * 8 + [top_max], [M29] * 9, [M29] * 8 + [top_max], [limb_max] + [0] * 8]
    for i in range(n):
        if i % 3 == 0: out.append([min(rng.choice(picks), limb_max) for _ in range(8)] + [min(rng.choice(picks), top_max)])
        else: out.append([rng.randrange(limb_max + 1) for _ in range(8)] + [rng.randrange(top_max + 1)])
    return out


def uniform_values(rng):
    """the wave-uniform factors the U forms are run with: one launch each. Coefficients are fr29_from of a record's words (below 2^256); the scan's own
    contract admits any normalised limbs, so those are here too."""
    vs = [0, 1, P - 1, P, P + 1, R1, T256 - 1, T261 - 1, M29, 1 << 29, (1 << 232) - 1, 1 << 232, sum(M29 << (29 * i) for i in range(0, 9, 2)), 5 * P + 1]
    vs += [rng.randrange(P) for _ in range(8)] + [rng.randrange(T256) for _ in range(6)] + [rng.randrange(T261) for _ in range(4)]
    return [(v, vs[(i * 7 + 3) % len(vs)]) for i, v in enumerate(vs)]


def byte_rows():
    """stored forms around the byte recognition: every byte, its neighbours, a non-byte that shares a byte's low ten bits (the key table's index)"""
    rows = [mont(d) for d in range(256)] + [mont(d) for d in (256, 257, 511, 512, M29, 1 << 29, (1 << 29) + 255, P - 1, P - 255, P - 256)]
    for d in range(0, 256, 5):
        x = mont(d) ^ (1 << (11 + d % 200))
        if x < P: rows.append(x)
    return rows


def inv_inputs(rng):
    """Montgomery representatives of 0, 1, p - 1, 2^k and p - 2^k for every k, of their inverses, and of 2 000 random values; the same as plain
    integers too (the routine sees an integer below p either way)"""
    a = [0, 1, P - 1]
    for k in range(254):
        a += [1 << k, P - (1 << k)]
    a += [pow(x, -1, P) for x in a if x]
    a += [rng.randrange(P) for _ in range(2000)]
    return [mont(x) for x in a] + [1 << k for k in range(0, 254, 3)] + [P - 1, P - 2]


@functools.lru_cache(maxsize=None)
def sections(name, seed=0xF12EF):
    """the launches of routine `name`: a tuple of (uniform words or None, items), items = a tuple of word tuples"""
    what = WHATS[name][0]
    rng = random.Random(seed * 64 + what)
    S, W = s_words, w_words
    flat = lambda *ws: tuple(x for w in ws for x in w)  # noqa: E731
    if name in ("fr_mul",):
        items = [flat(S(a), S(b)) for a, b in pairs(rng, T256, 1200, 500)]
    elif name in ("fr_mul_portable", "fr_add", "fr_sub"):
        items = [flat(S(a), S(b)) for a, b in pairs(rng, P, 1200, 500)]
    elif name in ("fr_sqr", "fr_to_canonical", "fr29_from"):
        items = [flat(S(a)) for a in values(rng, T256, 2500, 800)]
    elif name == "fr_neg":
        items = [flat(S(a)) for a in values(rng, P, 2500, 800)]
    elif name in ("fr_inv", "fr_inv_eea"):
        items = [flat(S(a)) for a in inv_inputs(random.Random(seed))]  # (the same inputs for both)
    elif name in ("fr_low_limb", "fr_is_byte"):
        items = [flat(S(a)) for a in byte_rows() + values(rng, P, 1500, 300)]
    elif name == "fr_from_byte":
        items = [(d,) for d in list(range(256)) + [256, 0x1ff, 0xabcdef12, M32, 0x100]]
    elif name == "fr29_pack":
        items = [flat(W(a)) for a in values(rng, T256, 2500, 800)]
    elif name in ("fr29_mul", "fr29_mul_b"):
        items = [flat(W(a), W(b)) for a, b in pairs(rng, 8 * P, 1500, 500) + pairs(rng, 4 * P, 600, 100)]
    elif name == "fr29_sqr":
        items = [flat(W(a)) for a in values(rng, 8 * P, 2500, 800) + values(rng, 4 * P, 600, 100)]
    elif name == "fr29_redc_low":
        items = [flat(W(a)) for a in values(rng, P, 2500, 800)]
    elif name in ("fr29_cond_sub_p", "fr29_is_zero_mod_p"):
        items = [flat(W(a)) for a in values(rng, 2 * P, 2500, 800)]
    elif name == "fr29_csub":
        vs = values(rng, T261, 800, 300)
        items = [flat(W(a), (k,)) for k in range(5) for a in vs + [(1 << k) * P - 1, (1 << k) * P, (1 << k) * P + 1]]
    elif name in ("fr29_lt2p", "fr29_canon"):
        items = [flat(W(a)) for a in values(rng, 8 * P, 2500, 800)]
    elif name == "fr29_weak":
        items = [flat(W(a)) for a in values(rng, T261, 3000, 1000)]
    elif name == "fr29_norm":
        items = [tuple(w) for w in raw_limbs(rng, 3000, 0xfffffff8, 0xfffffff8)]
    elif name == "fr29_subl":
        items = []
        for k in (1, 2, 3, 4):
            kp = (1 << k) * P
            bs = values(rng, kp + 1, 500, 100)
            as_ = raw_limbs(rng, len(bs), 0xbfffffff, 0xbfffffff)
            items += [flat(a, W(b), (k,)) for a, b in zip(as_, bs)]
            items += [flat(W(a), W(b), (k,)) for a in (0, 1, kp) for b in (0, 1, kp - 1, kp)]
    elif name == "fr29_addl":
        a, b = raw_limbs(rng, 2000, 0x7fffffff, 0x7fffffff), raw_limbs(rng, 2000, 0x80000000, 0x80000000)
        items = [flat(x, y) for x, y in zip(a, b)]
    elif name == "fr29_dbll":
        items = [tuple(w) for w in raw_limbs(rng, 2000, 0x7fffffff, 0x7fffffff)]
    elif name.startswith("fr29_dot<") or name in ("fr29_dot_add<1>", "fr29_dot_add<2>", "fr29_dot_add_b<1,0>", "fr29_dot_add_b<2,0>"):
        n = int(name[name.index("<") + 1])
        add = "add" in name
        # the block form and the C form of a scan get the SAME cases (both are compared with the integers, not with each other)
        rng = random.Random(seed * 64 + 1000 + 2 * n + add)
        cols = []
        for t in range(n):
            lim = (T261, T256, 8 * P)[t % 3]
            pr = pairs(rng, lim, 900, 300)
            rng.shuffle(pr) if t else None
            cols.append(pr)
        cnt = min(len(c) for c in cols)
        hs = h_words(rng, cnt) if add else None
        items = []
        for i in range(cnt):
            ws = [W(v) for t in range(n) for v in cols[t][i]]
            if add: ws.append(hs[(i * 5) % cnt])
            items.append(flat(*ws))
    elif name in UNIFORM:
        out = []
        for u0, u1 in uniform_values(rng):
            vs = values(rng, (T261, T256)[len(out) % 2], 60, 30)
            hs = h_words(rng, len(vs))
            pick = lambda: W(vs[rng.randrange(len(vs))])  # noqa: E731
            if name == "fr29_dot_add_b<1,1>": items = [flat(W(a), hs[i]) for i, a in enumerate(vs)]
            elif name == "fr29_dot_add_b<2,2>": items = [flat(W(a), pick(), pick(), hs[i]) for i, a in enumerate(vs)]
            else: items = [flat(W(a), pick(), hs[i]) for i, a in enumerate(vs)]
            out.append((flat(W(u0), W(u1)), tuple(items)))
        return tuple(out)
    else:
        raise KeyError(name)
    return ((None, tuple(items)),)


@functools.lru_cache(maxsize=None)
def expected(name, seed=0xF12EF):
    """per section the expected output words of every item; every documented output bound is asserted on the way"""
    out = []
    for u, items in sections(name, seed):
        rows = []
        for w in items:
            r = expect(name, w, u)
            assert len(w) == WHATS[name][1] and len(r) == WHATS[name][2] and all(0 <= x <= M32 for x in r), (name, w)
            check_bound(name, w, r, u)
            rows.append(tuple(r))
        out.append(tuple(rows))
    return tuple(out)


def n_cases(name):
    return sum(len(items) for _, items in sections(name))


def compare(name, got, section):
    """got: the uint32 array [n][words out] one launch of routine `name` returned; section: the launch's index. Every word must equal the reference's."""
    import numpy as np
    _, items = sections(name)[section]
    want = np.array(expected(name)[section], dtype=np.uint32)
    if name == "fr_is_byte":
        got = got.copy()
        got[got[:, 0] == 0, 1] = 0  # the byte is unspecified where the value is none
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (name, section, len(bad), [(list(map(hex, items[i])), list(map(hex, got[i])), list(map(hex, want[i]))) for i in bad[:2]])
