"""Pedersen, FixedBaseScalarMul and SchnorrVerify in affine coordinates and Python integers, with hashlib's Blake2s: a third
statement of the three functions beside the HIP kernels (acvm_amd/csrc/ops_grumpkin.hpp) and the C oracle (oracle/grumpkin.c), sharing no code and no
coordinate system with either. No device and no product code here. Built on tests/curve_table_ref.py (the curve, ec_add, endo, Model.ped); the 30 derived
generators D[i] are taken from the oracle as that file takes them (tests/test_oracle_grumpkin.py pins five of them to Appendix A).
The reference delegates the three functions to barretenberg, so what no reference vector pins stays UNPINNED (tests/test_grumpkin_cases.py says which
vectors this model reproduces).

glv_split and signed_windows5 restate the DEFINITIONS in the header's comment for classification only (which sign class, which digits a scalar has);
they carry their own asserts and are never used to compute a point."""
import functools
import hashlib

from curve_table_ref import GRUMPKIN, Model, ec_add, ec_mul, endo, generators_from_oracle

P = GRUMPKIN["p"]
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47   # the group order (BN254's base field modulus)
G = GRUMPKIN["g"]
LAMBDA = 0x59E26BCEA0D48BACD4F263F1ACDB5C4F5763473177FFFFFE                  # lambda (x, y) = (beta x, y)
assert (LAMBDA * LAMBDA + LAMBDA + 1) % Q == 0

FB_OK, FB_LIMB_LOW, FB_LIMB_HIGH, FB_SCALAR = "ok", "limb low", "limb high", "scalar"


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def on_curve(pt):
    return (pt[1] * pt[1] - pt[0] ** 3 + 17) % P == 0


class FixedMul:
    """k * base through 4-bit windows of precomputed affine multiples (the builders multiply G and three generators hundreds of times)"""

    def __init__(self, base):
        self.rows = []
        for _ in range(64):
            row, acc = [None], None
            for _ in range(15):
                acc = ec_add(GRUMPKIN, acc, base)
                row.append(acc)
            self.rows.append(row)
            base = ec_add(GRUMPKIN, acc, base)

    def __call__(self, k):
        assert 0 <= k < 1 << 256
        acc = None
        for w in range(64):
            acc = ec_add(GRUMPKIN, acc, self.rows[w][(k >> (4 * w)) & 15])
        return acc


class Ref:
    def __init__(self, D):
        self.model = Model(D)
        self.D = list(D)
        self.mul_g = FixedMul(G)
        self._mul_d = {}
        assert ec_mul(GRUMPKIN, LAMBDA, G) == endo(G) and self.mul_g(Q) is None and self.mul_g(Q - 1) == neg(G)
        self.schnorr_point = functools.lru_cache(maxsize=None)(self._schnorr_point)
        self.compress = functools.lru_cache(maxsize=None)(self._compress)
        self.hash_single = functools.lru_cache(maxsize=1 << 14)(self._hash_single)

    # ---- Pedersen (A.2)
    def _hash_single(self, v, parity):
        """slice s of 9 bits adds (slice + 1) D[15 parity + s / 2] to accumulator s % 2; accumulator 0 goes through the endomorphism"""
        assert 0 <= v < P
        acc = [None, None]
        for s in range(29):
            acc[s & 1] = ec_add(GRUMPKIN, acc[s & 1], self.model.ped(15 * parity + s // 2, ((v >> (9 * s)) & 511) + 1))
        return ec_add(GRUMPKIN, endo(acc[0]), acc[1])

    def hash_pair(self, left, right):
        """the whole point; its x is the chaining value"""
        return ec_add(GRUMPKIN, self.hash_single(left, 0), self.hash_single(right, 1))

    def pedersen(self, inputs, hash_index=0):
        assert 0 <= hash_index < 1 << 32
        n = len(inputs)
        if n == 0:
            return (0, 0)                      # UNPINNED: the encoding of the empty commitment
        r = self.mul_g(hash_index + 1)[0]      # IV = (hash_index + 1) G; UNPINNED for hash_index != 0
        pt = self.hash_pair(r, n)
        for v in inputs:
            pt = self.hash_pair(pt[0], v)
        return pt

    # ---- FixedBaseScalarMul (A.1)
    def fixed_base(self, low, high):
        """(FB_OK, point) -- (0, 0) for the scalar 0, UNPINNED -- or (failure class, None)"""
        if low >> 128:
            return FB_LIMB_LOW, None
        if high >> 128:
            return FB_LIMB_HIGH, None
        k = high << 128 | low
        if k >= Q:
            return FB_SCALAR, None
        return FB_OK, self.mul_g(k) or (0, 0)

    # ---- SchnorrVerify (A.3)
    def mul_d(self, i, k):
        if i not in self._mul_d:
            self._mul_d[i] = FixedMul(self.D[i])
        return self._mul_d[i](k)

    def ladder_term(self, v, j):
        assert 0 <= v < P
        V = v + 1 if v % 2 == 0 else v
        t = (V + 16) % 32
        lo = t if t < 16 else t - 32
        hi = (V - lo) // 16
        assert (V - lo) % 16 == 0 and lo % 2 == 1 and -15 <= lo <= 15
        aux = ec_mul(GRUMPKIN, abs(lo), self.D[3 * j + 1])
        pt = ec_add(GRUMPKIN, self.mul_d(3 * j, hi), aux if lo > 0 else neg(aux))
        return ec_add(GRUMPKIN, pt, neg(self.D[3 * j + 2])) if v % 2 == 0 else pt

    def _compress(self, vs):
        acc = None
        for j, v in enumerate(vs):
            acc = ec_add(GRUMPKIN, acc, self.ladder_term(v, j))
        return acc[0]

    def challenge(self, R, pk, msg):
        return hashlib.blake2s(self.compress((R[0], pk[0], pk[1])).to_bytes(32, "big") + bytes(msg)).digest()

    def schnorr_sign(self, sk, k, msg):
        """(pk, 64 signature bytes): R = k G, e = challenge, s = k - sk e (mod q)"""
        assert 0 < sk < Q and 0 < k < Q
        pk = self.mul_g(sk)
        e = self.challenge(self.mul_g(k), pk, msg)
        s = (k - sk * int.from_bytes(e, "big")) % Q
        return pk, s.to_bytes(32, "big") + e

    def _schnorr_point(self, pk, s, e):
        """R = e pk + s G for s, e already reduced; None: the point at infinity"""
        return ec_add(GRUMPKIN, ec_mul(GRUMPKIN, e, pk), self.mul_g(s))

    def schnorr_verify(self, pk, sig, msg):
        """sig: 64 bytes. The early rejects are UNPINNED (no reference vector rejects but by the digest)."""
        assert len(sig) == 64
        s, e = int.from_bytes(sig[:32], "big") % Q, int.from_bytes(sig[32:], "big") % Q
        if not on_curve(pk) or s == 0 or e == 0:
            return False
        R = self.schnorr_point(pk, s, e)
        return R is not None and self.challenge(R, pk, msg) == bytes(sig[32:])


@functools.lru_cache(maxsize=None)
def ref():
    """the one model of a test session, on the oracle's generators"""
    from oracle import binding
    binding.build()
    binding.lib()
    return Ref(generators_from_oracle(binding))


# ---- the scalar split of e * pk, from the definitions in the comment above glv_split (ops_grumpkin.hpp)
GLV_A = 0x89D3256894D213E2
GLV_B = 0x6F4D8248EEB859FC8211BBEB7D4F1129
GLV_BP = GLV_B + GLV_A
GLV_G1, GLV_G2 = (GLV_A << 384) // Q, (GLV_B << 384) // Q
assert GLV_A * GLV_A + GLV_B * GLV_BP == Q                                     # the determinant of the basis (A, -B), (B', A)
assert (GLV_A - GLV_B * LAMBDA) % Q == 0 and (GLV_BP + GLV_A * LAMBDA) % Q == 0  # both rows lie in the lattice u + v lambda = 0


def glv_split(k):
    """(k1, k2), signed, with k1 + k2 lambda = k (mod q). c1 and c2 are floors of k A / q and k B / q (g1, g2 are floors too: they only lower them further),
    so with d1 = k A / q - c1 >= 0 and d2 = k B / q - c2 >= 0 one has k1 = d1 A + d2 B' >= 0 and k2 = d2 A - d1 B exactly: k1 is never negative."""
    assert 0 <= k < Q
    c1, c2 = k * GLV_G1 >> 384, k * GLV_G2 >> 384
    k1, k2 = k - c1 * GLV_A - c2 * GLV_BP, c1 * GLV_B - c2 * GLV_A
    assert (k1 + k2 * LAMBDA - k) % Q == 0 and abs(k1) < 1 << 127 and abs(k2) < 1 << 127
    assert k1 >= 0
    return k1, k2


def signed_windows5(m):
    """26 digits d_i in [-15, 16] with sum d_i 32^i = m, for 0 <= m < 2^127: a window above 16 borrows 32 from the next one"""
    assert 0 <= m < 1 << 127
    digits, carry = [], 0
    for i in range(26):
        bits = ((m >> (5 * i)) & 31) + carry
        carry = 1 if bits > 16 else 0
        digits.append(bits - 32 * carry)
    assert carry == 0 and sum(d << (5 * i) for i, d in enumerate(digits)) == m and all(-15 <= d <= 16 for d in digits)
    return digits


def reduce_count(x):
    """how many times reduce_mod_q subtracts q from a 256-bit integer (0..5)"""
    assert 0 <= x < 1 << 256
    return x // Q
