"""The lookup tables of the Grumpkin and ECDSA kernels, restated in Python integers, and two checkers for entries read back from the device
(acvm_debug_table_read) or from the host copy (acvm_debug_grumpkin(0, ..)). Nothing here comes from the product: the base points are the curves'
published generators, the derived generators D[i] come from the CPU oracle, the definitions are the header comments of acvm_amd/csrc/grumpkin_host.hpp.

Storage (what `decode` undoes, and checks): an entry is 16 little-endian u32 -- x limbs 0..7, y limbs 0..7 -- of canonical values (below p). Grumpkin
entries and secp256r1 entries are Montgomery residues, the coordinate times 2^261 mod p (grumpkin_host.cpp put_point -> frh::to_device_form; secp_device.hpp
"secp256r1: Montgomery residues x R, R = 2^261"); secp256k1 entries are plain residues.

Definitions (table numbers of acvm_debug_table_read in brackets):
  ped   [0] [i][k-1]       = k D[i],                          i < 30, k = 1..512
  win   [1] [b][w][d-1]    = d 2^(8w) P_b,                    P_b = G, D[0], D[3], D[6], w < 32, d = 1..255
  small [2] [j][k-1]       = k D[3j+1],                       j < 3, k = 1..15
  skew  [3] [j]            = D[3j+2]
  ped2  [4] [g][a][b]      = endo((a+1) D[g]) + (b+1) D[g];   endo((a+1) D[g]) alone when g % 15 == 14, whatever b is
  win16 [5] [b][w][d-1]    = d 2^(16w) P_b,                   w < 16, d = 1..65535
  pedw  [6] [parity][j][v] = sum over the slices s = 0..28 that bits [24j, 24j+24) touch of (piece_s + [9s >= 24j]) E_s, E_s = D[15 parity + s/2] through
                             endo for even s; bits of v at positions 261 and up (bits 21..23 of the last window) contribute nothing
  gtab  [7, 8] [j][d]      = d 2^(16j) G_c, sixteen zero words at d = 0
endo(x, y) = (beta x, y)."""
import numpy as np

R_BITS = 261

GRUMPKIN = dict(name="grumpkin", p=0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001, a=0, b=-17, mont=True)
# G = (1, sqrt(-16)): the root barretenberg uses (the reference's vector fixed_base(1, 0) = (1, GY), tests/test_oracle_grumpkin.py)
GRUMPKIN["g"] = (1, 0x0000000000000002CF135E7506A45D632D270D45F1181294833FC48D823F272C)
BETA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd
SECP256K1 = dict(name="secp256k1", p=2**256 - 2**32 - 977, a=0, b=7, mont=False,
                 g=(0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8))
SECP256R1 = dict(name="secp256r1", p=2**256 - 2**224 + 2**192 + 2**96 - 1, a=-3, b=0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B, mont=True,
                 g=(0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296, 0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5))
for _cv in (GRUMPKIN, SECP256K1, SECP256R1):
    assert (_cv["g"][1] ** 2 - _cv["g"][0] ** 3 - _cv["a"] * _cv["g"][0] - _cv["b"]) % _cv["p"] == 0
assert (BETA ** 3 - 1) % GRUMPKIN["p"] == 0 and BETA != 1

TABLE_PED, TABLE_WIN, TABLE_SMALL, TABLE_SKEW, TABLE_PED2, TABLE_WIN16, TABLE_PEDW, TABLE_ECDSA_K1, TABLE_ECDSA_R1 = range(9)
TABLE_ENTRIES = {TABLE_PED: 30 * 512, TABLE_WIN: 4 * 32 * 255, TABLE_SMALL: 45, TABLE_SKEW: 3, TABLE_PED2: 30 << 18, TABLE_WIN16: 4 * 16 * 65535,
                 TABLE_PEDW: 2 * 11 << 24, TABLE_ECDSA_K1: 16 << 16, TABLE_ECDSA_R1: 16 << 16}


# ---- affine arithmetic; None = the point at infinity
def ec_add(cv, P, Q):
    p = cv["p"]
    if P is None:
        return Q
    if Q is None:
        return P
    if P[0] == Q[0]:
        if (P[1] + Q[1]) % p == 0:
            return None
        lam = (3 * P[0] * P[0] + cv["a"]) * pow(2 * P[1], -1, p) % p
    else:
        lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
    x = (lam * lam - P[0] - Q[0]) % p
    return x, (lam * (P[0] - x) - P[1]) % p


def ec_mul(cv, k, P):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(cv, acc, P)
        P = ec_add(cv, P, P)
        k >>= 1
    return acc


def multiples(cv, P, n):
    """[P, 2P, .., nP]"""
    out, acc = [], None
    for _ in range(n):
        acc = ec_add(cv, acc, P)
        out.append(acc)
    return out


def endo(pt):
    return BETA * pt[0] % GRUMPKIN["p"], pt[1]


# ---- storage form
def encode(cv, pt, mont=None):
    """the 16 words of an affine point as the tables hold it (mont: override of the curve's form, for the tests of the checkers)"""
    mont = cv["mont"] if mont is None else mont
    s = (1 << R_BITS) % cv["p"] if mont else 1
    raw = b"".join((c * s % cv["p"]).to_bytes(32, "little") for c in pt)
    return np.frombuffer(raw, dtype="<u4").astype(np.uint32)


class NotCanonical(AssertionError):
    def __init__(self, entry, text):
        super().__init__(text)
        self.entry = entry


def decode(cv, words):
    """words: uint32 [n][16] -> list of n affine points in plain integers. Asserts that every coordinate is canonical (below p) BEFORE it converts;
    the error (NotCanonical, an AssertionError) names the first entry that is not."""
    w = np.ascontiguousarray(words, dtype="<u4").reshape(-1, 16)
    raw = w.tobytes()
    p = cv["p"]
    f = int.from_bytes
    vals = [f(raw[o:o + 32], "little") for o in range(0, len(raw), 32)]
    if vals and max(vals) >= p:
        k = next(i for i, v in enumerate(vals) if v >= p)
        raise NotCanonical(k // 2, f"entry {k // 2}: coordinate {'xy'[k % 2]} = {vals[k]:#x} is not below p (not canonical)")
    if cv["mont"]:
        ri = pow(1 << R_BITS, -1, p)
        vals = [v * ri % p for v in vals]
    return list(zip(vals[0::2], vals[1::2]))


# ---- the two checkers
def check_exact(got, want):
    """got, want: lists of affine points; the index of the first entry that differs, or None"""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return i
    return None


def check_multiples(cv, pts, base):
    """pts[d-1] is to be d * base for d = 1..len(pts): entry 1 exactly, every later entry by the chord through entry 1 and its predecessor, without an
    inversion -- with dx = x_1 - x_{d-1}, dy = y_1 - y_{d-1} the sum (x_d, y_d) of the two is the only point with
        (x_d + x_{d-1} + x_1) dx^2 == dy^2   and   (y_d + y_{d-1}) dx == dy (x_{d-1} - x_d)            (dx != 0: asserted)
    (d = 2: the tangent, dx -> 2 y_1, dy -> 3 x_1^2 + a), so by induction a table that passes IS the table of multiples. Returns the first d that fails, or
    None. (Entries behind a failing one are not judged: their predecessor is wrong.)"""
    p, a = cv["p"], cv["a"]
    if not pts:
        return None
    if pts[0] != base:
        return 1
    x1, y1 = base
    xp, yp = base
    for d in range(2, len(pts) + 1):
        x, y = pts[d - 1]
        if d == 2:
            dx, dy = 2 * y1 % p, (3 * x1 * x1 + a) % p
        else:
            dx, dy = (x1 - xp) % p, (y1 - yp) % p
        if dx == 0:
            return d  # (d - 1) P = +-P: not a table of small multiples of a point of large order
        if ((x + xp + x1) * dx * dx - dy * dy) % p or ((y + yp) * dx - dy * (xp - x)) % p:
            return d
        xp, yp = x, y
    return None


def check_window_words(cv, words, base):
    """decode + check_multiples on the raw words of one window [n][16] holding base, 2 base, ..: the first d that is wrong (in value or in form), or None"""
    try:
        pts = decode(cv, words)
    except NotCanonical as e:
        bad = check_multiples(cv, decode(cv, words[:e.entry]), base)
        return bad if bad is not None else e.entry + 1
    return check_multiples(cv, pts, base)


# ---- the model
class Model:
    """Every table entry from the definitions above. D: the 30 derived Grumpkin generators (from the oracle, see generators_from_oracle)."""

    def __init__(self, D):
        assert len(D) == 30
        self.D = list(D)
        self.bases = [GRUMPKIN["g"], D[0], D[3], D[6]]
        self._ped = None
        self._pow = {}

    def ped_table(self):
        """[i][k-1] = k D[i]"""
        if self._ped is None:
            self._ped = [multiples(GRUMPKIN, d, 512) for d in self.D]
        return self._ped

    def ped(self, i, k):
        return self.ped_table()[i][k - 1]

    def shifted_base(self, cv, base, bits):
        """2^bits * base (cached)"""
        key = (cv["name"], base, bits)
        if key not in self._pow:
            pt = base
            for _ in range(bits):
                pt = ec_add(cv, pt, pt)
            self._pow[key] = pt
        return self._pow[key]

    def win(self, b, w, d):
        return ec_mul(GRUMPKIN, d, self.shifted_base(GRUMPKIN, self.bases[b], 8 * w))

    def small(self, j, k):
        return ec_mul(GRUMPKIN, k, self.D[3 * j + 1])

    def skew(self, j):
        return self.D[3 * j + 2]

    def win16(self, b, w, d):
        return ec_mul(GRUMPKIN, d, self.shifted_base(GRUMPKIN, self.bases[b], 16 * w))

    def ped2(self, g, a, b):
        first = endo(self.ped(g, a + 1))
        return first if g % 15 == 14 else ec_add(GRUMPKIN, first, self.ped(g, b + 1))

    def pedw(self, parity, j, v):
        lo_w, hi_w = 24 * j, 24 * j + 24
        acc = None
        for s in range(29):  # slices 29 and up do not exist: bits of v at 261 and above add nothing
            lo, hi = max(9 * s, lo_w), min(9 * s + 9, hi_w)
            if lo >= hi:
                continue
            piece = ((v >> (lo - lo_w)) & ((1 << (hi - lo)) - 1)) << (lo - 9 * s)
            factor = piece + (1 if 9 * s >= lo_w else 0)
            if factor == 0:
                continue
            e = self.ped(15 * parity + s // 2, factor)
            acc = ec_add(GRUMPKIN, acc, endo(e) if s % 2 == 0 else e)
        return acc

    def gtab(self, cv, j, d):
        return ec_mul(cv, d, self.shifted_base(cv, cv["g"], 16 * j))


def generators_from_oracle(oracle):
    """D[0..29] as the CPU oracle derives them (oracle_grumpkin_generator(i); tests/test_oracle_grumpkin.py pins i = 0, 2, 8, 15, 29 to SURVEY Appendix A)"""
    import ctypes as C
    out = C.create_string_buffer(64)
    D = []
    for i in range(30):
        oracle.lib().oracle_grumpkin_generator(i, out)
        D.append((int.from_bytes(out.raw[:32], "big"), int.from_bytes(out.raw[32:64], "big")))
    return D
