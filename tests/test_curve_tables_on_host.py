"""The four host-built Grumpkin tables, every entry, against the integer model of tests/curve_table_ref.py, and the model's two checkers shown to bite
before tests/test_gpu_curve_tables.py relies on them. No GPU: the tables are read through acvm_debug_grumpkin(0, ..), which answers from the host copy.

Cost of the integer side, measured by test_cost_of_the_checkers_per_entry on the build machine's CPU (python 3, one thread, 65 535-entry windows):
  secp256k1  decode 0.78 us/entry, chord check 3.47 us/entry, exact compare 0.11 us/entry
  secp256r1  decode 1.95 us/entry, chord check 2.23 us/entry, exact compare 0.07 us/entry
  grumpkin   decode 2.22 us/entry, chord check 3.17 us/entry, exact compare 0.10 us/entry
  one model point by double-and-add (256-bit scalar): 8.06 ms; one affine addition with its inversion: 28.6 us
So decode + chord check is 4.2 to 5.4 us per entry, 0.28 to 0.36 s per window of 65 536. The GPU module sizes its cases from that: 4 windows per ECDSA case
(1.2 s + 24 model points), 8 windows per win16 case (2.8 s + 56 model points), 20 000 affine additions for ped2 (0.6 s), about 1 400 entries of at most three
additions per pedw plane (0.12 s per plane, 11 planes per case): every case below 5 s."""
import random
import time

import numpy as np
import pytest

import curve_table_ref as ref
from curve_table_ref import GRUMPKIN, SECP256K1, SECP256R1


@pytest.fixture(scope="module")
def model(oracle):
    return ref.Model(ref.generators_from_oracle(oracle))


def host_table(table, n):
    import acvm_amd
    return [acvm_amd.debug_grumpkin(0, table << 24 | i) for i in range(n)]


def test_table_sizes_of_the_debug_abi():
    import acvm_amd
    for t, n in ref.TABLE_ENTRIES.items():
        got, _ = acvm_amd.debug_table_info(t)
        assert got == n, t
    with pytest.raises(acvm_amd.AcvmError):
        acvm_amd.debug_table_info(9)
    with pytest.raises(acvm_amd.AcvmError, match=r"entries\[1\] = 15360 is outside the ped table"):
        acvm_amd.debug_table_read(ref.TABLE_PED, [0, 30 * 512])  # refused on the host: no device is touched
    with pytest.raises(acvm_amd.AcvmError, match="no such table"):
        acvm_amd.debug_table_read(9, [0])


def test_generator_index_convention(model, oracle):
    """D[i] of the oracle is entry k = 1 of row i of ped, and the model's hash_single -- the sum of the eleven pedw windows of a value, which is the sum of its
    29 slices -- is the oracle's, including the two vectors of SURVEY Appendix A that tests/test_oracle_grumpkin.py pins"""
    import ctypes as C
    import acvm_amd
    for i in range(30):
        assert acvm_amd.debug_grumpkin(0, i * 512) == model.D[i], i
    out = C.create_string_buffer(64)
    r = random.Random(3)
    P = GRUMPKIN["p"]
    for v in [1, 0, 2, 511, 512, P - 1, (1 << 253) + 12345, r.randrange(P), r.randrange(P)]:
        for parity in (0, 1):
            acc = None
            for j in range(11):
                acc = ref.ec_add(GRUMPKIN, acc, model.pedw(parity, j, (v >> (24 * j)) & 0xFFFFFF))
            oracle.lib().oracle_pedersen_hash_single(v.to_bytes(32, "big"), parity, out)
            assert acc == (int.from_bytes(out.raw[:32], "big"), int.from_bytes(out.raw[32:], "big")), (hex(v), parity)
    oracle.lib().oracle_pedersen_hash_single((1).to_bytes(32, "big"), 0, out)
    assert int.from_bytes(out.raw[:32], "big") == 0x2A819004B81013BD13F8548BB6C4BE17B680F520FFEAEF3A896127486E815163


def test_endomorphism_and_last_window_rule(model):
    """endo is multiplication by a cube root of unity on the curve (stays on the curve, three applications are the identity, endo(P) + endo(Q) = endo(P + Q)),
    and the rule for bits at 261 and above: entry v of the last window is entry v mod 2^21"""
    P, Q = model.D[0], model.D[1]
    e = ref.endo(P)
    assert (e[1] ** 2 - e[0] ** 3 + 17) % GRUMPKIN["p"] == 0 and e != P and ref.endo(ref.endo(e)) == P
    assert ref.ec_add(GRUMPKIN, ref.endo(P), ref.endo(Q)) == ref.endo(ref.ec_add(GRUMPKIN, P, Q))
    for v in (0, 1, (1 << 14) - 1, 0x155555):
        for hi in (1, 5, 7):
            assert model.pedw(1, 10, v | hi << 21) == model.pedw(1, 10, v)
    assert model.pedw(0, 10, 1 << 20) != model.pedw(0, 10, 0)


def test_ped_every_entry(model):
    got = host_table(ref.TABLE_PED, 30 * 512)
    want = [pt for row in model.ped_table() for pt in row]
    assert ref.check_exact(got, want) is None
    for i in range(30):  # and the chord checker agrees on every row
        assert ref.check_multiples(GRUMPKIN, got[512 * i:512 * i + 512], model.D[i]) is None, i


def test_win_every_entry(model):
    got = host_table(ref.TABLE_WIN, 4 * 32 * 255)
    for b in range(4):
        for w in range(32):
            base = model.shifted_base(GRUMPKIN, model.bases[b], 8 * w)
            rows = got[(b * 32 + w) * 255:(b * 32 + w + 1) * 255]
            assert ref.check_exact(rows, ref.multiples(GRUMPKIN, base, 255)) is None, (b, w)
            assert ref.check_multiples(GRUMPKIN, rows, base) is None, (b, w)
    assert got[255 * 32 * 3 + 31 * 255 + 254] == model.win(3, 31, 255) and got[255] == model.win(0, 1, 1)  # (through ec_mul, not through the running sum)


def test_small_and_skew_every_entry(model):
    got = host_table(ref.TABLE_SMALL, 45)
    assert ref.check_exact(got, [model.small(j, k) for j in range(3) for k in range(1, 16)]) is None
    assert host_table(ref.TABLE_SKEW, 3) == [model.skew(j) for j in range(3)]
    import acvm_amd
    with pytest.raises(acvm_amd.AcvmError):  # the last entry is the last
        acvm_amd.debug_grumpkin(0, ref.TABLE_SKEW << 24 | 3)


# ---- the checkers bite
N_WINDOW = 300
CASES = [pytest.param(GRUMPKIN, id="grumpkin-montgomery"), pytest.param(SECP256K1, id="secp256k1-plain"), pytest.param(SECP256R1, id="secp256r1-montgomery")]


@pytest.fixture(scope="module")
def windows():
    """per curve: (the base 2^16 G, the clean words [N_WINDOW][16] of base, 2 base, ..)"""
    out = {}
    for cv in (GRUMPKIN, SECP256K1, SECP256R1):
        base = cv["g"]
        for _ in range(16):
            base = ref.ec_add(cv, base, base)
        pts = ref.multiples(cv, base, N_WINDOW + 1)
        out[cv["name"]] = (base, pts, np.stack([ref.encode(cv, pt) for pt in pts[:N_WINDOW]]))
    return out


@pytest.mark.parametrize("cv", CASES)
def test_checkers_pass_a_clean_window_in_its_own_form_only(windows, cv):
    base, pts, words = windows[cv["name"]]
    assert ref.check_window_words(cv, words, base) is None
    assert ref.check_exact(ref.decode(cv, words), pts[:N_WINDOW]) is None
    other = np.stack([ref.encode(cv, pt, mont=not cv["mont"]) for pt in pts[:N_WINDOW]])  # the whole table in the other form: wrong from entry 1
    assert ref.check_window_words(cv, other, base) == 1


@pytest.mark.parametrize("cv", CASES)
@pytest.mark.parametrize("k", [1, 2, 3, 150, N_WINDOW])
def test_checkers_name_the_corrupted_entry(windows, cv, k):
    """one corruption at entry d = k (1-based): both checkers report k, not a neighbour"""
    base, pts, clean = windows[cv["name"]]
    want = pts[:N_WINDOW]
    p = cv["p"]

    def both(words, at):
        assert ref.check_window_words(cv, words, base) == at
        try:
            assert ref.check_exact(ref.decode(cv, words), want) == at - 1
        except ref.NotCanonical as e:
            assert e.entry == at - 1

    for limb, bit in ((0, 0), (3, 7), (7, 20), (8, 0), (12, 31), (15, 3)):  # one bit of one limb (x: limbs 0..7, y: 8..15)
        w = clean.copy()
        w[k - 1, limb] ^= np.uint32(1 << bit)
        both(w, k)
    w = clean.copy()  # a limb bit that lifts the coordinate above p: refused as not canonical
    w[k - 1, :8] = 0xFFFFFFFF
    both(w, k)
    with pytest.raises(ref.NotCanonical, match=f"entry {k - 1}: coordinate x"):
        ref.decode(cv, w)
    for other in {1, 2, 77, N_WINDOW} - {k}:  # two entries swapped: the first of the two is reported
        w = clean.copy()
        w[[k - 1, other - 1]] = w[[other - 1, k - 1]]
        both(w, min(k, other))
    w = clean.copy()  # one entry negated
    w[k - 1] = ref.encode(cv, (want[k - 1][0], p - want[k - 1][1]))
    both(w, k)
    w = clean.copy()  # one entry left in the other form
    w[k - 1] = ref.encode(cv, want[k - 1], mont=not cv["mont"])
    both(w, k)
    w = clean.copy()  # one entry replaced by another point of the curve that is no multiple in range
    w[k - 1] = ref.encode(cv, cv["g"])
    both(w, k)
    w = clean.copy()  # the entry and everything behind it shifted by one: T[d] = (d + 1) P from d = k on
    w[k - 1:] = np.stack([ref.encode(cv, pt) for pt in pts[k:N_WINDOW + 1]])
    both(w, k)


@pytest.mark.parametrize("cv", CASES)
def test_zero_row_is_not_a_point(windows, cv):
    base, pts, clean = windows[cv["name"]]
    w = clean.copy()
    w[41] = 0
    assert ref.check_window_words(cv, w, base) == 42


def test_cost_of_the_checkers_per_entry(windows):
    """prints the figures the module docstring records (pytest -s); no assertion on time"""
    lines = []
    for cv in (SECP256K1, SECP256R1, GRUMPKIN):
        base = windows[cv["name"]][0]
        words = np.stack([ref.encode(cv, pt) for pt in ref.multiples(cv, base, 65535)])
        t0 = time.perf_counter()
        got = ref.decode(cv, words)
        t1 = time.perf_counter()
        assert ref.check_multiples(cv, got, base) is None
        t2 = time.perf_counter()
        ref.check_exact(got, got)
        t3 = time.perf_counter()
        lines.append(f"  {cv['name']:10s} decode {1e6 * (t1 - t0) / 65535:.2f} us/entry, chord check {1e6 * (t2 - t1) / 65535:.2f} us/entry, exact compare {1e6 * (t3 - t2) / 65535:.2f} us/entry")
    t0 = time.perf_counter()
    for d in range(1, 41):
        ref.ec_mul(SECP256R1, d << 240 | 0xFFFF, SECP256R1["g"])
    lines.append(f"  one model point by double-and-add (256-bit scalar): {1e3 * (time.perf_counter() - t0) / 40:.2f} ms; one affine addition with its inversion: "
                 f"{1e6 * _time_add():.1f} us")
    print("\n" + "\n".join(lines))


def _time_add():
    a, b = SECP256K1["g"], ref.ec_add(SECP256K1, SECP256K1["g"], SECP256K1["g"])
    t0 = time.perf_counter()
    for _ in range(2000):
        ref.ec_add(SECP256K1, a, b)
    return (time.perf_counter() - t0) / 2000
