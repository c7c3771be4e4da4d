"""Case list and integer reference of the precomputed coefficient x row reduction (acvm_amd/csrc/fr_device.hpp fr29_lin_add, lin_table.hpp), shared by
the host run (tests/test_lin_table_on_host.py, tools/lin_table_host_test.hip) and the device probe (tests/test_gpu_lin_table.py, acvm_debug_lin_add).
An item is one lane: one or two rows and a lazy sum h; the 64 items of a group share their one or two coefficients, as the lanes of a wave do."""
import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M29 = (1 << 29) - 1
ROW_SPECIALS = (0, 1, P - 1, P, (1 << 256) - 1)
COEF_SPECIALS = (1, 2, P - 1)


def words(v, n=8):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def cases(n_items, seed=1):
    """(n_terms [G], coef [G][2][8], rows [n][2][8], h [n][9]) as uint32 arrays, and the same as Python integers (coefs [G][2], rows [n][2])"""
    rng = np.random.default_rng(seed)
    n_groups = (n_items + 63) // 64

    def rnd256():
        return int.from_bytes(rng.bytes(32), "little")

    coefs, n_terms = [], []
    for g in range(n_groups):
        if g < 6:  # every special coefficient in either place, with one term and with two
            pair = (COEF_SPECIALS[g % 3], COEF_SPECIALS[(g + 1) % 3])
        elif g % 4 == 0:
            pair = (COEF_SPECIALS[(g // 4) % 3], rnd256() % P)
        else:
            pair = (rnd256() % P, rnd256() % P)
        coefs.append(pair)
        n_terms.append(1 + (g // 3) % 2 if g < 6 else 1 + g % 2)
    rows, hs = [], np.zeros((n_items, 9), dtype=np.uint32)
    rand_h = rng.integers(0, 1 << 32, size=(n_items, 9), dtype=np.uint64).astype(np.uint32)
    for j in range(n_items):
        a, b = j % 7, (j // 21 + 3 * j) % 7  # five specials and two random rows in either place; j % 7 against (j // 7) % 3 meets every kind of h
        rows.append((ROW_SPECIALS[a] if a < 5 else rnd256(), ROW_SPECIALS[b] if b < 5 else rnd256()))
        kind = (j // 7) % 3
        if kind == 1:
            hs[j] = 0xFFFFFFFF
        elif kind == 2:
            hs[j] = rand_h[j]
    coef_w = np.array([[words(c) for c in pair] for pair in coefs], dtype=np.uint32)
    row_w = np.array([[words(x) for x in pair] for pair in rows], dtype=np.uint32)
    return np.array(n_terms, dtype=np.uint32), coef_w, row_w, hs, coefs, rows


def table_of(c):
    """81 words: word [9 k + i] = limb k of c 2^(29 i + 58) mod p"""
    out = [0] * 81
    for i in range(9):
        ci = c * pow(2, 29 * i + 58, P) % P
        for k in range(9):
            out[9 * k + i] = (ci >> (29 * k)) & M29
    return out


def check_tables(n_terms, coefs, tables):
    for g, pair in enumerate(coefs):
        for t in range(int(n_terms[g])):
            assert tables[g][t].tolist() == table_of(pair[t]), (g, t, pair[t])


def check_results(n_terms, coefs, rows, hs, out):
    """Every item: limbs normalised below the top one, result = T + h (the top limb counts modulo 2^32, as in every scan of fr_device.hpp) with
    T = sum c x mod p and T < p (1 + 2^-25)."""
    bound = P + (P >> 25)
    hs, out = hs.astype(object), out.astype(object)
    w = np.array([1 << (29 * i) for i in range(9)], dtype=object)
    hv, rv = (hs * w).sum(axis=1), (out * w).sum(axis=1)
    assert int((np.asarray(out[:, :8], dtype=np.uint64) >> 29).max()) == 0, "a limb below the top one is not normalised"
    worst = 0
    for j in range(len(rows)):
        g = j // 64
        want = sum(coefs[g][t] * rows[j][t] for t in range(int(n_terms[g]))) % P
        T = (int(rv[j]) - int(hv[j])) % (1 << 264)
        assert T % P == want, (j, "residue")
        assert T < bound, (j, "bound", T / P)
        worst = max(worst, T)
    return worst / P
