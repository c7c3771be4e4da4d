"""Every device-built lookup table read back entry by entry (acvm_debug_table_read: raw words, no arithmetic on the device) and compared bit for bit with the
integer model of tests/curve_table_ref.py, and which table served a solve (acvm_debug_batch_tables).

  ECDSA generator tables, win16: EVERY entry -- entry 1 of a window exactly, the rest by the inversion-free chord check, exact spot values on top.
  ped2, pedw: exact at the structural edges of their build kernels in every generator / plane, plus seeded random entries.
  who served: the table a handle reads is the one the test's tuning asks for, and the solve matches the oracle either way.

Case sizes come from the per-entry cost measured in tests/test_curve_tables_on_host.py (4.2 to 5.4 us per entry for decode + chord check).
A case skips only for lack of device memory, by the library's own rule restated below; a table that does not build although the memory is there fails."""
import gc
import random

import numpy as np
import pytest

import curve_table_ref as ref
from curve_table_ref import GRUMPKIN, SECP256K1, SECP256R1

pytestmark = pytest.mark.gpu

# sizes documented in acvm_amd/csrc/grumpkin_host.hpp
HOST_TABLE_BYTES = (30 * 512 + 4 * 32 * 255 + 45 + 3) * 64
WIN16_BYTES = 4 * 16 * 65535 * 64          # 268 MB
PEDW_BYTES = (2 * 11 << 24) * 64           # 23.6 GB; built only where a quarter of the device's memory stays free behind it


@pytest.fixture(scope="module")
def model(oracle):
    return ref.Model(ref.generators_from_oracle(oracle))


def mem_info():
    """(free, total) bytes of the current device from hipMemGetInfo of the HIP runtime the library itself is linked to -- the call its own rule makes, on the
    runtime instance that holds the tables (a second HIP runtime in the process, such as the one bundled with torch, need not see the device at all)."""
    import ctypes as C
    import acvm_amd
    acvm_amd.lib()
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    free, total = C.c_size_t(), C.c_size_t()
    assert C.CDLL(path).hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value, total.value


def release_all_tables():
    import acvm_amd
    gc.collect()  # handles other tests dropped without free()
    acvm_amd.release_tables(0)


def base_missing_bytes():
    import acvm_amd
    return 0 if acvm_amd.debug_table_info(ref.TABLE_PED)[1] else HOST_TABLE_BYTES + WIN16_BYTES


def need_win16():
    """win16 on the device under the default tuning, or a skip for lack of its 268 MB"""
    import acvm_amd
    assert acvm_amd.tuning_get("win16") == 1
    if acvm_amd.debug_table_info(ref.TABLE_WIN16)[1]:
        return
    release_all_tables()  # (a set built under win16 = 0 never gets the table)
    free, _ = mem_info()
    need = HOST_TABLE_BYTES + WIN16_BYTES
    if free < need:
        pytest.skip(f"win16 needs {need} bytes of device memory, {free} are free")


def pedw_skip_reason():
    """None when the library's rule allows the window table: table bytes plus a quarter of the device's memory free (beside the tables built on the way)"""
    import acvm_amd
    if acvm_amd.debug_table_info(ref.TABLE_PEDW)[1]:
        return None
    free, total = mem_info()
    need = PEDW_BYTES + total // 4 + base_missing_bytes()
    return None if free >= need else f"pedw needs {need} bytes of device memory free (its {PEDW_BYTES} plus a quarter of {total}), {free} are free"


def read(table, entries):
    import acvm_amd
    return acvm_amd.debug_table_read(table, entries)


# ---------------------------------------------------------------------------------------------- the ABI's own edges
def test_read_refuses_bad_indices_and_reports_built(model):
    import acvm_amd
    n, _ = acvm_amd.debug_table_info(ref.TABLE_PED2)
    assert n == 30 << 18
    with pytest.raises(acvm_amd.AcvmError, match="outside the ped2 table"):
        read(ref.TABLE_PED2, [0, n])
    with pytest.raises(acvm_amd.AcvmError, match="outside the pedw table"):
        read(ref.TABLE_PEDW, [1 << 40])
    got = ref.decode(GRUMPKIN, read(ref.TABLE_SKEW, [2, 0, 1, 2]))  # order and repeats of the request are kept
    assert got == [model.skew(2), model.skew(0), model.skew(1), model.skew(2)]
    assert acvm_amd.debug_table_info(ref.TABLE_SKEW)[1] and acvm_amd.debug_table_info(ref.TABLE_PED)[1]
    assert read(ref.TABLE_PED, []).shape == (0, 16)


def test_host_built_tables_on_the_device_every_entry(model):
    """the device copy of ped, win, small and skew in its storage form (Montgomery, canonical), all 48 048 entries"""
    assert ref.check_exact(ref.decode(GRUMPKIN, read(ref.TABLE_PED, np.arange(30 * 512))), [pt for row in model.ped_table() for pt in row]) is None
    win = ref.decode(GRUMPKIN, read(ref.TABLE_WIN, np.arange(4 * 32 * 255)))
    for b in range(4):
        for w in range(32):
            assert ref.check_multiples(GRUMPKIN, win[(b * 32 + w) * 255:(b * 32 + w + 1) * 255], model.shifted_base(GRUMPKIN, model.bases[b], 8 * w)) is None, (b, w)
    assert ref.decode(GRUMPKIN, read(ref.TABLE_SMALL, np.arange(45))) == [model.small(j, k) for j in range(3) for k in range(1, 16)]
    assert ref.decode(GRUMPKIN, read(ref.TABLE_SKEW, np.arange(3))) == [model.skew(j) for j in range(3)]


# ---------------------------------------------------------------------------------------------- ECDSA generator tables: every entry
GTAB_GROUP = 4  # windows per case: 4 x 65 536 entries x ~5 us


@pytest.mark.parametrize("j0", range(0, 16, GTAB_GROUP))
@pytest.mark.parametrize("curve", [0, 1], ids=["secp256k1-plain", "secp256r1-montgomery"])
def test_ecdsa_generator_table_every_entry(model, curve, j0):
    cv = (SECP256K1, SECP256R1)[curve]
    words = read(ref.TABLE_ECDSA_K1 + curve, np.arange(j0 << 16, (j0 + GTAB_GROUP) << 16, dtype=np.uint64)).reshape(GTAB_GROUP, 65536, 16)
    for j in range(j0, j0 + GTAB_GROUP):
        w = words[j - j0]
        assert not w[0].any(), f"window {j}: row d = 0 is not sixteen zero words"
        base = model.shifted_base(cv, cv["g"], 16 * j)
        bad = ref.check_window_words(cv, w[1:], base)  # entry 1 exactly, 2..65535 by the chord through entry 1 and the predecessor
        assert bad is None, f"{cv['name']} window {j}: entry d = {bad} is not d * 2^{16 * j} * G"
        spots = [2, 255, 256, 257, 0x8000, 0xFFFF]
        assert ref.decode(cv, w[spots]) == [model.gtab(cv, j, d) for d in spots], j


# ---------------------------------------------------------------------------------------------- win16: every entry
WIN16_GROUP = 8  # windows per case: 8 x 65 535 entries x ~5.4 us
# the digits at which grumpkin_win16_table_kernel changes its path: low byte zero, high byte zero, both set; 0xFFFF of base 3, window 15 is the table's last
# entry, the one whose block of 64 lanes is partly filled
WIN16_EDGE_DIGITS = [0x0100, 0xFF00, 1, 0xFF, 0x0101, 0xFFFF]


@pytest.mark.parametrize("w0", range(0, 16, WIN16_GROUP))
@pytest.mark.parametrize("b", range(4), ids=["G", "D0", "D3", "D6"])
def test_win16_every_entry(model, b, w0):
    import acvm_amd
    need_win16()
    first = (b * 16 + w0) * 65535
    words = read(ref.TABLE_WIN16, np.arange(first, first + WIN16_GROUP * 65535, dtype=np.uint64)).reshape(WIN16_GROUP, 65535, 16)
    for w in range(w0, w0 + WIN16_GROUP):
        base = model.shifted_base(GRUMPKIN, model.bases[b], 16 * w)
        bad = ref.check_window_words(GRUMPKIN, words[w - w0], base)
        assert bad is None, f"base {b} window {w}: entry d = {bad} is not d * 2^{16 * w} * P"
        assert ref.decode(GRUMPKIN, words[w - w0][[d - 1 for d in WIN16_EDGE_DIGITS]]) == [model.win16(b, w, d) for d in WIN16_EDGE_DIGITS], (b, w)
    if b == 3 and w0 + WIN16_GROUP == 16:
        n, built = acvm_amd.debug_table_info(ref.TABLE_WIN16)
        assert built and first + WIN16_GROUP * 65535 == n  # the last entry read above is the last of the table


# ---------------------------------------------------------------------------------------------- ped2: edges and samples, exact
def test_ped2_edges_and_samples(model):
    r = random.Random(0x9ED2)
    corners = (0, 1, 510, 511)
    want = [(g, a, b) for g in range(30) for a in corners for b in corners]
    for g in (0, 14, 15, 29):
        want += [(g, 0, b) for b in range(512)] + [(g, a, 0) for a in range(512)]
    want += [(r.randrange(30), r.randrange(512), r.randrange(512)) for _ in range(20000)]
    want += [(g, r.randrange(512), r.randrange(512)) for g in (14, 29) for _ in range(500)]  # the single-slice generators, beyond their share of the random ones
    words = read(ref.TABLE_PED2, [g << 18 | a << 9 | b for g, a, b in want])
    got = ref.decode(GRUMPKIN, words)
    bad = ref.check_exact(got, [model.ped2(g, a, b) for g, a, b in want])
    assert bad is None, f"ped2[g][a][b] at (g, a, b) = {want[bad]} is not endo((a+1) D[g]) + (b+1) D[g]"
    # g % 15 == 14: one slice only, the entry must not depend on b -- whole rows a against their entry b = 0, in the stored words
    for g in (14, 29):
        for a in (0, 1, 255, 511, r.randrange(512)):
            row = read(ref.TABLE_PED2, [g << 18 | a << 9 | b for b in range(512)])
            assert (row == row[0]).all(), (g, a)
            assert ref.decode(GRUMPKIN, row[:1]) == [ref.endo(model.ped(g, a + 1))], (g, a)
    for g in (13, 15):  # ... and does depend on it next door
        row = read(ref.TABLE_PED2, [g << 18 | 5 << 9 | b for b in range(512)])
        assert len({r_.tobytes() for r_ in row}) == 512, g


# ---------------------------------------------------------------------------------------------- pedw: edges and samples in every plane, exact
def pedw_values(j, rng):
    """the values of window j (bits [24 j, 24 j + 24) of the scalar) at which pedersen_window_table_kernel can go wrong"""
    full = (1 << 24) - 1
    vals = {0, full}
    vals |= {1 << k for k in range(24)} | {(1 << k) - 1 for k in range(1, 25)}
    for s in range(24 * j // 9, 30):  # (slice 29 does not exist: its bits are the ones the rule of the last window ignores)
        lo, hi = max(9 * s, 24 * j), min(9 * s + 9, 24 * j + 24)
        if lo >= hi:
            break
        mask = ((1 << (hi - lo)) - 1) << (lo - 24 * j)
        vals |= {mask, full ^ mask}  # the slice's piece all ones among zeros, all zeros among ones
        if lo > 24 * j:              # a slice border inside the window: the two values either side of it, alone and under ones
            q = lo - 24 * j
            vals |= {(1 << q) - 1, 1 << q, full ^ ((1 << q) - 1), full ^ (1 << q), ((1 << q) - 1) ^ 1, (1 << q) | 1}
    vals |= {rng.randrange(1 << 24) for _ in range(1000)}
    return sorted(vals)


@pytest.mark.parametrize("parity", [0, 1])
def test_pedw_edges_and_samples_in_every_plane(model, parity):
    """11 planes per parity = every (parity, window) plane of the table: the byte offset of plane k is k GiB, so the planes from the fifth on lie beyond 4 GiB
    and the last beyond 21 GiB"""
    reason = pedw_skip_reason()
    if reason:
        pytest.skip(reason)
    rng = random.Random(0x9ED3 + parity)
    want = [(j, v) for j in range(11) for v in pedw_values(j, rng)]
    words = read(ref.TABLE_PEDW, np.array([((parity * 11 + j) << 24) | v for j, v in want], dtype=np.uint64))  # one gather for the eleven planes
    got = ref.decode(GRUMPKIN, words)
    bad = ref.check_exact(got, [model.pedw(parity, j, v) for j, v in want])
    assert bad is None, f"pedw[{parity}][j][v] at (j, v) = ({want[bad][0]}, {want[bad][1]:#x}) is not what grumpkin_host.hpp defines"
    # no two of these entries coincide, but for the ignored top bits of the last window: the planes and values are really distinct reads
    assert len({w.tobytes() for w in words}) == len({(j, v & 0x1FFFFF if j == 10 else v) for j, v in want})


@pytest.mark.parametrize("parity", [0, 1])
def test_pedw_last_window(model, parity):
    """Window 10 holds bits 240..263 of the scalar, slices stop at bit 261. What a solve can reach (operands below 2^254: v < 2^14), every entry, exactly;
    beyond it the header's rule: bits 21..23 of v contribute nothing, so entry v is entry v mod 2^21, word for word, and the entries below 2^21 follow the
    definition (sampled)."""
    reason = pedw_skip_reason()
    if reason:
        pytest.skip(reason)
    plane = (parity * 11 + 10) << 24
    reach = ref.decode(GRUMPKIN, read(ref.TABLE_PEDW, np.arange(plane, plane + (1 << 14), dtype=np.uint64)))
    bad = ref.check_exact(reach, [model.pedw(parity, 10, v) for v in range(1 << 14)])
    assert bad is None, f"pedw[{parity}][10][{bad:#x}]"
    rng = random.Random(0x9ED4 + parity)
    lows = [0, 1, (1 << 14) - 1, 1 << 14, (1 << 21) - 1, 1 << 20, 0x155555, 0x0AAAAA] + [rng.randrange(1 << 21) for _ in range(300)]
    low_words = read(ref.TABLE_PEDW, [plane | v for v in lows])
    assert ref.check_exact(ref.decode(GRUMPKIN, low_words), [model.pedw(parity, 10, v) for v in lows]) is None
    for hi in range(1, 8):
        assert (read(ref.TABLE_PEDW, [plane | hi << 21 | v for v in lows]) == low_words).all(), hi


# ---------------------------------------------------------------------------------------------- who served
def solve_against_oracle(oracle, circ, ids, rows, expect_mask, mask_of_interest, skip_reason=None):
    """one handle under the CURRENT tuning: the tables it reads are the expected ones, and its witness maps are the oracle's"""
    import acvm_amd
    from acvm_amd.synth import values_from_rows
    B, values, data = len(rows), values_from_rows(rows), circ.to_bytes()
    batch = acvm_amd.Batch(acvm_amd.Circuit(data), B, ids)
    try:
        mask = batch.tables() & mask_of_interest
        if mask != expect_mask and skip_reason:
            pytest.skip(skip_reason)
        assert mask == expect_mask, f"the handle reads tables {mask:#x}, the tuning asks for {expect_mask:#x}"
        batch.set_initial_witness(values)
        batch.solve()
        gres = batch.results()
        gasg, gvals = batch.witness_map()
    finally:
        batch.free()
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values, B)
    for i in range(B):
        assert gres[i].as_tuple() == ores[i].as_tuple(), i
    nw = min(oasg.shape[1], gasg.shape[1])
    assert np.array_equal(oasg[:, :nw], gasg[:, :nw]) and np.array_equal(ovals[:, :nw], gvals[:, :nw])
    return ores


def test_pedersen_is_served_by_the_table_its_tuning_names(oracle):
    """two Pedersen records, 130 instances: under pedersen_window_bits = 24 the handle reads pedw and not ped2, under 0 ped2 and not pedw"""
    import acvm_amd
    from acvm_amd.acir import BlackBoxFuncCall as BB, Circuit, FunctionInput as FI
    P = GRUMPKIN["p"]
    r = random.Random(0x9ED5)
    circ = Circuit(7, [BB("Pedersen", {"inputs": [FI(1, 254), FI(2, 254)], "domain_separator": 0, "outputs": [4, 5]}),
                       BB("Pedersen", {"inputs": [FI(3, 254)], "domain_separator": 0, "outputs": [6, 7]})])
    rows = [[r.randrange(P) for _ in range(3)] for _ in range(130)]
    rows[0], rows[1], rows[2] = [0, 0, 0], [P - 1, P - 1, P - 1], [(1 << 253) - 1, 1 << 252, (1 << 24) - 1]
    both = acvm_amd.TABLE_BIT_PED2 | acvm_amd.TABLE_BIT_PEDW
    reason = pedw_skip_reason()  # (asked BEFORE the handle: the handle's own rows change what is free)
    with acvm_amd.tuning(pedersen_window_bits=0):
        ores = solve_against_oracle(oracle, circ, [1, 2, 3], rows, acvm_amd.TABLE_BIT_PED2, both)
    assert all(ores[i].status == 0 for i in range(130))
    with acvm_amd.tuning(pedersen_window_bits=24):
        solve_against_oracle(oracle, circ, [1, 2, 3], rows, acvm_amd.TABLE_BIT_PEDW, both, skip_reason=reason)


@pytest.mark.parametrize("win16", [1, 0])
def test_fixed_base_is_served_by_the_table_its_tuning_names(oracle, model, win16):
    """FixedBaseScalarMul + SchnorrVerify with the device's tables built under win16 = 1 / 0: the handle reads win16 or does not, its results are the oracle's,
    and the fixed-base product (probe 3) of a scalar that is ONE edge digit in ONE window is the model's k * P_b for every base and window"""
    import acvm_amd
    from acvm_amd.acir import BlackBoxFuncCall as BB, Circuit, FunctionInput as FI
    from acvm_amd.synth import grumpkin_rows
    n_in = 2 + 2 + 64 + 10
    ids = list(range(1, n_in + 1))
    out = n_in + 1
    circ = Circuit(out + 2, [BB("FixedBaseScalarMul", {"low": FI(1, 128), "high": FI(2, 128), "outputs": [out, out + 1]}),
                             BB("SchnorrVerify", {"public_key_x": FI(3, 254), "public_key_y": FI(4, 254), "signature": [FI(w, 8) for w in ids[4:68]],
                                                  "message": [FI(w, 8) for w in ids[68:]], "output": out + 2})])
    rows = grumpkin_rows(70, n_pedersen_inputs=0, first_instance=8)
    for i, d in enumerate(WIN16_EDGE_DIGITS):  # the edge digits in the circuit's own scalars too, in windows 0, 4, 7, 9 and 14
        rows[2 * i][0], rows[2 * i][1] = d | d << 112, d << 16
        rows[2 * i + 1][0], rows[2 * i + 1][1] = d << 64, d << 96
    release_all_tables()
    try:
        skip = None
        if win16:
            free, _ = mem_info()
            if free < HOST_TABLE_BYTES + WIN16_BYTES:
                skip = f"win16 needs {HOST_TABLE_BYTES + WIN16_BYTES} bytes of device memory, {free} are free"
        with acvm_amd.tuning(win16=win16):
            ores = solve_against_oracle(oracle, circ, ids, rows, acvm_amd.TABLE_BIT_WIN16 if win16 else 0, acvm_amd.TABLE_BIT_WIN16, skip_reason=skip)
            assert any(ores[i].status == 0 for i in range(70))
            assert acvm_amd.debug_table_info(ref.TABLE_WIN16)[1] == bool(win16)
            for b in range(4):
                for w in range(16):
                    for d in WIN16_EDGE_DIGITS:
                        assert acvm_amd.debug_grumpkin(3, b, [d << (16 * w)]) == model.win16(b, w, d), (b, w, hex(d))
            assert acvm_amd.debug_table_info(ref.TABLE_WIN16)[1] == bool(win16)  # (the probes read the set the handle read)
    finally:
        release_all_tables()  # whoever comes next builds the set under its own tuning
