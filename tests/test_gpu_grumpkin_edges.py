"""The Grumpkin opcodes (acvm_amd/csrc/ops_grumpkin.hpp, kernels_grumpkin.hip, the black-box ops of the Brillig VM) on the device against Python integers
(tests/grumpkin_ref.py), on the lists of tests/grumpkin_cases.py -- inputs that random values never reach. Integers first, the CPU oracle second.

  formulas   gj_dbl, gj_add_aff29, gj_add and gj_to_aff through acvm_debug_grumpkin_items, one lane per item: the same-x branches (doubling, opposite
             points), infinity as Z = 0 and as Z = p, Y = 0 (mod p), every coordinate of the exceptional items in BOTH representatives v and v + p of the
             lazy 29-bit form. Every output limb is below 2^29 and every output value below 2p (the class the header documents); the group element is
             the model's, and Z = 0 (mod p) exactly when the model says infinity.
  split      glv_split + signed_windows5: magnitudes, signs and all 2 x 26 digits equal the restatement; e * pk equals the affine product.
  R          the point e pk + s G of SchnorrVerify, where the final addition doubles (s = e sk) or returns infinity (s = -e sk): at the opcode's output
             both read 0 whatever the formulas did.
  opcodes    every list through the level kernels and the exact kernels, the Pedersen lists again under every kernel shape (one or four waves, bundled
             or not, 24-bit windows or slice pairs) and the fixed-base and Schnorr lists under both window widths, with the table actually read asserted.
  Brillig    a subset of each list through the BlackBox bytecode, a doubling row and an infinity row of Schnorr included.
tests/test_grumpkin_cases.py (no GPU) proves what the lists cover and that the oracle agrees with the integers."""
import functools

import numpy as np
import pytest

import grumpkin_cases as gc
import grumpkin_ref as gr
from acvm_amd.acir import P, Brillig, Circuit, Expression as E
from acvm_amd.synth import values_from_rows
from curve_table_ref import GRUMPKIN, ec_mul
from grumpkin_ref import LAMBDA, Q
from test_gpu_curve_tables import HOST_TABLE_BYTES, WIN16_BYTES, mem_info, pedw_skip_reason, release_all_tables
from test_gpu_opcodes import both_paths

pytestmark = pytest.mark.gpu
W = E.from_witness
LIMB = 1 << 29


def words8(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def int8(words):
    return sum(int(x) << (32 * i) for i, x in enumerate(words))


# ---------------------------------------------------------------------------------------------- formulas
def class_a(limbs, at):
    """the coordinate of nine output limbs, after the two checks on its form: limbs below 2^29, value below 2p"""
    assert all(int(x) < LIMB for x in limbs), f"{at}: a limb at or above 2^29: {[hex(int(x)) for x in limbs]}"
    v, raw = gc.from_limbs29(limbs)
    assert raw < 2 * P, f"{at}: the value {raw:#x} is not below 2p"
    return v


def items_words(items):
    return np.array([[w for v, r in zip(it.coords, it.reps) for w in gc.limbs29(v, r)] for it in items], dtype=np.uint32)


@pytest.mark.parametrize("which", ["dbl", "add_aff29", "add"])
def test_point_formulas_on_both_representatives(which):
    import acvm_amd
    items = gc.formula_items(which)
    out = acvm_amd.debug_grumpkin_items({"dbl": 0, "add_aff29": 1, "add": 2}[which], items_words(items))
    for n, (it, o) in enumerate(zip(items, out)):
        at = f"{which} item {n} ({it.note}, representatives {it.reps})"
        X, Y, Z = (class_a(o[9 * i:9 * i + 9], at) for i in range(3))
        got = gc.jac_to_affine(X, Y, Z)
        assert (Z == 0) == (it.want is None), f"{at}: Z = {Z:#x}, the model says {'infinity' if it.want is None else 'a finite point'}"
        assert got == it.want, f"{at}: the device has {got}, the model {it.want}"
        if which == "add_aff29":
            if it.note == "ordinary":   # zr = Z3 / Z1
                zr = class_a(o[27:36], at + ", zr")
                assert zr * it.coords[2] % P == Z, f"{at}: zr = {zr:#x} is not Z3 / Z1"
            else:
                assert not o[27:36].any(), f"{at}: zr written off the ordinary path"


def test_to_affine_on_both_representatives():
    """gj_to_aff: canonical storage-form coordinates of the model's point, (0, 0) and the flag for Z = 0 and for Z = p"""
    import acvm_amd
    items = gc.formula_items("dbl")
    out = acvm_amd.debug_grumpkin_items(3, items_words(items))
    n_inf = 0
    for n, (it, o) in enumerate(zip(items, out)):
        x, y, inf = int8(o[0:8]), int8(o[8:16]), int(o[16])
        assert x < P and y < P, (n, it.note)
        want = gc.jac_to_affine(*it.coords)
        assert inf == (want is None) and (x * gc.MONT_INV % P, y * gc.MONT_INV % P) == (want or (0, 0)), (n, it.note, it.reps)
        n_inf += inf
    assert n_inf >= 32


def test_ladder_terms():
    import acvm_amd
    R = gr.ref()
    vs = [0, 1, 2, 3, 14, 15, 16, 17, 18, 30, 31, 32, 33, 47, 48, 49, (1 << 128) - 1, 1 << 128, (1 << 253) + 15, (1 << 253) + 16, P - 1, P - 2, P - 16, P - 17, gc.ALL, 0x1234567 << 200]
    for j in range(3):
        out = acvm_amd.debug_grumpkin_items(5, np.array([words8(v) for v in vs], dtype=np.uint32), param=j)
        for v, o in zip(vs, out):
            assert (int8(o[0:8]), int8(o[8:16]), int(o[16])) == (*R.ladder_term(v, j), 0), (hex(v), j)


# ---------------------------------------------------------------------------------------------- the scalar split
@functools.lru_cache(maxsize=None)
def all_split_scalars():
    ks = [k for k, _ in gc.split_scalars()]
    for n in gc.MSG_LENGTHS:
        ks += [int.from_bytes(s.sig[32:], "big") % Q for s in gc.signed_messages(n)]
    return tuple(dict.fromkeys(ks))


def test_split_magnitudes_signs_and_digits():
    import acvm_amd
    ks = all_split_scalars()
    out = acvm_amd.debug_grumpkin_items(4, np.array([words8(k) for k in ks], dtype=np.uint32))
    # a device digit is magnitude | 32 if negative. A window of 31 plus a carry leaves the magnitude 0 WITH the sign bit (32 - 32 = 0, borrowed): a digit
    # zero that the ladder skips like any other (it tests the magnitude), so digits are compared by value, and the form is pinned as it is
    dec = lambda x: -(int(x) & 31) if int(x) & 32 else int(x)  # noqa: E731
    classes, minus_zero = set(), 0
    for k, o in zip(ks, out):
        k1, k2 = gr.glv_split(k)
        got = (sum(int(x) << (32 * i) for i, x in enumerate(o[0:4])), sum(int(x) << (32 * i) for i, x in enumerate(o[4:8])), int(o[8]), int(o[9]))
        assert got == (abs(k1), abs(k2), int(k1 < 0), int(k2 < 0)), f"k = {k:#x}: the device splits into {got}, the definitions into {(k1, k2)}"
        assert all(int(x) < 64 and (int(x) & 31) <= 16 for x in o[10:62]), f"k = {k:#x}: a digit outside magnitude 0..16 with one sign bit"
        assert [dec(x) for x in o[10:36]] == gr.signed_windows5(abs(k1)), f"k = {k:#x}: digits of k1"
        assert [dec(x) for x in o[36:62]] == gr.signed_windows5(abs(k2)), f"k = {k:#x}: digits of k2"
        assert all(int(x) != 48 for x in o[10:62]), f"k = {k:#x}: -16 is no digit (a window of 16 stays +16)"
        minus_zero += sum(1 for x in o[10:62] if int(x) == 32)
        classes.add((int(o[8]), int(o[9]), k2 == 0))
    assert classes == {(0, 1, False), (0, 0, False), (0, 0, True)}   # neg1 never; k2 < 0, k2 > 0, k2 = 0
    assert minus_zero >= 1   # (2^253 has one: the list reaches the borrowed zero)


def test_var_base_product_on_every_split_class():
    """e * pk through the window-table path (s = 0: R = e pk + 0 G) on pk = G, -G, lambda G and a random multiple, over every scalar of the split list;
    and the one-lane probe 8 on the crafted scalars with k2 > 0"""
    import acvm_amd
    R = gr.ref()
    ks = all_split_scalars()
    pks = [gr.G, gr.neg(gr.G), R.mul_g(LAMBDA), R.mul_g(0xC0FFEE1234567 << 130 | 0x77)]
    items = [(pk, k) for pk in pks for k in ks]
    out = acvm_amd.debug_grumpkin_items(6, np.array([words8(pk[0]) + words8(pk[1]) + words8(0) + words8(k) for pk, k in items], dtype=np.uint32))
    for (pk, k), o in zip(items, out):
        want = ec_mul(GRUMPKIN, k, pk)
        assert (int8(o[0:8]), int8(o[8:16]), int(o[16])) == (*(want or (0, 0)), int(want is None)), (pk == gr.G, hex(k))
    crafted = [k for k, note in gc.split_scalars() if "k2 > 0" in note]
    assert len(crafted) >= 8
    for k in crafted:
        assert acvm_amd.debug_grumpkin(8, 0, [k, pks[3][0], pks[3][1]]) == ec_mul(GRUMPKIN, k, pks[3]), hex(k)


# ---------------------------------------------------------------------------------------------- R = e pk + s G
@pytest.mark.parametrize("table", [True, False], ids=["window table", "double-and-add"])
def test_schnorr_point_where_the_final_addition_doubles_or_cancels(table):
    import acvm_amd
    triples = gc.r_triples()
    words = np.array([words8(t.pk[0]) + words8(t.pk[1]) + words8(t.s) + words8(t.e) for t in triples], dtype=np.uint32)
    out = acvm_amd.debug_grumpkin_items(6 if table else 7, words)
    for t, o in zip(triples, out):
        got = (int8(o[0:8]), int8(o[8:16]), int(o[16]))
        assert got == (*(t.want or (0, 0)), int(t.want is None)), f"{t.note}: the device has {got}, the model {t.want}"


# ---------------------------------------------------------------------------------------------- opcodes
_EXPECTED = {}


def expected_arrays(case, nw):
    """the expectation of a case as the arrays Batch.witness_map returns: (assigned [B, nw], values [B, nw, 32]); kept per case object"""
    if (id(case), nw) not in _EXPECTED:
        asg = np.zeros((len(case.rows), nw), dtype=np.uint8)
        vals = np.zeros((len(case.rows), nw, 32), dtype=np.uint8)
        for j, x in enumerate(case.expect):
            for w, v in x.witnesses.items():
                asg[j, w] = 1
                vals[j, w] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
        _EXPECTED[(id(case), nw)] = (case, asg, vals)
    return _EXPECTED[(id(case), nw)][1:]


def device_against_integers(case, force_slow, expect_tables=None):
    """expect_tables: (mask of interest, expected mask, skip reason or None) of the tables the handle must read"""
    import acvm_amd
    batch = acvm_amd.Batch(acvm_amd.Circuit(case.circuit.to_bytes()), len(case.rows), case.ids)
    try:
        if expect_tables:
            interest, want, skip = expect_tables
            mask = batch.tables() & interest
            if mask != want and skip:
                pytest.skip(skip)
            assert mask == want, f"{case.name}: the handle reads tables {mask:#x}, the tuning asks for {want:#x}"
        batch.set_force_slow_path(force_slow)
        batch.set_initial_witness(values_from_rows(case.rows))
        batch.solve()
        res = batch.results()
        asg, vals = batch.witness_map()
    finally:
        batch.free()
    who = "device, exact kernels" if force_slow else "device, level kernels"
    nw = asg.shape[1]
    assert nw > max(max(x.witnesses) for x in case.expect)
    want_asg, want_vals = expected_arrays(case, nw)
    heads_agree = all((r.status, r.err) == (x.status, x.err) and (x.status != gc.ST_FAILURE or r.opcode_index == x.opcode_index) for r, x in zip(res, case.expect))
    if heads_agree and np.array_equal(asg != 0, want_asg != 0) and np.array_equal(vals * (want_asg[:, :, None] != 0), want_vals):
        return
    got = []  # something differs: row by row, so that the message names the row, the witness, got and want
    for j, r in enumerate(res):
        got.append((r.status, r.err, r.opcode_index, {int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])}))
    gc.compare(case, got, who)
    raise AssertionError(f"{case.name}: {who} differs from the expectation outside what compare() looks at")


@pytest.mark.parametrize("name", list(gc.CASE_BUILDERS))
def test_every_list_on_both_paths(oracle, name):
    """integers first, on the level kernels and on the exact kernels (set_force_slow_path); then the oracle, both paths, messages and aux words included"""
    case = gc.case(name)
    device_against_integers(case, False)
    device_against_integers(case, True)
    both_paths(oracle, case.circuit, case.ids, case.rows)


@pytest.mark.parametrize("name,what", gc.PERTURBATIONS)
def test_each_list_bites_on_the_device(name, what):
    """one expected value per list moved (a coordinate, a status, a verdict, a failing opcode): the comparison of the device's run with the integers fails
    and names that row, on the level kernels and on the exact kernels"""
    j, bad = gc.perturbed(name, what)
    for force_slow in (False, True):
        with pytest.raises(AssertionError, match=f"row {j} "):
            device_against_integers(bad, force_slow)


@pytest.mark.parametrize("window_bits", [24, 0])
@pytest.mark.parametrize("bundle", [0, 2])
@pytest.mark.parametrize("waves", [1, 4])
def test_pedersen_lists_under_every_kernel_shape(waves, bundle, window_bits):
    """the quad kernel with one wave and with four (whose serial tail rotates over the waves), the bundle kernel, the 24-bit window walk and the 18-bit
    pair walk, each on the three Pedersen lists: 321, 130 and 67 instances"""
    import acvm_amd
    both = acvm_amd.TABLE_BIT_PED2 | acvm_amd.TABLE_BIT_PEDW
    reason = pedw_skip_reason() if window_bits else None  # (asked BEFORE the handle: the handle's own rows change what is free)
    with acvm_amd.tuning(pedersen_waves=waves, pedersen_bundle=bundle, pedersen_window_bits=window_bits):
        for name in gc.PEDERSEN_CASES:
            device_against_integers(gc.case(name), False, (both, acvm_amd.TABLE_BIT_PEDW if window_bits else acvm_amd.TABLE_BIT_PED2, reason))


@pytest.mark.parametrize("win16", [1, 0])
def test_fixed_base_and_schnorr_lists_under_both_window_widths(win16):
    """fixed_base_mul walks 16 windows of 16 bits when the device holds win16 and 32 of 8 bits otherwise: the fixed-base list (every digit of either width at
    its ends) and the Schnorr lists whose s sits on the exceptional branches, with the set of tables built under the tuning asked for"""
    import acvm_amd
    release_all_tables()
    try:
        skip = None
        if win16:
            free, _ = mem_info()
            if free < HOST_TABLE_BYTES + WIN16_BYTES:
                skip = f"win16 needs {HOST_TABLE_BYTES + WIN16_BYTES} bytes of device memory, {free} are free"
        with acvm_amd.tuning(win16=win16):
            for name in ("fixed base", "schnorr rejecting", "schnorr accepting, 33 bytes"):
                device_against_integers(gc.case(name), False, (acvm_amd.TABLE_BIT_WIN16, acvm_amd.TABLE_BIT_WIN16 if win16 else 0, skip))
    finally:
        release_all_tables()  # whoever comes next builds the set under its own tuning


# ---------------------------------------------------------------------------------------------- the Brillig VM's black-box ops
def test_brillig_fixed_base_and_pedersen(oracle):
    """the bytecode shapes of tests/test_gpu_brillig.py test_grumpkin_black_box_ops: the whole fixed-base list (a refusal is BrilligFunctionFailed there),
    and Pedersen with two and with five inputs over the slice / pair / window values, the hash index a register: 0, 1, 3, 2^32 - 1, and 2^32 (refused)"""
    R = gr.ref()
    fixed = Brillig(inputs=[W(1), W(2)], outputs=[[3, 4]], bytecode=[("Const", 2, 50), ("BlackBox", "FixedBaseScalarMul", 0, 1, 2, 2), ("Mov", 0, 2), ("Stop",)])
    rows = [list(r) for r in gc.fixed_base_case().rows]
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(Circuit(4, [fixed]).to_bytes()), [1, 2], values_from_rows(rows), len(rows))
    for j, (lo, hi) in enumerate(rows):
        what, pt = R.fixed_base(lo, hi)
        if what == gr.FB_OK:
            assert ores[j].status == 0 and tuple(int.from_bytes(ovals[j, w].tobytes(), "big") for w in (3, 4)) == pt, (j, hex(lo), hex(hi))
        else:
            assert ores[j].err == oracle.E_BRILLIG_FAILED, (j, what)
    both_paths(oracle, Circuit(4, [fixed]), [1, 2], rows)

    vals = [v for v, _ in gc.pedersen_values()]
    for n in (2, 5):
        ids = list(range(1, n + 2))
        ped = Brillig(inputs=[[W(w) for w in ids[:n]], W(n + 1)], outputs=[[n + 2, n + 3]],
                      bytecode=[("Const", 2, n), ("Const", 3, 60), ("BlackBox", "Pedersen", 0, 2, 1, 3, 2), ("Mov", 0, 3), ("Stop",)])
        rows = [[vals[(n * j + i) % len(vals)] for i in range(n)] + [(gc.HASH_INDICES + [1 << 32])[j % 5]] for j in range(67)]
        circ = Circuit(n + 3, [ped])
        ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(circ.to_bytes()), ids, values_from_rows(rows), len(rows))
        for j, row in enumerate(rows):
            if row[n] >> 32:
                assert ores[j].err == oracle.E_BRILLIG_FAILED, j
            else:
                assert ores[j].status == 0 and tuple(int.from_bytes(ovals[j, w].tobytes(), "big") for w in (n + 2, n + 3)) == R.pedersen(row[:n], row[n]), (j, n)
        both_paths(oracle, circ, ids, rows)


def test_brillig_schnorr_on_the_exceptional_rows(oracle):
    """SchnorrVerify through the VM (double-and-add for e pk: no window table) on accepting rows and on rejecting rows of every reason, the row whose final
    addition doubles and the row whose R is the point at infinity among them"""
    acc, rej = gc.schnorr_accepting_case(33), gc.schnorr_rejecting_case()
    picked = [(acc, j) for j in range(0, len(acc.rows), 5)][:8]
    n_reasons = next(j for j, n in enumerate(rej.notes) if n.startswith("key 1"))
    picked += [(rej, j) for j in range(2 * n_reasons)]
    notes = [c.notes[j] for c, j in picked]
    assert any("doubles" in n for n in notes) and any("infinity" in n for n in notes) and any("pk = (0, 0)" in n for n in notes) and any("s = q" in n for n in notes)
    n_msg = 33
    ids = list(range(1, 2 + n_msg + 64 + 1))
    sch = Brillig(inputs=[W(1), W(2), [W(w) for w in ids[2:2 + n_msg]], [W(w) for w in ids[2 + n_msg:]]], outputs=[120],
                  bytecode=[("Const", 4, n_msg), ("Const", 5, 64), ("BlackBox", "SchnorrVerify", 0, 1, 2, 4, 3, 5, 6), ("Mov", 0, 6), ("Stop",)])
    circ = Circuit(120, [sch])
    rows, want = [], []
    for c, j in picked:   # the lists keep pk, the signature, the message; the VM's arrays come message first
        row = c.rows[j]
        rows.append(row[:2] + row[66:66 + n_msg] + row[2:66])
        want.append(c.expect[j].witnesses[max(c.expect[j].witnesses)])
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(circ.to_bytes()), ids, values_from_rows(rows), len(rows))
    for j in range(len(rows)):
        assert ores[j].status == 0 and oasg[j, 120] and int.from_bytes(ovals[j, 120].tobytes(), "big") == want[j], (j, notes[j])
    assert sum(want) >= 8 and len(want) - sum(want) >= 20
    both_paths(oracle, circ, ids, rows)
