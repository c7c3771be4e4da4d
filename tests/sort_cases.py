"""One builder of the rows that random inputs never bring to Directive::PermutationSort (acvm_amd/csrc/ops_sort.hpp op_perm_sort, which runs in the
scratch-carrying kernel of kernels_hash.hip, and the reservation of plan.cpp), with every expected outcome from the Python model of the reference
(tests/sort_ref.py): no oracle and no device here. tests/test_sort_cases.py runs the lists through the CPU oracle and asserts what they cover;
tests/test_gpu_sort_edges.py runs them on the device.

A list is a tuple of cases; a case is (name, circuit, ids, rows, expect, notes, filler).

  A  permutations: every one for n = 0 .. 6; structured ones (identity, reverse, rotations, the moves of the single wires, riffles, bit reversal, ties)
     for n around every power of two up to 257
  B  the comparator: keys that differ in one limb, 0 / 1 / p - 1 / (p +- 1) / 2, key expressions that wrap past p, every shape of sort_by, a column past
     the tuple behind a deciding column
  C  bits: fewer and more witnesses than switches, pre-assigned bits, one witness twice, a bit that is an input
  D  an input expression with an unassigned witness
  E  two sorts beside a mixed-width SHA256 and a variable-length Keccak in one scratch-carrying launch"""
import collections
import functools
import itertools
import random

import sort_ref as sr
from acvm_amd.acir import P, BlackBoxFuncCall as BB, Circuit, Expression as E, FunctionInput as FI, PermutationSort

SEED = 20264
W, K = E.from_witness, E.constant
SMALL_N = tuple(range(7))
LARGE_N = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)

Case = collections.namedtuple("Case", "name circuit ids rows expect notes filler")


def _case(name, circ, ids, rows, notes, filler=None, max_rows=200):
    assert len(rows) == len(notes) and 0 < len(rows) <= max_rows, (name, len(rows))
    assert all(len(row) == len(ids) and all(0 <= v < P for v in row) for row in rows), name
    expect = [sr.run(circ, dict(zip(ids, row))) for row in rows]
    if filler is not None:
        assert expect[filler].status == sr.ST_SOLVED, (name, "the filler row does not pass")
    return Case(name, circ, list(ids), [list(r) for r in rows], expect, list(notes), filler)


def padded(case, n):
    """the case with passing rows IN FRONT up to n rows, so that the rows the case is about lie in the last, partial wave"""
    k = n - len(case.rows)
    if k <= 0 or case.filler is None:
        return case
    f = case.filler
    return case._replace(rows=[case.rows[f]] * k + case.rows, expect=[case.expect[f]] * k + case.expect, notes=["filler"] * k + case.notes, filler=0)


def describe(case, j):
    return f"{case.name} row {j} ({case.notes[j]})"


def compare(case, got, who, expect=None):
    """got: (results, assigned [B, nw], values [B, nw, 32] big-endian); every field of the model's expectation, the whole map included"""
    import numpy as np
    res, asg, vals = got
    expect = expect or case.expect
    nw = asg.shape[1]
    assert nw > case.circuit.current_witness_index
    want_asg = np.zeros((len(expect), nw), dtype=np.uint8)
    want_vals = np.zeros((len(expect), nw, 32), dtype=np.uint8)
    for j, want in enumerate(expect):
        at = describe(case, j)
        assert tuple(res[j].as_tuple()) == tuple(want[:5]), f"{at}: {who} (status, error, opcode, aux0, aux1) {tuple(res[j].as_tuple())}, want {tuple(want[:5])}"
        if want.message is not None:
            assert res[j].message == want.message, f"{at}: {who} message {res[j].message!r}, want {want.message!r}"
        for w, x in want.witnesses.items():
            want_asg[j, w] = 1
            if x:
                want_vals[j, w] = np.frombuffer(x.to_bytes(32, "big"), dtype=np.uint8)
    bad = np.argwhere((asg != 0) != (want_asg != 0))
    if bad.size == 0:
        bad = np.argwhere((vals * (want_asg[:, :, None] != 0) != want_vals).any(axis=2))
    if bad.size:
        j, w = (int(x) for x in bad[0])
        g = int.from_bytes(vals[j, w].tobytes(), "big") if asg[j, w] else None
        x = expect[j].witnesses.get(w)
        raise AssertionError(f"{describe(case, j)}: witness {w}: {who} " + (hex(g) if g is not None else "unassigned") + ", want " + (hex(x) if x is not None else "unassigned")
                             + f" ({len(bad)} differ)")


def sort_circuit(n_inputs, elements, tuple_, sort_by, n_bits=None, bits=None, before=(), after=()):
    """one sort; bits: the witnesses (default: n_bits fresh ones, as many as the network has switches)"""
    nb = sr.switch_count(len(elements)) if n_bits is None else n_bits
    if bits is None:
        bits = list(range(n_inputs + 1, n_inputs + 1 + nb))
    top = max([n_inputs] + list(bits))
    return Circuit(top, list(before) + [PermutationSort([list(e) for e in elements], tuple_, list(bits), list(sort_by))] + list(after)), list(bits)


# ---------------------------------------------------------------------------------------------------------------- A: permutations
@functools.lru_cache(maxsize=None)
def every_permutation_case(n):
    """n keys (witnesses 1..n; one spare input where n = 0), a row per permutation of 0 .. n - 1"""
    n_in = max(n, 1)
    circ, _ = sort_circuit(n_in, [[W(1 + i)] for i in range(n)], 1, [0])
    perms = list(itertools.permutations(range(n)))
    rows = [list(p) + [0] * (n_in - n) for p in perms]
    if n <= 1:
        rows = rows * 3
    return _case(f"A, every permutation of {n}", circ, list(range(1, n_in + 1)), rows, [str(list(r[:n])) for r in rows], filler=0, max_rows=720)


def structured(n, rng):
    """[(name, keys)]: the sorted order of the keys is the named permutation's inverse (both are in the list where they differ in kind)"""
    ident = list(range(n))
    out = [("identity", ident), ("reverse", ident[::-1]), ("rotation by +1", ident[-1:] + ident[:-1]), ("rotation by -1", ident[1:] + ident[:1]),
           ("first two swapped", [1, 0] + ident[2:]), ("last two swapped", ident[:-2] + [n - 1, n - 2]), ("last to front", [n - 1] + ident[:-1]),
           ("first to last", ident[1:] + [0])]
    riffle = ident[0::2] + ident[1::2]
    inverse = [0] * n
    for i, v in enumerate(riffle):
        inverse[v] = i
    out += [("even / odd riffle", riffle), ("the riffle's inverse", inverse)]
    if n & (n - 1) == 0:
        bits = n.bit_length() - 1
        out.append(("bit reversal", [int(format(i, f"0{bits}b")[::-1], 2) for i in ident]))
    out += [("all keys equal", [5] * n), ("two keys alternating", [i % 2 for i in ident])]
    for k in range(3):
        keys = ident[:]
        rng.shuffle(keys)
        out.append((f"random {k}", keys))
    return out


@functools.lru_cache(maxsize=None)
def structured_case(n):
    rng = random.Random(SEED + n)
    circ, _ = sort_circuit(n, [[W(1 + i)] for i in range(n)], 1, [0])
    rows, notes = [], []
    for k, (name, keys) in enumerate(structured(n, rng)):
        stride = 1 if k % 2 else rng.randrange(1, P // (n + 1))   # every other row spreads the keys over all eight limbs
        rows.append([v * stride for v in keys])
        notes.append(name)
    return _case(f"A, n = {n}", circ, list(range(1, n + 1)), rows, notes, filler=0)


# ---------------------------------------------------------------------------------------------------------------- B: the comparator
@functools.lru_cache(maxsize=None)
def limb_case():
    """nine keys that are equal but for one 32-bit limb, for each of the eight limbs (twice: the differing limb ascending against the order of the others'
    would-be order, and shuffled); the keys 0, 1, p - 1, (p - 1) / 2, (p + 1) / 2 among others"""
    n = 9
    rng = random.Random(SEED + 1000)
    circ, _ = sort_circuit(n, [[W(1 + i)] for i in range(n)], 1, [0])
    rows, notes = [], []
    for limb in range(8):
        base = rng.randrange(P) & ~(0xFFFFFFFF << (32 * limb)) & ((1 << 253) - 1)
        for how in ("descending", "shuffled"):
            d = list(range(n, 0, -1))
            if how == "shuffled":
                rng.shuffle(d)
            rows.append([base | (x << (32 * limb)) for x in d])
            notes.append(f"the keys differ in limb {limb} only, {how}")
    special = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]
    for k in range(4):
        keys = special + [rng.randrange(P) for _ in range(n - 5)]
        rng.shuffle(keys)
        rows.append(keys)
        notes.append("0, 1, p - 1, (p - 1) / 2, (p + 1) / 2 and random keys")
    return _case("B, limbs", circ, list(range(1, n + 1)), rows, notes, filler=0)


@functools.lru_cache(maxsize=None)
def expression_case():
    """Inputs 1..6. Elements (tuple 1): w1 + c (c near p: wraps in some rows), w2 * w3, 5 (a constant), w1 (again), 2 w4 + w5 + 7, w6 * w6 + w1, p - 1 (a
    constant), w5"""
    rng = random.Random(SEED + 1100)
    c = P - 1000
    elements = [[E([], [(1, 1)], c)], [E([(1, 2, 3)], [], 0)], [K(5)], [W(1)], [E([], [(2, 4), (1, 5)], 7)], [E([(1, 6, 6)], [(1, 1)], 0)], [K(P - 1)], [W(5)]]
    circ, _ = sort_circuit(6, elements, 1, [0])
    rows, notes = [], []
    for k in range(12):
        w1 = rng.randrange(1000) if k % 2 == 0 else rng.randrange(1000, P)   # w1 + c stays below p, or wraps
        rows.append([w1] + [rng.randrange(P) if k % 3 else rng.randrange(8) for _ in range(5)])
        notes.append("w1 + c " + ("stays below p" if k % 2 == 0 else "wraps past p"))
    rows.append([5, 1, 5, 0, 5, 0])   # ties between a constant, a product and witnesses: 1005 - p.., 5, 5, 5, 12, 5, p - 1, 5
    notes.append("ties")
    return _case("B, key expressions", circ, list(range(1, 7)), rows, notes, filler=0)


def sort_by_shapes(t):
    return ([], [0], [1, 0], [t], [0, 0], [t, 0])


@functools.lru_cache(maxsize=None)
def sort_by_cases():
    """tuples of 1 .. 4 under sort_by = [], [0], [1, 0], [tuple], [0, 0], [tuple, 0]; seven elements, keys from 0 .. 2 (ties everywhere) and from the field"""
    out = []
    n = 7
    for t in range(1, 5):
        for sort_by in sort_by_shapes(t):
            rng = random.Random(SEED + 1200 + 10 * t + len(sort_by) + sum(sort_by))
            ids = list(range(1, n * t + 1))
            circ, _ = sort_circuit(n * t, [[W(1 + i * t + k) for k in range(t)] for i in range(n)], t, sort_by)
            rows = [[rng.randrange(3) for _ in ids] for _ in range(4)] + [[rng.randrange(P) for _ in ids] for _ in range(2)]
            out.append(_case(f"B, tuple {t}, sort_by {sort_by}", circ, ids, rows, ["keys 0 .. 2"] * 4 + ["field elements"] * 2, filler=0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def past_tuple_case(t):
    """sort_by = [0, tuple + 1]: rows whose column 0 holds distinct keys solve (the comparator never reaches the second column); rows with one tie panic
    with core's text. Both kinds in one batch. Six elements."""
    n = 6
    rng = random.Random(SEED + 1300 + t)
    ids = list(range(1, n * t + 1))
    circ, _ = sort_circuit(n * t, [[W(1 + i * t + k) for k in range(t)] for i in range(n)], t, [0, t + 1])
    rows, notes = [], []
    for k in range(10):
        keys = rng.sample(range(50), n)
        tie = k % 2 == 1
        if tie:
            a, b = rng.sample(range(n), 2)
            keys[a] = keys[b]
        row = [rng.randrange(P) for _ in ids]
        for i in range(n):
            row[i * t] = keys[i]
        rows.append(row)
        notes.append("one tie in column 0: the comparator reaches column tuple + 1" if tie else "column 0 decides every comparison")
    case = _case(f"B, tuple {t}, sort_by [0, {t + 1}]", circ, ids, rows, notes, filler=0)
    assert [x.err for x in case.expect] == [sr.E_NONE, sr.E_PANIC] * 5 and all(x.message == sr.msg_index(t + 1, t + 1) for x in case.expect[1::2])
    return case


# ---------------------------------------------------------------------------------------------------------------- C: bits
N_BITS = 6     # elements of the sorts of list C: 11 switches


@functools.lru_cache(maxsize=None)
def bits_cases():
    n = N_BITS
    nb = sr.switch_count(n)
    rng = random.Random(SEED + 2000)
    keys = list(range(1, n + 1))
    elements = [[W(k)] for k in keys]
    perms = [rng.sample(range(n), n) for _ in range(7)] + [list(range(n))]
    out = []
    for count in (0, 1, nb - 1, nb + 3):   # the shorter of bits and control wins: the witnesses past the switches stay unassigned
        circ, bits = sort_circuit(n, elements, 1, [0], n_bits=count)
        case = _case(f"C, {count} bit witnesses for {nb} switches", circ, keys, perms, [str(p) for p in perms], filler=0)
        assert all(sum(1 for w in bits if w in x.witnesses) == min(count, nb) for x in case.expect)
        out.append(case)
    # a bit that the row already knows: witness n + 1 is an input and stands at position 4 of the bits
    fresh = list(range(n + 2, n + 1 + nb))
    bits = fresh[:4] + [n + 1] + fresh[4:]
    circ, _ = sort_circuit(n + 1, elements, 1, [0], bits=bits)
    rows, notes = [], []
    for p in perms:
        right = sr.run(Circuit(circ.current_witness_index, circ.opcodes), dict(zip(keys, p))).witnesses[n + 1]
        for v, note in ((right, "right"), (1 - right, "wrong"), (2, "no bit at all")):
            rows.append(p + [v])
            notes.append(f"{p}, bit 4 pre-assigned {note}")
    case = _case("C, a pre-assigned bit", circ, keys + [n + 1], rows, notes, filler=0)
    for x in case.expect:
        if x.status == sr.ST_FAILURE:   # the bits in front of it stay, the ones behind it do not
            assert x.err == sr.E_UNSATISFIED and all(w in x.witnesses for w in bits[:5]) and not any(w in x.witnesses for w in bits[5:])
    out.append(case)
    # one witness at positions 2 and 7
    fresh = list(range(n + 1, n + nb))
    bits = fresh[:7] + [fresh[2]] + fresh[7:]
    circ, _ = sort_circuit(n, elements, 1, [0], bits=bits)
    every = [list(p) for p in itertools.permutations(range(n))][::19]
    case = _case("C, one bit witness twice", circ, keys, every, [str(p) for p in every], filler=0)
    kinds = collections.Counter(x.err for x in case.expect)
    assert kinds[sr.E_NONE] >= 5 and kinds[sr.E_UNSATISFIED] >= 5, kinds
    out.append(case)
    # the bit at position 3 is the key of element 0: the row passes where the key (0 or 1) is that control bit
    fresh = list(range(n + 1, n + nb))
    bits = fresh[:3] + [1] + fresh[3:]
    circ, _ = sort_circuit(n, elements, 1, [0], bits=bits)
    rows = [[b] + rng.sample(range(2, 9), n - 1) for b in (0, 1) for _ in range(6)] + [[b] + [0] * (n - 1) for b in (0, 1)]
    case = _case("C, a bit witness that is an input", circ, keys, rows, [str(r) for r in rows], filler=0)
    kinds = collections.Counter(x.err for x in case.expect)
    assert kinds[sr.E_NONE] >= 2 and kinds[sr.E_UNSATISFIED] >= 2, kinds
    out.append(case)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- D: unassigned inputs
@functools.lru_cache(maxsize=None)
def missing_cases():
    """five elements of three components; a witness nobody assigns in the first, a middle and the last component (and in two of them: the first one in
    the reference's order is reported)"""
    n, t = 5, 3
    rng = random.Random(SEED + 3000)
    ids = list(range(1, n * t + 1))
    nobody, nobody2 = n * t + 1, n * t + 2
    out = []
    for name, holes in (("first", {0: nobody}), ("middle", {7: nobody}), ("last", {n * t - 1: nobody}), ("middle and first", {7: nobody, 0: nobody2}), ("inside a product", {4: nobody})):
        elements = []
        for i in range(n):
            el = []
            for k in range(t):
                pos = i * t + k
                if pos in holes:
                    el.append(E([(1, 1 + pos, holes[pos])], [], 3) if name == "inside a product" else E([], [(1, 1 + pos), (2, holes[pos])], 0))
                else:
                    el.append(W(1 + pos))
            elements.append(el)
        nb = sr.switch_count(n)
        circ, _ = sort_circuit(n * t, elements, t, [0], bits=list(range(nobody2 + 1, nobody2 + 1 + nb)))
        rows = [[rng.randrange(1, P) for _ in ids] for _ in range(3)]
        case = _case(f"D, an unassigned witness in the {name} component", circ, ids, rows, [name] * 3)
        want = holes[min(holes)]
        assert all((x.err, x.aux0, len(x.witnesses)) == (sr.E_MISSING_ASSIGNMENT, want, len(ids)) for x in case.expect), case.name
        out.append(case)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- E: neighbours
@functools.lru_cache(maxsize=None)
def neighbours_case(n_rows):
    """one level: a sort of 33 pairs by [1, 0], a SHA256 over 300 bytes of mixed widths, a sort of 129 keys, a Keccak256VariableLength -- four records of the
    scratch-carrying launch, whose scratch slices lie side by side; every output is compared"""
    rng = random.Random(SEED + 4000 + n_rows)
    n1, n2 = 33, 129
    widths = [8, 16, 32, 64, 8, 128, 24, 40] * 7 + [8] * 20   # 7 x 40 + 20 bytes
    assert sum((w + 7) // 8 for w in widths) == 300
    n_in = 2 * n1 + n2 + len(widths) + 40 + 1
    ids = list(range(1, n_in + 1))
    a = ids[:2 * n1]
    b = ids[2 * n1:2 * n1 + n2]
    h = ids[2 * n1 + n2:2 * n1 + n2 + len(widths)]
    kin = ids[-41:-1]
    size = ids[-1]
    nxt = n_in + 1
    bits1 = list(range(nxt, nxt + sr.switch_count(n1)))
    nxt += len(bits1)
    bits2 = list(range(nxt, nxt + sr.switch_count(n2)))
    nxt += len(bits2)
    sha = list(range(nxt, nxt + 32))
    kec = list(range(nxt + 32, nxt + 64))
    ops = [PermutationSort([[W(a[2 * i]), W(a[2 * i + 1])] for i in range(n1)], 2, bits1, [1, 0]),
           BB("SHA256", {"inputs": [FI(w, bits) for w, bits in zip(h, widths)], "outputs": sha}),
           PermutationSort([[W(w)] for w in b], 1, bits2, [0]),
           BB("Keccak256VariableLength", {"inputs": [FI(w, 8) for w in kin], "var_message_size": FI(size, 64), "outputs": kec})]
    circ = Circuit(nxt + 63, ops)
    rows, notes = [], []
    for j in range(n_rows):
        small = j % 3 == 0
        row = [rng.randrange(4) if small else rng.randrange(P) for _ in a + b] + [rng.randrange(P) for _ in h] + [rng.randrange(256) for _ in kin] + [rng.randrange(41)]
        rows.append(row)
        notes.append("keys 0 .. 3" if small else "field elements")
    return _case(f"E, neighbours, {n_rows} rows", circ, ids, rows, notes, filler=0)


# ---------------------------------------------------------------------------------------------------------------- the lists
@functools.lru_cache(maxsize=None)
def lists():
    return {"A": tuple(every_permutation_case(n) for n in SMALL_N) + tuple(structured_case(n) for n in LARGE_N),
            "B": (limb_case(), expression_case()) + sort_by_cases() + tuple(past_tuple_case(t) for t in (1, 2, 3, 4)),
            "C": bits_cases(), "D": missing_cases(), "E": (neighbours_case(65), neighbours_case(130))}


def all_cases():
    return [c for cs in lists().values() for c in cs]
