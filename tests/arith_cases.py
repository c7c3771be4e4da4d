"""One builder of the rows that random circuits never bring to Opcode::Arithmetic (acvm_amd/csrc/plan.cpp level_gate, gate_eval.hpp, the inversion batches,
the hand-over of a flagged row to exact_run_kernel), with every expected outcome from the Python model of the reference (tests/arith_ref.py): no oracle and
no device here. tests/test_arith_cases.py runs the lists through the CPU oracle and asserts what they cover; tests/test_gpu_arith_edges.py runs them on the
device.

A list is a tuple of cases; a case is (name, circuit, ids, rows, expect, filler, notes): one list of initial values per row (in the order of ids), the
model's Expect per row, a row that passes (for padding a batch; None where the circuit lets no row pass), and what each row is for.

  A  shapes as written: zero coefficients, duplicate terms, x x, residual products, unsorted terms -- circuits of three to six opcodes
  B  rows that leave the generic path: zero partners of SOLVE_DYN gates and what follows them, failing asserts, the first failure in program order
  C  values and counts in the folded gate: forced outputs at the limb boundaries, sums that are k p as integers, the unit-term and general-term counts
     around the side-sum budget, the periodic reduction and the 8-bit count fields, the grid of record shapes
  D  initial sets that differ per row (MultiBatch)"""
import collections
import functools
import random

import arith_ref as ar
from acvm_amd.acir import P, BlackBoxFuncCall as BB, Circuit, Expression as E, FunctionInput as FI

SEED = 20263
M1 = P - 1
Case = collections.namedtuple("Case", "name circuit ids rows expect filler notes")


def general(rng):
    """a coefficient that is neither 0 nor +-1, nor small enough to become one by a coincidence of two of them"""
    return rng.randrange(1 << 200, P - (1 << 200))


class Builder:
    """opcodes of one circuit. Witnesses 1..n_free are the free inputs; every other witness is handed out by new(). An assert gets a compensating INPUT
    z (+1 z in its sum) whose value row() works out by running the model up to the assert, so that the assert holds whatever the free inputs are."""

    def __init__(self, n_free):
        self.free, self.next, self.steps, self.comps = list(range(1, n_free + 1)), n_free + 1, [], []

    def new(self):
        self.next += 1
        return self.next - 1

    def op(self, e):
        self.steps.append((e, None))

    def solve(self, lin, mul=(), qc=0, coef=M1):
        """coef out + sum = 0 (coef = -1: out = sum)"""
        out = self.new()
        self.op(E(list(mul), list(lin) + [(coef % P, out)], qc % P))
        return out

    def dyn(self, partner, lin, mul=(), qc=0, coef=M1, left=False):
        """coef partner out + sum = 0: out = sum / partner for coef = -1"""
        out = self.new()
        self.op(E(list(mul) + [(coef % P, out, partner) if left else (coef % P, partner, out)], list(lin), qc % P))
        return out

    def check(self, lin, mul=(), qc=0):
        """sum + z = 0 with z a compensating input"""
        z = self.new()
        self.comps.append(z)
        self.steps.append((E(list(mul), list(lin) + [(1, z)], qc % P), z))
        return z

    def range(self, w, bits=254):
        self.op(BB("RANGE", {"input": FI(w, bits)}))

    @property
    def ids(self):
        return sorted(self.free + self.comps)

    def circuit(self):
        return Circuit(self.next - 1, [op for op, _ in self.steps])

    def row(self, free_values):
        wm = dict(zip(self.free, free_values))
        alive = True
        for op, z in self.steps:
            if z is not None:
                mul, lin, qc = ar.evaluate(op, wm) if alive else ([], [(1, z)], 0)
                wm[z] = -qc % P if (not mul and lin == [(1, z)]) else 0
            if alive:
                try:
                    ar.range_check(op, wm) if isinstance(op, BB) else ar.gate(op, wm)
                except ar.Fail:
                    alive = False
        return [wm[w] for w in self.ids]


def _case(name, circ, ids, rows, notes=None, filler=None):
    notes = list(notes) if notes is not None else [""] * len(rows)
    assert len(rows) == len(notes) and 0 < len(rows) <= 135, (name, len(rows))
    assert len(circ.opcodes) <= 700, (name, len(circ.opcodes))
    assert all(len(row) == len(ids) and all(0 <= v < P for v in row) for row in rows), name
    expect = [ar.run(circ, dict(zip(ids, row))) for row in rows]
    if filler is not None:
        assert expect[filler].status == ar.ST_SOLVED, (name, "the filler row does not pass")
    return Case(name, circ, list(ids), [list(r) for r in rows], expect, filler, notes)


def padded(case, n):
    """the case with passing rows IN FRONT up to n rows, so that the rows the case is about lie in the last, partial wave"""
    k = n - len(case.rows)
    if k <= 0 or case.filler is None:
        return case
    f = case.filler
    return case._replace(rows=[case.rows[f]] * k + case.rows, expect=[case.expect[f]] * k + case.expect, notes=["filler"] * k + case.notes, filler=0)


def describe(case, j):
    return f"{case.name} row {j}" + (f" ({case.notes[j]})" if case.notes[j] else "")


def compare(case, got, who, expect=None):
    """got: per row (Result.as_tuple(), message, {witness: value}); every field of the model's expectation, the whole map included"""
    for j, (want, (head, message, wm)) in enumerate(zip(expect or case.expect, got)):
        at = describe(case, j)
        assert tuple(head) == tuple(want[:5]), f"{at}: {who} (status, error, opcode, aux0, aux1) {tuple(head)}, want {tuple(want[:5])}"
        if want.message is not None:
            assert message == want.message, f"{at}: {who} message {message!r}, want {want.message!r}"
        for w in sorted(set(wm) | set(want.witnesses)):
            g, x = wm.get(w), want.witnesses.get(w)
            assert g == x, (f"{at}: witness {w}: {who} " + (hex(g) if g is not None else "unassigned") + ", want " + (hex(x) if x is not None else "unassigned"))


NOT_TRUNCATED = 0xFFFFFFFF


def deviates(x):
    """the row leaves the generic path of the plan: it does not end Solved, or a partner of an unknown was zero (the gate the plan holds as SOLVE_DYN was an
    assert for it)"""
    return x.status != ar.ST_SOLVED or "eval_mul_folds_to_zero" in x.branches


def expected_truncation(case):
    """where the plan of the case has to end. List A: the opcode at which a row of nonzero random inputs is not solvable (TooManyUnknowns, the panic) -- what
    is unknown there is unknown for every row. List C: opcode 1 of the circuits whose gate of 256 general terms stands there (a record's count fields hold
    255). Everywhere else the plan covers the circuit: NOT_TRUNCATED."""
    if case.name.startswith("C, 256 general"):
        return 1
    if not case.name.startswith("A, "):
        return NOT_TRUNCATED
    x = case.expect[-1]
    assert case.notes[-1].startswith("random"), case.name
    return x.opcode_index if x.err in (ar.E_TOO_MANY_UNKNOWNS, ar.E_PANIC) else NOT_TRUNCATED


def value_rows(n, rng, n_random=5):
    """rows of n inputs: 0, 1 and p - 1 everywhere and one input at a time, on the first two together, and random rows"""
    rows, notes = [[v] * n for v in (0, 1, M1)], ["0 everywhere", "1 everywhere", "p - 1 everywhere"]
    for k in range(n):
        for v, what in ((0, "0"), (1, "1"), (M1, "p - 1")):
            rows.append([v if i == k else rng.randrange(1, P) for i in range(n)])
            notes.append(f"input {k + 1} = {what}")
    for v in (0, rng.randrange(1, P)):   # the first two inputs 0 together, the third 0 and not
        rows.append([0, 0, v] + [rng.randrange(1, P) for _ in range(n - 3)])
        notes.append("inputs 1 and 2 = 0")
    for _ in range(n_random):
        rows.append([rng.randrange(1, P) for _ in range(n)])
        notes.append("random")
    return rows, notes


# ---------------------------------------------------------------------------------------------------------------- A: shapes as written
def _shapes(rng):
    """[(name, opcodes over the inputs a, b, c, d = 1..4 and the witnesses 5.., what to make of a row of inputs so that some rows pass)]"""
    a, b, c, d = 1, 2, 3, 4
    g, h = general(rng), general(rng)
    same = lambda r: [r[0], r[0], r[2], r[3]]              # a == b
    csum = lambda r: [r[0], r[1], (r[0] + r[1]) % P, r[3]]  # c == a + b
    out = []
    out.append(("empty expressions, q_c zero", [E([], [], 0), E([], [(1, a), (1, b), (M1, 5)], 0), E([], [], 0), E([(1, 5, c)], [(M1, 6)], 0)], None))
    out.append(("empty expressions, q_c nonzero behind two gates", [E([], [], 0), E([], [(1, a), (1, b), (M1, 5)], 0), E([(1, 5, c)], [(M1, 6)], 0), E([], [], 7),
                                                                  E([], [(1, 6), (M1, 7)], 0)], None))
    out.append(("empty expression, q_c = p - 1 first", [E([], [], M1), E([], [(1, a), (M1, 5)], 0), E([], [(1, 5), (M1, 6)], 0)], None))
    out.append(("zero coefficient on a known linear term", [E([], [(1, a), (0, b), (1, c), (M1, 5)], 0), E([], [(0, d), (1, 5), (M1, a), (M1, c)], 0), E([], [(0, 5)], 0),
                                                            E([(2, 5, 5)], [(0, a), (M1, 6)], 1)], None))
    out.append(("zero coefficient on an unknown linear term", [E([], [(1, a), (0, 5), (M1, b)], 0),      # an assert of a == b; 5 stays unknown
                                                               E([], [(0, 5), (1, a), (M1, 6)], 0),      # 6 = a, beside the unknown 5
                                                               E([], [(0, 5), (0, 7)], 0),               # no unknown at all: 0 = 0
                                                               E([], [(1, 5), (1, c)], 0),               # 5 = -c: it WAS unknown
                                                               E([(1, 5, 6)], [(M1, 8)], 0)], same))
    out.append(("zero coefficient on a product of two knowns", [E([(0, a, b), (2, c, d)], [(M1, 5)], 1), E([(0, 5, 5), (0, a, 5)], [(1, 5), (M1, 6)], 0),
                                                                E([(0, a, b)], [], 0)], None))
    out.append(("zero coefficient on a product with one unknown", [E([(0, a, 5)], [(1, b), (M1, 6)], 0),  # 6 = b; 5 stays unknown
                                                                   E([(0, 5, a), (0, b, 5)], [], 0),      # 0 = 0
                                                                   E([(3, a, 5)], [(1, 6)], 0),           # 5 = -b / (3 a), or a = 0
                                                                   E([(1, 5, 6)], [(M1, 7)], 0)], None))
    out.append(("zero coefficient on a product of two unknowns", [E([(0, 5, 6)], [(1, a), (M1, 7)], 0), E([(0, 5, 6), (0, 6, 5), (0, 5, 5)], [(1, b), (M1, 8)], 3),
                                                                  E([(1, 7, 8)], [(M1, 9)], 0)], None))
    out.append(("one known witness in two linear terms", [E([], [(2, a), (3, a), (M1, 5)], 0), E([], [(g, a), (P - g, a), (1, b), (M1, 6)], 0),
                                                          E([], [(5, a), (M1, 5), (1, b), (M1, 6)], 0)], None))
    out.append(("(c, a, b) with (c', b, a)", [E([(3, a, b), (P - 5, b, a)], [(M1, 5)], 0), E([(g, a, b), (P - g, b, a)], [(1, c), (M1, 6)], 0),
                                             E([(1, 5, 6), (1, 6, 5)], [(M1, 7)], 0), E([(2, a, b)], [(1, 5)], 0)], None))
    out.append(("one unknown in two linear terms, c and -c", [E([], [(1, a), (M1, 5)], 0), E([], [(g, 6), (P - g, 6), (1, b)], 0), E([], [(1, 5), (M1, 7)], 0)], None))
    out.append(("one unknown in two linear terms, 1 and 2", [E([], [(1, a), (M1, 5)], 0), E([], [(1, 6), (2, 6), (1, b)], 0), E([], [(1, 5), (M1, 7)], 0)], None))
    out.append(("an unknown under two known partners", [E([(2, a, 5), (3, b, 5)], [(1, c)], 0),   # two linear terms; one where a or b is 0; an assert of c where both are
                                                        E([], [(1, 5), (M1, 6)], 1),               # 6 = 5 + 1, or two unknowns
                                                        E([(1, 6, d)], [(M1, 7)], 0)], None))
    out.append(("an unknown under a known partner and in a linear term", [E([(2, a, 5)], [(3, 5), (1, c)], 0), E([], [(1, 5), (M1, 6)], 1), E([(1, 6, d)], [(M1, 7)], 0)], None))
    out.append(("x x with x unknown", [E([], [(1, a), (M1, 5)], 0), E([(1, 6, 6)], [(1, b)], 0), E([], [(1, 5), (M1, 7)], 0)], None))
    out.append(("x x with x known", [E([], [(1, a), (1, b), (M1, 5)], 0), E([(1, 5, 5)], [(M1, 6)], 0), E([(g, a, a), (M1, 6, 6)], [(h, 7)], 0), E([(1, 7, 7), (1, 7, 7)], [(M1, 8)], 0)], None))
    for name, mul, lin in (("two residual products", [(1, 6, 7), (2, 7, 6)], [(1, b)]),
                           ("two residual products, one with coefficient zero", [(1, 6, 7), (0, 7, 6)], [(1, b)]),
                           ("three residual products, one with coefficient zero", [(0, 6, 7), (g, 7, 6), (1, 6, 6)], [(1, b)]),
                           ("three residual products, two with coefficient zero", [(0, 6, 7), (g, 7, 8), (0, 6, 6)], [(1, b)]),
                           ("a residual product beside a folded linear term", [(g, 6, 7), (3, a, 6)], [(1, b), (1, c)]),
                           ("two residual products beside two unknown linear terms", [(1, 6, 7), (2, 7, 6)], [(1, 6), (1, b), (3, 7)]),
                           ("three residual products beside a folded and an unknown linear term", [(1, 6, 7), (2, 7, 6), (3, a, 6), (h, 8, 8)], [(1, 8), (1, b)])):
        out.append((name, [E([], [(1, a), (M1, 5)], 0), E(mul, lin, 4), E([], [(1, 5), (M1, 9)], 0)], None))
    out.append(("terms in unsorted order", [E([(2, d, b), (3, c, a)], [(5, d), (M1, 7), (1, b), (4, a)], 9), E([(g, 7, c), (1, b, 7)], [(1, 7), (h, 6), (2, a)], 0),
                                            E([(1, 7, 6)], [(1, d), (M1, 5), (1, c)], 0), E([], [(1, c), (1, b), (1, a), (M1, c)], 0)], lambda r: [r[0], (-r[0]) % P, r[2], r[3]]))
    out.append(("the unknown as left and as right factor", [E([(3, 5, a)], [(1, b)], 0), E([(3, a, 6)], [(1, b)], 0), E([], [(1, 5), (M1, 6)], 0), E([(M1, 7, 5)], [(1, c)], 0),
                                                            E([(g, b, 8), (0, 8, a)], [(1, 7)], 2)], None))
    out.append(("a RANGE of 8 bits on a gate's output", [E([], [(1, a), (1, b), (M1, 5)], 0), BB("RANGE", {"input": FI(5, 8)}), E([(1, 5, c)], [(M1, 6)], 0), BB("RANGE", {"input": FI(6, 254)})],
                lambda r: [r[0] % 200, r[1] % 56, r[2], r[3]]))
    out.append(("an assert between solves", [E([], [(1, a), (1, b), (M1, 5)], 0), E([], [(1, 5), (M1, c)], 0), E([(1, 5, c)], [(M1, 6)], 0)], csum))
    return out


@functools.lru_cache(maxsize=None)
def shape_cases():
    rng = random.Random(SEED)
    cases = []
    for name, ops, fix in _shapes(rng):
        assert 3 <= len(ops) <= 6, name
        gates = [e for e in ops if isinstance(e, E)]
        nw = max([w for e in gates for _, l, r in e.mul_terms for w in (l, r)] + [w for e in gates for _, w in e.linear_combinations])
        rows, notes = value_rows(4, rng)
        if fix is not None:  # every row as it is (the assert fails) and mended (it holds)
            rows, notes = rows + [fix(r) for r in rows], notes + [n + ", mended" for n in notes]
        expect = [ar.run(Circuit(nw, ops), dict(zip([1, 2, 3, 4], r))) for r in rows]
        passing = [j for j, x in enumerate(expect) if x.status == ar.ST_SOLVED]
        cases.append(_case("A, " + name, Circuit(nw, ops), [1, 2, 3, 4], rows, notes, filler=passing[-1] if passing else None))
    return tuple(cases)


# ---------------------------------------------------------------------------------------------------------------- B: rows that leave the generic path
FOLLOW_UPS = ("an assert solves it", "too many unknowns", "missing assignment", "nobody reads it")
# (rows of the batch, the special rows): one row alone; the first, middle and last lane of a wave of 63 and of 64; the one lane of a partial last wave, and
# every other row; the lanes at the seams of two waves and a partial one, and every row
PLACEMENTS = ((1, (0,)), (1, ()), (63, (0, 31, 62)), (64, (0, 31, 63)), (65, (64,)), (65, tuple(range(0, 65, 2))), (130, (0, 63, 64, 127, 128, 129)), (130, tuple(range(130))))


def _dyn_circuit(follow):
    """Inputs: 1 = a (the partner), 2 = s, 3 = t. Opcode 0: a u + s = 0 with u = witness 4 unknown -- SOLVE_DYN for the plan; a = 0 makes it an assert of s.
    Then what `follow` says, and one more gate. The passing rows have s = -a u and t = -u."""
    a, s, t, u = 1, 2, 3, 4
    ops = [E([(1, a, u)], [(1, s)], 0)]
    if follow == "an assert solves it":
        ops += [E([], [(1, u), (1, t)], 0), E([(1, u, t)], [(M1, 5)], 1)]        # the plan knows u by now: an ASSERT record; a row without u solves it here
    elif follow == "too many unknowns":
        ops += [E([], [(1, s), (M1, 5)], 2), E([], [(1, u), (M1, 6), (1, t)], 0)]  # 6 = u + t, or two unknowns
    elif follow == "missing assignment":
        ops += [E([], [(1, s), (M1, 5)], 2), BB("RANGE", {"input": FI(u, 254)}), E([], [(1, 5), (M1, 6)], 0)]
    else:
        ops += [E([], [(1, s), (1, t), (M1, 5)], 0), E([(1, 5, 5)], [(M1, 6)], 0)]
    return Circuit(6, ops)


@functools.lru_cache(maxsize=None)
def dyn_cases(follow):
    cases = []
    for k, (B, special) in enumerate(PLACEMENTS):
        rng = random.Random(SEED + 100 + 10 * FOLLOW_UPS.index(follow) + k)
        rows, notes = [], []
        for j in range(B):
            a, u = rng.randrange(1, P), rng.randrange(P)
            if j not in special:
                rows.append([a, -a * u % P, -u % P])
                notes.append("passes")
            elif special.index(j) % 3 == 1:  # a third of the special rows: the partner is zero and the sum is not
                rows.append([0, rng.randrange(1, P), -u % P])
                notes.append("zero partner, nonzero sum")
            else:
                rows.append([0, 0, -u % P])
                notes.append("zero partner, zero sum")
        cases.append(_case(f"B, {follow}, {B} rows, special {len(special)}", _dyn_circuit(follow), [1, 2, 3], rows, notes,
                           filler=notes.index("passes") if "passes" in notes else None))
    return tuple(cases)


WIDE = 260
WIDE_ZEROS = (0, 127, 128, 259)


@functools.lru_cache(maxsize=None)
def wide_dyn_case():
    """WIDE SOLVE_DYN gates on one level: a_i u_i + s = 0 with the partners a_i = inputs 1..WIDE and s = input WIDE + 1 -- inversion chunks of 128, 128 and 4
    under the default inv_chunk. Behind them two readers: u_5 + u_200 and an assert-shaped gate on u_128."""
    n = WIDE
    s, t = n + 1, n + 2
    u = [n + 3 + i for i in range(n)]
    ops = [E([(1, 1 + i, u[i])], [(1, s)], 0) for i in range(n)]
    r1, r2 = u[-1] + 1, u[-1] + 2
    ops += [E([], [(1, u[5]), (1, u[200]), (M1, r1)], 0), E([], [(1, u[128]), (M1, r2), (1, t)], 0)]
    rng = random.Random(SEED + 200)
    rows, notes = [], []

    def row(zeros, s_zero, note):
        rows.append([0 if i in zeros else rng.randrange(1, P) for i in range(n)] + [0 if s_zero else rng.randrange(1, P), rng.randrange(P)])
        notes.append(note)

    row((), False, "passes")
    row((), True, "s = 0: every u is 0")
    for k in WIDE_ZEROS:
        row((k,), False, f"partner {k} zero, nonzero sum")
        row((k,), True, f"partner {k} zero, zero sum")
    row(WIDE_ZEROS, True, "the four partners zero, zero sum")
    row(tuple(range(n)), True, "every partner zero, zero sum")
    row(tuple(range(n)), False, "every partner zero, nonzero sum")
    row((5, 200), True, "both operands of the reader unassigned")
    row((), False, "passes")
    return _case("B, 260 gates on one level", Circuit(r2, ops), list(range(1, n + 3)), rows, notes, filler=0)


@functools.lru_cache(maxsize=None)
def order_cases():
    """first failures: the lowest opcode in program order wins, whatever level it runs on; what the levels wrote for opcodes behind it is not in the map"""
    rng = random.Random(SEED + 300)
    cases = []
    # two asserts, the lower opcode on the later level. Inputs a, b, c, d = 1..4 (d = a b c in the passing rows), e = 5 (= a)
    ops = [E([(1, 1, 2)], [(M1, 6)], 0), E([(1, 6, 3)], [(M1, 7)], 0), E([], [(1, 7), (M1, 4)], 0), E([], [(1, 1), (M1, 5)], 0), E([], [(1, 7), (1, 5), (M1, 8)], 0)]
    rows, notes = [], []
    for j in range(67):
        a, b, c = (rng.randrange(P) for _ in range(3))
        bad_late, bad_early = j % 5 == 1 or j % 7 == 3, j % 5 == 2 or j % 7 == 3
        rows.append([a, b, c, (a * b * c + bad_late) % P, (a + bad_early) % P])
        notes.append("the assert at opcode 2 (level 3) fails" * bad_late + " the assert at opcode 3 (level 1) fails" * bad_early or "passes")
    cases.append(_case("B, two asserts, the lower opcode on the later level", Circuit(8, ops), [1, 2, 3, 4, 5], rows, notes, filler=0))
    # a failing assert and a zero partner, in both orders. Inputs a, b (the assert a == b), c (the partner), d (the sum)
    for first in ("assert", "partner"):
        gate_a, gate_p = E([], [(1, 1), (M1, 2)], 0), E([(1, 3, 5)], [(1, 4)], 0)
        ops = ([gate_a, gate_p] if first == "assert" else [gate_p, gate_a]) + [E([], [(1, 1), (1, 3), (M1, 6)], 0)]
        rows, notes = [], []
        for j in range(66):
            a, c, d = rng.randrange(P), rng.randrange(1, P), rng.randrange(1, P)
            bad_a, zero_c, zero_d = j % 3 == 1 or j % 4 == 2, j % 4 == 2 or j % 5 == 3, j % 10 == 3
            rows.append([a, (a + bad_a) % P, 0 if zero_c else c, 0 if zero_d else d])
            notes.append(("a != b " * bad_a + "zero partner " * zero_c + "zero sum" * zero_d).strip() or "passes")
        cases.append(_case(f"B, a failing assert and a zero partner, the {first} first", Circuit(6, ops), [1, 2, 3, 4], rows, notes, filler=0))
    # early in program order, late in level order: a chain of 20 products, an assert on its end, then 40 gates of level 1
    n_chain, n_behind = 20, 40
    ops, last = [], 1
    w = 4
    for _ in range(n_chain):
        ops.append(E([(1, last, 2)], [(1, 1), (M1, w)], 0))
        last, w = w, w + 1
    ops.append(E([], [(1, last), (M1, 3)], 0))
    for i in range(n_behind):
        ops.append(E([], [(1 + i, 1), (1, 2), (M1, w)], i))
        w += 1
    circ = Circuit(w - 1, ops)
    rows, notes = [], []
    for j in range(65):
        a, b = rng.randrange(P), rng.randrange(P)
        end = ar.run(Circuit(3 + n_chain, ops[:n_chain]), {1: a, 2: b}).witnesses[last]
        bad = j in (0, 31, 63, 64)
        rows.append([a, b, (end + bad) % P])
        notes.append(f"the assert at opcode {n_chain} fails: the {n_behind} gates behind it ran on level 1" if bad else "passes")
    cases.append(_case("B, early in program order, late in level order", circ, [1, 2, 3], rows, notes, filler=1))
    return tuple(cases)


# ---------------------------------------------------------------------------------------------------------------- C: values and counts
P29_TOP = P >> 232   # p's ninth 29-bit limb


def forced_values():
    """[(name, value)]: the values an output is forced to"""
    out = [("0", 0), ("1", 1), ("2", 2), ("p - 1", M1), ("p - 2", P - 2), ("(p - 1) / 2", (P - 1) // 2), ("(p + 1) / 2", (P + 1) // 2)]
    ks = sorted({29 * i for i in range(1, 9)} | {32 * i for i in range(1, 8)})
    out += [(f"2^{k}", 1 << k) for k in ks] + [(f"p - 2^{k}", P - (1 << k)) for k in ks]
    low = P29_TOP << 232  # the least value whose ninth limb is p's; the greatest is p - 1, whose neighbours are p - 2 and 0
    out += [("least with p's ninth limb", low), ("... - 1", low - 1), ("... + 1", low + 1)]
    assert all(0 <= v < P for _, v in out) and low >> 232 == P29_TOP == M1 >> 232 and (low - 1) >> 232 == P29_TOP - 1
    return out


STORES = ("pinned", "relaxed", "operand of an assert")


@functools.lru_cache(maxsize=None)
def forced_case(store):
    """Inputs: 1 = t (the value), 2 = a, 3 = t - a, 4 = t / a, 5 = d, 6 = -t d. Outputs forced to t: a copy, the sum a + (t - a) (which wraps past p in the rows
    whose a is above t), the product a (t / a), the SOLVE_DYN quotient (t d) / d. `store`: a RANGE of 254 bits reads every output (it is stored canonical);
    only gates read it (it may be stored relaxed); an assert against t follows it."""
    t, a, b_sum, b_prod, d, n = 1, 2, 3, 4, 5, 6
    outs = [7, 8, 9, 10]
    ops = [E([], [(1, t), (M1, 7)], 0), E([], [(1, a), (1, b_sum), (M1, 8)], 0), E([(1, a, b_prod)], [(M1, 9)], 0), E([(1, d, 10)], [(1, n)], 0)]
    nw = 10
    if store == "pinned":
        ops += [BB("RANGE", {"input": FI(w, 254)}) for w in outs]
    elif store == "relaxed":
        ops += [E([(1, 7, 8)], [(1, 9), (M1, 10), (M1, 11)], 0), E([(general(random.Random(SEED + 1)), 11, 7)], [(1, 8), (M1, 9), (M1, 12)], 5)]
        nw = 12
    else:
        ops += [E([], [(1, w), (M1, t)], 0) for w in outs]
    rng = random.Random(SEED + 400)
    rows, notes = [], []
    for k, (name, v) in enumerate(forced_values()):
        av = rng.randrange(v + 1, P) if k % 2 and v < P - 1 else rng.randrange(1, v + 1) if v else rng.randrange(1, P)
        dv = rng.randrange(1, P)
        rows.append([v, av, (v - av) % P, v * pow(av, -1, P) % P, dv, -v * dv % P])
        notes.append(name + (", the sum wraps" if av > v else ""))
    case = _case(f"C, forced outputs, {store}", Circuit(nw, ops), [1, 2, 3, 4, 5, 6], rows, notes, filler=0)
    assert all(x.status == ar.ST_SOLVED and all(x.witnesses[w] == row[0] for w in outs) for x, row in zip(case.expect, case.rows)), store
    return case


N_FREE = 10   # free inputs of the count circuits: 1..8 operands, 9 and 10 partners of SOLVE_DYN gates


def count_rows(b, rng):
    """rows of a count circuit: p - 1 on every operand; 1; random rows; 0 on the operands (the partners never are 0: list B is about that)"""
    frees = [[M1] * 8 + [rng.randrange(1, P), M1], [1] * 10, [0] * 8 + [rng.randrange(1, P), 1]] + [[rng.randrange(1, P) for _ in range(N_FREE)] for _ in range(4)]
    frees.append([M1] * 4 + [rng.randrange(1, P) for _ in range(6)])
    return [b.row(f) for f in frees], ["p - 1 on every operand", "1 everywhere", "0 on every operand", "random", "random", "random", "random", "p - 1 on four operands"]


def _unit_gate(b, kind, n_lp, n_ln, n_pn, qc, pool, rng, pin=False):
    """a gate of n_lp (+1 w), n_ln (-1 w) and n_pn (-1 a b) terms over the witnesses of `pool`; kind: "solve" / "assert" / "dyn" """
    pick = lambda: pool[rng.randrange(len(pool))]
    lin = [(1, pick()) for _ in range(n_lp)] + [(M1, pick()) for _ in range(n_ln)]
    mul = [(M1, pick(), pick()) for _ in range(n_pn)]
    rng.shuffle(lin)
    if kind == "assert":
        return b.check(lin, mul, qc)
    out = b.solve(lin, mul, qc) if kind == "solve" else b.dyn(9 + rng.randrange(2), lin, mul, qc)
    if pin:
        b.range(out)
    return out


@functools.lru_cache(maxsize=None)
def count_cases():
    """the circuits of the unit-term and general-term counts and of the record grid, each with the rows of count_rows"""
    cases = []
    inputs = list(range(1, 9))

    def finish(name, b, rng):
        rows, notes = count_rows(b, rng)
        cases.append(_case("C, " + name, b.circuit(), b.ids, rows, notes, filler=3))

    # sums that are k p as integers: n operands of p - 1 under +1 terms, -1 terms and -1 products, as asserts (the compensating input is n, or p - n)
    rng = random.Random(SEED + 500)
    b = Builder(N_FREE)
    for n in (1, 2, 3, 5, 8, 13):
        b.check([(1, inputs[i % 8]) for i in range(n)])
        b.check([(M1, inputs[i % 8]) for i in range(n)])
        b.check([], [(M1, inputs[i % 8], inputs[(i + 3) % 8]) for i in range(n)])
        b.check([(1, inputs[i % 8]) for i in range(n)], [(M1, inputs[i % 8], inputs[(i + 1) % 8]) for i in range(n)], qc=n)
    finish("asserts whose sums are k p", b, rng)

    # unit-term counts 0..8 of each kind, with and without q_c; every third output pinned, the others feed later gates
    rng = random.Random(SEED + 510)
    b = Builder(N_FREE)
    k = 0
    relaxed = []
    for n in range(9):
        for lp, ln, pn in ((n, 0, 0), (0, n, 0), (0, 0, n), (n, n, n), (n, 8 - n, n // 2)):
            for qc in (0, general(rng)):
                k += 1
                kind = ("solve", "assert", "dyn")[k % 3] if lp + ln + pn else ("solve", "assert")[k % 2]
                w = _unit_gate(b, kind, lp, ln, pn, qc, inputs + relaxed[-6:], rng, pin=k % 9 == 0)
                if kind == "solve" and k % 9 and pn == 0:
                    relaxed.append(w)
    finish("unit-term counts 0..8", b, rng)

    rng = random.Random(SEED + 520)
    b = Builder(N_FREE)
    k = 0
    for n in range(13, 21):
        for lp, ln, pn in ((n, 0, 0), (0, n, 0), (0, 0, n)):
            k += 1
            _unit_gate(b, ("solve", "assert", "dyn", "solve")[k % 4], lp, ln, pn, 0, inputs, rng, pin=k % 5 == 0)
    finish("unit-term counts 13..20", b, rng)

    for n in (254, 255, 256, 257, 300):
        rng = random.Random(SEED + 530 + n)
        b = Builder(N_FREE)
        o1 = _unit_gate(b, "solve", n, 0, 0, 0, inputs, rng)
        o2 = _unit_gate(b, "solve", 0, n, 0, 3, inputs, rng, pin=True)
        o3 = _unit_gate(b, "dyn", 0, 0, n, 0, inputs, rng, pin=True)   # (pinned: the planner may not turn the -1 products of a free output into +1 products)
        o4 = b.solve([], [(1, inputs[rng.randrange(8)], inputs[rng.randrange(8)]) for _ in range(n)], coef=M1)
        b.range(o4)
        _unit_gate(b, "assert", n, n, 0, 0, inputs, rng)
        b.solve([(1, o1), (M1, o2), (1, o3), (M1, o4)])
        finish(f"{n} unit terms of each kind", b, rng)

    # general coefficients: 255 of each kind fit a record; at 256 the plan ends and the exact kernels finish
    for n in (255, 256):
        for what in ("products", "linear terms"):
            rng = random.Random(SEED + 540 + n + len(what))
            b = Builder(N_FREE)
            first = b.solve([(1, 1), (general(rng), 2)], [(1, 3, 4)])
            pick = lambda: inputs[rng.randrange(8)]
            if what == "products":
                wide = b.solve([(1, first)], [(general(rng), pick(), pick()) for _ in range(n)])
            else:
                wide = b.solve([(general(rng), pick()) for _ in range(n)], [(1, first, 5)])
            b.check([(1, wide), (general(rng), first)])
            b.solve([(1, wide), (1, first)], [(1, wide, first)])
            finish(f"{n} general {what}", b, rng)

    # 31..65 multiplied terms (16, 17, 32 and 33 reductions) on the inputs (p - 1 in row 0) and on relaxed operands
    rng = random.Random(SEED + 560)
    b = Builder(N_FREE)
    relaxed = [b.solve([(1, inputs[i]), (1, inputs[(i + 1) % 8]), (1, inputs[(i + 2) % 8]), (1, inputs[(i + 5) % 8])][:2 + i % 3]) for i in range(8)]
    for n in (31, 32, 33, 34, 63, 64, 65):
        for pool in (inputs, relaxed):
            pick = lambda: pool[rng.randrange(8)]
            n_prod = n // 3
            b.solve([(general(rng), pick()) for _ in range(n - n_prod)], [(general(rng), pick(), pick()) for _ in range(n_prod)])
            b.check([(general(rng), pick()) for _ in range(n)])
            b.dyn(9, [(general(rng), pick()) for _ in range(n)], [(1, pick(), pick())])
    finish("31..65 multiplied terms", b, rng)

    # the grid (np_pos, np_mac, nl_mac) in {0..3}^3 as SOLVE, ASSERT and SOLVE_DYN records, on the inputs; then records whose subtracted operands and sums
    # carry the large bounds (sub_k 2 and 3, PRESUM_WEAK, OUT_WEAK)
    rng = random.Random(SEED + 570)
    b = Builder(N_FREE)
    pick = lambda: inputs[rng.randrange(8)]
    for kind in ("solve", "assert", "dyn"):
        for np_pos in range(4):
            for np_mac in range(4):
                for nl_mac in range(4):
                    mul = [(1, pick(), pick()) for _ in range(np_pos)] + [(general(rng), pick(), pick()) for _ in range(np_mac)]
                    lin = [(general(rng), pick()) for _ in range(nl_mac)]
                    if kind == "solve":
                        b.solve(lin, mul)
                    elif kind == "assert":
                        b.check(lin, mul)
                    else:
                        b.dyn(10, lin, mul)
    finish("the grid of record shapes", b, rng)

    rng = random.Random(SEED + 580)
    b = Builder(N_FREE)
    sums = {n: [b.solve([(1, inputs[(i + j) % 8]) for i in range(n)]) for j in range(3)] for n in (2, 3, 4, 5, 7)}   # bounds of 2 p .. 7 p before the store
    for n in (2, 3, 4, 5, 7):
        b.solve([(M1, sums[n][0]), (M1, sums[n][1]), (1, 1)])
        b.check([(M1, sums[n][2]), (1, sums[n][0])])
        b.dyn(9, [(M1, sums[n][1]), (M1, 2)], qc=1)
    for n in (6, 7, 8, 9, 12):
        b.dyn(10, [(1, inputs[i % 8]) for i in range(n)])
        b.dyn(9, [(1, sums[5][i % 3]) for i in range(n)], [(1, 3, 4)])
    finish("large bounds under subtraction and in front of the inverse", b, rng)
    return tuple(cases)


# ---------------------------------------------------------------------------------------------------------------- D: initial sets
@functools.lru_cache(maxsize=None)
def initial_set_case():
    """(circuit, maps, expect, notes). Opcode 0: o = a b + c (o = witness 5); opcode 1: o - d = 0, an ASSERT for the plan of the plain set; opcode 2: r = o + d.
    One group of maps assigns a, b, c, d; one lacks d, so that opcode 1 solves it; one brings o, which makes opcode 0 an assert for those rows: consistent, or
    not (Unsatisfied at opcode 0, and the map keeps what the row brought)."""
    ops = [E([(1, 1, 2)], [(1, 3), (M1, 5)], 0), E([], [(1, 5), (M1, 4)], 0), E([], [(1, 5), (1, 4), (M1, 6)], 0)]
    circ = Circuit(6, ops)
    rng = random.Random(SEED + 700)
    maps, notes = [], []
    for j in range(28):
        a, b, c = ((0, 1, M1, rng.randrange(P))[(j // 4 + k) % 4] if j % 8 < 4 else rng.randrange(P) for k in range(3))
        o = (a * b + c) % P
        m = {1: a, 2: b, 3: c, 4: o}
        if j % 4 == 1:
            del m[4]
            notes.append("lacks d")
        elif j % 4 == 2:
            m[5] = o
            notes.append("brings o, consistent")
        elif j % 4 == 3:
            m[5] = (o + 1 + j) % P
            notes.append("brings o, inconsistent")
        else:
            if j % 8 == 4:
                m[4] = (o + 1) % P
            notes.append("the plain set, d wrong" if j % 8 == 4 else "the plain set")
        maps.append(m)
    expect = [ar.run(circ, m) for m in maps]
    return circ, tuple(maps), tuple(expect), tuple(notes)


# ---------------------------------------------------------------------------------------------------------------- the lists
@functools.lru_cache(maxsize=None)
def lists():
    """{letter: the cases that run as plain batches}; D's rows are maps: they have tests of their own"""
    return {"A": shape_cases(), "B": tuple(c for f in FOLLOW_UPS for c in dyn_cases(f)) + (wide_dyn_case(),) + order_cases(), "C": tuple(forced_case(s) for s in STORES) + count_cases()}


def all_cases():
    return [c for cs in lists().values() for c in cs]
