"""One builder of the rows that random inputs never bring to MemoryInit / MemoryOp (acvm_amd/csrc/ops_light.hpp op_mem_init / op_mem_op, the block passes of
plan.cpp, the replay of exact_run_kernel), with every expected outcome from the Python model of the reference (tests/mem_ref.py): no oracle and no
device here. tests/test_mem_cases.py runs the lists through the CPU oracle and asserts what they cover; tests/test_gpu_mem_edges.py runs them on the
device.

A list is a tuple of cases; a case is (name, circuit, ids, rows, expect, notes, traces, filler): one list of initial values per row, the model's
Expect per row, what the row is for, the MemoryOps the model's run reached (mem_ref.Model.trace), and a row that passes (for padding a batch; None
where the circuit lets no row pass). Where one row could only ever reach the first failing opcode, the opcodes carry a predicate witness each and a
row switches on the one it is about; where even that does not help (a panic comes before the predicate) the list has one small circuit per opcode.

  A  indices: forms x values x predicates, reads and writes, at block lengths 1, 6, 33, 67
  B  operation: constants, a witness, w_a - w_b; opcodes that read in some rows and write in others
  C  read targets: expressions that are a witness only after evaluation, or never
  D  written values: unknown witnesses in them, p - 1, 0, sums that wrap
  E  blocks: re-initialised shorter / longer / empty, never initialised, ids out of order, an init that cannot finish
  F  order: seeded programs of about 120 memory ops and 40 gates with RANGE tripwires
  G  re-entries: memory state across a foreign call and across a step-limit retry
  H  initial sets that differ per row (MultiBatch)"""
import collections
import functools
import random

import mem_ref as mr
from acvm_amd.acir import P, BlackBoxFuncCall as BB, Brillig, Circuit, Expression as E, FunctionInput as FI, MemoryInit, MemoryOp

SEED = 20262
LENGTHS = (1, 6, 33, 67)     # cells of a block: one, the size of the older tests, and past the 32 and 64 lanes of a half wave and a wave
U32, U64 = mr.U32, mr.U64
PREDICATES = (1, 2, P - 1)   # every non-zero predicate executes the op
W, K = E.from_witness, E.constant

Case = collections.namedtuple("Case", "name circuit ids rows expect notes traces filler")


class Builder:
    """opcodes of one circuit; witnesses 1..n_inputs are the inputs, every other one is handed out by new()"""

    def __init__(self, n_inputs):
        self.next, self.ops = n_inputs + 1, []

    def new(self):
        self.next += 1
        return self.next - 1

    def gate(self, lin, qc=0, mul=()):
        """out = sum of the terms + qc"""
        out = self.new()
        self.ops.append(E(list(mul), list(lin) + [(P - 1, out)], qc % P))
        return out

    def init(self, block, ws):
        self.ops.append(MemoryInit(block, list(ws)))

    def read(self, block, index, pred=None, operation=None, target=None):
        t = self.new() if target is None else target
        self.ops.append(MemoryOp(block, K(0) if operation is None else operation, index, W(t) if isinstance(t, int) else t, pred))
        return t

    def write(self, block, index, value, pred=None, operation=None):
        self.ops.append(MemoryOp(block, K(1) if operation is None else operation, index, value, pred))

    def access(self, kind, block, index, value, pred=None):
        """a read into a fresh witness, or a write of `value`"""
        return self.read(block, index, pred) if kind == "read" else self.write(block, index, value, pred)

    def range(self, w, bits=8):
        self.ops.append(BB("RANGE", {"input": FI(w, bits)}))

    def circuit(self):
        return Circuit(self.next - 1, self.ops)


def _case(name, circ, ids, rows, notes, filler=None):
    assert len(rows) == len(notes) and 0 < len(rows) <= 200, (name, len(rows))
    assert all(len(row) == len(ids) and all(0 <= v < P for v in row) for row in rows), name
    runs = [mr.run_traced(circ, dict(zip(ids, row))) for row in rows]
    if filler is not None:
        assert runs[filler][0].status == mr.ST_SOLVED, (name, "the filler row does not pass")
    return Case(name, circ, list(ids), [list(r) for r in rows], [x for x, _ in runs], list(notes), [t for _, t in runs], filler)


def padded(case, n):
    """the case with passing rows IN FRONT up to n rows, so that the rows the case is about lie in the last, partial wave"""
    k = n - len(case.rows)
    if k <= 0 or case.filler is None:
        return case
    f = case.filler
    return case._replace(rows=[case.rows[f]] * k + case.rows, expect=[case.expect[f]] * k + case.expect, notes=["filler"] * k + case.notes,
                         traces=[case.traces[f]] * k + case.traces, filler=0)


def describe(case, j):
    return f"{case.name} row {j} ({case.notes[j]})"


def compare(case, got, who, expect=None):
    """got: per row (Result.as_tuple(), message, {witness: value}); every field of the model's expectation, the whole map included"""
    for j, (want, (head, message, wm)) in enumerate(zip(expect or case.expect, got)):
        at = describe(case, j)
        if want.status == mr.ST_REQUIRES_FOREIGN_CALL:
            # (a result carries no instruction pointer for a row that waits: the callers check it where the run gives it -- the oracle's
            # instruction_pointer(), the device's foreign_call_sites())
            assert tuple(head[:2]) == (want.status, want.err), f"{at}: {who} {tuple(head)}, want a row that waits for a foreign call"
        else:
            assert tuple(head) == tuple(want[:5]), f"{at}: {who} (status, error, opcode, aux0, aux1) {tuple(head)}, want {tuple(want[:5])}"
        if want.message is not None:
            assert message == want.message, f"{at}: {who} message {message!r}, want {want.message!r}"
        for w in sorted(set(wm) | set(want.witnesses)):
            g, x = wm.get(w), want.witnesses.get(w)
            assert g == x, (f"{at}: witness {w}: {who} " + (hex(g) if g is not None else "unassigned") + ", want " + (hex(x) if x is not None else "unassigned"))


# ---------------------------------------------------------------------------------------------------------------- A: indices
def index_values(n):
    """[(class, value)] for a block of n cells"""
    return [("0", 0), ("len - 1", n - 1), ("len", n), ("len + 1", n + 1), ("2^32 - 1", U32 - 1), ("2^32", U32), ("2^64 - 2^32", U64 - U32), ("2^32 + len", U32 + n),
            ("2^64 - 1", U64 - 1), ("2^64", U64), ("p - 1", P - 1)]


INDEX_CLASSES = [c for c, _ in index_values(6)]
FORMS = ("witness", "witness + constant", "product", "sum of two gate outputs")


def index_classes(raw, n):
    """the classes an index belongs to (two at a time where the block has one cell: 0 is len - 1 there)"""
    return [c for c, v in index_values(n) if v == raw]


@functools.lru_cache(maxsize=None)
def index_case(n):
    """Inputs: the n cells, then i (the index), i - 3, a and b with a b = i, d = i - t and t, the value to write, and one predicate witness per predicated
    opcode. Opcodes: the gates g1 = d, g2 = t; a read and a write per form of the index, each under its own predicate, in an order rotated by the block
    length (an index that panics does so at the FIRST of them, whatever its predicate); the same eight without a predicate; a read and a write at every
    CONSTANT index that cannot panic, each under its own predicate; reads of some cells. A row sets the index and switches at most one predicate on."""
    rng = random.Random(SEED + n)
    consts = [v for _, v in index_values(n) if v < U64]
    n_pred = 8 + 2 * len(consts)
    cells = list(range(1, n + 1))
    wi, wi3, wa, wb, wd, wt, wv = range(n + 1, n + 8)
    preds = list(range(n + 8, n + 8 + n_pred))
    ids = cells + [wi, wi3, wa, wb, wd, wt, wv] + preds
    b = Builder(len(ids))
    b.init(0, cells)
    g1, g2 = b.gate([(1, wd)]), b.gate([(1, wt)])
    forms = {"witness": W(wi), "witness + constant": E([], [(1, wi3)], 3), "product": E([(1, wa, wb)], [], 0), "sum of two gate outputs": E([], [(1, g1), (1, g2)], 0)}
    eight = [(kind, f) for f in FORMS for kind in ("read", "write")]
    rot = LENGTHS.index(n)
    eight = eight[rot:] + eight[:rot]
    slot_of = {}
    for k, (kind, f) in enumerate(eight):
        slot_of[k] = f"{kind}, index as {f}"
        b.access(kind, 0, forms[f], W(wv), W(preds[k]))
    for kind, f in eight:
        b.access(kind, 0, forms[f], W(wv))
    for k, c in enumerate(consts):
        for h, kind in enumerate(("read", "write")):
            slot = 8 + 2 * k + h
            slot_of[slot] = f"{kind}, constant index {c:#x}"
            b.access(kind, 0, K(c), W(wv), W(preds[slot]))
    for c in sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n))):
        b.read(0, K(c))
    rows, notes = [], []

    def row(v, slot, pred, wrap, note):
        t = rng.randrange(v + 1, P) if wrap and v < P - 1 else rng.randrange(v + 1)
        kb = rng.randrange(1, P)
        r = [rng.randrange(P) for _ in cells] + [v, (v - 3) % P, v * pow(kb, -1, P) % P, kb, (v - t) % P, t, rng.randrange(P)] + [0] * n_pred
        if slot is not None:
            r[len(cells) + 7 + slot] = pred
        rows.append(r)
        notes.append(note)

    k = 0
    for c, v in index_values(n):
        for slot in [None] + list(range(8)):
            pred = PREDICATES[k % 3]
            k += 1
            row(v, slot, pred, k % 2, f"index {c}, " + ("no predicate switched on" if slot is None else f"predicate {pred:#x} on the {slot_of[slot]}"))
    for slot in range(8, n_pred):
        for _ in range(2):
            k += 1
            row(rng.randrange(n), slot, PREDICATES[k % 3], k % 2, f"predicate on the {slot_of[slot]}")
    if len(rows) % 64 == 0:
        row(0, None, 1, 0, "filler")
    return _case(f"A, {n} cells", b.circuit(), ids, rows, notes, filler=0)


# ---------------------------------------------------------------------------------------------------------------- B: operation
@functools.lru_cache(maxsize=None)
def operation_case():
    """Inputs 1..6 the cells, 7 = v (a known value), 8 = o1, 9 = o2, 10 = a1, 11 = b1, 12 = a2, 13 = b2. Opcodes: constant operations 0, 1, 2 and p - 1 (one
    read, three writes, read back); then four opcodes whose operation differs by row -- witness o1 with an UNKNOWN witness as value (operation 0: the
    read succeeds; else the write is MissingAssignment of that witness), witness o2 with the KNOWN v (non-zero: the write succeeds; 0: the read panics),
    a1 - b1 with an unknown witness, a2 - b2 with v -- and reads of the cells they touch. The first of the four truncates the plan."""
    ids = list(range(1, 14))
    b = Builder(13)
    b.init(0, range(1, 7))
    b.read(0, K(0), operation=K(0))
    for c, op in ((1, 1), (2, 2), (3, P - 1)):
        b.write(0, K(c), E([], [(1, 7)], op), operation=K(op))
        b.read(0, K(c))
    duals = []
    for operation, value in ((W(8), None), (W(9), W(7)), (E([], [(1, 10), (P - 1, 11)], 0), None), (E([], [(1, 12), (P - 1, 13)], 0), E([], [(1, 7)], 0))):
        duals.append(len(b.ops))
        if value is None:
            b.read(0, K(4), operation=operation)
        else:
            b.write(0, K(5), value, operation=operation)
        b.read(0, K(4))
        b.read(0, K(5))
    rng = random.Random(SEED + 100)
    rows, notes = [], []
    for o1 in (0, 1, 7):
        for o2 in (1, 0, 7):
            for d1 in (0, 1):
                for d2 in (1, 0):
                    a1, a2 = rng.randrange(P), rng.randrange(P)
                    rows.append([rng.randrange(P) for _ in range(6)] + [rng.randrange(P), o1, o2, a1, (a1 - d1 * rng.randrange(1, P)) % P, a2, (a2 - d2 * rng.randrange(1, P)) % P])
                    notes.append(f"o1 = {o1}, o2 = {o2}, a1 - b1 {'!=' if d1 else '='} 0, a2 - b2 {'!=' if d2 else '='} 0")
    case = _case("B, operations", b.circuit(), ids, rows, notes, filler=0)
    return case, tuple(duals)


@functools.lru_cache(maxsize=None)
def unassigned_cases():
    """an operation, then an index, that names a witness nobody assigns: MissingAssignment of that witness, the operation's before the index's"""
    rng = random.Random(SEED + 150)
    rows = [[rng.randrange(P) for _ in range(7)] for _ in range(3)]
    out = []
    for what in ("operation", "index", "operation and index"):
        b = Builder(7)
        b.init(0, range(1, 7))
        b.read(0, K(1))
        n1, n2, n3 = b.new(), b.new(), b.new()
        operation = E([], [(1, 7), (2, n1)], 0) if "operation" in what else K(1)
        index = E([(1, n2, n3)], [(1, 7)], 0) if "index" in what else K(2)
        b.write(0, index, W(7), operation=operation)
        case = _case(f"B, {what} unassigned", b.circuit(), list(range(1, 8)), rows, [what] * 3)
        assert all((x.err, x.aux0, x.opcode_index) == (mr.E_MISSING_ASSIGNMENT, n1 if "operation" in what else n2, 2) for x in case.expect)
        out.append(case)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- C: read targets
TARGETS = ("w", "2 w", "w + 1", "w + w_a - w_b", "c w_known w", "w + 0 u", "constant", "initial witness")


def _target(kind, t, u):
    """the value expression of a read whose fresh witness is t; inputs: 7 = w_a, 8 = w_b, 9 = w_known (3 or 1 / 3), 10 = an initial witness"""
    return {"w": W(t), "2 w": E([], [(2, t)], 0), "w + 1": E([], [(1, t)], 1), "w + w_a - w_b": E([], [(1, t), (1, 7), (P - 1, 8)], 0),
            "c w_known w": E([(3, 9, t)], [], 0), "w + 0 u": E([], [(1, t), (0, u)], 0), "constant": K(5), "initial witness": W(10)}[kind]


INV3 = pow(3, -1, P)


def _target_rows(n_extra):
    """w_a = w_b or not, 3 w_known = 1 or not, the index inside and outside; then n_extra predicate witnesses, switched on one at a time and all at once"""
    rng = random.Random(SEED + 200)
    rows, notes = [], []
    for eq in (1, 0):
        for unit in (1, 0):
            for index in (2, 9):
                for on in ([None] if n_extra == 0 else list(range(n_extra)) + ["all", "none"]):
                    a = rng.randrange(P)
                    preds = [PREDICATES[(len(rows) // 3 + len(rows)) % 3] if on in (k, "all") else 0 for k in range(n_extra)]
                    rows.append([rng.randrange(P) for _ in range(6)] + [a, a if eq else (a + 1) % P, INV3 if unit else 3, rng.randrange(P), index] + preds)
                    notes.append(f"w_a {'=' if eq else '!='} w_b, 3 w_known {'=' if unit else '!='} 1, index {index}" + (f", predicates on: {on}" if n_extra else ""))
    return rows, notes


@functools.lru_cache(maxsize=None)
def target_cases():
    """Inputs 1..6 the cells, 7..10 as _target says, 11 the index, then predicate witnesses. One circuit holds the four targets that can be a witness
    (each under its own predicate, then each without one) followed by a gate on what they read; every target that never is a witness has a circuit of
    its own, with a predicate witness (the panic comes before the zero-predicate test); and every target has one more circuit whose predicate
    witness nobody assigns (MissingAssignment comes before the panic)."""
    can = ("w", "w + 0 u", "w + w_a - w_b", "c w_known w")
    out = []
    b = Builder(15)
    b.init(0, range(1, 7))
    u = b.new()  # never assigned
    got = []
    for k, kind in enumerate(can):
        t = b.new()
        b.read(0, W(11), W(12 + k), target=_target(kind, t, u))
        got.append(t)
    for kind in can:
        t = b.new()
        b.read(0, K(3), target=_target(kind, t, u))
        got.append(t)
    b.gate([(1 + k, t) for k, t in enumerate(got)])
    rows, notes = _target_rows(4)
    out.append(_case("C, targets that can be a witness", b.circuit(), list(range(1, 16)), rows, notes, filler=[n.endswith("none") for n in notes].index(True)))
    for kind in TARGETS:
        for missing in (False, True):
            if kind in can and not missing:
                continue
            b = Builder(12)
            b.init(0, range(1, 7))
            u, t = b.new(), b.new()
            absent = b.new()  # the predicate nobody assigns
            b.read(0, W(11), W(absent if missing else 12), target=_target(kind, t, u))
            b.gate([(1, 11)])
            rows, notes = _target_rows(1)
            out.append(_case(f"C, target {kind}" + (", predicate unassigned" if missing else ""), b.circuit(), list(range(1, 13)), rows, notes))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- D: written values
@functools.lru_cache(maxsize=None)
def value_case():
    """Inputs 1..6 the cells, 7 = x, 8 = y, 9 = z, then predicates. Writes whose value holds witnesses nobody assigns (u1, u2, u3), each under its own
    predicate: MissingAssignment names the first linear witness of the EVALUATED value, else the left witness of its first product; under a zero
    predicate nothing happens. Then writes of x, of x + y, of x y + z, of 2 x + (p - 1) y + 5, each read back."""
    b = Builder(15)
    b.init(0, range(1, 7))
    u1, u2, u3 = b.new(), b.new(), b.new()
    bad = [("u1", W(u1), u1), ("3 u1 + x", E([], [(3, u1), (1, 7)], 0), u1), ("x u2 (linear after evaluation)", E([(1, 7, u2)], [], 4), u2),
           ("u1 u2 + u3 (the linear witness wins)", E([(1, u1, u2)], [(1, u3)], 0), u3), ("u2 u1 (the left witness)", E([(5, u2, u1)], [(1, 8)], 0), u2),
           ("x u3 + u1 (the product comes first)", E([(1, 7, u3)], [(1, u1)], 0), u3)]
    for k, (_, value, _) in enumerate(bad):
        b.write(0, K(k % 6), value, W(10 + k))
    good = [W(7), E([], [(1, 7), (1, 8)], 0), E([(1, 7, 8)], [(1, 9)], 0), E([], [(2, 7), (P - 1, 8)], 5), K(P - 1), K(0)]
    back = []
    for k, value in enumerate(good):
        b.write(0, K(k), value)
        back.append(b.read(0, K(k)))
    b.gate([(1, t) for t in back])
    rng = random.Random(SEED + 300)
    rows, notes = [], []
    for x, y, z, note in ((0, 0, 0, "zeros"), (P - 1, P - 1, P - 1, "p - 1 everywhere"), (P - 1, 1, 0, "x + y wraps to 0"), (P - 1, 2, P - 1, "x + y = 1"), (1, P - 1, 1, "x y + z = 0"),
                          (P // 2 + 1, P // 2 + 1, 5, "2 x wraps"), (rng.randrange(P), rng.randrange(P), rng.randrange(P), "random"), (2, 3, 4, "small")):
        rows.append([rng.randrange(P) for _ in range(6)] + [x, y, z] + [0] * 6)
        notes.append(note)
    for k, (what, _, w) in enumerate(bad):
        for pred in PREDICATES:
            rows.append([rng.randrange(P) for _ in range(6)] + [rng.randrange(1, P), rng.randrange(P), rng.randrange(P)] + [pred if i == k else 0 for i in range(6)])
            notes.append(f"value {what} under predicate {pred:#x}: MissingAssignment of witness {w}")
    case = _case("D, written values", b.circuit(), list(range(1, 16)), rows, notes, filler=7)
    for j, x in enumerate(case.expect[8:]):
        assert (x.err, x.aux0, x.opcode_index) == (mr.E_MISSING_ASSIGNMENT, bad[j // 3][2], 1 + j // 3), (j, x[:5])
    return case


# ---------------------------------------------------------------------------------------------------------------- E: blocks
@functools.lru_cache(maxsize=None)
def block_cases():
    """Inputs 1..8 values, 9..12 predicates (0 in the rows that pass). See each circuit's name."""
    rng = random.Random(SEED + 400)
    ids = list(range(1, 13))
    out = []

    def rows_for(n_preds):
        rows, notes = [], []
        for on in [None] + list(range(n_preds)):
            for rep in range(2):
                rows.append([rng.randrange(P) for _ in range(8)] + [PREDICATES[(rep + (on or 0)) % 3] if k == on else 0 for k in range(4)])
                notes.append("nothing switched on" if on is None else f"predicate {on} on")
        return rows, notes

    # 4 cells, a write, 2 cells from other witnesses: the keys 2 and 3 stay readable and hold the OLD cells (one of them the written one)
    b = Builder(12)
    b.init(0, [1, 2, 3, 4])
    b.write(0, K(3), W(5))
    b.write(0, K(0), W(5))
    b.init(0, [6, 7])
    back = [b.read(0, K(c)) for c in range(4)]
    b.write(0, K(2), W(8), W(9))        # out of bounds: (2, 2)
    b.read(0, K(4), W(10))              # out of bounds: (4, 2)
    b.write(0, K(1), W(8), W(11))       # in bounds
    back.append(b.read(0, K(1)))
    b.init(0, [8, 7, 6, 5, 4, 3])       # longer again
    back += [b.read(0, K(c)) for c in range(6)]
    b.read(0, K(6), W(12))              # out of bounds: (6, 6)
    b.gate([(1 + k, t) for k, t in enumerate(back)])
    out.append(_case("E, 4 cells then 2 then 6", b.circuit(), ids, *rows_for(4), filler=0))

    b = Builder(12)
    b.init(5, [1, 2, 3])
    b.init(5, [])
    back = [b.read(5, K(c)) for c in range(3)]   # stale keys
    b.write(5, K(0), W(4), W(9))        # (0, 0)
    b.read(5, K(3), W(10))              # (3, 0)
    back.append(b.read(5, K(U32 + 1), W(11)))   # wraps to 1: a stale key again
    b.gate([(1, t) for t in back])
    b.ops.append(E([], [(1, back[0]), (P - 1, 8)], 0))   # the stale cell 0 still is witness 1: the rows carry it in witness 8 too, but for the last two
    rows, notes = rows_for(3)
    rows = [r[:7] + [r[0]] + r[8:] for r in rows] + [r[:7] + [(r[0] + 1 + k) % P] + [0] * 4 for k, r in enumerate(rows[:2])]
    out.append(_case("E, 3 cells then none", b.circuit(), ids, rows, notes + ["the stale cell is not what witness 8 says"] * 2, filler=0))

    b = Builder(12)
    t0 = b.read(9, K(0), W(9))          # a block no MemoryInit names: length 0; under a zero predicate the target is 0
    b.write(9, K(0), W(1), W(10))
    t1 = b.read(9, K(5), W(11))
    b.gate([(1, t0), (1, t1), (1, 3)])
    out.append(_case("E, a block without init", b.circuit(), ids, *rows_for(3), filler=0))

    # ids 7, 2^32 - 1, 0 in that order; witness 1 twice in an init; a block initialised from another block's read targets
    b = Builder(12)
    b.init(7, [1, 2, 1])
    b.init(U32 - 1, [3, 4])
    b.init(0, [5])
    r7 = [b.read(7, K(c)) for c in (2, 0, 1)]
    b.write(U32 - 1, K(1), W(r7[0]))
    rmax = [b.read(U32 - 1, K(c)) for c in (1, 0)]
    b.write(7, K(0), W(6))              # one of the two cells that came from witness 1
    b.init(3, r7 + rmax)
    r3 = [b.read(3, K(c)) for c in range(5)]
    r0 = b.read(0, K(0))
    b.read(7, K(3), W(9))               # (3, 3)
    b.read(0, K(1), W(10))              # (1, 1)
    b.write(U32 - 1, K(2), W(7), W(11))  # (2, 2)
    again = [b.read(7, K(c)) for c in range(3)]
    b.gate([(1 + k, t) for k, t in enumerate(r3 + [r0] + again)])
    out.append(_case("E, block ids 7, 2^32 - 1, 0, 3", b.circuit(), ids, *rows_for(3), filler=0))

    b = Builder(12)
    b.init(1, [1, 2])
    t = b.read(1, K(1))
    nobody = b.new()
    b.init(2, [3, t, nobody, 4])
    b.read(2, K(0))
    rows, notes = rows_for(0)
    case = _case("E, an init that names an unassigned witness", b.circuit(), ids, rows, notes)
    assert all((x.err, x.aux0, x.opcode_index) == (mr.E_MISSING_ASSIGNMENT, nobody, 2) for x in case.expect)
    out.append(case)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- F: order
ORDER_SEEDS = (1, 2, 3)
ORDER_BLOCKS = ((0, 6), (1, 33), (2, 67))


@functools.lru_cache(maxsize=None)
def order_case(seed):
    """A seeded program: three blocks of 6, 33 and 67 cells, about 120 MemoryOps with constant operations and about 40 gates. Every cell and every
    written value is 0, 1 or 2, so a read target (plus a constant) is an index inside the block, and a predicate that is zero in some rows; the gates
    turn earlier targets into later indices, values and predicates. Inputs: the 106 cells, then s (0, 1 or 2), z (0: added into one index in
    mid-program; 100 takes it out of bounds), and four RANGE tripwires r1..r4 (8 bits) standing at a quarter, a half, three quarters and the end of
    the program. Returns (case, failing rows, tripwire positions)."""
    rng = random.Random(SEED + 500 + seed)
    n_cells = sum(n for _, n in ORDER_BLOCKS)
    ws, wz = n_cells + 1, n_cells + 2
    trip = [n_cells + 3 + k for k in range(4)]
    ids = list(range(1, n_cells + 7))
    b = Builder(len(ids))
    first = 1
    for blk, n in ORDER_BLOCKS:
        b.init(blk, range(first, first + n))
        first += n
    small = [ws]          # witnesses that hold 0, 1 or 2 in every passing row
    n_mem = n_gates = 0
    trip_at, z_at = [], None
    total = 120
    while n_mem < total:
        k = n_mem
        if len(trip_at) < 3 and k >= (len(trip_at) + 1) * total // 4:
            trip_at.append(len(b.ops))
            b.range(trip[len(trip_at) - 1])
        blk, n = ORDER_BLOCKS[rng.randrange(3)]
        t = rng.choice(small[-12:])
        c = rng.randrange(n - 2)      # a witness of `small` plus c stays inside the block
        choice = rng.random()
        pred = None if rng.random() < 0.6 else W(rng.choice(small))
        if choice < 0.33:
            if z_at is None and k >= total // 2:
                z_at = len(b.ops) + 1
                g = b.gate([(1, t), (1, wz)], c)
                pred = None
            else:
                g = b.gate([(1, t)], c)
            n_gates += 1
            index = W(g)
        else:
            index = K(c) if choice < 0.55 else E([], [(1, t)], c)
        if rng.random() < 0.55:
            small.append(b.read(blk, index, pred))
        else:
            b.write(blk, index, W(rng.choice(small)), pred)
        n_mem += 1
    for blk, n in ORDER_BLOCKS:
        for c in range(n):
            b.read(blk, K(c))
    trip_at.append(len(b.ops))
    b.range(trip[3])
    assert z_at is not None and len(trip_at) == 4

    def row(z=0, tripped=None):
        return [rng.randrange(3) for _ in range(n_cells)] + [rng.randrange(3), z] + [256 + rng.randrange(1 << 20) if k == tripped else rng.randrange(256) for k in range(4)]

    rows = [row() for _ in range(20)]
    notes = ["passes"] * 20
    failing = []
    for k in range(4):
        failing.append(len(rows))
        rows.append(row(tripped=k))
        notes.append(f"tripwire {k + 1} at opcode {trip_at[k]}")
    failing.append(len(rows))
    rows.append(row(z=100))
    notes.append(f"index out of bounds at opcode {z_at}")
    rows += [row() for _ in range(45)]
    notes += ["passes"] * 45
    case = _case(f"F, seed {seed}", b.circuit(), ids, rows, notes, filler=0)
    for k in range(4):
        x = case.expect[failing[k]]
        assert (x.status, x.err, x.opcode_index) == (mr.ST_FAILURE, mr.E_UNSATISFIED, trip_at[k]), (seed, k, x[:5])
    x = case.expect[failing[4]]
    assert (x.err, x.opcode_index, x.aux0 >= 100) == (mr.E_INDEX_OOB, z_at, True), (seed, x[:5], z_at)
    assert all(x.status == mr.ST_SOLVED for j, x in enumerate(case.expect) if j not in failing), seed
    return case, tuple(failing), tuple(trip_at)


# ---------------------------------------------------------------------------------------------------------------- G: re-entries
LOOP = [("Const", 1, 0), ("Const", 2, 1), ("BinaryFieldOp", 3, "Equals", 1, 0), ("JumpIf", 3, 6), ("BinaryFieldOp", 1, "Add", 1, 2), ("Jump", 2), ("Mov", 0, 1), ("Stop",)]
LOOP_STEPS_LOG2 = 8     # the level kernels' step limit the device tests lower to (2^8): the loop needs 4 n + 5 steps, so n = 62 stays below and 63 is past it
LOOP_COUNTS = (0, 1, 62, 63, 64, 100, 300)


def answer_of(row):
    """what the host answers to the foreign call of a row: three times its input plus one"""
    return [(3 * row[7] + 1) % P]


@functools.lru_cache(maxsize=None)
def reentry_case(form, dynamic):
    """Inputs 1..6 the cells, 7 = v, 8 = n (the loop count, or the foreign call's input), 9 = o (an operation that writes: 1, 2 or p - 1), 10 = o0 (0 in every
    row: an operation that reads), 11 = z (a predicate: 0 in two rows of three, else 1). Opcodes: block 0 from the six cells; block 1 from four of them and
    again from two (keys 2 and 3 stay readable, the length is 2); a read, static writes into cells 0, 1 and 4; with `dynamic`, a write under the operation o
    into cell 2, and three reads under the operation o0 -- opcodes a replay of memory side effects takes for writes of their own targets: of cell 1 (a static
    write over that cell follows), of cell 3 under the predicate z (where z = 0 the target is 0 and the cell must keep its value), and of the stale key 3 of
    block 1 (past the block's length: nothing may be written) --; a straight-line Brillig opcode (v + v, which the planner may inline) whose output is
    written into cell 0; then the Brillig opcode that re-enters -- form "call": it stops at a foreign call; form "loop": n iterations --, a write of its
    output, and reads of every cell and key of both blocks."""
    ids = list(range(1, 12))
    b = Builder(11)
    b.init(0, range(1, 7))
    b.init(1, [1, 2, 3, 4])
    b.init(1, [5, 6])
    first = b.read(0, K(4))
    b.write(0, K(0), W(7))
    b.write(0, K(1), E([], [(1, 7), (1, first)], 1))
    b.write(0, K(4), E([(1, 7, 7)], [], 0))
    targets = []
    if dynamic:
        b.write(0, K(2), E([], [(2, 7)], 0), operation=W(9))
        targets.append(b.read(0, K(1), operation=W(10)))
        b.write(0, K(1), W(first))
        targets.append(b.read(0, K(3), W(11), operation=W(10)))
        targets.append(b.read(1, K(3), operation=W(10)))
    twice = b.new()
    b.ops.append(Brillig(inputs=[W(7)], outputs=[twice], bytecode=[("BinaryFieldOp", 0, "Add", 0, 0), ("Stop",)]))
    b.write(0, K(0), W(twice))
    out = b.new()
    if form == "call":
        b.ops.append(Brillig(inputs=[W(8)], outputs=[b.new(), out], bytecode=[("ForeignCall", "answer", [("Register", 1)], [("Register", 0)]), ("Stop",)]))
    else:
        b.ops.append(Brillig(inputs=[W(8)], outputs=[out], bytecode=LOOP))
    b.write(0, K(5), W(out))
    back = [b.read(0, K(c)) for c in range(6)] + [b.read(1, K(c)) for c in range(4)]
    b.gate([(1 + k, t) for k, t in enumerate(back + targets)])
    rng = random.Random(SEED + 600 + len(form) + dynamic)
    rows, notes = [], []
    for j in range(67):
        n = LOOP_COUNTS[j % 7] if form == "loop" else rng.randrange(P)
        z = 1 if j % 3 == 2 else 0
        rows.append([rng.randrange(1, P) for _ in range(6)] + [rng.randrange(P), n, (1, 2, P - 1)[j % 3], 0, z])
        notes.append((f"n = {n}" if form == "loop" else "waits") + f", z = {z}")
    return _case(f"G, {form}, {'with' if dynamic else 'without'} dynamic operations", b.circuit(), ids, rows, notes, filler=0 if form == "loop" else None)


def answered_expect(case):
    return [mr.run(case.circuit, dict(zip(case.ids, row)), answers=[answer_of(row)]) for row in case.rows]


REENTRIES = tuple((form, dynamic) for form in ("call", "loop") for dynamic in (False, True))


# ---------------------------------------------------------------------------------------------------------------- H: initial sets
@functools.lru_cache(maxsize=None)
def initial_set_case():
    """(circuit, maps, expect, notes): one group of maps assigns witnesses 1..4; one also knows witness 5, the target of the first read (the panic of
    to_witness); one lacks witness 2, which the init names (MissingAssignment of 2 at opcode 0)"""
    b = Builder(4)
    b.init(0, [1, 2, 3])
    t = b.read(0, W(4))
    assert t == 5
    b.write(0, K(0), W(t))
    t2 = b.read(0, K(0))
    b.gate([(1, t), (1, t2)])
    circ = b.circuit()
    rng = random.Random(SEED + 700)
    maps, notes = [], []
    for j in range(21):
        m = {1: rng.randrange(P), 2: rng.randrange(P), 3: rng.randrange(P), 4: j % 3}
        if j % 3 == 1:
            m[5] = m[1 + j % 3] if j % 2 else rng.randrange(P)
            notes.append("knows the read target")
        elif j % 3 == 2:
            del m[2]
            notes.append("lacks an init witness")
        else:
            notes.append("the plain set")
        maps.append(m)
    expect = [mr.run(circ, m) for m in maps]
    assert {(x.err, x.opcode_index) for x in expect} == {(mr.E_NONE, 0), (mr.E_PANIC, 1), (mr.E_MISSING_ASSIGNMENT, 0)}
    return circ, tuple(maps), tuple(expect), tuple(notes)


# ---------------------------------------------------------------------------------------------------------------- the lists
@functools.lru_cache(maxsize=None)
def lists():
    """{letter: the cases that run as plain batches}; G's cases wait or need a lowered limit, H's rows are maps: they have tests of their own"""
    return {"A": tuple(index_case(n) for n in LENGTHS), "B": (operation_case()[0],) + unassigned_cases(), "C": target_cases(), "D": (value_case(),), "E": block_cases(),
            "F": tuple(order_case(s)[0] for s in ORDER_SEEDS), "G": tuple(reentry_case("loop", d) for d in (False, True))}


def all_cases():
    return [c for cs in lists().values() for c in cs]
