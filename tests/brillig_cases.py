"""One builder of the inputs that reach the edges of the Brillig VM (acvm_amd/csrc/ops_brillig.hpp; the straight-line inliner, plan.cpp
emit_straight_line and ops_light.hpp op_brillig_sl), with every expected outcome from the Python-integer model tests/brillig_ref.py: no oracle and
no device here. Random rows never reach these branches (a random address is a panic, a random program has no call stack), so every list is built
around the memory's length, the register file's end, the bytecode's end, the shape of a foreign-call result and the operands of a black box.
tests/test_brillig_cases.py runs the lists through the CPU oracle and asserts what they cover; tests/test_gpu_brillig_edges.py runs them on the device.

A case is int_cases.Case(name, circuit, ids, rows, expect, labels, notes); per row Expect(status, err, opcode_index, witnesses, message, call_stack,
pending, kind, branches): `witnesses` the WHOLE witness map the reference leaves behind (outputs inserted before a panic included), `call_stack`
the reference's whole error stack (compare() cuts it by the ABI's rule), `pending` (function, inputs) of a row that waits, `kind` and `branches`
the model's outcome kind and branch labels.

Batches are no multiples of 64, and stored addresses stay below 4096: no row meets a device maximum (tests/test_gpu_brillig_limits.py has those).
Left out because nothing pins the value (tests/grumpkin_ref.py says what is UNPINNED): Pedersen with no inputs, and Pedersen with a domain separator
other than 0 -- 2^32 - 1 and 2^128 + 3; the truncation of to_u128 is reached with 2^128 (-> 0, pinned) and 2^128 + 2^32 (-> 2^32, fails) instead."""
import collections
import functools

import brillig_ref as br
import int_cases as ic
from acvm_amd.acir import P, Brillig, Circuit, Expression as E

W = E.from_witness
K = E.constant
ST_SOLVED, ST_FAILURE, ST_REQUIRES_FOREIGN_CALL = 0, 2, 3     # as oracle/binding.py numbers them (tests/test_brillig_cases.py asserts that)
E_NONE, E_MISSING_ASSIGNMENT, E_TOO_MANY_UNKNOWNS, E_UNSATISFIED, E_BRILLIG_FAILED, E_PANIC = 0, 1, 2, 4, 7, 8
HEAD = {br.SOLVED: (ST_SOLVED, E_NONE), br.UNSATISFIED: (ST_FAILURE, E_UNSATISFIED), br.TOO_MANY_UNKNOWNS: (ST_FAILURE, E_TOO_MANY_UNKNOWNS),
        br.MISSING_ASSIGNMENT: (ST_FAILURE, E_MISSING_ASSIGNMENT), br.BRILLIG_FAILED: (ST_FAILURE, E_BRILLIG_FAILED), br.PANIC: (ST_FAILURE, E_PANIC),
        br.REQUIRES_FOREIGN_CALL: (ST_REQUIRES_FOREIGN_CALL, E_NONE)}
U32, U64 = 1 << 32, 1 << 64

Expect = collections.namedtuple("Expect", "status err opcode_index witnesses message call_stack pending kind branches")
Case = ic.Case


def model(circ, ids, row, answers=()):
    """the reference's solve loop (pwg/mod.rs:203-304) over the opcodes in program order; answers: what the host resolved so far for the opcode that
    waits, one result per round (the opcode is solved again from its start with them appended)"""
    wm = dict(zip(ids, row))
    branches = set()
    for oi, op in enumerate(circ.opcodes):
        if not isinstance(op, Brillig):
            bad = ic._step(op, wm)
            if bad:
                return Expect(ST_FAILURE, bad[0], oi, wm, bad[1], None, None, None, frozenset(branches))
            continue
        out = br.run(op, wm, answers)
        branches |= out.labels
        if out.kind != br.SOLVED:
            pending = (out.function, out.inputs) if out.kind == br.REQUIRES_FOREIGN_CALL else None
            return Expect(*HEAD[out.kind], oi, wm, out.message, out.call_stack, pending, out.kind, frozenset(branches))
    return Expect(ST_SOLVED, E_NONE, 0, wm, None, None, None, br.SOLVED, frozenset(branches))


def describe(case, j):
    return f"{case.name} row {j} ({case.notes[j]}), inputs {[hex(v) for v in case.rows[j][:8]]}"


def compare(case, got, who, expect=None):
    """got: per row (status, err, opcode_index, message, witness map, call stack, pending) -- pending None where the run was not asked for it"""
    for j, (want, (status, err, opcode, message, wm, call_stack, pending)) in enumerate(zip(expect or case.expect, got)):
        at = describe(case, j)
        assert (status, err) == (want.status, want.err), f"{at}: {who} status / error {(status, err)}, want {(want.status, want.err)} ({want.kind})"
        if want.status == ST_FAILURE:
            assert opcode == want.opcode_index, f"{at}: {who} fails at opcode {opcode}, want {want.opcode_index}"
        if want.message is not None:
            assert message == want.message.encode(), f"{at}: {who} message {message!r}, want {want.message!r}"
        if want.call_stack is not None:
            assert list(call_stack) == br.abi_call_stack(want.call_stack), f"{at}: {who} call stack {list(call_stack)}, want {br.abi_call_stack(want.call_stack)}"
        if want.pending is not None and pending is not None:
            assert pending[0] == want.pending[0], f"{at}: {who} waits for {pending[0]!r}, want {want.pending[0]!r}"
            assert [list(x) for x in pending[1]] == want.pending[1], f"{at}: {who} pending inputs {pending[1]}, want {want.pending[1]}"
        for w in sorted(set(wm) | set(want.witnesses)):
            g, x = wm.get(w), want.witnesses.get(w)
            assert g == x, (f"{at}: witness {w} ({case.labels.get(w, 'input')}): {who} " + (hex(g) if g is not None else "unassigned") +
                            ", want " + (hex(x) if x is not None else "unassigned"))


def _case(name, ops, ids, rows, notes, labels=None):
    if isinstance(ops, Brillig):
        ops = [ops]
    nw = max([0] + list(ids) + [w for op in ops for o in op.outputs for w in ([o] if isinstance(o, int) else o)])
    circ = Circuit(nw, list(ops))
    rows = [list(r) for r in rows]
    assert len(rows) == len(notes) and len(rows) % 64 and len(rows) <= 135, (name, len(rows))
    assert all(0 <= v < P for row in rows for v in row) and all(len(row) == len(ids) for row in rows), name
    return Case(name, circ, list(ids), rows, [model(circ, ids, row) for row in rows], labels or {}, list(notes))


def inlinable(b):
    """plan.cpp emit_straight_line, restated: single-value inputs and outputs, at most four registers, and nothing but field / integer operations,
    Const, Mov, Stop, Trap and FORWARD jumps"""
    if not b.bytecode or len(b.inputs) > 4 or len(b.outputs) > 4 or any(not isinstance(i, E) for i in b.inputs) or any(not isinstance(o, int) for o in b.outputs):
        return False
    fixed, used = max(len(b.inputs), len(b.outputs)), set()
    for k, op in enumerate(b.bytecode):
        if op[0] in ("BinaryFieldOp",):
            regs = (op[1], op[3], op[4])
        elif op[0] == "BinaryIntOp":
            regs = (op[1], op[4], op[5])
        elif op[0] == "Const":
            regs = (op[1],)
        elif op[0] == "Mov":
            regs = (op[1], op[2])
        elif op[0] in ("JumpIf", "JumpIfNot", "Jump"):
            regs = (op[1],) if op[0] != "Jump" else ()
            if op[-1] <= k:
                return False
        elif op[0] in ("Stop", "Trap"):
            regs = ()
        else:
            return False
        used |= {r for r in regs if r >= fixed}
    return fixed + len(used) <= 4 and all(r < 65536 for r in used)


def n_inlinable(case):
    """how many opcodes of the case the level schedule runs inlined: the inlinable ones whose inputs and predicate name only witnesses that the initial
    map or an earlier opcode assigns (an opcode that can never be solved has no level, and only the exact path reports it)"""
    known, n = set(case.ids), 0
    for op in case.circuit.opcodes:
        if not isinstance(op, Brillig):
            continue
        exprs = [e for i in op.inputs for e in ([i] if isinstance(i, E) else i)] + ([op.predicate] if op.predicate is not None else [])
        reads = {w for e in exprs for _, l, r in e.mul_terms for w in (l, r)} | {w for e in exprs for _, w in e.linear_combinations}
        n += inlinable(op) and reads <= known
        known |= {w for o in op.outputs for w in ([o] if isinstance(o, int) else o)}
    return n


# ---- memory
MEM_CAP_ESTIMATE = 4 + 0 + 64   # plan.cpp's first capacity for the program below: the input arrays' cells + the largest small Const (none) + 64


@functools.lru_cache(maxsize=None)
def memory_case():
    """Inputs: witnesses 1-4 an array (register 0 = 0), 5 the Store address, 6 the stored value, 7 the Load address, 8 the base of the output array.
    Store mem[r1] = r2; Load r0 = mem[r3]; r1 = r4. Outputs: witness 9 = r0 (the loaded cell), witnesses 10-12 = mem[r1 .. r1 + 3]."""
    b = Brillig(inputs=[[W(1), W(2), W(3), W(4)], W(5), W(6), W(7), W(8)], outputs=[9, [10, 11, 12]],
                bytecode=[("Store", 1, 2), ("Load", 0, 3), ("Mov", 1, 4), ("Stop",)])
    rows, notes = [], []
    far = [U32 - 1, U32, U64 - 1, U64, P - 1]
    for j, s in enumerate([0, 3, 4, 5, MEM_CAP_ESTIMATE - 1, MEM_CAP_ESTIMATE, 1000]):
        n = max(4, s + 1)  # the memory's length behind the Store
        loads = [0, 3, 4, n - 2, n - 1, n, n + 1] + far
        for a in loads:
            rows.append([11, 12, 13, 14, s, 100 + j, a, 0])
            notes.append(f"store at {s}, load at {a:#x} of {n} cells")
        if s in (0, 5, MEM_CAP_ESTIMATE):
            for base in [0, 1, n - 4, n - 3, n - 2, n - 1, n, n + 1] + far:
                rows.append([11, 12, 13, 14, s, 100 + j, n - 1 if s == 5 else 0, base])
                notes.append(f"store at {s}, outputs from {base:#x} of {n} cells")
    ic._pad(rows, notes, [1, 2, 3, 4, 0, 5, 0, 0])
    return _case("memory", b, range(1, 9), rows, notes, {9: "the loaded cell", 10: "output cell 0", 11: "output cell 1", 12: "output cell 2"})


# ---- registers
@functools.lru_cache(maxsize=None)
def registers_case():
    """r0, r1 select: neither, write then read register 65535; r0, read register 65536; r1, write register 65536. 65 536 registers are 2 MiB of
    scratch per lane on the device: seven rows."""
    b = Brillig(inputs=[W(1), W(2)], outputs=[3, 4, 5],
                bytecode=[("JumpIf", 0, 5), ("JumpIf", 1, 7), ("Const", 65535, 77), ("Mov", 2, 65535), ("Stop",), ("Mov", 2, 65536), ("Stop",), ("Const", 65536, 1), ("Stop",)])
    rows = [[0, 0], [0, 0], [1, 0], [5, 0], [0, 1], [0, P - 1], [1, 1]]
    notes = ["register 65535", "register 65535", "read 65536", "read 65536", "write 65536", "write 65536", "read 65536 first"]
    return _case("registers", b, [1, 2], rows, notes, {5: "register 2"})


# ---- control flow
CONDITIONS = [0, 1, P - 1, U64, 2]
TARGETS = [3, 4, 5, U32 - 1, U32, U64 - 1]   # n - 1, n, n + 1, ... of the four-instruction programs below


@functools.lru_cache(maxsize=None)
def jump_case(kind):
    """One program per target: r1 = 5; <kind> to the target; r1 = 9; Stop. Register 0 is the condition (Jump and Call ignore it). A target past the
    end finishes the VM with r1 = 5. The three jumps are forward jumps: the planner inlines these programs, and both engines run them."""
    ops = []
    for i, t in enumerate(TARGETS):
        ins = (kind, t) if kind in ("Jump", "Call") else (kind, 0, t)
        ops.append(Brillig(inputs=[W(1)], outputs=[2 + 2 * i, 3 + 2 * i], bytecode=[("Const", 1, 5), ins, ("Const", 1, 9), ("Stop",)]))
    return _case(f"{kind} to every target", ops, [1], [[c] for c in CONDITIONS], [f"condition {c:#x}" for c in CONDITIONS])


@functools.lru_cache(maxsize=None)
def endings_case():
    """Opcode 0: Call is the last instruction, and its subroutine's Return lands on n. Opcode 1: the last instruction is no Stop. Opcode 2: more
    outputs than the bytecode names registers. Opcode 3: field Div by the input (x / 0 = 0)."""
    ops = [Brillig(inputs=[W(1)], outputs=[2, 3], bytecode=[("Jump", 3), ("Const", 1, 7), ("Return",), ("Call", 1)]),
           Brillig(inputs=[W(1)], outputs=[4, 5], bytecode=[("Const", 1, 3), ("BinaryFieldOp", 1, "Add", 0, 1)]),
           Brillig(inputs=[W(1)], outputs=[6, 7, 8, 9, 10, 11], bytecode=[("Mov", 1, 0), ("Const", 2, 4), ("Stop",)]),
           Brillig(inputs=[W(1), K(7)], outputs=[12, 13, 14], bytecode=[("BinaryFieldOp", 2, "Div", 1, 0), ("Stop",)])]
    vals = [0, 0, 1, 2, P - 1, U64]
    return _case("endings", ops, [1], [[v] for v in vals], [f"input {v:#x}" for v in vals])


@functools.lru_cache(maxsize=None)
def return_case():
    b = Brillig(inputs=[W(1)], outputs=[2], bytecode=[("JumpIf", 0, 2), ("Stop",), ("Return",)])
    return _case("return on an empty stack", b, [1], [[0], [1], [P - 1]], ["stops", "returns", "returns"])


@functools.lru_cache(maxsize=None)
def int_panic_case():
    """an integer operation that panics inside the VM (a loop keeps the program out of the inliner): the division by zero, the signed quotient past 2^bits"""
    b = Brillig(inputs=[W(1), W(2)], outputs=[3, 4], bytecode=[("BinaryIntOp", 0, "SignedDiv", 8, 0, 1), ("Const", 2, 0), ("JumpIf", 2, 0), ("BinaryIntOp", 1, "Shl", 8, 0, 1), ("Stop",)])
    rows = [[6, 3], [7, 0], [0, 0], [P - 1, 255], [250, 255], [1, 1 << 128]]
    return _case("integer panics", b, [1, 2], rows, ["6 / 3", "7 / 0", "0 / 0", "P - 1 over -1: past 2^8", "-6 / -1", "shift by 2^128"])


@functools.lru_cache(maxsize=None)
def empty_bytecode_case():
    b = Brillig(inputs=[W(1)], outputs=[2], bytecode=[])
    return _case("empty bytecode", b, [1], [[0], [1], [7]], ["panics"] * 3)


TRAP_DEPTHS = [0, 1, 2, 14, 15, 16, 17, 14, 17]


@functools.lru_cache(maxsize=None)
def trap_case():
    """r0 = depth: the program calls itself r0 times, from pc 5 at even remaining depths and from pc 7 at odd ones, then traps at pc 8: the error
    stack is the frames, oldest first, and 8. The result ABI keeps the first 15 frames and the 8."""
    b = Brillig(inputs=[W(1)], outputs=[2],
                bytecode=[("Const", 1, 1), ("JumpIfNot", 0, 8), ("BinaryIntOp", 0, "Sub", 64, 0, 1), ("BinaryIntOp", 2, "And", 1, 0, 1), ("JumpIf", 2, 7), ("Call", 1), ("Stop",),
                          ("Call", 1), ("Trap",)])
    return _case("trap at a call depth", b, [1], [[d] for d in TRAP_DEPTHS], [f"depth {d}" for d in TRAP_DEPTHS])


# ---- foreign-call results carried by the circuit
def vector_program(results):
    """Inputs: witnesses 1-3 an array (r0 = 0), 4 the pointer (r1), 5 and 6 two Load addresses (r2, r3). One ForeignCall into HeapVector(r1, size in r4),
    then r5 = mem[r2], r6 = mem[r3]. Outputs: witness 7 the size register, 8 and 9 the loaded cells, 10 the pointer register."""
    return Brillig(inputs=[[W(1), W(2), W(3)], W(4), W(5), W(6)], outputs=[7, 8, 9, 10], foreign_call_results=results,
                   bytecode=[("ForeignCall", "f", [("HeapVector", 1, 4)], [("Register", 1), ("HeapVector", 0, 4)]), ("Load", 5, 2), ("Load", 6, 3), ("Mov", 0, 4), ("Mov", 3, 1), ("Mov", 1, 5),
                             ("Mov", 2, 6), ("Stop",)])


def vector_rows(n, pointers=(0, 1, 2, 3, 4, 7)):
    """(pointer, load, load) around a vector of n values written to a memory of 3 cells"""
    rows, notes = [], []
    for ptr in pointers:
        end = max(3, ptr + n)  # the memory's length behind the write: a write of NO values grows it to ptr all the same
        for a, b in ((0, 2), (ptr, 3), (max(ptr - 1, 0), end - 1), (end - 1, end), (end, 0), (ptr + n, ptr), (min(3, end - 1), max(ptr - 2, 0)), (ptr + 4, 2), (ptr + 5, 0)):
            rows.append([21, 22, 23, ptr, a, b])
            notes.append(f"{n} values at {ptr}, loads at {a} and {b} of {end} cells")
    ic._pad(rows, notes, [1, 2, 3, 0, 0, 0])
    return rows, notes


@functools.lru_cache(maxsize=None)
def vector_case(n):
    rows, notes = vector_rows(n)
    return _case(f"foreign call, vector of {n}", vector_program([[list(range(31, 31 + n))]]), range(1, 7), rows, notes, {7: "the size register", 8: "first load", 9: "second load"})


@functools.lru_cache(maxsize=None)
def vector_size_is_pointer_case():
    """HeapVector(r1, r1): the size register is set FIRST, so the two values land at address 2 whatever the pointer was"""
    b = Brillig(inputs=[[W(1), W(2), W(3)], W(4)], outputs=[[5, 6, 7, 8], 9], foreign_call_results=[[[41, 42]]],
                bytecode=[("ForeignCall", "f", [("HeapVector", 1, 1)], []), ("Stop",)])
    return _case("foreign call, size register is the pointer", b, range(1, 5), [[1, 2, 3, p] for p in (0, 1, 3, 9, U64)], ["pointer %#x" % p for p in (0, 1, 3, 9, U64)])


def array_program(values, last):
    """Inputs: witnesses 1-2 an array (r0 = 0), 3 the pointer (r1). ForeignCall into [Register 2, HeapArray(r1, 2), Register 3], the last instruction or
    not. Outputs: the four cells from 0 (the pointer stays below 3), then r1, r2, r3."""
    return Brillig(inputs=[[W(1), W(2), K(0), K(0)], W(3)], outputs=[[4, 5, 6, 7], 8, 9, 10], foreign_call_results=[values],
                   bytecode=[("ForeignCall", "g", [("Register", 2), ("HeapArray", 1, 2), ("Register", 3)], [])] + ([] if last else [("Stop",)]))


ARRAY_SHAPES = collections.OrderedDict([
    ("sizes equal", [11, [12, 13], 14]), ("array too long", [11, [12, 13, 15], 14]), ("array too short", [11, [12], 14]), ("empty array", [11, [], 14]),
    ("fewer values", [11, [12, 13]]), ("one value", [11]), ("no values", []), ("more values", [11, [12, 13], 14, 15]), ("more values, wrong size", [11, [12], 14, [15]]),
    ("single where the array is due", [11, 12, 14]), ("array where the single is due", [[11], [12, 13], 14]), ("array where the last single is due", [11, [12, 13], [14]])])


@functools.lru_cache(maxsize=None)
def array_case(shape, last):
    rows = [[51, 52, p] for p in (0, 1, 2)]
    return _case(f"foreign call, {shape}, {'last' if last else 'in the middle'}", array_program(ARRAY_SHAPES[shape], last), [1, 2, 3], rows, [f"pointer {r[2]}" for r in rows])


@functools.lru_cache(maxsize=None)
def loop_case():
    """One ForeignCall instruction in a loop of r0 rounds; the circuit carries two results: three rounds wait, with the inputs of the third"""
    b = Brillig(inputs=[W(1)], outputs=[2, 3, 4], foreign_call_results=[[10], [20]],
                bytecode=[("Const", 4, 1), ("ForeignCall", "next", [("Register", 1)], [("Register", 0), ("Register", 2)]), ("BinaryFieldOp", 2, "Add", 2, 1),
                          ("BinaryIntOp", 0, "Sub", 64, 0, 4), ("JumpIf", 0, 1), ("Stop",)])
    return _case("foreign call in a loop", b, [1], [[1], [2], [3], [2], [1], [4]], ["%d rounds" % r for r in (1, 2, 3, 2, 1, 4)])


PENDING_ROWS = [(0, 3, "the whole memory"), (1, 2, "two cells"), (3, 0, "empty at the end"), (2, 0, "empty inside"), (0, 0, "empty at 0"), (3, 1, "one cell past the end"),
                (1, 3, "crosses the end"), (4, 0, "empty past the end"), (U64, 0, "pointer above u64"), (0, U64, "size above u64"), (U64 - 1, 2, "pointer + size past usize"), (2, 1, "the last cell")]


@functools.lru_cache(maxsize=None)
def pending_case():
    """No result at all: the opcode waits, and its inputs are a register, a HeapArray and a HeapVector(r1, r2) -- or the slice panics"""
    b = Brillig(inputs=[[W(1), W(2), W(3)], W(4), W(5)], outputs=[6],
                bytecode=[("ForeignCall", "ask", [("Register", 0)], [("Register", 1), ("HeapArray", 0, 2), ("HeapVector", 1, 2)]), ("Stop",)])
    return _case("foreign call, pending inputs", b, range(1, 6), [[61, 62, 63, p, n] for p, n, _ in PENDING_ROWS], [note for _, _, note in PENDING_ROWS])


@functools.lru_cache(maxsize=None)
def answered_case():
    """vector_program without a result: every row waits once and the host answers it (ANSWERS by row): an empty array, one element, five, each
    with the pointer below, at and past the memory's end"""
    rows, notes = [], []
    for answer in ANSWERS:  # the same 27 rows under each answer
        r, n = vector_rows(len(answer[0]), (1, 3, 7))
        rows, notes = rows + r[:27], notes + n[:27]
    return _case("foreign call, answered by the host", vector_program([]), range(1, 7), rows, notes)


ANSWERS = [[[]], [[71]], [[72, 73, 74, 75, 76]]]


def answer_of(j):
    return ANSWERS[j // 27]


def answered_expect(case):
    """the outcomes behind the host's answers"""
    return [model(case.circuit, case.ids, row, answers=[answer_of(j)]) for j, row in enumerate(case.rows)]


@functools.lru_cache(maxsize=None)
def answered_single_case():
    """the host answers a single into a register (and the wrong kind in every third row: a panic)"""
    b = Brillig(inputs=[W(1)], outputs=[2, 3], bytecode=[("ForeignCall", "one", [("Register", 1)], [("Register", 0)]), ("Stop",)])
    return _case("foreign call, a single answered by the host", b, [1], [[v] for v in (0, 1, 2, 3, P - 1)], ["input"] * 5)


# ---- black boxes
HASHES = ("Sha256", "Blake2s", "Keccak256")
CELLS = [0, 1, 255, 256, P - 1, 0x1234, 97, 98]


def hash_rows():
    """(message pointer, message length, digest pointer) on a memory of 8 cells"""
    rows, notes = [], []
    for mp, ml, note in ((0, 8, "the whole memory"), (0, 0, "empty at 0"), (8, 0, "empty at the end"), (9, 0, "empty past the end"), (5, 4, "one cell too many"), (2, 5, "inside"),
                         (0, U64, "length above u64"), (U64, 0, "pointer above u64")):
        for op in (0, 4, 8, 20, U64):
            rows.append(CELLS + [mp, ml, op])
            notes.append(f"message {note}, digest at {op:#x}")
    ic._pad(rows, notes, CELLS + [0, 1, 0])
    return rows, notes


@functools.lru_cache(maxsize=None)
def hash_case(name):
    """The digest of mem[r1 .. r1 + r2] to mem[r3 ..], then THE SAME message range hashed once more to mem[r3 + 32 ..] (where the first digest lies over
    the message, the second one hashes digest bytes), r0 = r3. Outputs: the 64 cells from r0."""
    b = Brillig(inputs=[[W(i) for i in range(1, 9)], W(9), W(10), W(11)], outputs=[list(range(12, 76))],
                bytecode=[("BlackBox", name, 1, 2, 3, 32), ("Const", 4, 32), ("BinaryFieldOp", 5, "Add", 3, 4), ("BlackBox", name, 1, 2, 5, 32), ("Mov", 0, 3), ("Stop",)])
    rows, notes = hash_rows()
    return _case(f"black box {name}", b, range(1, 12), rows, notes)


@functools.lru_cache(maxsize=None)
def hash_to_field_case():
    b = Brillig(inputs=[[W(i) for i in range(1, 9)], W(9), W(10), W(11)], outputs=[12, 13], bytecode=[("BlackBox", "HashToField128Security", 1, 2, 0), ("Mov", 1, 0), ("Stop",)])
    rows, notes = hash_rows()
    return _case("black box HashToField128Security", b, range(1, 12), rows, notes)


PEDERSEN_DOMAINS = [(0, "0"), (U32, "2^32: fails"), (1 << 128, "2^128: truncates to 0"), ((1 << 128) + U32, "2^128 + 2^32: truncates, fails"), (U32 + 5, "2^32 + 5: fails"),
                    (0, "0"), (P - 1, "P - 1: fails")]


@functools.lru_cache(maxsize=None)
def pedersen_case():
    """Pedersen of mem[0 .. 2] under the domain separator r1, the point to mem[r2 ..]; outputs: the two cells from r0 = r2"""
    b = Brillig(inputs=[[W(1), W(2)], W(3), W(4)], outputs=[[5, 6]],
                bytecode=[("Const", 3, 2), ("BlackBox", "Pedersen", 0, 3, 1, 2, 2), ("Mov", 0, 2), ("Stop",)])
    rows = [[7 + j, P - 1 - j, d, (0, 2, 5)[j % 3]] for j, (d, _) in enumerate(PEDERSEN_DOMAINS)]
    return _case("black box Pedersen", b, range(1, 5), rows, [n for _, n in PEDERSEN_DOMAINS])


ECDSA_SIZES = [("EcdsaSecp256k1", 0, 31), ("EcdsaSecp256k1", 0, 33), ("EcdsaSecp256r1", 1, 31), ("EcdsaSecp256r1", 1, 33), ("EcdsaSecp256k1", 2, 63), ("EcdsaSecp256r1", 2, 65),
                ("EcdsaSecp256r1", 0, 0), ("EcdsaSecp256k1", 1, 0)]


@functools.lru_cache(maxsize=None)
def ecdsa_size_case(name, group, size):
    """70 constant cells; public key x, public key y and signature all at r0, the literal size of one of them wrong. Where the memory holds the
    slices up to the wrong one, the VM fails with that array's text; where a slice in front of it does not fit, it panics first."""
    sizes = [32, 32, 64]
    sizes[group] = size
    b = Brillig(inputs=[W(1), [K(c % 251) for c in range(70)]], outputs=[2],
                bytecode=[("Const", 2, 32), ("Const", 3, 0), ("BlackBox", name, 3, 2, 0, sizes[0], 0, sizes[1], 0, sizes[2], 4), ("Stop",)])
    ptrs = [0, 70 - 65, 70 - 64, 70 - 63, 70 - 33, 70 - 32, 70 - 31, 70, 71, U64]
    return _case(f"black box {name}, array {group} of {size}", b, [1], [[p] for p in ptrs], [f"arrays at {p:#x} of 70 cells" for p in ptrs])


@functools.lru_cache(maxsize=None)
def ecdsa_verdict_case():
    """a valid secp256k1 signature in 160 constant cells (hash, x, y, signature); r0 shifts the hashed message's pointer: 0 verifies"""
    import ecdsa_ref
    import hashlib
    z = hashlib.sha256(b"brillig edges").digest()
    sk = 0x1F3C5A7E9B2D4F60718293A4B5C6D7E8F9010B1C2D3E4F5061728394A5B6C7D8
    x, y = ecdsa_ref.public_key(0, sk)
    r, s = ecdsa_ref.sign(0, sk, 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE, int.from_bytes(z, "big"))
    cells = z + x.to_bytes(32, "big") + y.to_bytes(32, "big") + r.to_bytes(32, "big") + s.to_bytes(32, "big")
    b = Brillig(inputs=[W(1), [K(c) for c in cells]], outputs=[2, 3],
                bytecode=[("Const", 2, 32), ("Const", 3, 32), ("Const", 4, 64), ("Const", 5, 96), ("BlackBox", "EcdsaSecp256k1", 0, 2, 3, 32, 4, 32, 5, 64, 1), ("Stop",)])
    return _case("black box EcdsaSecp256k1, verdicts", b, [1], [[0], [1], [0], [129], [U64]], ["verifies", "another hash", "verifies", "hash crosses the end", "pointer above u64"])


@functools.lru_cache(maxsize=None)
def schnorr_case():
    """Memory: signature over the empty message (64 cells), one more cell, signature over b"brillig" (64), the message (7). Inputs: the public key, then the
    message's pointer and length and the signature's pointer and length."""
    import grumpkin_ref
    ref = grumpkin_ref.ref()
    sk = 0x1F3C5A7E9B2D4F60718293A4B5C6D7E8F9010B1C2D3E4F5061728394A5B6C7D8 % grumpkin_ref.Q
    pk, sig0 = ref.schnorr_sign(sk, 0x0123456789ABCDEF, b"")
    _, sig1 = ref.schnorr_sign(sk, 0x0FEDCBA987654321, b"brillig")
    cells = sig0 + b"\x05" + sig1 + b"brillig"
    b = Brillig(inputs=[W(1), W(2), W(3), W(4), W(5), W(6), [K(c) for c in cells]], outputs=[7, 8, 9],
                bytecode=[("BlackBox", "SchnorrVerify", 0, 1, 2, 3, 4, 5, 2), ("Stop",)])
    n = len(cells)
    shapes = [(129, 0, 0, 64, "empty message, 64 cells: verifies"), (n, 0, 0, 65, "empty message at the end, 65 cells: verifies"), (0, 0, 0, 63, "63 cells: panics"),
              (129, 7, 65, 64, "message, 64 cells: verifies"), (129, 6, 65, 64, "message cut: rejects"), (129, 7, 65, 63, "63 cells: panics"), (129, 7, 64, 65, "signature shifted: rejects"),
              (129, 8, 65, 64, "message crosses the end: panics"), (129, 7, 65, n - 64, "signature crosses the end: panics"), (n + 1, 0, 0, 64, "empty message past the end: panics"),
              (129, 7, 65, 71, "71 cells: verifies")]
    rows = [[pk[0], pk[1], mp, ml, sp, sl] for mp, ml, sp, sl, _ in shapes]
    return _case("black box SchnorrVerify", b, range(1, 7), rows, [s[-1] for s in shapes], {9: "the verdict"})


@functools.lru_cache(maxsize=None)
def fixed_base_case():
    """low = r0, high = 0, the point to mem[r1 ..] of three cells; outputs: five cells from 0 where they exist"""
    b = Brillig(inputs=[W(1), W(2), [K(1), K(2), K(3)]], outputs=[3, 4, [5, 6, 7]], bytecode=[("Const", 3, 0), ("BlackBox", "FixedBaseScalarMul", 0, 3, 1, 2), ("Mov", 2, 3), ("Stop",)])
    rows = [[5, 0], [6, 1], [7, 2], [8, 3], [9, 7], [10, U64]]
    return _case("black box FixedBaseScalarMul", b, [1, 2], rows, [f"the point to {r[1]:#x} of 3 cells" for r in rows])


# ---- inputs, outputs, predicate
@functools.lru_cache(maxsize=None)
def inputs_case():
    """Opcode 0: an array, an EMPTY array (its register is the memory's length, 2), a single, an array right behind; outputs: the four registers and the three
    cells. Opcode 1: constant-only expressions. Opcode 2: an empty output array behind register 0 = witness 1 (2^70 in some rows: it is never converted),
    then a simple output. Opcode 3: one witness twice among the outputs (r0, then r1)."""
    ops = [Brillig(inputs=[[W(1), W(2)], [], W(3), [E([(1, 1, 2)], [(2, 3)], 5)]], outputs=[4, 5, 6, 7, [8, 9, 10]], bytecode=[("Const", 4, 0), ("Stop",)]),
           Brillig(inputs=[K(5), [K(6), K(P - 1)], E()], outputs=[11, 12, 13, [14, 15]], bytecode=[("Mov", 3, 1), ("Stop",)]),
           Brillig(inputs=[W(1), W(2)], outputs=[[], 16], bytecode=[("Stop",)]),
           Brillig(inputs=[W(2), W(3)], outputs=[17, 17], bytecode=[("Stop",)])]
    rows = [[5, 7, 7], [1 << 70, 3, 3], [P - 1, 0, 0], [1 << 70, 3, 4], [2, 9, 8], [U64, 1, 1], [0, 0, 0]]
    notes = ["equal", "2^70 in front of the empty output array", "P - 1", "2^70; the doubled output differs", "the doubled output differs", "2^64", "zeros"]
    return _case("inputs and outputs", ops, [1, 2, 3], rows, notes, {17: "the witness named twice"})


@functools.lru_cache(maxsize=None)
def inlined_conflict_case():
    """an inlinable program whose FIRST output is an input that differs in some rows: the reference stops there, and the second output stays unassigned"""
    b = Brillig(inputs=[W(1), W(2)], outputs=[3, 4], bytecode=[("BinaryFieldOp", 1, "Mul", 0, 1), ("Stop",)])
    rows = [[2, 3, 2], [2, 3, 5], [0, 9, 0], [P - 1, 2, 1], [7, 7, 7]]
    return _case("output conflict in an inlined program", b, [1, 2, 3], rows, ["equal", "differs", "equal", "differs", "equal"], {3: "the output that is an input"})


@functools.lru_cache(maxsize=None)
def unknown_cases():
    """witness 9 is never assigned: as a single input, inside an array, in the predicate"""
    out = []
    for name, b in (("unknown single input", Brillig(inputs=[W(1), W(9)], outputs=[2], bytecode=[("Stop",)])),
                    ("unknown inside an array", Brillig(inputs=[W(1), [W(1), W(9), W(1)]], outputs=[2], bytecode=[("Stop",)])),
                    ("unknown in the predicate", Brillig(inputs=[W(1)], outputs=[2], bytecode=[("Stop",)], predicate=E([], [(1, 1), (1, 9)], 0)))):
        out.append(_case(name, b, [1], [[0], [1], [P - 1]], ["input"] * 3))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def predicate_case():
    """Inputs: witness 1 the predicate, 2 and 3 an array and 3 again a single (r1), 4 ALREADY ASSIGNED and an output. Outputs: witnesses 5, 6 = the array,
    4 = r1, 7 = r2 = r1: a run needs witness 4 to equal witness 3, and with predicate 0 every output is zeroed and witness 4 must have been 0."""
    b = Brillig(inputs=[[W(2), W(3)], W(3)], outputs=[[5, 6], 4, 7], bytecode=[("Mov", 2, 1), ("Stop",)], predicate=W(1))
    rows = [[1, 8, 9, 9], [0, 8, 9, 0], [0, 8, 9, 9], [P - 1, 8, 9, 9], [P - 1, 8, 9, 0], [2, 1, 2, 3], [0, 0, 0, 0], [0, 1, 2, P - 1], [1, 3, 4, 4], [U64, 5, 6, 6]]
    notes = ["runs", "skipped", "skipped, conflicting output", "predicate P - 1", "predicate P - 1, conflicting output", "conflicting output", "skipped", "skipped, conflicting output", "runs",
             "predicate 2^64"]
    return _case("predicate", b, [1, 2, 3, 4], rows, notes, {4: "the output that is an input"})


CASE_BUILDERS = collections.OrderedDict()
for _name, _fn in ([("memory", memory_case), ("registers", registers_case)] + [(f"{k} to every target", functools.partial(jump_case, k)) for k in ("Jump", "JumpIf", "JumpIfNot", "Call")] +
                   [("endings", endings_case), ("return on an empty stack", return_case), ("empty bytecode", empty_bytecode_case), ("integer panics", int_panic_case), ("trap at a call depth", trap_case)] +
                   [(f"foreign call, vector of {n}", functools.partial(vector_case, n)) for n in (0, 1, 5)] +
                   [("foreign call, size register is the pointer", vector_size_is_pointer_case)] +
                   [(f"foreign call, {s}, {'last' if last else 'in the middle'}", functools.partial(array_case, s, last)) for s in ARRAY_SHAPES for last in (False, True)] +
                   [("foreign call in a loop", loop_case), ("foreign call, pending inputs", pending_case), ("foreign call, answered by the host", answered_case),
                    ("foreign call, a single answered by the host", answered_single_case)] +
                   [(f"black box {h}", functools.partial(hash_case, h)) for h in HASHES] + [("black box HashToField128Security", hash_to_field_case), ("black box Pedersen", pedersen_case)] +
                   [(f"black box {n}, array {g} of {s}", functools.partial(ecdsa_size_case, n, g, s)) for n, g, s in ECDSA_SIZES] +
                   [("black box EcdsaSecp256k1, verdicts", ecdsa_verdict_case), ("black box SchnorrVerify", schnorr_case), ("black box FixedBaseScalarMul", fixed_base_case),
                    ("inputs and outputs", inputs_case), ("output conflict in an inlined program", inlined_conflict_case), ("unknown single input", lambda: unknown_cases()[0]), ("unknown inside an array", lambda: unknown_cases()[1]),
                    ("unknown in the predicate", lambda: unknown_cases()[2]), ("predicate", predicate_case)]):
    CASE_BUILDERS[_name] = _fn
NAMES = list(CASE_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASE_BUILDERS[name]()
    assert c.name == name, (c.name, name)
    return c


def all_cases():
    return [case(n) for n in NAMES]


# ---- perturbed expectations: each must make compare() fail (tests/test_brillig_cases.py on the oracle, tests/test_gpu_brillig_edges.py on the device)
PERTURBATIONS = [("memory", "zero-filled cell"), ("predicate", "status"), ("inputs and outputs", "failing opcode"), ("trap at a call depth", "call-stack entry"),
                 ("foreign call, array too long, in the middle", "message"), ("foreign call, pending inputs", "pending input")]
DEVICE_PERTURBATIONS = [PERTURBATIONS[0], PERTURBATIONS[3], PERTURBATIONS[4], PERTURBATIONS[5]]


def perturbed(name, what):
    """(case, expectations with ONE row changed in one place, that row)"""
    c = case(name)
    expect = list(c.expect)
    if what == "zero-filled cell":  # a Load inside the gap that a Store past the end left behind
        j = next(j for j, x in enumerate(expect) if "write_gap_zero_fill" in x.branches and x.status == ST_SOLVED and x.witnesses[9] == 0 and c.rows[j][6] >= 4)
        expect[j] = expect[j]._replace(witnesses={**expect[j].witnesses, 9: 1})
    elif what == "status":
        j = next(j for j, x in enumerate(expect) if x.kind == br.UNSATISFIED)
        expect[j] = expect[j]._replace(status=ST_SOLVED, err=E_NONE)
    elif what == "failing opcode":
        j = next(j for j, x in enumerate(expect) if x.status == ST_FAILURE)
        expect[j] = expect[j]._replace(opcode_index=expect[j].opcode_index - 1)
    elif what == "call-stack entry":  # the 15th frame of a stack of 17: the last one the ABI keeps
        j = next(j for j, x in enumerate(expect) if x.call_stack and len(x.call_stack) == 18)
        stack = list(expect[j].call_stack)
        stack[14] = 12 - stack[14]
        expect[j] = expect[j]._replace(call_stack=stack)
    elif what == "message":
        j = 1
        expect[j] = expect[j]._replace(message=br.msg_fc_count(3, 3))
    elif what == "pending input":  # the empty vector at the memory's end becomes one cell
        j = next(j for j, x in enumerate(expect) if x.pending and "read_slice_empty_at_len" in x.branches)
        fn, inputs = expect[j].pending
        expect[j] = expect[j]._replace(pending=(fn, inputs[:2] + [[0]]))
    else:
        raise AssertionError(what)
    return c, expect, j
