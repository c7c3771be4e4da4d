"""MemoryInit / MemoryOp and the solve loop around them in Python integers, restated from the reference's Rust alone: no oracle, no device and no product
code here (the Brillig opcodes of list G go through tests/brillig_ref.py). tests/mem_cases.py builds the inputs, tests/test_mem_cases.py runs them
through the CPU oracle, tests/test_gpu_mem_edges.py on the device.

run(circuit, witness map) solves the opcodes in program order and returns Expect(status, err, opcode_index, aux0, aux1, message, witnesses,
branches, pending): the head as Result.as_tuple() carries it (aux: index and array size of IndexOutOfBounds, the witness of MissingAssignment), the
panic text, the WHOLE witness map the reference leaves behind, the set of branch labels the run passed through (LABELS lists every one), and the pending
foreign call of a row that waits.

The rules and where they stand:
  the solve loop, block_solvers.entry(id).or_default()   acvm/src/pwg/mod.rs:243-303 (:252-259)
  MemoryOpSolver                                         acvm/src/pwg/memory_op.rs:16-124
      write_memory_index :22-36   index >= block_len is IndexOutOfBounds { index, array_size: block_len }, else the key is inserted
      read_memory_index  :38-44   KEY PRESENCE alone decides (block_value is a HashMap that init never clears); the error reports block_len
      init               :47-60   block_len = init.len() FIRST, then cell by cell: a missing witness stops it with the cells before it written
      solve_memory_op    :62-124  in this order: operation (get_value), index (get_value), try_to_u64().unwrap(), `as u32`, evaluate(value),
                                  predicate (get_value), then for a read to_witness().expect(..) BEFORE the zero-predicate test
  get_value, any_witness_from_expression                 acvm/src/pwg/mod.rs:321-332, 362-372
  insert_value, witness_to_value                         acvm/src/pwg/mod.rs:338-357, 309-317
  ArithmeticSolver::evaluate                             acvm/src/pwg/arithmetic.rs:212-239 (product terms first; a term whose coefficient is or becomes
                                                         zero is dropped; terms of one witness are NOT merged)
  ArithmeticSolver::solve                                acvm/src/pwg/arithmetic.rs:27-127, solve_mul_term :133-161, solve_fan_in_term :176-209
  Expression::to_witness, to_const                       acir/src/native_types/expression/mod.rs:148-172
  FieldElement::try_to_u64                               acir_field/src/generic_ark.rs:236-238 (num_bits() <= 64)
  RANGE                                                  acvm/src/pwg/blackbox/range.rs:7-18

A Variant is the same model wrong in ONE way; tests/test_mem_cases.py uses them to prove that each list of tests/mem_cases.py would notice."""
import collections

import arith_ref
import brillig_ref
from acvm_amd.acir import P, Arithmetic, BlackBoxFuncCall, Brillig, Expression, MemoryInit, MemoryOp
from arith_ref import (ST_SOLVED, ST_IN_PROGRESS, ST_FAILURE, ST_REQUIRES_FOREIGN_CALL,  # ACVMStatus and the error kinds as oracle/binding.py numbers them
                       E_NONE, E_MISSING_ASSIGNMENT, E_TOO_MANY_UNKNOWNS, E_UNSATISFIED, E_INDEX_OOB, E_BRILLIG_FAILED, E_PANIC,
                       Fail as _Fail, evaluate, insert_value)  # ArithmeticSolver::evaluate and insert_value are restated in tests/arith_ref.py

U32, U64 = 1 << 32, 1 << 64

# the texts of the two panics. The first is core's wording of Option::unwrap on None; the result ABI (oracle/pwg.c and the device alike) appends which
# unwrap it was. The second is the text of memory_op.rs:94-96.
MSG_INDEX = b"called `Option::unwrap()` on a `None` value (memory index)"
MSG_READ_TARGET = b"Memory must be read into a specified witness index, encountered an Expression"

Expect = collections.namedtuple("Expect", "status err opcode_index aux0 aux1 message witnesses branches pending")

LABELS = (
    # blocks
    "init", "init_empty", "init_again_shorter", "init_again_longer", "init_missing_witness", "block_default",
    # the checks of solve_memory_op, in the reference's order
    "operation_constant", "operation_dynamic", "operation_missing", "operation_other_than_0_1", "index_missing", "index_above_u64", "index_wraps_u32",
    "pred_absent", "pred_missing", "pred_zero", "pred_one", "pred_other",
    # reads
    "read", "read_stale_key", "read_oob", "read_pred_zero", "read_pred_zero_oob_index", "read_target_syntactic", "read_target_after_evaluation",
    "read_target_not_witness", "read_target_not_witness_pred_zero",
    # writes
    "write", "write_oob", "write_stale_key_oob", "write_pred_zero", "write_pred_zero_unknown_value", "write_missing_value",
    # the opcodes around them
    "gate_solves", "gate_satisfied", "gate_unsatisfied", "range_passes", "range_fails", "brillig",
)

# ways in which a Variant is wrong (each names the rule it breaks). replay_style leaves out the insert of every static read, so it moves almost every row;
# dynamic_read_writes_back is the narrow form of the same mistake: everything is right but that a read under an operation that is no constant also
# stores what it read (0 under a zero predicate) into the cell -- what a careless replay of memory side effects would do.
VARIANTS = ("readable_is_len", "pred_counts_only_as_one", "index_not_wrapped", "pred_before_to_witness", "replay_style", "dynamic_read_writes_back")


class Block:
    """MemoryOpSolver: block_value (keys are never removed), block_len"""

    def __init__(self):
        self.cells, self.len = {}, 0


def get_value(e, wm):
    """get_value: the constant, or MissingAssignment(any_witness_from_expression of the EVALUATED expression)"""
    mul, lin, qc = evaluate(e, wm)
    if mul or lin:
        raise _Fail(E_MISSING_ASSIGNMENT, lin[0][1] if lin else mul[0][1])
    return qc


def to_witness(ev):
    mul, lin, qc = ev
    return lin[0][1] if not mul and len(lin) == 1 and lin[0][0] == 1 and qc == 0 else None


def is_constant(e):
    return not e.mul_terms and not e.linear_combinations


class Model:
    def __init__(self, variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.variant = variant
        # per MemoryOp that got as far as its index: (opcode, is a read, the index before `as u32`, the predicate -- "absent" where the opcode has
        # none, None where the index panicked before the predicate was looked at)
        self.trace = []
        self.at = 0
        self.snapshots = None  # a list: takes, per solve_opcode step that succeeds, the (witness, value) pairs the step added to the map

    # ---- memory_op.rs
    def write_index(self, b, index, value, hit):
        if index >= b.len:
            hit("write_stale_key_oob" if index in b.cells else "write_oob")
            raise _Fail(E_INDEX_OOB, index % U32, b.len)
        b.cells[index] = value

    def read_index(self, b, index, hit):
        if self.variant == "readable_is_len":
            if index < b.len:
                return b.cells.get(index, 0)
            raise _Fail(E_INDEX_OOB, index % U32, b.len)
        if index not in b.cells:
            hit("read_oob")
            raise _Fail(E_INDEX_OOB, index % U32, b.len)
        if index >= b.len:
            hit("read_stale_key")
        return b.cells[index]

    def init(self, b, op, wm, hit, fresh):
        if not fresh:
            hit("init_again_shorter" if len(op.init) < b.len else "init_again_longer")
        hit("init" if op.init else "init_empty")
        b.len = len(op.init)
        for i, w in enumerate(op.init):
            if w not in wm:
                hit("init_missing_witness")
                raise _Fail(E_MISSING_ASSIGNMENT, w)
            self.write_index(b, i, wm[w], hit)

    def memory_op(self, b, op, wm, hit):
        replay = self.variant == "replay_style"
        try:
            operation = get_value(op.operation, wm)
        except _Fail:
            hit("operation_missing")
            raise
        hit("operation_constant" if is_constant(op.operation) else "operation_dynamic")
        if operation > 1:
            hit("operation_other_than_0_1")
        try:
            index = get_value(op.index, wm)
        except _Fail:
            hit("index_missing")
            raise
        is_read = operation == 0
        if index >= U64:  # try_to_u64().unwrap()
            self.trace.append((self.at, is_read, index, None))
            hit("index_above_u64")
            raise _Fail(E_PANIC, message=MSG_INDEX)
        if index >= U32:
            hit("index_wraps_u32")
        raw_index = index
        if self.variant != "index_not_wrapped":
            index %= U32  # `as MemoryIndex`
        value = evaluate(op.value, wm)
        if replay:  # what a replay of side effects does: a static read is nothing, an op whose operation is no constant is a write
            if is_constant(op.operation) and is_read:
                return
            is_read = False
        if op.predicate is None:
            hit("pred_absent")
            pred = 1
        else:
            try:
                pred = get_value(op.predicate, wm)
            except _Fail:
                hit("pred_missing")
                raise
            hit("pred_zero" if pred == 0 else "pred_one" if pred == 1 else "pred_other")
            if self.variant == "pred_counts_only_as_one" and pred != 1:
                pred = 0
        self.trace.append((self.at, is_read, raw_index, "absent" if op.predicate is None else pred))
        if is_read:
            if self.variant == "pred_before_to_witness" and pred == 0:
                w = to_witness(value)
                if w is not None:
                    insert_value(wm, w, 0)
                return
            w = to_witness(value)
            if w is None:
                hit("read_target_not_witness_pred_zero" if pred == 0 else "read_target_not_witness")
                raise _Fail(E_PANIC, message=MSG_READ_TARGET)
            hit("read_target_syntactic" if (not op.value.mul_terms and len(op.value.linear_combinations) == 1) else "read_target_after_evaluation")
            if pred == 0:
                hit("read_pred_zero_oob_index" if index not in b.cells else "read_pred_zero")
                got = 0
            else:
                got = self.read_index(b, index, hit)
                hit("read")
            insert_value(wm, w, got)
            if self.variant == "dynamic_read_writes_back" and not is_constant(op.operation):
                b.cells[index] = got  # a replay that takes the opcode for a write of its target and looks at neither predicate nor length
            return
        mul, lin, qc = value
        if pred == 0:
            hit("write_pred_zero_unknown_value" if mul or lin else "write_pred_zero")
            return
        if mul or lin:  # get_value(&value_write)
            hit("write_missing_value")
            raise _Fail(E_MISSING_ASSIGNMENT, lin[0][1] if lin else mul[0][1])
        self.write_index(b, index, qc, hit)
        hit("write")

    # ---- the opcodes around them
    def gate(self, e, wm, hit):
        """ArithmeticSolver::solve (tests/arith_ref.py gate); the arms the memory lists reach, under this model's labels"""
        seen = set()
        try:
            arith_ref.gate(e, wm, seen.add)
        finally:
            for arm, label in (("arm_solved_solvable_assigns", "gate_solves"), ("arm_solved_satisfied_ok", "gate_satisfied"), ("arm_solved_satisfied_unsatisfied", "gate_unsatisfied")):
                if arm in seen:
                    hit(label)

    def range(self, op, wm, hit):
        f = op.args["input"]
        if f.witness not in wm:
            raise _Fail(E_MISSING_ASSIGNMENT, f.witness)
        if wm[f.witness].bit_length() > f.num_bits:
            hit("range_fails")
            raise _Fail(E_UNSATISFIED)
        hit("range_passes")

    def run(self, circ, wm, n_opcodes=None, answers=()):
        """ACVM::solve over the opcodes in program order on the map wm (which it changes); n_opcodes: stop after that many solve_opcode steps (a row
        that has not ended by then is InProgress and reports the opcode it stands on); answers: what the host resolved so far for the Brillig opcode
        that waits (the opcode is solved again from its start with them appended)"""
        blocks, branches = {}, set()

        def hit(label):
            assert label in LABELS, label
            branches.add(label)

        def end(status, err=E_NONE, at=0, aux0=0, aux1=0, message=None, pending=None):
            return Expect(status, err, at, aux0, aux1, message, wm, frozenset(branches), pending)

        ops = circ.opcodes
        n_seen = len(wm)
        for oi, op in enumerate(ops):
            if n_opcodes is not None and oi == n_opcodes:
                return end(ST_IN_PROGRESS, at=oi)
            self.at = oi
            try:
                if isinstance(op, (MemoryInit, MemoryOp)):
                    fresh = op.block_id not in blocks
                    b = blocks.setdefault(op.block_id, Block())  # entry(id).or_default()
                    if isinstance(op, MemoryInit):
                        self.init(b, op, wm, hit, fresh)
                    else:
                        if fresh:
                            hit("block_default")
                        self.memory_op(b, op, wm, hit)
                elif isinstance(op, (Arithmetic, Expression)):
                    self.gate(op.expr if isinstance(op, Arithmetic) else op, wm, hit)
                elif isinstance(op, BlackBoxFuncCall) and op.name == "RANGE":
                    self.range(op, wm, hit)
                elif isinstance(op, Brillig):
                    hit("brillig")
                    out = brillig_ref.run(op, wm, answers)
                    if out.kind == brillig_ref.REQUIRES_FOREIGN_CALL:
                        return end(ST_REQUIRES_FOREIGN_CALL, at=oi, pending=(out.function, out.inputs))
                    assert out.kind == brillig_ref.SOLVED, out
                else:
                    raise AssertionError(f"no model for {op!r}")
            except _Fail as f:
                err, aux0, aux1, message = f.head
                return end(ST_FAILURE, err, oi, aux0, aux1, message)
            if self.snapshots is not None:
                self.snapshots.append([(w, wm[w]) for w in list(wm)[n_seen:]])
                n_seen = len(wm)
        return end(ST_SOLVED)


def run(circ, wm, n_opcodes=None, answers=(), variant=None):
    return Model(variant).run(circ, dict(wm), n_opcodes, answers)


def run_stepped(circ, wm):
    """(Expect, per opcode that succeeded the (witness, value) pairs it added: a step that succeeds never changes a value the map already holds)"""
    m = Model()
    m.snapshots = []
    return m.run(circ, dict(wm)), m.snapshots


def run_traced(circ, wm):
    """(Expect, the trace of the MemoryOps the run reached)"""
    m = Model()
    return m.run(circ, dict(wm)), m.trace
