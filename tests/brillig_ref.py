"""The Brillig VM and its ACVM glue in Python integers, restated from the reference's Rust alone: no oracle, no device and no product code here (the
curve black boxes come from tests/ecdsa_ref.py and tests/grumpkin_ref.py, the hashes from hashlib and tests/keccak_ref.py). tests/brillig_cases.py
builds the inputs, tests/test_brillig_cases.py runs them through the CPU oracle, tests/test_gpu_brillig_edges.py on the device.

run(brillig, wm) solves ONE Opcode::Brillig on the witness map wm (which it changes as the reference does, outputs inserted before a failure
included) and returns Outcome(kind, message, call_stack, function, inputs, labels):
  kind        SOLVED, UNSATISFIED, TOO_MANY_UNKNOWNS, MISSING_ASSIGNMENT, BRILLIG_FAILED, PANIC or REQUIRES_FOREIGN_CALL
  message     of BRILLIG_FAILED: the reference's text; a panic's text stays None (the oracle words panics itself)
  call_stack  of BRILLIG_FAILED: the WHOLE error stack, every frame and the failing pc last (abi_call_stack cuts it as the result ABI does)
  function, inputs  of REQUIRES_FOREIGN_CALL: ForeignCallWaitInfo
  labels      the set of branch labels the run passed through; LABELS lists every label a rule below can emit

The rules and where they stand:
  BrilligSolver::solve                acvm/src/pwg/brillig.rs:20-130 (predicate :28-37, inputs :40-74, outputs :95-111, failure :114-125, wait :126-128)
  zero_out_brillig_outputs            acvm/src/pwg/brillig.rs:133-150
  get_value / insert_value            acvm/src/pwg/mod.rs:321-357
  VM::process_opcodes / process_opcode    brillig_vm/src/lib.rs:136-307, fail :127-133, set_program_counter :322-329
  get_register_value_or_memory_values brillig_vm/src/lib.rs:331-349
  Registers                           brillig_vm/src/registers.rs:13-42 (65 536 registers, unset ones read 0)
  Memory                              brillig_vm/src/memory.rs:18-39
  Value::to_u128 / to_usize           brillig/src/value.rs:32-42, acir_field/src/generic_ark.rs:227-238
  field ALU                           brillig_vm/src/arithmetic.rs:7-20, acir_field/src/generic_ark.rs:240-245,375-381 (x / 0 = 0)
  integer ALU                         brillig_vm/src/arithmetic.rs:23-98 (int_cases.ref_int_op; Shl / Shr :70-79 here)
  black boxes                         brillig_vm/src/black_box.rs:10-165, blackbox_solver/src/lib.rs:17-99 (the error's Display)"""
import collections
import hashlib

from acvm_amd.acir import P, Expression
from keccak_ref import keccak256

(SOLVED, UNSATISFIED, TOO_MANY_UNKNOWNS, MISSING_ASSIGNMENT, BRILLIG_FAILED, PANIC, REQUIRES_FOREIGN_CALL) = KINDS = (
    "Solved", "Unsatisfied", "TooManyUnknowns", "MissingAssignment", "BrilligFunctionFailed", "Panic", "RequiresForeignCall")
Outcome = collections.namedtuple("Outcome", "kind message call_stack function inputs labels")

MAX_REGISTERS = 1 << 16           # registers.rs:13
ABI_CALL_STACK = 16               # entries of the result ABI (include/acvm_amd.h, oracle/binding.py Result.call_stack)

MSG_RETURN = "return opcode hit, but callstack already empty"                   # lib.rs:186
MSG_TRAP = "explicit trap hit in brillig"                                       # lib.rs:269
MSG_FC_SIZE = "Function result size does not match brillig bytecode"            # lib.rs:258


def msg_fc_count(n_values, n_destinations):                                     # lib.rs:255
    return f"{n_values} output values were provided as a foreign call result for {n_destinations} destination slots"


def msg_black_box(func, reason):                                                # blackbox_solver/src/lib.rs:19-20
    return f"failed to solve blackbox function: {func}, reason: {reason}"


MSG_PEDERSEN_DOMAIN = msg_black_box("pedersen", "Invalid signature length")     # black_box.rs:153-159 (the text is the reference's)
ECDSA_LENGTH_REASONS = ("Invalid public key x length", "Invalid public key y length", "Invalid signature length")  # black_box.rs:94-116
# every BrilligFunctionFailed text that brillig_vm itself words (the backend's own failures, wasm/mod.rs, are not the VM's)
MESSAGES = ([MSG_RETURN, MSG_TRAP, MSG_FC_SIZE, "<n> output values were provided as a foreign call result for <m> destination slots", MSG_PEDERSEN_DOMAIN] +
            [msg_black_box(f, r) for f in ("ecdsa_secp256k1", "ecdsa_secp256r1") for r in ECDSA_LENGTH_REASONS])


def message_class(message):
    """the entry of MESSAGES a failure's text belongs to"""
    return MESSAGES[3] if message.endswith("destination slots") else message


def abi_call_stack(call_stack):
    """ABI rule, not a VM rule: a result keeps 16 call-stack entries, the first 15 frames and the failing pc"""
    return list(call_stack[:-1][:ABI_CALL_STACK - 1]) + [call_stack[-1]]


# every branch label a rule below can emit (tests/test_brillig_cases.py: each is reached by at least two rows of tests/brillig_cases.py)
LABELS = (
    # glue
    "pred_zero_outputs_zeroed", "pred_zero_conflict", "pred_missing", "pred_nonzero", "input_single", "input_array", "input_array_empty", "input_unknown_single",
    "input_unknown_in_array", "out_simple", "out_array", "out_array_empty_no_conversion", "out_array_oob", "out_array_base_above_u64", "out_conflict",
    # registers
    "reg_unset_reads_zero", "reg_read_past_max", "reg_write_past_max", "reg_write_grows",
    # memory
    "load", "load_oob", "to_usize_above_u64", "write_in_place", "write_at_len", "write_gap_zero_fill", "write_zero_len_grows", "write_zero_len_no_growth",
    "read_slice", "read_slice_empty_at_len", "read_slice_empty_inside", "read_slice_oob",
    # control flow
    "bytecode_empty", "stop", "pc_increment_past_end", "pc_target_past_end", "jump", "jump_if_taken", "jump_if_not_taken", "jump_if_not_jumps", "jump_if_not_falls_through",
    "call", "return", "return_empty_stack", "trap", "fail_with_frames",
    # ALU
    "field_op", "field_div_by_zero", "int_op", "int_op_panic",
    # foreign calls
    "fc_wait", "fc_wait_register", "fc_wait_heap_array", "fc_wait_heap_vector", "fc_single_into_register", "fc_array_into_heap_array", "fc_array_into_heap_vector",
    "fc_array_size_mismatch", "fc_array_for_register_panics", "fc_single_for_array_panics", "fc_count_mismatch", "fc_failed", "fc_size_mismatch_then_finished",
    "fc_count_mismatch_then_finished", "fc_second_result",
    # black boxes
    "bb_sha256", "bb_blake2s", "bb_keccak256", "bb_hash_to_field", "bb_low_byte_of_wide_cell", "bb_pedersen", "bb_pedersen_domain_truncated", "bb_pedersen_domain_fails",
    "bb_ecdsa_length_fails", "bb_ecdsa_verdict", "bb_schnorr_verdict", "bb_schnorr_short_signature", "bb_fixed_base",
)


class _Panic(Exception):
    pass


def get_value(e, wm):
    """get_value (pwg/mod.rs:321-332): (value, None), or (None, a witness without a value). A term with coefficient 0 is no term."""
    acc = e.q_c
    for c, l, r in e.mul_terms:
        if c % P == 0:
            continue
        for w in (l, r):
            if w not in wm:
                return None, w
        acc += c * wm[l] * wm[r]
    for c, w in e.linear_combinations:
        if c % P == 0:
            continue
        if w not in wm:
            return None, w
        acc += c * wm[w]
    return acc % P, None


def insert_value(wm, w, v):
    """insert_value (pwg/mod.rs:338-357): the map takes the new value FIRST, then the displaced one is compared"""
    old = wm.get(w)
    wm[w] = v
    return old is None or old == v


class VM:
    def __init__(self, registers, memory, bytecode, results, labels):
        self.regs, self.mem, self.bytecode, self.results, self.labels = list(registers), list(memory), bytecode, results, labels
        self.pc = self.fc_counter = 0
        self.call_stack = []
        self.status = ("InProgress",)

    def hit(self, label):
        assert label in LABELS, label
        self.labels.add(label)

    def panic(self, label):
        self.hit(label)
        raise _Panic(label)

    # ---- registers.rs:25-42
    def get(self, r):
        if r >= MAX_REGISTERS:
            self.panic("reg_read_past_max")
        if r >= len(self.regs):
            self.hit("reg_unset_reads_zero")
            return 0
        return self.regs[r]

    def set(self, r, v):
        if r >= MAX_REGISTERS:
            self.panic("reg_write_past_max")
        if r >= len(self.regs):
            self.hit("reg_write_grows")
            self.regs.extend([0] * (r + 1 - len(self.regs)))
        self.regs[r] = v % P

    def to_usize(self, v):
        """value.rs:39-42"""
        if v >> 64:
            self.panic("to_usize_above_u64")
        return v

    # ---- memory.rs:18-39
    def read(self, ptr):
        if ptr >= len(self.mem):
            self.panic("load_oob")
        self.hit("load")
        return self.mem[ptr]

    def read_slice(self, ptr, n):
        if ptr + n > len(self.mem):  # (&inner[ptr..ptr + len]: start past the end, end past the end, or ptr + len past usize)
            self.panic("read_slice_oob")
        self.hit("read_slice" if n else "read_slice_empty_at_len" if ptr == len(self.mem) else "read_slice_empty_inside")
        return self.mem[ptr:ptr + n]

    def write_slice(self, ptr, values):
        old, n = len(self.mem), len(values)
        if n == 0:  # resize(max(len, ptr + 0)) grows all the same
            self.hit("write_zero_len_grows" if ptr > old else "write_zero_len_no_growth")
        else:
            self.hit("write_gap_zero_fill" if ptr > old else "write_at_len" if ptr + n > old else "write_in_place")
        assert ptr + n <= 1 << 20, "the model keeps writes small (the device limits are not its subject)"
        if ptr + n > old:
            self.mem.extend([0] * (ptr + n - old))
        self.mem[ptr:ptr + n] = [v % P for v in values]

    # ---- lib.rs:127-133, 322-329
    def fail(self, message):
        stack = [self.to_usize(v) for v in self.call_stack] + [self.pc]
        if self.call_stack:
            self.hit("fail_with_frames")
        self.status = ("Failure", message, stack)
        return self.status

    def set_pc(self, value, label):
        assert self.pc < len(self.bytecode)
        self.pc = value
        if self.pc >= len(self.bytecode):
            self.hit(label)
            self.status = ("Finished",)
        return self.status

    def increment_pc(self):
        return self.set_pc(self.pc + 1, "pc_increment_past_end")

    def resolve(self, x):
        """get_register_value_or_memory_values (lib.rs:331-349)"""
        if x[0] == "Register":
            self.hit("fc_wait_register")
            return [self.get(x[1])]
        start = self.get(x[1])
        if x[0] == "HeapArray":
            self.hit("fc_wait_heap_array")
            return self.read_slice(self.to_usize(start), x[2])
        self.hit("fc_wait_heap_vector")
        size = self.get(x[2])
        return self.read_slice(self.to_usize(start), self.to_usize(size))

    def process_opcode(self):
        if self.pc >= len(self.bytecode):  # (only an empty bytecode gets here: bytecode[0], lib.rs:155)
            self.panic("bytecode_empty")
        op = self.bytecode[self.pc]
        k = op[0]
        if k == "BinaryFieldOp":
            _, dst, name, lhs, rhs = op
            a, b = self.get(lhs), self.get(rhs)
            self.hit("field_op")
            if name == "Div" and b == 0:
                self.hit("field_div_by_zero")
            r = {"Add": a + b, "Sub": a - b, "Mul": a * b, "Div": a * (pow(b, -1, P) if b else 0), "Equals": int(a == b)}[name]
            self.set(dst, r)
            return self.increment_pc()
        if k == "BinaryIntOp":
            _, dst, name, bits, lhs, rhs = op
            a, b = self.get(lhs), self.get(rhs)
            r = int_op(name, a, b, bits)
            if r is None:
                self.panic("int_op_panic")
            self.hit("int_op")
            self.set(dst, r)
            return self.increment_pc()
        if k == "Jump":
            self.hit("jump")
            return self.set_pc(op[1], "pc_target_past_end")
        if k == "JumpIf":
            if self.get(op[1]) != 0:
                self.hit("jump_if_taken")
                return self.set_pc(op[2], "pc_target_past_end")
            self.hit("jump_if_not_taken")
            return self.increment_pc()
        if k == "JumpIfNot":
            if self.get(op[1]) == 0:
                self.hit("jump_if_not_jumps")
                return self.set_pc(op[2], "pc_target_past_end")
            self.hit("jump_if_not_falls_through")
            return self.increment_pc()
        if k == "Return":
            if self.call_stack:
                self.hit("return")
                return self.set_pc(self.to_usize(self.call_stack.pop()) + 1, "pc_target_past_end")
            self.hit("return_empty_stack")
            return self.fail(MSG_RETURN)
        if k == "ForeignCall":
            return self.foreign_call(*op[1:])
        if k == "Mov":
            self.set(op[1], self.get(op[2]))
            return self.increment_pc()
        if k == "Trap":
            self.hit("trap")
            return self.fail(MSG_TRAP)
        if k == "Stop":
            self.hit("stop")
            self.status = ("Finished",)
            return self.status
        if k == "Load":
            source = self.get(op[2])
            self.set(op[1], self.read(self.to_usize(source)))
            return self.increment_pc()
        if k == "Store":
            destination = self.to_usize(self.get(op[1]))
            self.write_slice(destination, [self.get(op[2])])
            return self.increment_pc()
        if k == "Call":
            self.hit("call")
            self.call_stack.append(self.pc)
            return self.set_pc(op[1], "pc_target_past_end")
        if k == "Const":
            self.set(op[1], op[2])
            return self.increment_pc()
        if k == "BlackBox":
            error = black_box(self, op[1], op[2:])
            return self.increment_pc() if error is None else self.fail(error)
        raise AssertionError(op)

    def foreign_call(self, function, destinations, inputs):
        """lib.rs:189-263"""
        if self.fc_counter >= len(self.results):
            self.hit("fc_wait")
            self.status = ("ForeignCallWait", function, [self.resolve(x) for x in inputs])
            return self.status
        if self.fc_counter:
            self.hit("fc_second_result")
        values = self.results[self.fc_counter]
        invalid = False
        for d, out in zip(destinations, values):
            is_array = not isinstance(out, int)
            if d[0] == "Register":
                if is_array:
                    self.panic("fc_array_for_register_panics")
                self.hit("fc_single_into_register")
                self.set(d[1], out)
                continue
            if not is_array:
                self.panic("fc_single_for_array_panics")
            if d[0] == "HeapArray":
                if len(out) != d[2]:
                    self.hit("fc_array_size_mismatch")
                    invalid = True
                    break
                self.hit("fc_array_into_heap_array")
            else:
                self.hit("fc_array_into_heap_vector")
                self.set(d[2], len(out))  # the size register FIRST: it may be the pointer register
            self.write_slice(self.to_usize(self.get(d[1])), list(out))
        # both fail() calls only record (the second one over the first); the counter advances all the same
        failed = None
        if len(destinations) != len(values):
            self.hit("fc_count_mismatch")
            self.fail(msg_fc_count(len(values), len(destinations)))
            failed = "fc_count_mismatch_then_finished"
        if invalid:
            self.fail(MSG_FC_SIZE)
            failed = "fc_size_mismatch_then_finished"
        self.fc_counter += 1
        status = self.increment_pc()
        if failed:
            self.hit(failed if status == ("Finished",) else "fc_failed")
        return status

    def process_opcodes(self):
        while self.process_opcode()[0] == "InProgress":
            pass
        return self.status


def int_op(name, a, b, bits):
    """evaluate_binary_bigint_op: None where the reference panics"""
    from int_cases import ref_int_op
    if name in ("Shl", "Shr"):  # arithmetic.rs:70-79
        if bits > 128 or b >> 128:
            return None
        assert b < 4096, "the model keeps shifts small"
        return ((a << b) if name == "Shl" else (a >> b)) % (1 << bits) % P
    return ref_int_op(name, a, b, bits)


def _low_bytes(vm, cells):
    """to_u8_vec (black_box.rs:28-36): the last big-endian byte of every value"""
    if any(v > 255 for v in cells):
        vm.hit("bb_low_byte_of_wide_cell")
    return bytes(v & 0xff for v in cells)


def _heap_vector(vm, pointer, size):
    return vm.read_slice(vm.to_usize(vm.get(pointer)), vm.to_usize(vm.get(size)))


def _heap_array(vm, pointer, size):
    return vm.read_slice(vm.to_usize(vm.get(pointer)), size)


def black_box(vm, name, w):
    """evaluate_black_box (black_box.rs:42-165): None, or the error's Display text"""
    if name in ("Sha256", "Blake2s", "Keccak256"):
        message = _low_bytes(vm, _heap_vector(vm, w[0], w[1]))
        vm.hit("bb_" + name.lower())
        digest = {"Sha256": lambda m: hashlib.sha256(m).digest(), "Blake2s": lambda m: hashlib.blake2s(m).digest(), "Keccak256": keccak256}[name](message)
        vm.write_slice(vm.to_usize(vm.get(w[2])), list(digest))  # (the array's declared size w[3] is never read)
        return None
    if name == "HashToField128Security":
        message = _low_bytes(vm, _heap_vector(vm, w[0], w[1]))
        vm.hit("bb_hash_to_field")
        vm.set(w[2], int.from_bytes(hashlib.blake2s(message).digest(), "big") % P)
        return None
    if name in ("EcdsaSecp256k1", "EcdsaSecp256r1"):
        import ecdsa_ref
        func = "ecdsa_secp256k1" if name == "EcdsaSecp256k1" else "ecdsa_secp256r1"
        parts = []
        for g, want in enumerate((32, 32, 64)):  # each array is READ (a slice panic) before its length is judged
            cells = _low_bytes(vm, _heap_array(vm, w[2 + 2 * g], w[3 + 2 * g]))
            if len(cells) != want:
                vm.hit("bb_ecdsa_length_fails")
                return msg_black_box(func, ECDSA_LENGTH_REASONS[g])
            parts.append(cells)
        hashed = _low_bytes(vm, _heap_vector(vm, w[0], w[1]))
        verdict = ecdsa_ref.verify(0 if name == "EcdsaSecp256k1" else 1, hashed, parts[0], parts[1], parts[2])
        assert verdict in (0, 1), "the model keeps ECDSA off its exceptional paths (tests/secp_cases.py has them)"
        vm.hit("bb_ecdsa_verdict")
        vm.set(w[8], verdict)
        return None
    if name == "SchnorrVerify":
        import grumpkin_ref
        pk = (vm.get(w[0]), vm.get(w[1]))
        message = _low_bytes(vm, _heap_vector(vm, w[2], w[3]))
        signature = _low_bytes(vm, _heap_vector(vm, w[4], w[5]))
        if len(signature) < 64:  # signature[0..32] / [32..64] (barretenberg_blackbox_solver/src/lib.rs:51-52); bytes past 64 are never read
            vm.panic("bb_schnorr_short_signature")
        vm.hit("bb_schnorr_verdict")
        vm.set(w[6], int(grumpkin_ref.ref().schnorr_verify(pk, signature[:64], message)))
        return None
    if name == "Pedersen":
        import grumpkin_ref
        inputs = _heap_vector(vm, w[0], w[1])
        domain = vm.get(w[2]) & ((1 << 128) - 1)  # to_u128: the low 128 bits
        if domain != vm.get(w[2]):
            vm.hit("bb_pedersen_domain_truncated")
        if domain >> 32:
            vm.hit("bb_pedersen_domain_fails")
            return MSG_PEDERSEN_DOMAIN
        assert inputs and domain == 0, "grumpkin_ref pins neither the empty commitment nor a hash index other than 0"
        vm.hit("bb_pedersen")
        vm.write_slice(vm.to_usize(vm.get(w[3])), list(grumpkin_ref.ref().pedersen(list(inputs), domain)))
        return None
    if name == "FixedBaseScalarMul":
        import grumpkin_ref
        low, high = vm.get(w[0]), vm.get(w[1])
        kind, point = grumpkin_ref.ref().fixed_base(low, high)
        assert kind == grumpkin_ref.FB_OK and point != (0, 0), "the model keeps the fixed base off its failures (tests/grumpkin_cases.py has them)"
        vm.hit("bb_fixed_base")
        vm.write_slice(vm.to_usize(vm.get(w[2])), list(point))
        return None
    raise AssertionError(name)


def run(brillig, wm, extra_results=()):
    """BrilligSolver::solve. extra_results: what the caller resolved so far (ACVM::resolve_pending_foreign_call, pwg/mod.rs:214-228, appends
    to the opcode's foreign_call_results and the opcode is solved again from its start)."""
    labels = set()

    def hit(label):
        assert label in LABELS, label
        labels.add(label)

    def out(kind, message=None, call_stack=None, function=None, inputs=None):
        return Outcome(kind, message, call_stack, function, inputs, frozenset(labels))

    pred = 1
    if brillig.predicate is not None:  # brillig.rs:28-31: the error of get_value passes through
        pred, missing = get_value(brillig.predicate, wm)
        if pred is None:
            hit("pred_missing")
            return out(MISSING_ASSIGNMENT)
    if pred == 0:  # brillig.rs:34-37, 133-150
        for o in brillig.outputs:
            for w in ([o] if isinstance(o, int) else o):
                if not insert_value(wm, w, 0):
                    hit("pred_zero_conflict")
                    return out(UNSATISFIED)
        hit("pred_zero_outputs_zeroed")
        return out(SOLVED)
    if brillig.predicate is not None:
        hit("pred_nonzero")
    registers, memory = [], []
    for i in brillig.inputs:  # brillig.rs:46-74
        if isinstance(i, Expression):
            v, _ = get_value(i, wm)
            if v is None:
                hit("input_unknown_single")
                return out(TOO_MANY_UNKNOWNS)
            hit("input_single")
            registers.append(v)
            continue
        pointer = len(memory)
        for e in i:
            v, _ = get_value(e, wm)
            if v is None:
                hit("input_unknown_in_array")
                return out(TOO_MANY_UNKNOWNS)
            memory.append(v)
        hit("input_array" if i else "input_array_empty")
        registers.append(pointer)
    vm = VM(registers, memory, brillig.bytecode, list(brillig.foreign_call_results) + list(extra_results), labels)
    try:
        status = vm.process_opcodes()
        if status[0] == "Finished":  # brillig.rs:95-111
            for i, o in enumerate(brillig.outputs):
                value = vm.get(i)
                if isinstance(o, int):
                    hit("out_simple")
                    if not insert_value(wm, o, value):
                        hit("out_conflict")
                        return out(UNSATISFIED)
                    continue
                if not o:
                    hit("out_array_empty_no_conversion")  # to_usize stands INSIDE the loop over the witnesses (:104-105)
                for k, w in enumerate(o):
                    if value >> 64:
                        vm.panic("out_array_base_above_u64")
                    if value + k >= len(vm.mem):
                        vm.panic("out_array_oob")
                    hit("out_array")
                    if not insert_value(wm, w, vm.mem[value + k]):
                        hit("out_conflict")
                        return out(UNSATISFIED)
            return out(SOLVED)
    except _Panic:
        return out(PANIC)
    if status[0] == "Failure":
        return out(BRILLIG_FAILED, status[1], status[2])
    assert status[0] == "ForeignCallWait"
    return out(REQUIRES_FOREIGN_CALL, function=status[1], inputs=[list(x) for x in status[2]])

