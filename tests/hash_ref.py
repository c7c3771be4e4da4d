"""The hash black boxes (SHA256, Blake2s, Keccak256, Keccak256VariableLength, HashToField128Security) and the solve loop around them in Python integers,
restated from the reference's Rust alone: no oracle, no device and no product code here. tests/hash_cases.py builds the inputs, tests/test_hash_cases.py
runs them through the CPU oracle, tests/test_gpu_hash_edges.py on the device.

run(circuit, witness map) solves the opcodes in program order and returns Expect(status, err, opcode_index, aux0, aux1, message, witnesses, branches): the
head as Result.as_tuple() carries it (aux0: the witness of MissingAssignment, the BlackBoxFunc of BlackBoxFunctionFailed), the text of a panic or of a
failed black box, the WHOLE witness map the reference leaves behind, and the set of branch labels the run passed through (LABELS lists every one).

The rules and where they stand:
  the pre-check of every black box          acvm/src/pwg/blackbox/mod.rs:55-62   the first unassigned witness in get_inputs_vec order
  get_inputs_vec                            acir/src/circuit/opcodes/black_box_function_call.rs:205-292  (inputs, then var_message_size)
  get_black_box_func                        :174-203   Keccak256VariableLength reports as Keccak256
  solve_hash_to_field                       acvm/src/pwg/blackbox/hash.rs:13-24
  solve_generic_256_hash_opcode             :28-48     the message and the digest are formed BEFORE the 32-output check
  get_hash_input                            :51-86     `num_bits as usize`; `to_u128() as usize`; `>` message_input.len()
  write_digest_to_outputs                   :89-103    stops at the first conflict (insert_value's `?`)
  FieldElement::fetch_nearest_bytes         acir_field/src/generic_ark.rs:305-317  bytes[0..(num_bits + 7) / 8] of the 32 little-endian bytes; the byte
                                                       count is a usize, so no width wraps: every width above 256 is core's slice panic
  FieldElement::to_u128                     :232-235   the low 128 bits
  from_be_bytes_reduce                      :281-283
  sha256, blake2s, keccak256, hash_to_field_128_security   blackbox_solver/src/lib.rs:47-65, 86-99
  insert_value                              acvm/src/pwg/mod.rs:338-357 (tests/arith_ref.py)

A Variant is the same model wrong in ONE way; tests/test_hash_cases.py uses them to prove that each list of tests/hash_cases.py would notice."""
import collections
import hashlib

import arith_ref
from acvm_amd.acir import P, Arithmetic, BlackBoxFuncCall, Expression
from arith_ref import (ST_SOLVED, ST_IN_PROGRESS, ST_FAILURE,  # noqa: F401  ACVMStatus and the error kinds as oracle/binding.py numbers them
                       E_NONE, E_MISSING_ASSIGNMENT, E_UNSATISFIED, E_PANIC, Fail as _Fail, insert_value)
from keccak_ref import keccak256

E_BLACKBOX_FAILED = 6
U64 = 1 << 64

# BlackBoxFuncCall tags (black_box_function_call.rs:20-115) as the error head reports them
FUNC_TAG = {"SHA256": 3, "Blake2s": 4, "HashToField128Security": 7, "Keccak256": 11, "Keccak256VariableLength": 11}
HASHES = tuple(FUNC_TAG)

Expect = collections.namedtuple("Expect", "status err opcode_index aux0 aux1 message witnesses branches")

LABELS = (
    # the pre-check
    "input_missing", "var_size_missing",
    # fetch_nearest_bytes
    "width_0", "width_byte", "width_2_to_31_bytes", "width_32_bytes", "width_panics", "width_panics_wrapping", "value_wider_than_width", "message_empty",
    # the variable length
    "var_size_cuts", "var_size_is_len", "var_size_too_large", "var_size_truncated_to_usize",
    # the functions
    "sha256", "blake2s", "keccak256", "hash_to_field", "hash_to_field_reduces",
    # the outputs
    "outputs_not_32", "output_new", "output_same", "output_conflict",
    # the opcodes around them
    "gate_solves", "range_passes", "range_fails",
)

# ways in which a Variant is wrong (each names the rule it breaks)
VARIANTS = ("width_rounded_down", "bytes_big_endian", "var_size_geq", "sha3_domain_byte", "digest_not_reduced", "outputs_past_conflict")


def msg_slice(end):
    """core::slice::index::slice_end_index_len_fail"""
    return b"range end index %d out of range for slice of length 32" % end


def msg_var_len(take, have):
    return b"the number of bytes to take from the message is more than the number of bytes in the message. %d > %d" % (take, have)


def msg_outputs(n):
    return b"Expected 32 outputs but encountered %d" % n


def sha3_256_padding_keccak(data):
    """Keccak-f[1600] with SHA-3's domain byte 0x06: what hashlib calls sha3_256 (the variant's mistake)"""
    return hashlib.sha3_256(bytes(data)).digest()


class Model:
    def __init__(self, variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.variant = variant
        self.messages = []  # per hash opcode that formed its message: (opcode, function name, the bytes hashed)
        self.at = 0

    def fetch_nearest_bytes(self, value, num_bits, hit):
        n = num_bits // 8 if self.variant == "width_rounded_down" else (num_bits + 7) // 8  # a usize: nothing wraps
        if n > 32:
            hit("width_panics_wrapping" if (num_bits + 7) % (1 << 32) // 8 <= 32 else "width_panics")
            raise _Fail(E_PANIC, message=msg_slice(n))
        hit("width_0" if n == 0 else "width_byte" if n == 1 else "width_32_bytes" if n == 32 else "width_2_to_31_bytes")
        if value >> (8 * n):
            hit("value_wider_than_width")
        le = value.to_bytes(32, "little")
        return (value.to_bytes(32, "big")[32 - n:] if self.variant == "bytes_big_endian" else le[:n])

    def hash_input(self, inputs, size, wm, hit):
        message = b""
        for f in inputs:
            message += self.fetch_nearest_bytes(wm[f.witness], f.num_bits, hit)  # (witness_to_value cannot fail behind the pre-check)
        if size is None:
            return message
        take = wm[size.witness] % (1 << 128) % U64  # to_u128() as usize
        if take != wm[size.witness]:
            hit("var_size_truncated_to_usize")
        if take > len(message) or (self.variant == "var_size_geq" and take == len(message)):
            hit("var_size_too_large")
            raise _Fail(E_BLACKBOX_FAILED, FUNC_TAG["Keccak256"], 0, msg_var_len(take, len(message)))
        hit("var_size_is_len" if take == len(message) else "var_size_cuts")
        return message[:take]

    def digest(self, name, message, hit):
        if name == "SHA256":
            hit("sha256")
            return hashlib.sha256(message).digest()
        if name in ("Blake2s", "HashToField128Security"):
            hit("blake2s")
            return hashlib.blake2s(message).digest()
        hit("keccak256")
        return sha3_256_padding_keccak(message) if self.variant == "sha3_domain_byte" else keccak256(message)

    def black_box(self, op, wm, hit):
        a = op.args
        size = a.get("var_message_size")
        for f in a["inputs"]:
            if f.witness not in wm:
                hit("input_missing")
                raise _Fail(E_MISSING_ASSIGNMENT, f.witness)
        if size is not None and size.witness not in wm:
            hit("var_size_missing")
            raise _Fail(E_MISSING_ASSIGNMENT, size.witness)
        message = self.hash_input(a["inputs"], size, wm, hit)
        if not message:
            hit("message_empty")
        self.messages.append((self.at, op.name, message))
        d = self.digest(op.name, message, hit)
        if op.name == "HashToField128Security":
            hit("hash_to_field")
            v = int.from_bytes(d, "big")
            if v >= P:
                hit("hash_to_field_reduces")
            self.insert(wm, a["output"], v if self.variant == "digest_not_reduced" else v % P, hit)
            return
        if len(a["outputs"]) != 32:
            hit("outputs_not_32")
            raise _Fail(E_BLACKBOX_FAILED, FUNC_TAG[op.name], 0, msg_outputs(len(a["outputs"])))
        failed = None
        for w, byte in zip(a["outputs"], d):
            try:
                self.insert(wm, w, byte, hit)
            except _Fail as f:
                if self.variant != "outputs_past_conflict":
                    raise
                failed = failed or f
        if failed:
            raise failed

    @staticmethod
    def insert(wm, w, v, hit):
        old = wm.get(w)
        try:
            insert_value(wm, w, v)
        except _Fail:
            hit("output_conflict")
            raise
        hit("output_new" if old is None else "output_same")

    def gate(self, e, wm, hit):
        seen = set()
        try:
            arith_ref.gate(e, wm, seen.add)
        finally:
            if "arm_solved_solvable_assigns" in seen:
                hit("gate_solves")

    def run(self, circ, wm, n_opcodes=None, snapshots=None):
        """ACVM::solve over the opcodes in program order on the map wm (which it changes); n_opcodes: stop after that many solve_opcode steps; snapshots:
        a list that takes, per step that succeeds, the (witness, value) pairs the step added"""
        branches = set()

        def hit(label):
            assert label in LABELS, label
            branches.add(label)

        def end(status, err=E_NONE, at=0, aux0=0, aux1=0, message=None):
            return Expect(status, err, at, aux0, aux1, message, wm, frozenset(branches))

        n_seen = len(wm)
        for oi, op in enumerate(circ.opcodes):
            if n_opcodes is not None and oi == n_opcodes:
                return end(ST_IN_PROGRESS, at=oi)
            self.at = oi
            try:
                if isinstance(op, (Arithmetic, Expression)):
                    self.gate(op.expr if isinstance(op, Arithmetic) else op, wm, hit)
                elif isinstance(op, BlackBoxFuncCall) and op.name == "RANGE":
                    arith_ref.range_check(op, wm, lambda l: hit(l) if l != "range_missing" else None)
                elif isinstance(op, BlackBoxFuncCall) and op.name in HASHES:
                    self.black_box(op, wm, hit)
                else:
                    raise AssertionError(f"no model for {op!r}")
            except _Fail as f:
                err, aux0, aux1, message = f.head
                return end(ST_FAILURE, err, oi, aux0, aux1, message)
            if snapshots is not None:
                snapshots.append([(w, wm[w]) for w in list(wm)[n_seen:]])
                n_seen = len(wm)
        return end(ST_SOLVED)


def run(circ, wm, n_opcodes=None, variant=None):
    return Model(variant).run(circ, dict(wm), n_opcodes)


def run_traced(circ, wm):
    """(Expect, the messages the run's hash opcodes formed)"""
    m = Model()
    return m.run(circ, dict(wm)), m.messages


def run_stepped(circ, wm):
    m, snaps = Model(), []
    return m.run(circ, dict(wm), snapshots=snaps), snaps
