// batch_messages.cpp -- what a solve says about an instance: results and message texts (OpcodeResolutionError, acvm/src/pwg/mod.rs:100-114), the
// assert messages of the circuit, the error string and expression of acvm_js/src/execute.rs:79-108.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "batch_internal.hpp"
#include "display.hpp"

// message text of a failure, rebuilt from the device's DevMsg code (ops_common.hpp) + payload
void format_message(acvm_batch *b, uint32_t j, const SlowResult &sr, acvm_result_t &r) {
    const Plan &p = b->plan();
    const uint32_t *rec = sr.opcode_index < p.n_opcodes ? &p.prog[p.prog_offset[sr.opcode_index]] : nullptr;
    char hx[65];
    // texts that two codes share: the device reports them from an opcode (12, 13, 26) and from inside the Brillig VM (16 with x0 = 100, 101, 111 ..)
    static const char *ecdsa_texts[7] = {"", "ecdsa: signature scalars must be in [1, n-1] (Signature::try_from unwrap)",
                                         "ecdsa: public key x is not on the curve (PublicKey::from_encoded_point unwrap)",
                                         "ecdsa: hashed message must be 32 bytes (GenericArray::from_slice)",
                                         "ecdsa: hashed message is not below the group order (Scalar::from_repr unwrap)",
                                         "ecdsa: R is the identity (unreachable!)", "ecdsa: R.x is not below the group order (Scalar::from_repr unwrap)"};
    static const char *overran = "Message overran wasm scratch space";
    auto slice_text = [&](uint32_t len) { snprintf(r.message, sizeof r.message, "range end index 64 out of range for slice of length %u", len); };
    switch (sr.msg) {
    case 1: snprintf(r.message, sizeof r.message, "Mul term in the arithmetic opcode must contain either zero or one term"); break;
    case 2: snprintf(r.message, sizeof r.message, "number of bits specified for each input must be the same"); break;
    // the slice panic of fetch_nearest_bytes (generic_ark.rs:316) on the first input wider than 256 bits: x0 is its num_bits, the end index its byte count as a usize
    case 3: snprintf(r.message, sizeof r.message, "range end index %llu out of range for slice of length 32", ((unsigned long long)sr.x0 + 7) / 8); break;
    case 4: snprintf(r.message, sizeof r.message, "Expected 32 outputs but encountered %u", sr.x0); break;
    case 5: {
        unsigned long long len = 0;
        if (rec && rec[0] == PK_HASH)
            for (uint32_t i = 0; i < rec[3]; i++) len += ((unsigned long long)rec[6 + 2 * i + 1] + 7) / 8;
        snprintf(r.message, sizeof r.message,
                 "the number of bytes to take from the message is more than the number of bytes in the message. %llu > %llu",
                 (unsigned long long)sr.x1 << 32 | sr.x0, len);
        break;
    }
    case 6: snprintf(r.message, sizeof r.message, "called `Option::unwrap()` on a `None` value (memory index)"); break;
    case 7: snprintf(r.message, sizeof r.message, "Memory must be read into a specified witness index, encountered an Expression"); break;
    case 8: snprintf(r.message, sizeof r.message, "The radix must be within 2...256"); break;
    case 9: case 10: case 11: {
        // the offending value: a witness of the FixedBaseScalarMul opcode, or the VM register value the device quoted
        const bool in_brillig = sr.err == ACVM_ERR_BRILLIG_FAILED;
        uint8_t val[32] = {0};
        if (in_brillig) {
            for (int i = 0; i < 32; i++) val[31 - i] = (uint8_t)(sr.val[i / 4] >> (8 * (i % 4)));
        } else if (rec && rec[0] == PK_FIXED_BASE) {
            if (sr.msg == 11) {
                uint8_t lo[32] = {0}, hi[32] = {0};
                fetch_one(b, j, rec[2], lo);
                fetch_one(b, j, rec[3], hi);
                memcpy(val, hi + 16, 16);
                memcpy(val + 16, lo + 16, 16);
            } else fetch_one(b, j, rec[sr.msg == 9 ? 2 : 3], val);
        }
        char reason[160];
        if (sr.msg == 11) {  // hex::encode(BigUint::to_bytes_be()) of high * 2^128 + low: minimal big-endian bytes
            int st = 0;
            while (st < 31 && val[st] == 0) st++;
            char hexs[65];
            for (int i = st; i < 32; i++) snprintf(hexs + 2 * (i - st), 3, "%02x", val[i]);
            snprintf(reason, sizeof reason, "Value %s is not a valid grumpkin scalar", hexs);
        } else {
            for (int i = 0; i < 32; i++) snprintf(hx + 2 * i, 3, "%02x", val[i]);
            snprintf(reason, sizeof reason, "Limb %s is not less than 2^128", hx);
        }
        if (in_brillig) snprintf(r.message, sizeof r.message, "failed to solve blackbox function: fixed_base_scalar_mul, reason: %s", reason);
        else snprintf(r.message, sizeof r.message, "%s", reason);
        break;
    }
    case 12: slice_text(sr.x0); break;
    case 13: snprintf(r.message, sizeof r.message, "%s", overran); break;
    case 14: snprintf(r.message, sizeof r.message, "explicit trap hit in brillig"); break;
    case 15: snprintf(r.message, sizeof r.message, "return opcode hit, but callstack already empty"); break;
    case 16: {
        static const char *texts[17] = {"", "Reading register past maximum!", "Writing register past maximum!", "register does not fit into u64",
                                        "memory read out of range", "", "bit_size > 256 is not supported", "attempt to subtract with overflow",
                                        "attempt to divide by zero", "unsupported bit size for right shift",
                                        "called `Option::unwrap()` on a `None` value", "bad int op", "index out of bounds: bytecode",
                                        "bad brillig opcode", "", "index out of bounds: brillig memory", "bad black box op"};
        if (sr.x0 == 100) slice_text(sr.x1);
        else if (sr.x0 == 101) snprintf(r.message, sizeof r.message, "%s", overran);
        else if (sr.x0 == 102) snprintf(r.message, sizeof r.message, "Function result size does not match brillig bytecode (expected 1 result)");
        else if (sr.x0 == 103) snprintf(r.message, sizeof r.message, "Function result size does not match brillig bytecode size");
        else if (sr.x0 > 110 && sr.x0 < 117) snprintf(r.message, sizeof r.message, "%s", ecdsa_texts[sr.x0 - 110]);
        else snprintf(r.message, sizeof r.message, "%s", sr.x0 < 17 ? texts[sr.x0] : "brillig vm panic");
        break;
    }
    // 17 / 18 / 28: device limits of the Brillig VM. retry_device_limits retries such lanes or ends them with ACVM_ERR_DEVICE_LIMIT (29); the texts are for debugging only
    case 17: snprintf(r.message, sizeof r.message, "brillig memory write at %u beyond the device capacity", sr.x0); break;
    case 18: snprintf(r.message, sizeof r.message, "brillig step limit reached on the device"); break;
    case 28: snprintf(r.message, sizeof r.message, "brillig call depth limit reached on the device"); break;
    case 19: {
        static const char *what[3] = {"Invalid public key x length", "Invalid public key y length", "Invalid signature length"};
        snprintf(r.message, sizeof r.message, "failed to solve blackbox function: %s, reason: %s", sr.x0 / 4 ? "ecdsa_secp256r1" : "ecdsa_secp256k1",
                 what[sr.x0 % 4 < 3 ? sr.x0 % 4 : 0]);
        break;
    }
    case 20: snprintf(r.message, sizeof r.message, "failed to solve blackbox function: pedersen, reason: Invalid signature length"); break;
    case 21: snprintf(r.message, sizeof r.message, "%u output values were provided as a foreign call result for %u destination slots", sr.x0, sr.val[0]); break;
    case 22: snprintf(r.message, sizeof r.message, "Function result size does not match brillig bytecode"); break;
    case 23: snprintf(r.message, sizeof r.message, "foreign call inputs exceed the device staging buffer"); break;
    case 25: {
        static const char *what[3] = {"pubkey_x", "pubkey_y", "signature"};
        snprintf(r.message, sizeof r.message, "expected %s size %u but received %u", what[sr.x0 < 3 ? sr.x0 : 0], sr.x0 == 2 ? 64u : 32u, sr.x1);
        break;
    }
    case 26: snprintf(r.message, sizeof r.message, "%s", sr.x0 < 7 ? ecdsa_texts[sr.x0] : ""); break;
    case 27: snprintf(r.message, sizeof r.message, "index out of bounds: the len is %u but the index is %u", sr.x0, sr.x1); break;
    case 29: {  // ACVM_ERR_DEVICE_LIMIT: not a reference outcome (include/acvm_amd.h)
        static const char *what[5] = {"", "VM steps", "nested calls", "cells of VM memory", "MiB of VM scratch on the device"};
        const uint32_t k = sr.aux0 < 5 ? sr.aux0 : 0;
        if (k == ACVM_LIMIT_BRILLIG_MEMORY)
            snprintf(r.message, sizeof r.message, "device limit: the Brillig program writes VM memory cell %u, beyond the %u cells this library runs it with; "
                                                  "the reference has no such limit: solve this instance with it", sr.x0, sr.aux1);
        else
            snprintf(r.message, sizeof r.message, "device limit: the Brillig program needs more than %u %s; the reference has no such limit: solve this "
                                                  "instance with it", sr.aux1, what[k]);
        break;
    }
    case 24: {
        auto it = b->host_bb_msg.find(j);
        if (it == b->host_bb_msg.end()) {  // (a callback made from inside a Brillig program: its text outlives the re-solve that reports it)
            it = b->fc_fail_msg.find(j);
            if (it == b->fc_fail_msg.end()) it = b->host_bb_msg.end();
        }
        snprintf(r.message, sizeof r.message, "%s", it == b->host_bb_msg.end() ? "" : it->second.c_str());
        break;
    }
    default: break;
    }
}

void result_head(const SlowResult &sr, acvm_result_t &r) {
    memset(&r, 0, sizeof r);
    r.status = sr.status; r.err = sr.err; r.opcode_index = sr.opcode_index; r.aux0 = sr.aux0; r.aux1 = sr.aux1;
    r.n_call_stack = sr.n_call_stack > 16 ? 16 : sr.n_call_stack;
    for (uint32_t k = 0; k < r.n_call_stack; k++) r.call_stack[k] = sr.call_stack[k];
}

void fill_result(acvm_batch *b, uint32_t j, acvm_result_t &r) {
    memset(&r, 0, sizeof r);
    if (b->plan().n_opcodes == 0 || b->slow_index[j] < 0) { r.status = ACVM_STATUS_SOLVED; return; }
    if (b->pending) { r.status = ACVM_STATUS_IN_PROGRESS; return; }  // its exact job is still running (batch_finish_pending)
    const SlowResult &sr = b->slow_res[b->slow_index[j]];
    result_head(sr, r);
    if (sr.status == ACVM_STATUS_FAILURE && sr.msg) format_message(b, j, sr, r);
}

int acvm_batch_results(acvm_batch_t *b, acvm_result_t *out) try {
    if (!b || !out) return set_err(ACVM_E_INVALID, "null argument");
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    HIPCHK(hipSetDevice(b->device));
    for (uint32_t j = 0; j < b->B; j++) fill_result(b, j, out[j]);
    return 0;
} ABI_CATCH

// ---------------------------------------------------------------------------------------------- after solve
int acvm_circuit_assert_message(const acvm_circuit_t *c, uint32_t acir_index, uint32_t brillig_index, char *out, size_t cap) {
    if (!c) return set_err(ACVM_E_INVALID, "null argument");
    const bool want_brillig = brillig_index != ACVM_LOCATION_ACIR;
    for (const AssertMessage &m : c->c->assert_messages) {  // first match, like the reference's linear find
        if (m.is_brillig != want_brillig || m.acir_index != acir_index || (want_brillig && m.brillig_index != brillig_index)) continue;
        if (out && cap) snprintf(out, cap, "%s", m.message.c_str());
        return (int)m.message.size();
    }
    if (out && cap) out[0] = 0;
    return -1;
}

// The expression OpcodeNotSolvable::ExpressionHasTooManyUnknowns carries for `instance` (pwg/mod.rs:72-78): the opcode partially evaluated
// on the instance's map for Opcode::Arithmetic (arithmetic.rs:31,38-42), the first input expression that does not reduce to a constant, as
// written, for Opcode::Brillig (brillig.rs:46-74, get_value pwg/mod.rs:321-332). Witnesses the instance has assigned are read back one by
// one, their rows of the assigned bitmap once each (rare path: one failing instance). false: the opcode carries no such expression.
static bool too_many_unknowns_expr(acvm_batch *b, const Circuit &circ, uint32_t instance, uint32_t opcode_index, Expr &out) {
    if (opcode_index >= circ.opcodes.size()) return false;
    AssignedView assigned = batch_assigned(b);  // (a failing copy of a row reads as "not assigned")
    auto known = [&](uint32_t w) { return assigned.assigned(instance, w); };
    auto value = [&](uint32_t w) {
        uint8_t be[32] = {0};
        fetch_one(b, instance, w, be);
        return frh::from_be_bytes32_reduce(be, 32);
    };
    // ArithmeticSolver::evaluate (arithmetic.rs:212-239)
    auto evaluate = [&](const Expr &e) {
        Expr r;
        for (const MulTerm &t : e.mul) {
            const bool kl = known(t.l), kr = known(t.r);
            if (kl && kr) r.qc = frh::add(r.qc, frh::mul(frh::mul(t.c, value(t.l)), value(t.r)));
            else if (!kl && !kr) { if (!t.c.is_zero()) r.mul.push_back(t); }
            else {
                const FrH v = frh::mul(t.c, value(kl ? t.l : t.r));
                if (!v.is_zero()) r.lin.push_back({v, kl ? t.r : t.l});
            }
        }
        for (const LinTerm &t : e.lin) {
            if (known(t.w)) r.qc = frh::add(r.qc, frh::mul(t.c, value(t.w)));
            else if (!t.c.is_zero()) r.lin.push_back(t);
        }
        r.qc = frh::add(r.qc, e.qc);
        return r;
    };
    const Opcode &o = circ.opcodes[opcode_index];
    if (o.kind == OP_ARITHMETIC) { out = evaluate(o.expr); return true; }
    if (o.kind == OP_BRILLIG) {  // the first input, in order, that does not reduce to a constant (get_value, pwg/mod.rs:321-332)
        auto stuck = [&](const Expr &e) { const Expr r = evaluate(e); return !r.mul.empty() || !r.lin.empty(); };
        for (const BrilligInput &in : o.brillig->inputs) {
            if (!in.is_array) { if (stuck(in.single)) { out = in.single; return true; } }
            else for (const Expr &e : in.arr) if (stuck(e)) { out = e; return true; }
        }
    }
    return false;
}
static std::string too_many_unknowns_expression(acvm_batch *b, const Circuit &circ, uint32_t instance, uint32_t opcode_index) {
    Expr e;
    return too_many_unknowns_expr(b, circ, instance, opcode_index, e) ? expression_display(e) : std::string();
}

int acvm_batch_error_expression(acvm_batch_t *b, const acvm_circuit_t *c, uint32_t instance, acvm_expression_t *head, uint8_t *mul_coef_be32,
                                uint32_t *mul_witnesses, uint32_t cap_mul, uint8_t *lin_coef_be32, uint32_t *lin_witnesses, uint32_t cap_lin) try {
    if (!b || !c || !head) return set_err(ACVM_E_INVALID, "null argument");
    memset(head, 0, sizeof *head);
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (instance >= b->B) return set_err(ACVM_E_INVALID, "instance out of range");
    HIPCHK(hipSetDevice(b->device));
    acvm_result_t r;
    fill_result(b, instance, r);
    if (r.status != ACVM_STATUS_FAILURE || r.err != ACVM_ERR_TOO_MANY_UNKNOWNS) return 0;
    Expr e;
    if (!too_many_unknowns_expr(b, *c->c, instance, r.opcode_index, e)) return 0;
    auto put_be = [](uint8_t *dst, const FrH &x) {
        uint64_t can[4];
        frh::to_canonical(x, can);
        for (int k = 0; k < 32; k++) dst[31 - k] = (uint8_t)(can[k / 8] >> (8 * (k % 8)));
    };
    head->n_mul = (uint32_t)e.mul.size();
    head->n_lin = (uint32_t)e.lin.size();
    head->opcode_index = r.opcode_index;
    put_be(head->q_c, e.qc);
    for (uint32_t i = 0; i < head->n_mul && i < cap_mul; i++) {
        if (mul_coef_be32) put_be(mul_coef_be32 + 32 * (size_t)i, e.mul[i].c);
        if (mul_witnesses) { mul_witnesses[2 * i] = e.mul[i].l; mul_witnesses[2 * i + 1] = e.mul[i].r; }
    }
    for (uint32_t i = 0; i < head->n_lin && i < cap_lin; i++) {
        if (lin_coef_be32) put_be(lin_coef_be32 + 32 * (size_t)i, e.lin[i].c);
        if (lin_witnesses) lin_witnesses[i] = e.lin[i].w;
    }
    return 1;
} ABI_CATCH

int acvm_batch_error_string(acvm_batch_t *b, const acvm_circuit_t *c, uint32_t instance, char *out, size_t cap) try {
    if (!b || !out || !cap) return set_err(ACVM_E_INVALID, "null argument");
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (instance >= b->B) return set_err(ACVM_E_INVALID, "instance out of range");
    HIPCHK(hipSetDevice(b->device));
    acvm_result_t r;
    fill_result(b, instance, r);
    out[0] = 0;
    if (r.status != ACVM_STATUS_FAILURE) return 0;
    static const char *bb_name[BB_COUNT] = {"and", "xor", "range", "sha256", "blake2s", "schnorr_verify", "pedersen", "hash_to_field_128_security",
                                           "ecdsa_secp256k1", "ecdsa_secp256r1", "fixed_base_scalar_mul", "keccak256", "keccak256",
                                           "recursive_aggregation"};
    const char *func = r.aux0 < BB_COUNT ? bb_name[r.aux0] : "?";
    char msg[512];
    int have = -1;
    if (c) {
        if (r.err == ACVM_ERR_UNSATISFIED || r.err == ACVM_ERR_INDEX_OOB)
            have = acvm_circuit_assert_message(c, r.opcode_index, ACVM_LOCATION_ACIR, msg, sizeof msg);
        else if (r.err == ACVM_ERR_BRILLIG_FAILED && r.n_call_stack)
            have = acvm_circuit_assert_message(c, r.opcode_index, r.call_stack[r.n_call_stack - 1], msg, sizeof msg);
    }
    if (have >= 0) return snprintf(out, cap, "Assertion failed: %s", msg);
    switch (r.err) {
    case ACVM_ERR_MISSING_ASSIGNMENT: return snprintf(out, cap, "Cannot solve opcode: missing assignment for witness index %u", r.aux0);
    case ACVM_ERR_TOO_MANY_UNKNOWNS: {
        // OpcodeNotSolvable::ExpressionHasTooManyUnknowns(Expression) (pwg/mod.rs:72-78): the text carries the expression -- the opcode
        // partially evaluated on the instance's map for Opcode::Arithmetic (arithmetic.rs:31,38-42), the input expression as written for
        // Opcode::Brillig (brillig.rs:46-74)
        const std::string e = c ? too_many_unknowns_expression(b, *c->c, instance, r.opcode_index) : std::string();
        return snprintf(out, cap, "Cannot solve opcode: expression has too many unknowns %s", e.c_str());
    }
    case ACVM_ERR_UNSUPPORTED_BLACKBOX:
        return snprintf(out, cap, "Backend does not currently support the %s opcode. ACVM does not currently have a fallback for this opcode.", func);
    case ACVM_ERR_UNSATISFIED: return snprintf(out, cap, "Cannot satisfy constraint");
    case ACVM_ERR_INDEX_OOB: return snprintf(out, cap, "Index out of bounds, array has size %u, but index was %u", r.aux1, r.aux0);
    case ACVM_ERR_BLACKBOX_FAILED: return snprintf(out, cap, "Failed to solve blackbox function: %s, reason: %s", func, r.message);
    case ACVM_ERR_BRILLIG_FAILED: return snprintf(out, cap, "Failed to solve brillig function, reason: %s", r.message);
    case ACVM_ERR_PANIC: return snprintf(out, cap, "panicked: %s", r.message);
    case ACVM_ERR_DEVICE_LIMIT: return snprintf(out, cap, "Not solved by this library (%s)", r.message);
    default: return snprintf(out, cap, "unknown error %u", r.err);
    }
} ABI_CATCH
