/*
 * acvm_amd.h -- C ABI of the MI355X-native batched ACIR witness solver (libacvm_amd.so).
 *
 * This header is the drop-in boundary for ONE hot path of noir-lang/acvm v0.27.0:
 * `acvm::pwg::ACVM::solve()` and what it calls, for B independent witness instances of one circuit.
 * Plain pointers and sizes only; no torch / HIP types. Every entry point cites the reference
 * interface it replaces (paths relative to the acvm repository root).
 *
 *   reference                                               this ABI
 *   ------------------------------------------------------  -------------------------------------------
 *   acir::circuit::Circuit::read   circuit/mod.rs:154-161    acvm_circuit_from_bytes
 *   ACVM::new(backend, opcodes, initial_witness)
 *                         acvm/src/pwg/mod.rs:146-156        acvm_batch_new + acvm_batch_set_initial_witness
 *   ACVM::solve           acvm/src/pwg/mod.rs:236-241        acvm_batch_solve
 *   ACVMStatus / OpcodeResolutionError  mod.rs:33-51,100-114 acvm_result_t via acvm_batch_results
 *   ACVM::witness_map / finalize        mod.rs:161,176-181   acvm_batch_witness_map / acvm_batch_witness
 *   ACVM::instruction_pointer           mod.rs:171           acvm_result_t.opcode_index
 *   ACVM::get_pending_foreign_call      mod.rs:203-209       acvm_batch_pending_foreign_call*
 *   ACVM::resolve_pending_foreign_call  mod.rs:214-228       acvm_batch_resolve_foreign_call
 *   trait BlackBoxFunctionSolver  blackbox_solver/src/lib.rs:27-45   acvm_bb_solver_t (vtable)
 *
 * Threading (reference: `&mut self`, backend not Sync): one batch handle = one host thread + one HIP
 * device + one stream set. Handles are independent, also on one device; the only process-wide state is read-mostly
 * (the tuning table; the per-device lookup tables, built once under a per-device lock and reference-counted by the handles).
 * acvm_node_* drives one handle per device.
 * Errors: functions return 0 on success or a negative ACVM_E_* code; acvm_last_error() gives text.
 * The library requires a gfx950 device for every compute entry point and fails loudly without one;
 * there is no CPU fallback.
 */
#ifndef ACVM_AMD_H
#define ACVM_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACVM_AMD_ABI_VERSION 6

/* library-level error codes */
enum {
    ACVM_OK = 0,
    ACVM_E_INVALID = -1,     /* bad argument / handle */
    ACVM_E_MALFORMED = -2,   /* circuit bytes do not decode (the reference would panic in bincode::deserialize) */
    ACVM_E_UNSUPPORTED = -3, /* opcode outside the accelerated set -- refused at batch creation (an instance whose Brillig program
                                exceeds the device's VM limits is a per-instance outcome, ACVM_ERR_DEVICE_LIMIT, not a failed call) */
    ACVM_E_DEVICE = -4,      /* no gfx950 device / HIP runtime error */
    ACVM_E_STATE = -5,       /* call not valid in the current state (reference: panic) */
    ACVM_E_NOMEM = -6        /* host allocation failed (nothing unwinds through this ABI) */
};

/* ACVMStatus (acvm/src/pwg/mod.rs:33-51) */
enum { ACVM_STATUS_SOLVED = 0, ACVM_STATUS_IN_PROGRESS = 1, ACVM_STATUS_FAILURE = 2, ACVM_STATUS_REQUIRES_FOREIGN_CALL = 3 };

/* OpcodeResolutionError (mod.rs:100-114) with OpcodeNotSolvable (mod.rs:72-78) flattened */
enum {
    ACVM_ERR_NONE = 0,
    ACVM_ERR_MISSING_ASSIGNMENT = 1,   /* aux0 = witness index */
    ACVM_ERR_TOO_MANY_UNKNOWNS = 2,    /* OpcodeNotSolvable::ExpressionHasTooManyUnknowns */
    ACVM_ERR_UNSUPPORTED_BLACKBOX = 3, /* aux0 = BlackBoxFunc tag */
    ACVM_ERR_UNSATISFIED = 4,          /* UnsatisfiedConstrain{Resolved(Acir(opcode_index))} */
    ACVM_ERR_INDEX_OOB = 5,            /* IndexOutOfBounds{index = aux0, array_size = aux1} */
    ACVM_ERR_BLACKBOX_FAILED = 6,      /* BlackBoxFunctionFailed(func = aux0, message) */
    ACVM_ERR_BRILLIG_FAILED = 7,       /* BrilligFunctionFailed{message, call_stack} */
    ACVM_ERR_PANIC = 8,                /* the reference would panic at this opcode (message) */
    /* NOT a reference outcome. The reference's Brillig VM has no resource limits (brillig_vm/src/memory.rs:27-39, lib.rs:154-307); the device
     * runs a program with limits, raises them on the exact path, and past the stated maxima of the library (acvm_tuning_set: brillig_steps_max_log2,
     * brillig_call_depth_max, brillig_mem_max_log2) or of the device's memory THIS INSTANCE ends here: status Failure at its Brillig opcode,
     * aux0 = ACVM_LIMIT_* (what was reached), aux1 = the limit. With brillig_resume = 1 a lane is continued at a limit instead of started over,
     * brillig_steps_max_log2 bounds one pass only, and the step limit that ends an instance is the total 2^brillig_steps_total_log2
     * (aux1 = min(that, 2^32 - 1)): below a total the caller chooses, ACVM_LIMIT_BRILLIG_STEPS is not reached. It says "this library could not finish the instance", not "the circuit is
     * unsatisfied": re-run the instance with the reference (or with raised maxima). Every other instance of the batch keeps its result, as the
     * reference's caller loop loses one instance at most (acvm_js/src/execute.rs:60-119). */
    ACVM_ERR_DEVICE_LIMIT = 9
};
enum { ACVM_LIMIT_BRILLIG_STEPS = 1, ACVM_LIMIT_BRILLIG_CALL_DEPTH = 2, ACVM_LIMIT_BRILLIG_MEMORY = 3 /* cells of 32 bytes */,
       ACVM_LIMIT_DEVICE_MEMORY = 4 /* MiB of VM scratch the device could not provide */ };

/* Per-instance outcome. Same layout and numbering as the CPU oracle's result record. */
typedef struct {
    uint32_t status;       /* ACVM_STATUS_* */
    uint32_t err;          /* ACVM_ERR_* when status == FAILURE */
    uint32_t opcode_index; /* instruction pointer of the failing opcode (ACVM::instruction_pointer) */
    uint32_t aux0, aux1;
    uint32_t n_call_stack;
    uint32_t call_stack[16]; /* Brillig indices for BrilligFunctionFailed */
    char message[200];
} acvm_result_t;

/*
 * BlackBoxFunctionSolver (blackbox_solver/src/lib.rs:27-45) as a vtable. Field elements cross as 32-byte
 * canonical big-endian. Return 0 = Ok, 1 = BlackBoxResolutionError::Failed(err text), 2 = Unsupported, 3 = the
 * implementation panicked (err text; the instance fails with ACVM_ERR_PANIC -- what StubbedBackend does).
 * A NULL solver selects the built-in HIP implementation of barretenberg's three functions.
 *
 * The *_batch members are optional (NULL = call the per-instance function n times): one call serves the n instances of a
 * batch that reach the opcode. Arrays are instance-major host memory; rc[i] uses the return codes above, err is
 * [n][err_stride] NUL-terminated texts. They are what a backend that is itself batched (a GPU backend, a thread pool)
 * implements; the library gathers all instances once, makes ONE call per opcode and scatters the results once.
 *
 * The solver is the Brillig VM's solver too, as in the reference (brillig_vm/src/lib.rs:61,81,298; black_box.rs:139-163): a Brillig
 * program's BlackBoxOp::{SchnorrVerify, Pedersen, FixedBaseScalarMul} reach the same table (ABI 5; refused before). Inside
 * acvm_batch_solve / acvm_batch_solve_opcode every instance that stands at such an op is answered in one pass (one *_batch call per call
 * shape) and the opcode re-runs its VM with the answers; a callback's failure fails the VM at the op with BlackBoxResolutionError's Display
 * string. The caller never sees these round trips. ACVM_BATCH_REUSE_SLOTS takes a solver for the ACIR-level black boxes; a solver inside
 * Brillig is refused there with every other foreign call.
 */
typedef struct {
    void *ctx;
    int (*schnorr_verify)(void *ctx, const uint8_t pkx[32], const uint8_t pky[32], const uint8_t *sig, size_t sig_len,
                          const uint8_t *msg, size_t msg_len, uint8_t *ok, char *err, size_t err_len);
    int (*pedersen)(void *ctx, const uint8_t *inputs_be32, size_t n_inputs, uint32_t domain_separator, uint8_t x[32],
                    uint8_t y[32], char *err, size_t err_len);
    int (*fixed_base_scalar_mul)(void *ctx, const uint8_t low[32], const uint8_t high[32], uint8_t x[32], uint8_t y[32],
                                 char *err, size_t err_len);
    /* pk_be32 [n][2][32], sig [n][sig_len], msg [n][msg_len], ok [n] */
    int (*schnorr_verify_batch)(void *ctx, size_t n, const uint8_t *pk_be32, const uint8_t *sig, size_t sig_len, const uint8_t *msg,
                                size_t msg_len, uint8_t *ok, uint8_t *rc, char *err, size_t err_stride);
    /* inputs_be32 [n][n_inputs][32], xy_be32 [n][2][32] */
    int (*pedersen_batch)(void *ctx, size_t n, const uint8_t *inputs_be32, size_t n_inputs, uint32_t domain_separator, uint8_t *xy_be32,
                          uint8_t *rc, char *err, size_t err_stride);
    /* low_high_be32 [n][2][32], xy_be32 [n][2][32] */
    int (*fixed_base_scalar_mul_batch)(void *ctx, size_t n, const uint8_t *low_high_be32, uint8_t *xy_be32, uint8_t *rc, char *err,
                                       size_t err_stride);
} acvm_bb_solver_t;

/* The two fakes of the reference's own tests as ready-made vtables (static storage, never freed):
 *   acvm_bb_stubbed  StubbedBackend       acvm/tests/solver.rs:20-46      every function panics "Path not trodden by this test"
 *   acvm_bb_dummy    DummyBlackBoxSolver  brillig_vm/src/lib.rs:392-420   schnorr_verify = true, pedersen = (2, 3), fixed_base = (4, 5) */
const acvm_bb_solver_t *acvm_bb_stubbed(void);
const acvm_bb_solver_t *acvm_bb_dummy(void);

typedef struct acvm_circuit acvm_circuit_t;
typedef struct acvm_batch acvm_batch_t;

/* Statistics of the static plan and of the last solve (measurement). */
typedef struct {
    uint32_t n_opcodes, n_witnesses, n_levels, n_fast_gates, n_dyn_gates;
    uint32_t max_level_width, n_kernel_launches, n_slow_instances;
    uint64_t algorithmic_bytes_per_instance; /* sum over gates of 32 B x (distinct known operands + written witness) */
    uint64_t arith_algorithmic_bytes_per_instance; /* the part moved by arith_level_kernel */
    double plan_ms;         /* one-time levelisation, host */
    double solve_device_ms; /* HIP events around the whole last solve, on the batch's stream */
    double arith_kernel_ms; /* sum of HIP-event durations of the arithmetic level kernels of the last solve */
    double slow_path_ms;
    double dyn_kernel_ms;   /* same for the batched denominator inversions (inverse_batch_kernel, beside the former on a 2nd stream) */
    uint64_t dyn_algorithmic_bytes_per_instance;
    /* non-arithmetic opcodes, by kernel class: 0 light (range / logic / directives / memory), 1 hashes, 2 Grumpkin, 3 Brillig */
    uint32_t n_other_records;
    uint32_t truncated_at; /* first opcode the generic instance cannot execute (all instances take the exact kernels from there), or 0xFFFFFFFF */
    uint64_t class_algorithmic_bytes_per_instance[4];
    double class_kernel_ms[4]; /* summed HIP-event durations of the class's level kernels of the last solve (profiling on) */
    uint32_t n_gate_pairs;     /* arithmetic gates that run in their producer's wave and take its output from registers */
    uint32_t n_inverse_slots;  /* rows of the inverse table (denominators of the n_dyn_gates gates, rows reused) */
    uint32_t n_scaled_witnesses; /* witnesses the level kernels keep as scale x value (unscaled on export and for the exact path) */
    uint32_t n_arith_launches; /* launches of arith_level_kernel per solve (levels that hold gates) */
    uint32_t n_table_rows;     /* rows of the device witness table: n_witnesses, or fewer with ACVM_BATCH_REUSE_SLOTS */
    uint32_t n_digest_segments; /* records of leaves of the folded digest (ACVM_BATCH_FOLD_DIGEST), 0 if the digest is not folded */
    uint32_t n_brillig_inlined; /* Brillig opcodes whose straight-line program the level schedule runs as a light record (no VM) */
    uint32_t n_brillig_retries; /* passes of the last solve that re-ran Brillig opcodes of the exact path with raised VM limits */
    uint32_t n_hash_chained;   /* byte-message hashes that run in the workgroup of the hash whose digest they consume (no launch of their own) */
    /* relaxed rows (ABI 5): SOLVE gates that store their result as the column scan left it (any representative below 2^256) / after one
     * quotient-estimate reduction (below 1.03 p) / canonical; the largest bound a gate's result reaches, in units of p / 256 */
    uint32_t n_gate_out_asis, n_gate_out_weak, n_gate_out_canon, max_gate_bound;
    /* byte planes (ABI 5): initial witnesses that byte-message hashes read carry a 4-byte copy per instance (low limb + is-byte flag) written by the
     * import; n_byte_plane_reads inputs of hash records read it in place of the 32-byte row. The algorithmic-byte figures above keep the reference's
     * unit (32 bytes per witness read): what the hash kernel itself moves is 28 bytes less per such input, what the import moves 4 bytes more per plane. */
    uint32_t n_byte_planes, n_byte_plane_reads;
    /* ABI 6: launches of the level schedule by stream (main, inversions, the three heavy lanes, the digest lane) and the cross-stream waits of one solve */
    uint32_t n_stream_launches[6], n_stream_waits;
} acvm_stats_t;

const char *acvm_last_error(void);
int acvm_abi_version(void);
int acvm_device_count(void);
int acvm_set_device(int device);
int acvm_device_synchronize(void);
/* name of the current device's gcnArch ("gfx950...") into out */
int acvm_device_arch(char *out, size_t out_len);
/*
 * The per-device lookup tables (Grumpkin: 3 MB of fixed-base and Pedersen slice tables, 268 MB of 16-bit windows, the 503 MB pair table
 * or the 23.6 GB window table of the level Pedersen kernel; ECDSA: 2 x 64 MiB of generator windows) are built on the device at the first
 * handle whose circuit needs them -- under a lock of that device only, on a stream of their own -- and shared by every later handle of the
 * device. They stay until this call: frees the tables of `device` and returns the bytes given back, or ACVM_E_STATE while a handle of
 * that device still uses them (free the handles first). The next handle that needs a table rebuilds it (0.3 s for the largest).
 * acvm_tuning_set("tables_keep", 0) makes the destruction of a device's last handle release them without this call.
 * The reference keeps its counterpart -- the wasm instance with barretenberg's tables -- for the lifetime of the solver object
 * (barretenberg_blackbox_solver/src/wasm/mod.rs:59-82).
 */
long long acvm_device_release_tables(int device);

/*
 * Planner / scheduler modes and the device's Brillig VM limits, process-wide (csrc/tuning.hpp lists every key with its default;
 * acvm_tuning_key(i) enumerates them, NULL past the end). A batch keeps the values it was created with. No mode changes a result --
 * the parity tests sweep them against the oracle; the defaults are the measured optimum. The limits: the reference's Brillig VM has
 * none (brillig_vm/src/memory.rs:27-39 grows memory on write, lib.rs:154-307 runs any number of steps at any call depth); the device
 * runs with brillig_steps_log2 / brillig_call_depth / the planner's memory estimate, retries an instance that reaches one with the
 * limit raised, and past brillig_steps_max_log2 / brillig_call_depth_max / brillig_mem_max_log2 that instance ends with
 * ACVM_ERR_DEVICE_LIMIT (the others keep their results). brillig_resume = 1 (default 0) continues such an instance from a checkpoint instead of
 * running its opcode again: brillig_steps_max_log2 is then the most steps of ONE pass, and brillig_steps_total_log2 (default 32, 0..62) the most
 * steps of one run of an opcode over all its passes. Command-line tools may preset values through the environment: ACVM_TUNING="key=value,key=value".
 */
int acvm_tuning_set(const char *key, long long value);
int acvm_tuning_get(const char *key, long long *value);
const char *acvm_tuning_key(unsigned index);

/* Device self test of the field library: n pseudo-random operand pairs; returns the number of lanes whose
 * hand-scheduled routines disagree with the portable ones (0 = pass), or a negative error. */
int acvm_selftest(uint32_t n, uint64_t seed);

/* Component probes of the Grumpkin kernels (parity tests of barretenberg's building blocks against SURVEY Appendix A):
 * what 0 = host table point (param = table << 24 | index; tables: 0 Pedersen k*D[i] at i*512+k-1, 1 8-bit windows,
 * 2 ladder k*D[3j+1], 3 skew D[3j+2]); 1 = device hash_single(in[0], parity param); 2 = device hash-ladder
 * compress(in[0..n_in)), 3 = device fixed-base product (window table param, 256-bit integer in[0]); 4 = device table point;
 * 8 / 9 = in[0] * (in[1], in[2]) for a 256-bit integer and an affine point: 8 through SchnorrVerify's GLV + window-table path, 9 by double-and-add.
 * in: n_in x 32 bytes big-endian; out: 64 bytes (x || y) big-endian. */
int acvm_debug_grumpkin(uint32_t what, uint32_t param, const uint8_t *in_be32, uint32_t n_in, uint8_t *out_be64);
/* One routine of the Grumpkin device header per call, ONE DEVICE LANE PER ITEM, raw u32 words in and out (tests/test_gpu_grumpkin_edges.py compares with
 * Python integers). Field elements of what 0..3 are the nine 29-bit limbs of the lazy working form (the Montgomery residue v 2^261 mod p or that plus p:
 * the caller picks the representative, values below 2p) and leave as the limbs the routine returned; integers are 8 x u32, little-endian, canonical.
 * what (words in -> out per item): 0 X Y Z -> gj_dbl (27 -> 27); 1 X Y Z x2 y2 -> gj_add_aff29, then zr = Z3 / Z1, zero limbs off the ordinary path
 * (45 -> 36); 2 two Jacobian points -> gj_add (54 -> 27); 3 X Y Z -> gj_to_aff: x, y in the storage form, the infinity flag (27 -> 17); 4 k < q ->
 * glv_split: |k1|, |k2| (4 words each), neg1, neg2, then the 26 + 26 digits of signed_windows5, magnitude | 32 if negative (8 -> 62); 5 v < p ->
 * ladder_term(v, param), param = 0..2: canonical x, y, the infinity flag (8 -> 17); 6 / 7 pkx pky s e -> R = e pk + s G as SchnorrVerify forms it
 * (s, e reduced mod q first): canonical x, y, the infinity flag, 6 with a per-lane window table the probe allocates, 7 without one, the Brillig
 * VM's path (32 -> 17). ACVM_E_INVALID for another `what`, a ladder position above 2 or more than 2^20 items; nothing is launched for n_items = 0. */
int acvm_debug_grumpkin_items(uint32_t what, uint32_t param, const uint32_t *in_words, uint32_t n_items, uint32_t *out_words);
/* Read-back of the lookup tables of the Grumpkin and ECDSA kernels, entry by entry (tests/test_gpu_curve_tables.py compares every word with integers).
 * table: 0 ped [30][512], 1 win [4][32][255], 2 small [3][15], 3 skew [3], 4 ped2 [30][512][512], 5 win16 [4][16][65535], 6 pedw [2][11][2^24],
 * 7 / 8 the generator table [16][65536] of secp256k1 / secp256r1 (definitions and storage forms: acvm_amd/csrc/grumpkin_host.hpp). An entry is one affine
 * point of 16 u32: x limbs 0..7, y limbs 0..7, little-endian.
 * acvm_debug_table_info: the number of entries, and whether the current device holds the table right now (builds nothing; 0 without a device).
 * acvm_debug_table_read: builds the table on the current device if it is missing -- with the functions a batch handle builds it with, under the same
 * conditions (pedw: its 23.6 GB plus a quarter of the device's memory free; win16: tuning win16 set when the device's first Grumpkin table is built) --
 * and copies the RAW 16 words of entries[0..n) to out_words16, one device lane per entry, without arithmetic or change of form. ACVM_E_INVALID for an
 * unknown table or an index at or beyond the number of entries (checked on the host, nothing is launched); ACVM_E_DEVICE with the table's name when it
 * cannot be built. */
int acvm_debug_table_info(uint32_t table, uint64_t *n_entries, int *built);
int acvm_debug_table_read(uint32_t table, const uint64_t *entries, uint32_t n, uint32_t *out_words16);
/* Which device-built tables the kernels of this handle read: bit 0 ped2, bit 1 win16, bit 2 pedw, bit 3 the ECDSA generator tables (the level Pedersen
 * kernel reads pedw when the handle has it and ped2 otherwise: never both bits). Reads the handle's device program; changes nothing. */
int acvm_debug_batch_tables(const acvm_batch_t *b, uint32_t *mask);
/* Component probes of the ECDSA kernels (secp_device.hpp run ON THE DEVICE against integers: k256 / p256 are the spec of blackbox_solver/src/lib.rs:66-210,
 * the tests compare with Python): curve 0 = secp256k1, 1 = secp256r1; one device lane per item. what: 0 a b -> a b; 1 a -> a^2; 2 a b -> a + b; 3 a b -> a - b;
 * 4 a -> 1 / a (0 for 0); 5 a -> a^((p + 1) / 4), all mod p; 6 X Y Z -> the Jacobian double; 7 X Y Z x y -> the Jacobian sum with the affine point (x, y);
 * compositions the formulas are made of: 8 a -> a^4 (a product fed to a product); 9 a b -> (a + b)^2 (an unreduced sum into a product); 10 a b -> a - 4 b
 * (a difference against a multiple of p); 11 a -> a^32 (the squaring loop of the square-root chains);
 * what a verification is made of above the base field: 12 a b -> a b mod n; 13 a -> 1 / a mod n (0 for 0); 14 k -> |k1|, neg1, |k2|, neg2 of secp256k1's
 * endomorphism split (curve 0 only: ACVM_E_INVALID for curve 1); 15 u1 qx qy u2 -> X Y Z of u1 G + u2 (qx, qy) (Jacobian, Z = 0 for the identity; Q affine and
 * canonical); 16 r s x y n_msg z -> result, panic code of the whole verification with public_key_y = y, as the opcodes call it. 15 and 16 read the device's
 * own generator tables (the ones the handles of this device read; built on first use, ACVM_E_DEVICE when they cannot be).
 * in: n_items x (2, 1, 2, 2, 1, 1, 3, 5, 1, 2, 2, 1, 2, 1, 1, 4, 6) x 32 bytes big-endian, values < p (12..16: any 256-bit value the routine takes);
 * out: n_items x (1, 1, 1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 1, 1, 4, 3, 2) x 32 bytes. */
int acvm_debug_secp(uint32_t curve, uint32_t what, const uint8_t *in_be32, uint32_t n_items, uint8_t *out_be32);
/* Component probe of the BN254-Fr field library (acvm_amd/csrc/fr_device.hpp and the byte helpers of ops_common.hpp run ON THE DEVICE against integers:
 * the tests compare every word with Python, tests/fr_ref.py): one device lane per item, RAW limbs in and out -- S = the storage form, 8 x u32 little-endian,
 * W = the 29-bit working form, 9 x u32, k = one u32; nothing is converted or reduced on the way, so unreduced representatives go in and the routine's own
 * result comes out. what (acvm_amd/csrc/fr_probe.hpp): 0 fr_mul S S -> S; 1 fr_mul_portable S S -> S; 2 fr_sqr S -> S; 3 fr_add, 4 fr_sub S S -> S; 5 fr_neg,
 * 6 fr_inv, 7 fr_inv_eea, 8 fr_to_canonical S -> S; 9 fr_low_limb S -> k limb, k is_byte; 10 fr_is_byte S -> k is_byte, k byte; 11 fr_from_byte k -> S;
 * 12 fr29_from S -> W; 13 fr29_pack W -> S; 14 fr29_mul, 15 fr29_mul_b W W -> W; 16 fr29_sqr W -> W; 17 fr29_redc_low W -> k; 18 fr29_cond_sub_p W -> W;
 * 19 fr29_csub W k -> W (k = log2 of the multiple of p, 0..4); 20 fr29_lt2p, 21 fr29_weak, 22 fr29_canon, 23 fr29_norm W -> W; 24 fr29_subl W W k -> W
 * (k = 1..4); 25 fr29_addl W W -> W; 26 fr29_dbll W -> W; 27 fr29_is_zero_mod_p W -> k; 28 / 29 / 30 fr29_dot<1 / 2 / 3> (W a_t, W b_t) x N -> W;
 * 31 / 32 fr29_dot_add<1 / 2> (W a_t, W b_t) x N, W h -> W; 33 fr29_dot_add_b<1, 0> as 31; 34 fr29_dot_add_b<2, 0> as 32; 35 fr29_dot_add_b<1, 1>
 * W a0, W h -> a0 u0 + h; 36 fr29_dot_add_b<2, 2> W a0, W b0, W a1, W h -> a0 b0 + a1 u0 + h; 37 fr29_dot_add_b<2, 3> W a0, W a1, W h -> a0 u0 + a1 u1 + h.
 * uniform18: the wave-uniform factors u0, u1 of 35..37 (2 x W; null: zeros) -- ONE value per call, handed to the kernel as an argument, because those forms
 * read them from scalar registers. in: n_items x words-in u32, out: n_items x words-out u32, host memory. */
int acvm_debug_fr(uint32_t what, const uint32_t *in, uint32_t n_items, const uint32_t *uniform18, uint32_t *out);
/* The precomputed coefficient x row reduction of the gate kernel (fr_device.hpp fr29_lin_add<1 / 2>, lin_table.hpp) ON THE DEVICE against integers: one lane
 * per item, and the 64 items of a wave share their coefficients, as in the gate kernel (the tables are read by scalar loads). With n_groups =
 * ceil(n_items / 64): n_terms [n_groups] = 1 | 2; coef [n_groups][2][8] = the coefficients as canonical integers, little-endian words (the second unused for
 * one term); rows [n_items][2][8] = any 256-bit patterns (the storage form); h [n_items][9] = any limbs. tables_out (may be NULL) [n_groups][2][81]: the
 * tables the planner's builder made -- word [9 k + i] = limb k of c 2^(29 i + 58) mod p; out [n_items][9]: the routine's raw limbs. Host memory. */
int acvm_debug_lin_add(const uint32_t *n_terms, const uint32_t *coef, const uint32_t *rows, const uint32_t *h, uint32_t n_items, uint32_t *tables_out, uint32_t *out);
/* Host-only: the linear tables of the plan a handle of these options would get, under the hazard checker (acvm_circuit_check_schedule: same arguments, same
 * return), optionally after a mutation of a copy of the plan: 0 none, 1 the first two tables that differ change places, 2 the first wave program with
 * tables starts one table later. counts[6]: wave programs, wave programs with tables, gate records, records that take the table form, tables, findings. */
int acvm_debug_lin_plan(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids, uint32_t n_keep,
                        uint32_t n_instances, uint32_t mutation, uint64_t *counts, char *report, size_t report_len);
/* Host-only: the bundles of the plan a handle of these options would get -- the wave programs of each gate launch that one wave runs one after the other
 * with one shared operand row loaded once (tuning share, max_bundle) -- and the hazard checker's verdict on them, optionally after a mutation of a copy of
 * the plan: 0 none, 1 the grouped list names a wave program twice. out: [n_levels, n_bundles, n_programs, n_shared_bundles, n_shared_loads_saved (row loads
 * per instance), findings, bundle_level_start[n_levels + 1], bundle_start[n_bundles + 1], bundle_row[n_bundles] (0xFFFFFFFE: none), bundle_prog[n_programs]
 * (indices of wave programs in level-major order, as acvm_debug_gate_records lists them)]. Returns the number of words that is; the first min(that, cap)
 * are written (out may be NULL with cap = 0). */
int acvm_debug_bundle_plan(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids, uint32_t n_keep,
                           uint32_t n_instances, uint32_t mutation, uint32_t *out, uint32_t cap);
/* The inversion batch of the level schedule (inverse_batch_kernel through its launcher, exactly as a solve starts it) on a table made for the call.
 * den: [n_jobs][B] canonical denominators in the storage form (8 x u32; zero = the instance leaves the generic path at that job). Job k reads row k,
 * carries opcode index k and owns row slot_of[k] of the inverse table (null: row k; otherwise a permutation of [0, n_jobs)); the rows have the batch's
 * stride, the event words the header of a batch. inv_chunk: the tuning's jobs per wave. Out: inv_out [n_jobs][B] x 8 u32 = the RAW rows of the
 * inverse table (row slot_of[k] holds 1 / den[k]), event_out [B] event words, *device_count = the device's count of flagged instances (the word four in
 * front of the event words), *host_count = the host-mapped counter the same kernels keep. The waves that share one field inversion are the
 * process-wide tuning's ("inv_share": what a handle created now would get). */
int acvm_debug_inverse_batch(const uint32_t *den, uint32_t n_jobs, uint32_t B, uint32_t inv_chunk, const uint32_t *slot_of, uint32_t *inv_out,
                             uint32_t *event_out, uint32_t *device_count, uint32_t *host_count);
/* The same with inv_share of the caller's: 1 = the one-wave kernel, 2 / 4 / 8 = the workgroup of that many waves around one field inversion (anything
 * else: the next lower of those). The rows of a lane without a zero denominator do not depend on it, bit for bit. */
int acvm_debug_inverse_batch_shared(const uint32_t *den, uint32_t n_jobs, uint32_t B, uint32_t inv_chunk, uint32_t inv_share, const uint32_t *slot_of,
                                    uint32_t *inv_out, uint32_t *event_out, uint32_t *device_count, uint32_t *host_count);
/* The ordered selection of acvm_batch_outcomes_device (the shipped kernels through their launcher) on a status array of the caller's, host in and host
 * out: out_list[0 .. *n_selected) = the i < n, ascending, with bit status[i] of select_mask set (a status byte of 32 or more is never selected); what
 * lies behind *n_selected in out_list ([n] capacity) keeps the caller's bytes. out_list may be NULL: the count alone. */
int acvm_debug_select(const uint8_t *status, uint32_t n, uint32_t select_mask, uint32_t *out_list, uint32_t *n_selected);

/* Peak of the ALU roofline of the integer-bound kernels: back-to-back Montgomery products (fr29_mul, the product every
 * kernel uses) on every SIMD, waves_per_simd dependent chains of 2 * iters products interleaved per SIMD; the best of three timed
 * launches as modmul/s, and the number of products one launch executes. */
int acvm_debug_modmul_rate(uint32_t iters, uint32_t waves_per_simd, double *modmul_per_s, uint64_t *n_modmul);
/* The same for the ECDSA kernels: back-to-back base-field products of secp256k1 (curve 0) / secp256r1 (curve 1), a product and a square in turn
 * (acvm_amd/csrc/secp_device.hpp sp_mul / sp_sqr). */
int acvm_debug_secp_rate(uint32_t curve, uint32_t iters, uint32_t waves_per_simd, double *products_per_s, uint64_t *n_products);
/* The measured streaming ceiling of the device for the gate kernel's access shape (reported beside the 8 TB/s spec peak of the HBM
 * roofline): two rows of `bytes` bytes read and one written, 16 bytes per lane, the grid covering the data like a level launch;
 * bytes moved (3 x bytes) per second of the best of four launches, in GB/s. */
int acvm_debug_stream_rate(size_t bytes, double *gb_per_s);

/* Circuit::read: gzip(bincode) or raw bincode bytes. */
acvm_circuit_t *acvm_circuit_from_bytes(const uint8_t *bytes, size_t len);
void acvm_circuit_free(acvm_circuit_t *c);
uint32_t acvm_circuit_num_opcodes(const acvm_circuit_t *c);
uint32_t acvm_circuit_num_witnesses(const acvm_circuit_t *c); /* 1 + highest witness index referenced */
/*
 * ACVM::opcodes (acvm/src/pwg/mod.rs:166-168) seen through the ABI: for opcodes [first, first + n) of the circuit, kinds[2 i] = the variant of
 * acir::circuit::Opcode in declaration order (opcodes.rs:15-34: 0 Arithmetic, 1 BlackBoxFuncCall, 2 Directive, 3 Brillig, 4 MemoryOp,
 * 5 MemoryInit) and kinds[2 i + 1] = what tells its instances apart at a glance: the BlackBoxFuncCall variant (black_box_function_call.rs:20-115,
 * the tags of ACVM_ERR_UNSUPPORTED_BLACKBOX's aux0), the Directive variant (0 Quotient, 1 ToLeRadix, 2 PermutationSort), the length of a
 * Brillig bytecode, the block id of a memory opcode, 0 for Arithmetic. With acvm_circuit_num_opcodes and acvm_result_t.opcode_index (the
 * instruction pointer) a binding serves `opcodes()` from the Vec<Opcode> it was constructed with and can assert it is the circuit the
 * handle runs.
 */
int acvm_circuit_opcode_kinds(const acvm_circuit_t *c, uint32_t first, uint32_t n, uint32_t *kinds /*[n][2]*/);
/* Host-only levelisation against a set of initial witness ids (no device needed): plan statistics in *out. Returns 0, or
 * ACVM_E_UNSUPPORTED (reason in acvm_last_error) if the circuit holds an opcode no kernel implements. */
int acvm_circuit_plan_stats(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, acvm_stats_t *out);
/* how often this circuit handle has been levelised so far: handles created for the same (initial ids, options, tuning) share one immutable plan */
uint64_t acvm_circuit_plans_built(const acvm_circuit_t *c);
/* the same for a batch created with acvm_batch_new_ex's flags (n_table_rows, n_digest_segments) */
int acvm_circuit_plan_stats_ex(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids,
                               uint32_t n_keep, acvm_stats_t *out);

/*
 * Host-only: the hazard checker of the level schedule (acvm_amd/csrc/schedule_check.cpp). One solve is enqueued on up to six streams with
 * partial waits, recycled rows and rows whose representation depends on the consumer; the reference's semantics are strictly in order
 * (acvm/src/pwg/mod.rs:236-303). For the plan and schedule a handle of n_instances instances with these flags (acvm_batch_new_ex's, | 0x100 =
 * planned for a caller-supplied solver) would use, the checker derives every launch's reads and writes from the record words, builds
 * happens-before from stream order + event edges, and proves: every conflicting pair of accesses is ordered, every read sees the write of the
 * witness the original opcode names, every reader outside the gate kernels sees a canonical row, no bound passes 2^256. Returns 0 (proved),
 * 1 (findings; the first 32 as text in report) or a negative error. counts[0..5) = launches, waits, accesses, records, findings.
 * drop_wait = k leaves the k-th cross-stream wait out of the schedule (mutation testing: the checker must then name the resource and the
 * two launches); 0xFFFFFFFF = the schedule as enqueued.
 */
int acvm_circuit_check_schedule(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids, uint32_t n_keep,
                                uint32_t n_instances, uint32_t drop_wait, uint64_t *counts /*[5]*/, char *report, size_t report_len);
/* Host-only: 64-bit fingerprints of the static plan (gate stream, in-order program, level and dependency tables, row assignment ...), one per
 * component, into out[0, cap); returns the number of components. flags: acvm_batch_new_ex's, | 0x100 = planned for a caller-supplied solver.
 * For tests and tools that assert that a change of the planner moved nothing (tests/test_plan_host.py). */
int acvm_debug_plan_fingerprint(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids,
                                uint32_t n_keep, uint64_t *out, uint32_t cap);
/* Host-only: the gate stream of the same plan word for word (acvm_amd/csrc/gate_record.hpp says what a record's words mean), for tests that assert which
 * record shapes their inputs reach. out[0] = wave programs, out[1] = words of the stream, then the offset of every wave program in the stream, then the
 * offset of every wave program's linear tables (0xFFFFFFFF: it has none), then the stream. Returns the number of words that is and writes the first
 * min(that, cap) of them (out may be NULL with cap = 0). */
int acvm_debug_gate_records(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids,
                            uint32_t n_keep, uint32_t *out, uint32_t cap);
/* Host-only: the per-lane scratch words the same plan reserves for the record of each opcode (hash messages, the working memory of
 * Directive::PermutationSort, Schnorr's preimage, the Brillig VM), one word per opcode in program order, 0 where a record takes none. Returns the
 * number of opcodes and writes the first min(that, cap) words (out may be NULL with cap = 0). */
int acvm_debug_record_scratch(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids,
                              uint32_t n_keep, uint32_t *out, uint32_t cap);
/*
 * ACVM::new for n_instances instances that all assign the same initial witness ids.
 * The circuit is levelised once against that set. `solver` may be NULL (built-in HIP backend).
 */
acvm_batch_t *acvm_batch_new(const acvm_circuit_t *c, const acvm_bb_solver_t *solver, uint32_t n_instances,
                             const uint32_t *initial_ids, uint32_t n_initial);
/*
 * The same with options for callers that keep only the return witnesses and a digest of every map:
 *   ACVM_BATCH_FOLD_DIGEST  the per-instance digest (acvm_batch_digest) is computed DURING the solve, leaf by leaf as the witnesses
 *                           of a segment complete, beside the level kernels: acvm_batch_digest then only hashes the leaves.
 *   ACVM_BATCH_REUSE_SLOTS  witness-slot liveness reuse: a witness occupies a row of the device table from the level that writes it
 *                           to the level of its last reader, rows are recycled (implies the folded digest: a row is hashed before
 *                           it is reused). Afterwards only the initial witnesses and keep_ids can be read back (acvm_batch_witness
 *                           / _extract_witnesses), plus results and digests; acvm_batch_witness_map returns ACVM_E_STATE. Instances
 *                           that leave the generic path are re-solved from their initial witnesses in a table of their own
 *                           (all witnesses x flagged instances, padded to 64; acvm_batch_solve returns ACVM_E_UNSUPPORTED when
 *                           that table would be larger than both the level table and 8 GiB: solve such a tile without the flag).
 */
#define ACVM_BATCH_FOLD_DIGEST 1u
#define ACVM_BATCH_REUSE_SLOTS 2u
acvm_batch_t *acvm_batch_new_ex(const acvm_circuit_t *c, const acvm_bb_solver_t *solver, uint32_t n_instances, const uint32_t *initial_ids,
                                uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids, uint32_t n_keep);
void acvm_batch_free(acvm_batch_t *b);
/* values_be32: [n_instances][n_initial][32] canonical big-endian (reduced mod p like from_be_bytes_reduce). */
int acvm_batch_set_initial_witness(acvm_batch_t *b, const uint8_t *values_be32);
/* same, from a device-resident buffer of the same layout (no PCIe in the call) */
int acvm_batch_set_initial_witness_device(acvm_batch_t *b, const void *d_values_be32);
/* Device buffers for callers that keep their inputs resident (acvm_batch_set_initial_witness_device): plain hipMalloc / hipFree /
 * hipMemcpy on the current device, so that a caller needs no HIP headers. */
void *acvm_device_malloc(size_t bytes);
int acvm_device_free(void *p);
int acvm_device_upload(void *dst_device, const void *src_host, size_t bytes);
int acvm_device_download(void *dst_host, const void *src_device, size_t bytes); /* its twin: what a caller inspects of an acvm_batch_export_device buffer */
/* ACVM::solve for every instance. Returns the number of instances not Solved, or a negative error. */
int acvm_batch_solve(acvm_batch_t *b);
/*
 * The same solve for a caller that runs tile after tile through one handle (a 10k-gate circuit at 2^20 instances is eight tiles of one
 * handle's table): d_next_values_be32 is the device buffer of the NEXT tile's initial witnesses (layout of acvm_batch_set_initial_witness_device,
 * valid until the solve after this one returns). Its import is enqueued behind this solve and gated on the device: it runs if, and only if, no
 * instance of this solve left the generic path (the exact path needs this tile's rows otherwise). The call returns when this solve's outcome
 * is known, while that import may still be running; the following acvm_batch_set_initial_witness_device with the SAME pointer then costs
 * nothing (or performs the import, had it been held back), and the next tile's kernels follow the import without a gap. Until then results,
 * statistics and every witness that is not an initial one can be read as after acvm_batch_solve; reading an initial witness, a whole map
 * or an unfolded digest returns ACVM_E_STATE -- those rows may already hold the next tile. Not with a caller-supplied solver, stepping or
 * resumed foreign calls (then it is acvm_batch_solve). The reference has no counterpart: one ACVM solves one instance (pwg/mod.rs:236-241).
 */
int acvm_batch_solve_then_import(acvm_batch_t *b, const void *d_next_values_be32);
/*
 * ACVM::solve_opcode (acvm/src/pwg/mod.rs:243-303) for the batch: executes ONE opcode -- the one at the smallest instruction
 * pointer among the instances that are InProgress -- for every InProgress instance standing on it, through the exact in-order
 * kernels (one lane per instance). Instances only ever differ in their instruction pointer after a foreign call: one that
 * waited is behind the others once it is resolved, and catches up one call at a time. Starts from a batch whose initial
 * witness was just set (or acvm_batch_reset); ACVM_E_STATE after a plain acvm_batch_solve. acvm_batch_solve after some steps
 * runs the rest. Returns the number of instances not Solved; acvm_batch_results gives status and instruction pointer
 * (InProgress instances report the opcode they stand on).
 */
int acvm_batch_solve_opcode(acvm_batch_t *b);
/* back to the state right after set_initial_witness (same inputs, nothing solved) */
int acvm_batch_reset(acvm_batch_t *b);
/* The handle serves any batch size up to the n_instances it was created with (its plan and tables are kept): from the next
 * acvm_batch_set_initial_witness on, every call covers instances [0, n), 1 <= n <= that capacity; the lanes behind n are dead. A caller whose
 * batches vary in size creates ONE handle for the largest (planning a 10^6-opcode circuit takes seconds) instead of one per size. */
int acvm_batch_set_instances(acvm_batch_t *b, uint32_t n);
/* force every instance through the exact in-order kernel instead of the level-parallel one (validation) */
int acvm_batch_set_force_slow_path(acvm_batch_t *b, int on);
int acvm_batch_results(acvm_batch_t *b, acvm_result_t *out /*[n_instances]*/);
/* one witness across the batch: out_be32 [n_instances][32], assigned [n_instances] (0/1) */
int acvm_batch_witness(acvm_batch_t *b, uint32_t witness, uint8_t *out_be32, uint8_t *assigned);
/* full witness maps of instances [first, first+n): assigned [n][nw], values_be32 [n][nw][32] (zeros if unassigned) */
int acvm_batch_witness_map(acvm_batch_t *b, uint32_t first, uint32_t n, uint8_t *assigned, uint8_t *values_be32);
int acvm_batch_stats(acvm_batch_t *b, acvm_stats_t *out);

/*
 * Brillig foreign calls. An instance whose Brillig VM reaches a ForeignCall without a result stops with status
 * ACVM_STATUS_REQUIRES_FOREIGN_CALL and its instruction pointer on that opcode (pwg/mod.rs:262-268).
 *   acvm_batch_pending_foreign_call        = ACVM::get_pending_foreign_call (mod.rs:203-209): returns 1 and fills *info if
 *                                            the instance waits, 0 if it does not
 *   acvm_batch_pending_foreign_call_inputs = ForeignCallWaitInfo::inputs (pwg/brillig.rs:157-163): lens[n_inputs], then the
 *                                            values of all inputs back to back, 32 bytes big-endian each (info.n_values)
 *   acvm_batch_resolve_foreign_call        = ACVM::resolve_pending_foreign_call (mod.rs:214-228): one ForeignCallResult =
 *                                            n_values outputs, output i a single value (is_array[i] == 0) or an array of
 *                                            lens[i] values; values back to back. ACVM_E_STATE if the instance is not waiting
 *                                            (the reference panics).
 * After resolving any number of instances, acvm_batch_solve continues them (the opcode re-runs its VM with the results so far).
 */
typedef struct {
    uint32_t opcode_index;   /* the Brillig opcode the instance waits at */
    uint32_t brillig_index;  /* index of the ForeignCall inside its bytecode */
    uint32_t n_inputs, n_values;
    char function[64];
} acvm_foreign_call_info_t;
int acvm_batch_pending_foreign_call(acvm_batch_t *b, uint32_t instance, acvm_foreign_call_info_t *info);
int acvm_batch_pending_foreign_call_inputs(acvm_batch_t *b, uint32_t instance, uint32_t *lens, uint8_t *values_be32);
int acvm_batch_resolve_foreign_call(acvm_batch_t *b, uint32_t instance, uint32_t n_values, const uint8_t *is_array, const uint32_t *lens,
                                    const uint8_t *values_be32);
/*
 * The same round trip for the whole batch, where both halves of the data already are: the inputs of the waiting instances as DEVICE columns, the
 * answers read from DEVICE columns -- a GPU oracle (a note database, a Merkle-path service, a logger that discards its input) answers a batch
 * without a value crossing PCIe and without a call per instance. Encodings, layouts, stride and alignment are those of acvm_batch_export_device /
 * acvm_batch_import_device below (ACVM_ENC_*, ACVM_LAYOUT_*).
 *
 * Sites and rows. A waiting instance waits at a site = (opcode_index, brillig_index). acvm_batch_foreign_call_sites writes up to `cap` of the distinct
 * sites at which instances of the batch wait, ascending by (opcode, brillig index), and returns their number (0 for a batch that is not solved);
 * it is host only and copies nothing. The calls the library answers itself (a caller's BlackBoxFunctionSolver inside a Brillig program) are never
 * listed. The WAITING LIST of a site is its instances in ascending instance number; it is fixed from one acvm_batch_solve / acvm_batch_solve_opcode
 * to the next: answering a row does not remove it (n_resolved counts the answered ones). Row r below is position r of that list, and element row
 * i = r - first_row of the caller's buffer.
 *
 * acvm_batch_foreign_call_inputs_device: for rows [first_row, first_row + n_rows) of the site
 *   - d_instances[i] = the row's absolute instance number; d_lens[i * n_inputs + k] = the number of values of input k (n_inputs of the site);
 *   - element (i, v) of d_values = the v-th value of the row's inputs back to back -- the values acvm_batch_pending_foreign_call_inputs returns for
 *     that instance -- encoded as the export encodes a witness, at (i * stride + v) * size instance-major, (v * stride + i) * size witness-major
 *     (stride in elements, 0 = dense: n_columns resp. n_rows); d_mask, same layout and stride, one byte per element: 1 = the value exists (and fits
 *     a narrow encoding), 2 = it exists but is 2^(8 size) or more. A column at or beyond the row's total is zero bytes, mask 0.
 *   - *max_values (may be NULL) = the largest total over the rows, found on the device (four bytes come back). With d_values and d_mask NULL this is
 *     the sizing call. n_columns below that maximum is ACVM_E_INVALID when d_values or d_mask is given; the message states the needed width and nothing
 *     is written.
 *   - Each of the four pointers may be NULL. ACVM_E_INVALID: a null descriptor, rows outside the list, an unknown encoding or layout, a stride below
 *     the dense one, a d_values that is not aligned as the export asks. ACVM_E_STATE: a batch that is not solved.
 *   - The host knows which lanes wait where (it holds every instance's status): the calls upload 8 bytes per listed row (lane and
 *     instance number), once per range between two solves, and no value; each returns after the batch's stream is synchronised.
 *
 * acvm_batch_resolve_foreign_calls_device: ACVM::resolve_pending_foreign_call (pwg/mod.rs:214-228) for rows [first_row, first_row + n_rows) at once:
 * ONE ForeignCallResult shape for all of them -- n_values outputs, output k a single value (is_array[k] == 0) or an array of lens[k] values; both
 * arrays on the HOST -- and the values of row i back to back in columns 0 .. total - 1 of d_values, read as acvm_batch_import_device reads a buffer
 * (row = the instance axis). One result is appended to each instance's results of that opcode.
 *   - Every 256-bit string is accepted and reduced as the per-instance call reduces it (BE32: from_be_bytes_reduce; LE32, MONT256_LE and the narrow
 *     encodings as acvm_batch_import_device decodes them).
 *   - The shape is not checked against the bytecode: a count or size that does not match fails the VM when it runs again, exactly as after the
 *     per-instance call.
 *   - Refused as a whole, the handle left as it was: ACVM_E_STATE for a batch that is not solved or a row that was already answered since the last
 *     solve; ACVM_E_INVALID for rows outside the list, n_columns below the shape's total, a bad stride, alignment, encoding or layout, null arrays;
 *     ACVM_E_UNSUPPORTED for a handle with a caller's BlackBoxFunctionSolver (its internal calls keep the result store on the host).
 *   - Afterwards acvm_batch_solve / acvm_batch_solve_opcode continue the rows exactly as after per-instance resolves. Both forms may be mixed, in
 *     any order, on one handle: acvm_batch_resolve_foreign_call appends through the same kernel once an opcode's results live on the device.
 *   - Uploads the shape words, and 8 bytes per listed row unless the inputs call left them there for the same range; returns after the batch's
 *     stream is synchronised. However many calls answer the rows of one round, the result store grows by one result per instance and round.
 * acvm_debug_foreign_call_stats: the cumulative bytes BOTH forms of the round trip copied host-to-device / device-to-host for this handle, and the
 * device times (HIP events) of the last inputs and append kernels, and the device bytes the result store's tables hold right now (they grow by one
 * result per column and round, however many calls answer a round's rows). Each pointer may be NULL.
 * The node form is acvm_node_set_foreign_call_handler below.
 * Not here: an asynchronous variant; rows whose outputs differ in number or kind (the per-instance call); parking a waiting tile beside the next one.
 */
typedef struct {
    uint32_t opcode_index, brillig_index;
    uint32_t n_inputs;      /* inputs of the ForeignCall as written in the bytecode */
    uint32_t n_waiting;     /* instances whose status is RequiresForeignCall at this site */
    uint32_t n_resolved;    /* of those, how many were answered since the last solve */
    char function[64];
} acvm_foreign_call_site_t;
int acvm_batch_foreign_call_sites(acvm_batch_t *b, acvm_foreign_call_site_t *out, uint32_t cap);
typedef struct {
    uint32_t opcode_index, brillig_index;
    uint32_t first_row, n_rows;      /* rows [first_row, first_row + n_rows) of the site's list */
    uint32_t encoding, layout;       /* any ACVM_ENC_*; ACVM_LAYOUT_INSTANCE_MAJOR (row-major) or ACVM_LAYOUT_WITNESS_MAJOR (column-major) */
    uint32_t n_columns;              /* capacity in values per row */
    uint64_t stride;                 /* elements, 0 = dense */
    uint32_t *d_instances;           /* [n_rows] absolute instance numbers (may be NULL) */
    uint32_t *d_lens;                /* [n_rows][n_inputs] values per input, row-major (may be NULL) */
    void     *d_values;              /* (may be NULL) */
    uint8_t  *d_mask;                /* same layout and stride, one byte per element (may be NULL) */
} acvm_foreign_call_inputs_desc_t;
int acvm_batch_foreign_call_inputs_device(acvm_batch_t *b, const acvm_foreign_call_inputs_desc_t *d, uint32_t *max_values);
typedef struct {
    uint32_t opcode_index, brillig_index;
    uint32_t first_row, n_rows;
    uint32_t n_values;               /* outputs of ONE ForeignCallResult, the same shape for every row */
    const uint8_t *is_array;         /* HOST [n_values] */
    const uint32_t *lens;            /* HOST [n_values], length of an array output (ignored for a single value) */
    uint32_t encoding, layout;
    uint32_t n_columns;
    uint64_t stride;
    const void *d_values;            /* the row's values back to back in columns 0 .. total - 1 */
} acvm_foreign_call_answers_desc_t;
int acvm_batch_resolve_foreign_calls_device(acvm_batch_t *b, const acvm_foreign_call_answers_desc_t *d);
/*
 * acvm_batch_resolve_foreign_calls_device_rows: the same call with PER-ROW answers -- what a handler per instance can do (pwg/mod.rs:214-228 takes one
 * ForeignCallResult of any shape per instance): a slice-returning oracle (a HeapVector output) returns a different length per row, and a GPU oracle
 * finds an entry for some rows and not for others. The descriptor is acvm_foreign_call_answers_desc_t plus two optional DEVICE columns:
 *   d_lens      [n_rows][n_values] row-major: the number of values of array output k of row i (ignored where is_array[k] == 0). NULL: the host
 *               `lens` hold for every row. The values of row i stay back to back in columns 0 .. total_i - 1.
 *   d_answered  [n_rows]: 0 = the row is NOT answered -- it keeps waiting, n_resolved does not count it, nothing is appended for it and a later call
 *               of the same round may answer it; nonzero = answered. NULL: every row is answered.
 *   - With d_lens a sizing launch runs before anything is written: the largest total among the answered rows, summed in 64 bits (four bytes come
 *     back). n_columns below it is ACVM_E_INVALID, the message states the needed width; a total of 2^31 or more is refused the same way. The result
 *     store is sized from that largest total.
 *   - With d_answered the call downloads the mask (n_rows bytes): the host must know which lanes resume. Without it nothing more comes back than
 *     from acvm_batch_resolve_foreign_calls_device. The mask is read once, into memory of the handle: the rows judged and the rows appended are the
 *     same whatever the caller does to d_answered meanwhile. d_lens must stay unchanged until the call returns.
 *   - The refusals are those of acvm_batch_resolve_foreign_calls_device, the handle left as it was; a row that was already answered since the last
 *     solve AND is marked answered again is ACVM_E_STATE, an already answered row that is masked out is fine. The host `lens` are not read, and may be NULL,
 *     when d_lens is given.
 *   - The per-instance call, acvm_batch_resolve_foreign_calls_device and this call may be mixed on one handle in any order.
 */
typedef struct {
    uint32_t opcode_index, brillig_index;
    uint32_t first_row, n_rows;
    uint32_t n_values;               /* outputs of one ForeignCallResult; which of them are arrays is the same for every row */
    const uint8_t *is_array;         /* HOST [n_values] */
    const uint32_t *lens;            /* HOST [n_values]: the lengths of every row when d_lens is NULL */
    uint32_t encoding, layout;
    uint32_t n_columns;
    uint64_t stride;
    const void *d_values;            /* row i's values back to back in columns 0 .. total_i - 1 */
    const uint32_t *d_lens;          /* DEVICE [n_rows][n_values], may be NULL */
    const uint8_t *d_answered;       /* DEVICE [n_rows], may be NULL */
} acvm_foreign_call_answers_rows_desc_t;
int acvm_batch_resolve_foreign_calls_device_rows(acvm_batch_t *b, const acvm_foreign_call_answers_rows_desc_t *d);
int acvm_debug_foreign_call_stats(const acvm_batch_t *b, uint64_t *h2d_bytes, uint64_t *d2h_bytes, double *inputs_kernel_ms, double *append_kernel_ms,
                                  uint64_t *store_bytes);
/* What the Brillig retry passes of the last solve did under brillig_resume = 1 (acvm_tuning_set; all zero otherwise): out[0] passes, out[1] lanes
 * continued from a checkpoint, out[2] lanes that ran their opcode again, out[3] memory cells relocated between two scratches (live cells only),
 * out[4] VM steps executed in those passes summed over lanes and passes, out[5] relocation launches (a change of buffers with nothing live to copy launches nothing and is not counted). Counted like n_brillig_retries: cleared by
 * acvm_batch_solve, accumulated over the acvm_batch_solve_opcode steps and the continuations after a foreign call. */
int acvm_debug_brillig_resume_stats(const acvm_batch_t *b, uint64_t out[6]);
/* enable per-kernel HIP-event timing of the level kernels (small overhead) */
int acvm_batch_set_profiling(acvm_batch_t *b, int on);

/*
 * What a caller does right after solve.
 *
 * Circuit::get_assert_message (acir/src/circuit/mod.rs:43-51) for OpcodeLocation::Acir(acir_index) (brillig_index =
 * ACVM_LOCATION_ACIR) or OpcodeLocation::Brillig{acir_index, brillig_index}. Copies the NUL-terminated message (truncated to
 * cap) and returns its full length, or returns -1 when the location has no message.
 */
#define ACVM_LOCATION_ACIR 0xFFFFFFFFu
int acvm_circuit_assert_message(const acvm_circuit_t *c, uint32_t acir_index, uint32_t brillig_index, char *out, size_t cap);
/*
 * Witness sets of the circuit, ascending (they are BTreeSets in the reference): private_parameters, public_parameters,
 * return_values (circuit/mod.rs:25-32), public_inputs() = public_parameters U return_values (:115-121),
 * circuit_arguments() = private U public parameters (:109-113). Writes up to cap indices, returns the size of the set.
 */
enum { ACVM_SET_PRIVATE_PARAMETERS = 0, ACVM_SET_PUBLIC_PARAMETERS = 1, ACVM_SET_RETURN_VALUES = 2, ACVM_SET_PUBLIC_INPUTS = 3,
       ACVM_SET_CIRCUIT_ARGUMENTS = 4 };
int acvm_circuit_witness_set(const acvm_circuit_t *c, int which, uint32_t *out, uint32_t cap);
/*
 * The error string acvm_js reports for a failed instance (acvm_js/src/execute.rs:79-108): "Assertion failed: <message>" when
 * the failing location -- the opcode of UnsatisfiedConstrain / IndexOutOfBounds, the last call-stack entry of
 * BrilligFunctionFailed -- has an assert message in `c`, else the Display text of the OpcodeResolutionError
 * (acvm/src/pwg/mod.rs:100-114). Returns the full length; 0 and an empty string for an instance that did not fail.
 * ExpressionHasTooManyUnknowns carries its expression like the reference's Display: the opcode partially evaluated on the instance's map
 * for Opcode::Arithmetic (acvm/src/pwg/arithmetic.rs:31,38-42), the offending input expression for Opcode::Brillig (brillig.rs:46-74), in the
 * formats of acir_field/src/generic_ark.rs:13-74 and acir/src/circuit/opcodes.rs:88-102 (needs `c`; without it the text ends after "unknowns ").
 */
int acvm_batch_error_string(acvm_batch_t *b, const acvm_circuit_t *c, uint32_t instance, char *out, size_t cap);
/*
 * The same expression as DATA: OpcodeNotSolvable::ExpressionHasTooManyUnknowns(Expression) (acvm/src/pwg/mod.rs:72-78) carries the opcode
 * partially evaluated on the instance's witness map (arithmetic.rs:31,38-42; for Opcode::Brillig the offending input expression as written,
 * brillig.rs:46-74), and a binding rebuilds that variant from it instead of from a Default::default(). Returns 1 and fills *head and the
 * arrays when `instance` failed with ACVM_ERR_TOO_MANY_UNKNOWNS, 0 (head zeroed) when it did not. Expression (acir/src/native_types/
 * expression/mod.rs:17-28) = sum mul_coef[i] * w[mul_witnesses[2 i]] * w[mul_witnesses[2 i + 1]] + sum lin_coef[i] * w[lin_witnesses[i]] + q_c,
 * terms in the order the reference's evaluate() leaves them (mul terms that stay, then mul terms that folded into linear ones, then the
 * linear terms); coefficients canonical 32-byte big-endian. Up to cap_mul / cap_lin terms are written (any array may be NULL); head has the counts.
 */
typedef struct {
    uint32_t n_mul, n_lin;
    uint32_t opcode_index; /* the opcode that could not be solved */
    uint8_t q_c[32];
} acvm_expression_t;
int acvm_batch_error_expression(acvm_batch_t *b, const acvm_circuit_t *c, uint32_t instance, acvm_expression_t *head, uint8_t *mul_coef_be32,
                                uint32_t *mul_witnesses /*[cap_mul][2]*/, uint32_t cap_mul, uint8_t *lin_coef_be32, uint32_t *lin_witnesses,
                                uint32_t cap_lin);
/*
 * Per-instance 32-byte digest of the solved witness map for instances [first, first + n), out32 = [n][32] (SURVEY 8d, config 5:
 * callers that keep only the return witnesses use it to compare whole maps without moving them -- the map of the reference is
 * what ACVM::finalize returns, acvm/src/pwg/mod.rs:176-181). Definition: with the two fixed elements of BN254-Fr
 *     g = Blake2s-256("acvm_amd witness map digest: g"),  h = Blake2s-256("acvm_amd witness map digest: h")
 * (the 32 digest bytes read as a big-endian integer, reduced modulo p),
 *     D = sum over the ASSIGNED witnesses w of ( value_w * g^(w+1) + h^(w+1) )  in BN254-Fr,
 *     digest = Blake2s-256( D as 32 big-endian bytes )          (value_w: FieldElement, acir_field/src/generic_ark.rs:156-406).
 * A polynomial fingerprint of the map (two maps differ in D unless g is a root of their difference: probability < 2^-230 for maps
 * that do not depend on g; it is an integrity check, not a commitment against an adversary who knows g). The h-term tells an
 * unassigned witness from one assigned zero. Linear and order-free on purpose: one field product per witness -- a witness the level
 * kernels keep scaled (DESIGN.md "projective witnesses") is folded into its coefficient -- summed in any order, so the library adds
 * a witness as soon as it exists (ACVM_BATCH_FOLD_DIGEST) and may recycle its row (ACVM_BATCH_REUSE_SLOTS). Works for solved,
 * failed and waiting instances alike (the map as it stands). oracle/binding.py witness_map_digest restates it with Python integers.
 */
int acvm_batch_digest(acvm_batch_t *b, uint32_t first, uint32_t n, uint8_t *out32);
/*
 * The same map hashed AS BYTES (ABI 6): SURVEY 8d's "blake2s over the full witness vector", collision-resistant, in tree form so that a map of a
 * million witnesses is not one sequential chain:
 *     leaf_k = Blake2s-256( for w in [256 k, min(256 k + 256, nw)):  value_w as 32 big-endian bytes if the instance assigned w, else 0xFF x 32 )
 *     digest = Blake2s-256( u32_le(nw)  ||  leaf_0  ||  leaf_1  || ... ),        nw = acvm_circuit_num_witnesses
 * (0xFF x 32 is no canonical field element, so an unassigned witness cannot be mistaken for a value.) About as much device work as the solve of a
 * 10^6-opcode tile itself (557 k compressions and 1.1 M canonicalising products per instance) and it needs every row: for audits -- ACVM_E_STATE with
 * ACVM_BATCH_REUSE_SLOTS; acvm_batch_digest above is the one that folds into the solve. oracle/binding.py witness_map_blake2s restates it with hashlib.
 */
int acvm_batch_digest_blake2s(acvm_batch_t *b, uint32_t first, uint32_t n, uint8_t *out32);
/*
 * extract_indices (acvm_js/src/public_witness.rs:10-21; getReturnWitness / getPublicParametersWitness / getPublicWitness
 * with the sets above): values of the listed witnesses for instances [first, first + n), values_be32 = [n][n_witnesses][32].
 * Fails with ACVM_E_STATE and "Failed to extract witness W from witness map. Witness not found." (instance appended) when
 * one of them is unassigned in one of the instances.
 */
int acvm_batch_extract_witnesses(acvm_batch_t *b, const uint32_t *witnesses, uint32_t n_witnesses, uint32_t first, uint32_t n,
                                 uint8_t *values_be32);

/*
 * The witness map where it already is: ACVM::witness_map / finalize (acvm/src/pwg/mod.rs:161,176-181) written into DEVICE memory of the
 * caller, in the encoding and layout of the GPU program that consumes it (a prover's wire columns, a commitment kernel, the initial
 * witnesses of the next circuit of a pipeline). Every export above stages through host memory; this one moves no value over PCIe.
 *   - d_values / d_assigned are plain device pointers on the batch's device. d_values holds one element per (instance, witness): 32 bytes, 16-byte
 *     aligned, for the 32-byte encodings; the integer's 1, 2, 4, 8 or 16 bytes, aligned to that size, for the narrow ones (else ACVM_E_INVALID).
 *     d_assigned, which may be NULL, holds one byte per element in the same layout and stride (in elements): 0 / 1 for the 32-byte encodings.
 *   - A narrow element is the low `size` bytes of the canonical value, little-endian: the truncation of FieldElement::to_u128
 *     (acir_field/src/generic_ark.rs:227-230). Its mask byte says whether that is the whole value: 0 = unassigned (zero bytes), 1 = assigned and
 *     the value fits, 2 = assigned but the value is 2^(8 size) or more (the low bytes are written all the same).
 *   - witnesses: HOST array of n_witnesses indices, any order, repeats allowed; NULL = the whole map 0 .. acvm_circuit_num_witnesses - 1.
 *   - An unassigned element is zero bytes (32, or the narrow element's size) and mask 0, in every encoding; a listed index beyond the circuit's witnesses is unassigned.
 *     Unlike acvm_batch_extract_witnesses an unassigned witness is not an error: the mask says it.
 *   - stride, in elements: see the layouts; 0 = dense. The bytes between rows are never written. A stride below the dense one is ACVM_E_INVALID.
 *   - The call enqueues on the batch's stream and returns after that stream is synchronised. No value is copied to the host and no host loop
 *     runs per instance; at most one small host-to-device copy is made (the index list, the lanes of the instances of the exact path).
 *   - Answers in every state in which acvm_batch_extract_witnesses answers, with the same values: solved, failed and waiting instances (the
 *     map as it stands), after acvm_batch_solve_opcode steps, with the forced slow path, with ACVM_BATCH_REUSE_SLOTS (initial witnesses and
 *     keep_ids only). The same refusals (ACVM_E_STATE): not solved; a witness that was not kept, or the whole map, of a batch that recycles
 *     rows or keeps exact lanes in its side table; initial witnesses or the whole map after acvm_batch_solve_then_import.
 * Not here: an asynchronous variant (the node's form is acvm_node_solve_device); the host exports above are unchanged.
 */
enum { ACVM_ENC_BE32 = 0,          /* canonical, 32 bytes big-endian: byte for byte what acvm_batch_witness_map writes */
       ACVM_ENC_LE32 = 1,          /* canonical, 4 x u64 little-endian limbs (= 32 bytes little-endian) */
       ACVM_ENC_MONT256_LE = 2,    /* value * 2^256 mod p, 4 x u64 little-endian limbs (ark-ff BigInt<4> / barretenberg fr in memory) */
       /* The narrow encodings: an element is an unsigned little-endian integer of 1, 2, 4, 8 or 16 bytes -- message and digest bytes, flags,
        * counters, 128-bit scalar limbs. Noir's signed types (i8 .. i64) are their two's-complement bit pattern at that width, bool is U8.
        * 3 .. 15 and 21 and up are ACVM_E_INVALID. Not here: big-endian or sign-extending narrow types. */
       ACVM_ENC_U8 = 16, ACVM_ENC_U16 = 17, ACVM_ENC_U32 = 18, ACVM_ENC_U64 = 19, ACVM_ENC_U128 = 20 };
/* size = bytes per element: 32, or the integer's width for the narrow encodings; stride is in elements */
enum { ACVM_LAYOUT_INSTANCE_MAJOR = 0,   /* element (i, k) at (i * stride + k) * size, stride >= n_witnesses (0 = dense) */
       ACVM_LAYOUT_WITNESS_MAJOR = 1,    /* element (i, k) at (k * stride + i) * size, stride >= n           (0 = dense) */
       ACVM_LAYOUT_BROADCAST = 16 };     /* parts of acvm_batch_import_device_parts only: element (i, c) at c * size -- one value for every instance */
typedef struct {
    uint32_t encoding, layout;
    uint32_t first, n;         /* instances [first, first + n): i = instance - first */
    const uint32_t *witnesses; /* k = position in this list (NULL: k = witness index) */
    uint32_t n_witnesses;      /* ignored when witnesses == NULL */
    uint64_t stride;
} acvm_export_desc_t;
int acvm_batch_export_device(acvm_batch_t *b, const acvm_export_desc_t *d, void *d_values, uint8_t *d_assigned);
/*
 * Which instances are usable, where the witnesses already are: the outcome of every instance of [first, first + n) as device columns, and the ascending
 * list of those whose status is one of select_mask -- what a GPU consumer needs of acvm_batch_results (300 bytes per instance on the host) between
 * one tile and the next.
 *   - d_status[i] / d_err[i] / d_opcode_index[i] equal the fields of the same names of acvm_batch_results for instance first + i (a Solved instance:
 *     0 / ACVM_ERR_NONE / 0). Each column may be NULL. The message text, the aux words and the call stack stay host-only: acvm_batch_results.
 *   - select_mask: bit s set = instances whose status is s (ACVM_STATUS_*) are selected. d_selected[0 .. *n_selected) receives their ABSOLUTE instance
 *     numbers in ascending order; it needs room for n entries, and what lies behind *n_selected is not written. d_selected may be NULL with n_selected
 *     given: the count alone. Both NULL: no selection is made.
 *   - Answers in every state in which acvm_batch_results answers (after acvm_batch_solve_opcode steps, with the forced slow path, with
 *     ACVM_BATCH_REUSE_SLOTS, with instances waiting at a foreign call, after acvm_batch_solve_then_import), waits for a pending exact job like it and
 *     refuses like it. ACVM_E_INVALID: a null descriptor; a descriptor with nothing to write (the four pointers and n_selected all NULL); a range
 *     beyond the live instances.
 *   - The call enqueues on the batch's stream and returns after that stream is synchronised. Going up: 16 bytes per instance of the exact path in the
 *     range. Coming back: the count, four bytes. Nothing proportional to n crosses PCIe.
 * Not here: an asynchronous variant (the node's form is acvm_node_solve_device); acvm_batch_results is unchanged.
 */
typedef struct {
    uint32_t first, n;          /* instances [first, first + n) */
    uint8_t  *d_status;         /* [n] ACVM_STATUS_*            (may be NULL) */
    uint8_t  *d_err;            /* [n] ACVM_ERR_*               (may be NULL) */
    uint32_t *d_opcode_index;   /* [n] acvm_result_t.opcode_index (may be NULL) */
    uint32_t select_mask;       /* bit s set: instances whose status is s are selected */
    uint32_t *d_selected;       /* [n] capacity; ascending ABSOLUTE instance numbers (may be NULL) */
} acvm_outcomes_desc_t;
int acvm_batch_outcomes_device(acvm_batch_t *b, const acvm_outcomes_desc_t *d, uint32_t *n_selected);
/*
 * acvm_batch_export_device for LISTED instances: row i of the output is instance d_instances[i] -- with the list acvm_batch_outcomes_device wrote, the
 * map of exactly the solved instances, dense, in the consumer's encoding and layout.
 *   - d is read as by acvm_batch_export_device, except that d->n is the length of the list and d->first must be 0 (else ACVM_E_INVALID).
 *   - d_instances: DEVICE array of d->n absolute instance numbers, any order, repeats allowed. An entry at or beyond the live instance count is not an
 *     error (the host never reads the list): its row is that of an instance that assigned nothing -- zero bytes, mask 0 -- and nothing is read for it.
 *   - Every encoding, both layouts, stride, witness list or whole map, optional mask: as for the range export, with the same checks (n = the list's
 *     length) and the same refusals.
 *   - Host-to-device traffic per call: the witness list, and 4 bytes per instance of the exact path when the set of those instances changed since the
 *     last list export of the handle. Never anything per instance of the batch or per list entry (acvm_debug_export_h2d_bytes: the cumulative bytes
 *     the three device-outcome entry points -- range export, list export, outcomes -- have copied to the device for this handle).
 * Not here: a node form (acvm_node_solve_device writes every row and the selection), an asynchronous variant.
 */
int acvm_batch_export_device_list(acvm_batch_t *b, const acvm_export_desc_t *d, const uint32_t *d_instances, void *d_values, uint8_t *d_assigned);
uint64_t acvm_debug_export_h2d_bytes(const acvm_batch_t *b);
/*
 * The way in as the mirror image of that way out: ACVM::new's initial WitnessMap (pwg/mod.rs:146-156) read from DEVICE memory of the caller in
 * the encoding and layout its producer writes -- a prover's wire columns (ACVM_ENC_MONT256_LE, ACVM_LAYOUT_WITNESS_MAJOR), or the buffer
 * acvm_batch_export_device of another batch filled, whole map and all: the column list picks the initial witnesses out of it.
 *   - Element (instance i, column c) lies at (i * stride + c) * size instance-major and at (c * stride + i) * size witness-major (size: 32, or
 *     the width of a narrow encoding); i runs over the live
 *     instances [0, B) (acvm_batch_set_instances is honoured). stride in elements, 0 = dense: n_columns instance-major, the live B witness-major.
 *     The bytes between rows are never read.
 *   - columns: HOST array, one entry per initial witness in the order of initial_ids given to acvm_batch_new: columns[k] = the column of the
 *     buffer that holds it; repeats allowed. NULL: column k, and n_columns is taken as n_initial. The list is copied before the call returns.
 *   - Every 256-bit string is accepted, as by acvm_batch_set_initial_witness: BE32 is int(bytes, big) mod p, LE32 int(bytes, little) mod p,
 *     MONT256_LE m * 2^-256 mod p for m = int(bytes, little) -- any m < 2^256, m >= p is not an error. The inverse of what the export writes.
 *     A narrow element (ACVM_ENC_U8 .. U128) is the integer itself: it is below p, nothing is reduced.
 *   - ACVM_E_INVALID: a stride below the dense one, columns[k] >= n_columns, an unknown encoding or layout, a null descriptor, null values with
 *     n_initial > 0, and a d_values that is not aligned -- to 16 bytes for the 32-byte encodings, to the element's size for the narrow ones (U8
 *     takes any pointer) -- except for BE32, instance-major, columns == NULL, dense: that descriptor IS
 *     acvm_batch_set_initial_witness_device, takes the same kernel and reads any pointer. A refused call leaves the handle as it was.
 *   - Leaves the handle in the state acvm_batch_set_initial_witness_device leaves it in and returns after the batch's stream is synchronised;
 *     at most one small host-to-device copy is made (the column list, when it differs from the last call's).
 * acvm_batch_solve_then_import_ex is acvm_batch_solve_then_import for such a buffer: the same gate, the same refusals, a plain solve in the same
 * cases. The following acvm_batch_import_device costs nothing only when the pointer AND the descriptor's contents, column list included, are the
 * same (the library keeps a copy of the descriptor, not the caller's pointer); anything else imports again.
 * Not here: an asynchronous variant (the node's form is acvm_node_solve_device); the host import and the two entry points above keep their
 * behaviour. Instances that do not all assign the same ids: acvm_batch_import_device_masked below.
 */
typedef struct {
    uint32_t encoding, layout;   /* ACVM_ENC_*, ACVM_LAYOUT_* */
    const uint32_t *columns;     /* HOST array of n_initial entries, or NULL */
    uint32_t n_columns;          /* width of the caller's buffer in columns (ignored when columns == NULL: n_initial) */
    uint64_t stride;             /* elements; 0 = dense */
} acvm_import_desc_t;
int acvm_batch_import_device(acvm_batch_t *b, const acvm_import_desc_t *d, const void *d_values);
int acvm_batch_solve_then_import_ex(acvm_batch_t *b, const acvm_import_desc_t *d_next, const void *d_next_values);
/*
 * Per-instance PARTIAL initial witness maps: ACVM::new takes a WitnessMap in which absence means unassigned (pwg/mod.rs:146-156), and
 * acvm_batch_export_device writes exactly that -- zero bytes and mask 0 for what an instance did not assign. The masked import reads both:
 *   - d, d_values: exactly as acvm_batch_import_device, with every check, refusal and alignment rule of it, the narrow encodings included.
 *   - d_assigned: DEVICE pointer, any alignment, one byte per element in the layout, the stride (in elements) and the column list of the values:
 *     element (i, c) is byte i * stride + c instance-major and c * stride + i witness-major -- what acvm_batch_export_device writes into its
 *     d_assigned. 0: instance i does NOT hold that initial witness; 1: it does, with the value read from d_values. NULL: the call IS
 *     acvm_batch_import_device -- the same kernels, the same plan, nothing else launched.
 *   - An instance with an absent input is solved as ACVM::solve solves that map: in order from opcode 0 on the exact path, where an opcode that
 *     needs the witness ends it as OpcodeNotSolvable(MissingAssignment(w)) and a gate that has it as its only unknown solves it. The row of an
 *     absent element holds zero afterwards; nothing reads it as a value. A handle with a caller's BlackBoxFunctionSolver and a handle with
 *     ACVM_BATCH_REUSE_SLOTS are supported alike. acvm_debug_import_missing: the instances with at least one absent input after the last import.
 *   - Any other byte is refused -- the 2 of a narrow export whose value did not fit too: the buffer does not hold that value. The host cannot see
 *     the bytes beforehand, so this refusal comes behind the import: ACVM_E_INVALID, the message gives the number of offending elements and
 *     names the one of the lowest instance and, in it, the lowest position of initial_ids, and the handle is left WITHOUT initial witnesses --
 *     acvm_batch_solve is ACVM_E_STATE until another import. It is the only refusal of the call that does not leave the handle as it was.
 *   - Synchronous like the rest. What comes back from the device is three words, nothing per instance.
 *   - Every other import entry point leaves every instance holding every input again; acvm_batch_reset keeps what the last import said, as it
 *     keeps the rows.
 * acvm_batch_set_initial_witness_masked is the host form: values as acvm_batch_set_initial_witness, assigned [B][n_initial] bytes 0 / 1, both
 * staged and read by the device path above (BE32, instance-major, dense).
 * Instance-major, the mask row of an instance is read in 16-byte units where no column list is given; under a column list one byte per input.
 * Not here: a mask for acvm_batch_solve_then_import_ex (a masked import never rides behind a solve), masks for the parts of
 * acvm_batch_import_device_parts, masks for the inputs of acvm_node_solve_device, acvm_multi_* on top of a masked batch.
 */
int acvm_batch_import_device_masked(acvm_batch_t *b, const acvm_import_desc_t *d, const void *d_values, const uint8_t *d_assigned);
int acvm_batch_set_initial_witness_masked(acvm_batch_t *b, const uint8_t *values_be32, const uint8_t *assigned /* [B][n_initial] */);
uint64_t acvm_debug_import_missing(const acvm_batch_t *b);   /* instances with at least one absent input after the last import */
/*
 * One import from several buffers: fn main(msg: [u8; 64], root: Field) takes its bytes from one producer and its root, the same for every
 * instance, from another. Each part names the initial witnesses it supplies (positions in the initial_ids given to acvm_batch_new) and how
 * its buffer is to be read, exactly as a descriptor does -- plus ACVM_LAYOUT_BROADCAST: one element per column, the value of every instance.
 *   - Every initial witness must be supplied by exactly one part: a position that no part or more than one part supplies, or a position
 *     >= n_initial, is ACVM_E_INVALID and the message names the position. Every part gets the checks of acvm_batch_import_device (no part is
 *     exempt from the alignment rule). Nothing is enqueued before every part has passed: a refused call leaves the handle as it was.
 *   - Leaves the handle exactly as acvm_batch_import_device leaves it -- rows, planes and event words are written once -- and returns after the
 *     batch's stream is synchronised. At most one small host-to-device copy is made: all lists of the call in one buffer, which is reused while
 *     they do not change (acvm_debug_import_list_copies counts the copies a handle has made).
 *   - n_parts == 0 is valid only for a circuit without initial witnesses; a part with n == 0 supplies nothing.
 * Not here: an acvm_batch_solve_then_import form for parts, an asynchronous variant, parts for the inputs of acvm_node_solve_device.
 */
typedef struct {
    const void *d_values;        /* device, aligned to the element size (16 bytes for the 32-byte encodings) */
    uint32_t encoding, layout;   /* any ACVM_ENC_*; ACVM_LAYOUT_* or ACVM_LAYOUT_BROADCAST */
    const uint32_t *positions;   /* HOST, n entries: which initial witnesses (positions in initial_ids) this part supplies */
    const uint32_t *columns;     /* HOST, n entries or NULL (the k-th position reads column k; n_columns is then n) */
    uint32_t n, n_columns;
    uint64_t stride;             /* elements; 0 = dense; ignored for BROADCAST */
} acvm_import_part_t;
int acvm_batch_import_device_parts(acvm_batch_t *b, const acvm_import_part_t *parts, uint32_t n_parts);
uint64_t acvm_debug_import_list_copies(const acvm_batch_t *b);
/*
 * Record import: the initial witnesses as an array of structs. Each instance is one packed record of mixed-width fields at a fixed pitch --
 * { msg: [u8; 64], root: Field, idx: u32, flags: [bool; 8] } as a Rust #[repr(C, packed)] row, a numpy structured dtype, a database row -- and
 * every initial witness is one field of it: an encoding and a byte offset inside the record.
 *   - Addressing: instance i of the live instances reads its field at byte i * pitch + offset of d_records. d_records, pitch and the offsets
 *     may have ANY alignment (as ACVM_ENC_U8 already allows for a pointer): a 32-byte field behind 64 bytes of a 108-byte record is fine.
 *   - Decoding: exactly as acvm_batch_import_device decodes an element of that encoding -- every 256-bit string is accepted and reduced, a
 *     narrow element is the integer itself, little-endian; byte planes are filled as the typed import fills them; the event words are reset
 *     exactly once per instance, whatever the order of the fields.
 *   - Every initial witness must be supplied by exactly one field. Two positions may read the same or overlapping bytes, the fields may come
 *     in any order, and bytes of a record that no field covers are padding: they influence nothing. No load touches a 4-byte-aligned word that
 *     holds no byte of [d_records, d_records + B * pitch).
 *   - Refused with ACVM_E_INVALID, the message naming the field or the position, the handle left as it was: a null descriptor; null fields
 *     with n_fields > 0; a position >= n_initial; a position supplied twice, or never; an unknown encoding; offset + size > pitch (judged
 *     without overflow); null records while there are fields and live instances. A circuit without initial witnesses takes n_fields == 0 and
 *     reads nothing.
 *   - Leaves the handle exactly as acvm_batch_import_device leaves it and returns after the batch's stream is synchronised. At most one small
 *     host-to-device copy is made: the field table, which is reused while it does not change (acvm_debug_import_list_copies counts it).
 *     Works with ACVM_BATCH_REUSE_SLOTS (rows are not ids), with a caller's solver, and after acvm_batch_set_instances.
 * acvm_batch_set_initial_witness_records is the host form: B * pitch bytes go through the handle's staging buffer, then the device path runs.
 * Not here: a mask byte inside the record (acvm_batch_import_device_records_masked below reads one); an acvm_batch_solve_then_import form;
 * records for the lanes of acvm_node_solve_device; big-endian or sign-extending narrow fields.
 */
typedef struct {
    uint32_t position;   /* which initial witness: position in the initial_ids given to acvm_batch_new */
    uint32_t encoding;   /* any ACVM_ENC_*: BE32, LE32, MONT256_LE, U8 .. U128 */
    uint64_t offset;     /* byte offset of the element inside a record; ANY alignment */
} acvm_record_field_t;
typedef struct {
    uint64_t pitch;                       /* bytes from one record to the next; any value >= the end of the last field */
    const acvm_record_field_t *fields;    /* HOST, copied before the call returns */
    uint32_t n_fields;
} acvm_record_desc_t;
int acvm_batch_import_device_records(acvm_batch_t *b, const acvm_record_desc_t *d, const void *d_records);
int acvm_batch_set_initial_witness_records(acvm_batch_t *b, const acvm_record_desc_t *d, const void *records /* host */);
/*
 * Record export: the way out in the same form. Each instance of the range (or of a device list of instances) becomes one packed record of
 * mixed-width fields -- { digest: [u8; 32], root: Field, idx: u32, ok: bool } -- in the caller's device buffer: what the record import of the
 * next circuit reads, a database row, a Rust #[repr(C, packed)] slice. A field is a witness, an encoding, a byte offset, and optionally the
 * offset of a mask byte.
 *   - Addressing: row i writes its field at byte i * pitch + offset of d_records. d_records, pitch and every offset may have ANY alignment.
 *   - Values: byte for byte what acvm_batch_export_device writes for that witness, instance and encoding -- scaled, relaxed and recycled rows
 *     and the instances of the exact path are handled as there. A field of ACVM_ENC_MONT256_LE takes the Montgomery-256 factor table, every
 *     other field the plain one; both can be live in one call. An unassigned element is zero bytes. A witness index >=
 *     acvm_circuit_num_witnesses is unassigned. A witness may appear in several fields, say as ACVM_ENC_U8 and as ACVM_ENC_BE32.
 *   - Mask byte: for a 32-byte field 0 or 1; for a narrow field 0, 1 or 2 -- 2: assigned, but the value does not fit the width; the low bytes
 *     are written all the same.
 *   - What is never written: a byte of the buffer that no field and no mask byte covers -- not the padding inside a record, not the bytes
 *     before d_records, not the bytes behind d_records + n * pitch, even where they share an aligned dword with a covered byte. No byte of
 *     d_records is ever loaded: there is no read-modify-write of global memory.
 *   - d_instances (DEVICE) or NULL: with a list, rows are read as by acvm_batch_export_device_list -- any order, repeats allowed, an entry at or
 *     beyond the live count is an instance that assigned nothing -- and first must be 0, n the list's length. NULL: row i is instance first + i.
 *     The instances of the exact path are found through the handle's lane map, with its rule for host-to-device traffic;
 *     acvm_debug_export_h2d_bytes counts this call too.
 *   - Refused with ACVM_E_INVALID, the message naming the field, nothing enqueued: a null descriptor; null fields with n_fields > 0; an unknown
 *     encoding; offset + size > pitch or mask_offset >= pitch (judged without overflow); two covered byte ranges that overlap -- elements and
 *     mask bytes alike, unlike the import, where overlapping reads are harmless; a range beyond the live instances; first != 0 with a list; a
 *     null buffer while there is something to write.
 *   - ACVM_E_STATE exactly where acvm_batch_export_device returns it for the same witness set: not solved; a witness that was not kept under
 *     ACVM_BATCH_REUSE_SLOTS; after acvm_batch_solve_then_import.
 *   - n_fields == 0 or n == 0 writes nothing and succeeds.
 *   - Synchronous like the export. At most one small host-to-device copy is made -- the window and field tables -- which is reused while they
 *     do not change.
 * acvm_batch_witness_records is the host form: the device path runs into a zero-filled staging buffer, then n * pitch bytes are copied down.
 * Here the padding IS written, as zero.
 * Not here: a node form; an asynchronous variant; outcome columns (status, err) as record fields; big-endian or sign-extending narrow fields.
 * (The mask bytes written here are read by acvm_batch_import_device_records_masked below.)
 */
#define ACVM_RECORD_NO_MASK UINT64_MAX
typedef struct {
    uint32_t witness;      /* witness index; one >= acvm_circuit_num_witnesses is unassigned, as in the export */
    uint32_t encoding;     /* any ACVM_ENC_*: BE32, LE32, MONT256_LE, U8 .. U128 */
    uint64_t offset;       /* byte offset of the element inside a record; ANY alignment */
    uint64_t mask_offset;  /* byte offset of this field's mask byte inside the record, or ACVM_RECORD_NO_MASK */
} acvm_record_out_field_t;
typedef struct {
    uint64_t pitch;                          /* bytes from one record to the next */
    const acvm_record_out_field_t *fields;   /* HOST, copied before the call returns */
    uint32_t n_fields;
    uint32_t first, n;                       /* instances [first, first + n); with a list: first == 0, n = its length */
} acvm_record_out_desc_t;
int acvm_batch_export_device_records(acvm_batch_t *b, const acvm_record_out_desc_t *d, const uint32_t *d_instances /* DEVICE, or NULL = the range */,
                                     void *d_records);
int acvm_batch_witness_records(acvm_batch_t *b, const acvm_record_out_desc_t *d, void *records /* host, n * pitch bytes */);
/*
 * Masked record import: the record import for per-instance PARTIAL initial witness maps. A field may name a presence byte inside the record -- a
 * Rust Option<T> laid out as { valid: u8, value: T }, a nullable database column, and what the record export above writes: its field list with
 * witness -> position IS this call's field list, so the records of one circuit feed the next without a pass in between.
 *   - Values and checks: those of acvm_batch_import_device_records on (pitch, position, encoding, offset), unchanged and in the same order.
 *   - Mask byte 1: the instance holds that initial witness, with the decoded value. 0: it does not -- the row is zero afterwards, its byte-plane
 *     word is 0x80000000, the bit of (instance, position) is set in the handle's missing set, and the bytes of the absent element influence
 *     nothing, non-canonical 256-bit strings included. A field with ACVM_RECORD_NO_MASK is always held.
 *   - Any other byte is refused exactly as acvm_batch_import_device_masked refuses it -- the 2 the record export writes for a narrow value that
 *     did not fit too: behind the import, ACVM_E_INVALID, the message gives the number of offending elements (a mask byte that several fields
 *     name counts once per field) and names the one of the lowest instance and, in it, the lowest position, and the handle is left WITHOUT
 *     initial witnesses.
 *   - mask_offset >= pitch is refused on the host, naming the field, behind the checks of the unmasked call; the handle is left as it was.
 *   - Several fields may name the same mask byte (one `valid` byte for a whole struct). A mask byte may lie anywhere in the record, inside another
 *     field's bytes included; reads may overlap, as the import allows anyway.
 *   - No field has a mask: the call IS acvm_batch_import_device_records -- word for word the same tables, the same kernel, nothing else launched,
 *     and acvm_debug_import_missing is 0.
 *   - Leaves the handle exactly as acvm_batch_import_device_masked leaves it for the same values and presence bits: rows, planes, the event
 *     words reset once, every word of the missing set of the live instances rewritten (a bit of an earlier masked import does not survive),
 *     acvm_debug_import_missing. Everything behind it -- the solve of an instance with an absent input, reset, stepping, slot reuse, a caller's
 *     solver -- is what is described there. Every other import entry point leaves every instance holding every input again.
 *   - No load touches a 4-byte-aligned word that holds no byte of [d_records, d_records + B * pitch). A mask byte further than 256 bytes from its
 *     element in a longer record is read with a byte load of its own; every other one comes with the lines the element needs anyway.
 *   - Synchronous. What comes back from the device is three words, nothing per instance.
 * acvm_batch_set_initial_witness_records_masked is the host form: B * pitch bytes go through the handle's staging buffer, then the device path.
 * acvm_debug_import_state reads back what any import left: for the tests that compare two entry points bit for bit.
 * Not here: masks for acvm_node_solve_records; an acvm_batch_solve_then_import form; big-endian or sign-extending narrow fields.
 */
typedef struct {
    uint32_t position;     /* as acvm_record_field_t */
    uint32_t encoding;
    uint64_t offset;
    uint64_t mask_offset;  /* byte offset of this field's presence byte inside the record, or ACVM_RECORD_NO_MASK */
} acvm_record_masked_field_t;      /* same layout as acvm_record_out_field_t, witness -> position */
typedef struct {
    uint64_t pitch;
    const acvm_record_masked_field_t *fields;   /* HOST, copied before the call returns */
    uint32_t n_fields;
} acvm_record_masked_desc_t;
int acvm_batch_import_device_records_masked(acvm_batch_t *b, const acvm_record_masked_desc_t *d, const void *d_records);
int acvm_batch_set_initial_witness_records_masked(acvm_batch_t *b, const acvm_record_masked_desc_t *d, const void *records /* host */);
/* What the last import left on the device, copied down (each pointer may be NULL): rows [n_initial][2][B][4] words -- the two 16-byte halves of
 * each initial witness' row as the kernels keep them; planes [n_initial][B] -- the byte-plane word, 0 for an input without a plane; events
 * [2 + B] -- the two header words, then one word per live instance; missing [(n_initial + 31) / 32][B] -- the missing set, zero for a handle no
 * masked import has touched. B: the live instances. Waits for the batch's stream. */
int acvm_debug_import_state(acvm_batch_t *b, uint32_t *rows, uint32_t *planes, uint32_t *events, uint32_t *missing);

/*
 * WitnessMap wire format (acir/src/native_types/witness_map.rs:108-146; acvm_js compressWitness / decompressWitness):
 * gzip(bincode(BTreeMap<Witness, FieldElement>)), a FieldElement being its 64-character hex string.
 * decode: writes up to cap (index, canonical 32-byte big-endian value) pairs in ascending index order, returns the number of
 *         entries of the map (values are reduced like FieldElement::from_hex). Raw bincode without the gzip layer is accepted.
 * encode: returns the number of bytes of the serialised map (written if it fits cap). Same map, same bincode bytes as the
 *         reference; the gzip layer is zlib's at level 9 (any inflater reads it; the compressed bytes are not pinned).
 * acvm_batch_witness_map_bytes: the witness map of one instance as it stands (finalize() for a solved instance, the partial
 *         map otherwise), serialised.
 */
long long acvm_witness_map_decode(const uint8_t *bytes, size_t len, uint32_t *ids, uint8_t *values_be32, uint32_t cap);
long long acvm_witness_map_encode(const uint32_t *ids, const uint8_t *values_be32, uint32_t n, uint8_t *out, size_t cap);
long long acvm_batch_witness_map_bytes(acvm_batch_t *b, uint32_t instance, uint8_t *out, size_t cap);
/*
 * The same format for MANY instances, written on the device: output row i receives the serialised WitnessMap of its instance in the slot at
 * d_bytes + i * pitch, in one synchronous call without a round trip per instance.
 *   - Which entries: one per witness the instance has ASSIGNED, of the whole map or of the listed witnesses, ascending -- the entries of
 *     acvm_batch_witness_map_bytes. A failed or waiting instance gives the map as it stands; a listed witness beyond the circuit is unassigned.
 *   - Body (ACVM_WIRE_BINCODE, what acvm_witness_map_decode also accepts): u64le N, then per entry u32le witness, u64le 64 and the 64 lowercase
 *     hex characters of the canonical big-endian value. The entry of rank r lies at 8 + 76 r, the body is 8 + 76 N bytes.
 *   - ACVM_WIRE_GZIP_STORED: one gzip member around the body -- what WitnessMap::try_from(&[u8]) and every inflater read -- that does not
 *     compress, with every byte pinned: the header 1f 8b 08 08 00 00 00 00 00 ff 00 (FNAME, an empty name, MTIME 0, OS 255); the body in stored
 *     blocks of 65 532 bytes (the last one shorter), each behind its 5-byte header BFINAL, LEN, ~LEN; three empty non-final stored blocks
 *     (00 00 00 ff ff) in front of every block header but the first; CRC-32 of the body and ISIZE = its length mod 2^32. The body starts at
 *     byte 16 of the slot, and a map of N entries takes 16 + L + 20 (ceil(L / 65532) - 1) + 8 bytes, L = 8 + 76 N.
 *   - acvm_batch_wire_bound: the length of the longest map the descriptor can give -- every listed witness assigned, or every witness of the
 *     circuit -- rounded up to 16 (ACVM_WIRE_GZIP_DEFLATE: see there); negative for a null batch, a null descriptor, an unknown container.
 *   - d_lengths[i] (DEVICE, may be NULL): the bytes of row i's map.
 *   - What is never written: a byte of a slot at or behind its row's length, a byte between slots, a byte in front of d_bytes. No byte of
 *     d_bytes is loaded.
 *   - d_instances (DEVICE) or NULL: with a list, rows are read as by acvm_batch_export_device_list -- any order, repeats allowed, an entry at
 *     or beyond the live count is an instance that assigned nothing: a map of 0 entries -- and first must be 0, n the list's length.
 *   - States and host traffic: those of acvm_batch_export_device / _list for the same witness set. It answers after stepping, under the
 *     forced slow path and with instances waiting at a foreign call; under ACVM_BATCH_REUSE_SLOTS it serves kept and initial witnesses only.
 *     ACVM_E_STATE: not solved; a witness that was not kept (the whole map under slot reuse); after acvm_batch_solve_then_import. Host to
 *     device go the witness list, the plan's tables and the exact lanes' map when it changed, never anything per instance
 *     (acvm_debug_export_h2d_bytes counts it).
 *   - Refused with ACVM_E_INVALID, the message naming the cause, nothing enqueued: a null descriptor; an unknown container; a list that is
 *     not strictly ascending; a pitch below the bound or not a multiple of 16; a misaligned d_bytes; a range beyond the live instances;
 *     first != 0 with a list; a null buffer while n > 0.
 *   - acvm_batch_witness_maps_wire: the same into host memory, range form. The slots are made in the handle's staging buffer in chunks of
 *     instances and copied down once per chunk; row i's bytes [0, lengths[i]) of out + i * pitch are written, lengths must not be NULL, out
 *     needs no alignment.
 *   - ACVM_WIRE_GZIP_DEFLATE (= 8, gzip's CM byte; these three calls only, the two import calls refuse it as an unknown container): one gzip
 *     member around the body that COMPRESSES, every byte pinned, made of these pieces in order.
 *       Head: the 11 bytes 1f 8b 08 08 00 00 00 00 00 ff 00.
 *       One deflate block, BFINAL = 1, BTYPE = 10 (dynamic Huffman), LSB first as RFC 1951 packs it. Its code description is a constant of the
 *       format, 265 bits, the same in every row of every call: HLIT = 21 (278 literal/length codes), HDIST = 12 (13 distance codes), HCLEN = 14;
 *       the code-length code is STATED, not derived: symbol 16 has 1 bit, 9 has 2, 7 has 3, and 1, 5, 10, 18 have 5 each (the 18 three-bit
 *       entries in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1); the 278 + 13 lengths are one sequence cut into runs of equal
 *       lengths -- a run of n zeros: while n >= 11 one symbol 18 over min(n, 138), then while n >= 3 one symbol 17 over min(n, 10), the rest
 *       as 0s; a run of n lengths v > 0: v itself, then while 3 or more remain one symbol 16 over min(remaining, 6) (the longest repeat
 *       first: 7 remaining are 6 + v), the rest as v.
 *       Literal/length code, canonical over symbols 0..277: the 16 bytes '0'-'9' 'a'-'f' 5 bits; symbols 257..277 (match lengths 3..82) 7 bits;
 *       the remaining 241 symbols (the other 240 literals and end-of-block) in ascending order: the first 103 get 9 bits, the rest 10. The
 *       Kraft sum is exactly 1: 16/32 + 21/128 + 103/512 + 138/1024.
 *       Distance code: symbol 0 (distance 1) and symbol 12 (distances 65..96, 5 extra bits, 76 is extra 11), one bit each.
 *       Token stream, a function of the body alone: the 8 count bytes as 8 literals; then each entry (rank e, its 76 bytes cur, prev = the entry
 *       of rank e - 1) parsed greedily from p = 0: L76 = the run of positions from p on with cur[q] == prev[q] (0 when e = 0), L1 = the run
 *       with cur[q] == cur[q - 1] (0 when p = 0); if max(L76, L1) >= 3 a match of that length with distance 76 if L76 >= L1, else distance
 *       1, and p advances by the length; otherwise the literal cur[p]. No token spans two entries. Then end-of-block; the last byte is
 *       zero-padded.
 *       Trailer: CRC-32 of the body and ISIZE = its length mod 2^32, little-endian, at the next BYTE: generally not dword-aligned.
 *     Bound (acvm_batch_wire_bound): the block is at most 265 + 8 * 10 + n_positions * (12 * 10 + 64 * 5) + 10 bits -- no match costs more
 *     than the literals it replaces: at most 7 + 4 + 1 + 5 = 17 bits against 5 per byte -- and the member 11 + ceil(bits / 8) + 8 bytes,
 *     rounded up to 16: about 0.72 of the stored container's. d_lengths[i] is the member's length; a row that names no instance is a map of
 *     0 entries, 63 bytes. Descriptor, pitch and alignment rule, states, refusals, what is never written or loaded and the host-to-device
 *     traffic (the plan's tables, 1 384 bytes of code table among them) are the other containers'. The position inside a row is 64-bit.
 * Not here: a node form, an asynchronous variant (the way back in is acvm_batch_import_device_wire_gzip, below), adaptive codes or longer match distances, any change to
 * acvm_batch_witness_map_bytes. A body of 4 GiB or more wraps ISIZE as gzip defines it. A packed output with an offsets column instead of a
 * pitch is acvm_batch_witness_maps_wire_packed_device, below; these three calls are as they were.
 */
enum { ACVM_WIRE_BINCODE = 0,        /* the bincode body alone */
       ACVM_WIRE_GZIP_STORED = 1,    /* one gzip member around it, stored blocks */
       ACVM_WIRE_GZIP_DEFLATE = 8 }; /* one gzip member around it, one dynamic-Huffman block (export only; the value is gzip's CM byte) */
typedef struct {
    uint32_t container;
    uint32_t first, n;           /* instances [first, first + n); with a list: first == 0, n = its length */
    const uint32_t *witnesses;   /* HOST, strictly ascending, or NULL = the whole map */
    uint32_t n_witnesses;
    uint64_t pitch;              /* bytes from one instance's slot to the next; 0 = the bound; a multiple of 16 */
} acvm_wire_desc_t;
long long acvm_batch_wire_bound(const acvm_batch_t *b, const acvm_wire_desc_t *d);
int acvm_batch_witness_maps_wire_device(acvm_batch_t *b, const acvm_wire_desc_t *d, const uint32_t *d_instances /* DEVICE or NULL */,
                                        void *d_bytes /* DEVICE, 16-byte aligned */, uint64_t *d_lengths /* DEVICE [n], may be NULL */);
int acvm_batch_witness_maps_wire(acvm_batch_t *b, const acvm_wire_desc_t *d, uint8_t *out /* host, n * pitch */, uint64_t *lengths /* host [n] */);
/*
 * The way back in: the same bytes READ on the device as per-instance, possibly partial, initial witness maps. The reference starts an execution
 * from them -- executeCircuit takes the initial WitnessMap, and decompressWitness / WitnessMap::try_from(&[u8]) (witness_map.rs:121-146) is how
 * one arrives from a file or another process. Instance j's map is the slot at d_bytes + j * pitch.
 *   - Container, alignment and pitch rule are the export's: the buffer acvm_batch_witness_maps_wire_device wrote is this call's input with no
 *     pass in between. Body: u64le N, then per entry u32le witness, u64le 64 and 64 hex characters, the entry of rank r at body byte 8 + 76 r;
 *     ACVM_WIRE_GZIP_STORED: the pinned stored-block member described above, the body from byte 16 on with 20 bytes of joint in front of
 *     every block but the first.
 *   - An entry's value is the 32 bytes its 64 characters spell, EITHER letter case (hex::decode takes both), reduced mod p like
 *     FieldElement::from_hex -> from_be_bytes_reduce (generic_ark.rs:263-283): a string >= p is legal input.
 *   - A witness the row names is held with that value. An initial witness of the handle the row does not name is ABSENT, as for a mask byte 0 of
 *     acvm_batch_import_device_masked: the row is zero, the plane word 0x80000000, the bit set in the missing set. The handle is left exactly as
 *     acvm_batch_import_device_masked leaves it for the same values and presence -- rows and planes, the event words reset once, every word of
 *     the missing set of the live instances rewritten, acvm_debug_import_missing -- and everything behind it is as documented there: solve,
 *     reset, stepping, slot reuse, a caller's solver. When every row names every initial witness the missing set is empty and none of the three
 *     missing-set passes behind the schedule is launched.
 *   - d_lengths[j] (DEVICE, may be NULL) must be the bytes of a map of N_j entries exactly: the reference refuses trailing bytes. With NULL
 *     the row's own count word gives the length.
 *   - The bytes are untrusted. No load touches a byte outside [d_bytes, d_bytes + B * pitch); within a slot nothing at or behind
 *     min(derived length, pitch) influences anything. N is judged before any entry of the row is read: the map's bytes must fit the pitch, and
 *     N <= n_initial (which follows from the key rule, so the grid is sized by n_initial and never by a value read from the device).
 *   - Findings, which only the device can see, each with a class code:
 *       1  the count word cannot be a map of this slot: too long for the pitch, more than n_initial entries, or not what d_lengths[j] says
 *       2  an entry's length word is not 64
 *       3  a character that is not a hex digit -- a string starting 0x is one: 64 characters with that prefix are 31 bytes in the reference,
 *          a shape the device form does not read
 *       4  a key that is not an initial witness of this handle
 *       5  keys not strictly ascending: every BTreeMap serialiser writes them ascending, and a repeat ("last one wins" in serde) has no
 *          parallel meaning
 *       6  GZIP_STORED: a head, joint, ISIZE or block-header word that is not the pinned one for this body length
 *       7  GZIP_STORED: the trailer's CRC-32 is not the body's
 *     A row with a class-1 finding reads no entries and has exactly that one; an entry gives its lowest class; a row gives 6 or else 7. Any
 *     finding is ACVM_E_INVALID: the message gives the number of findings and names the smallest (instance, class, entry rank), and the handle
 *     is left WITHOUT initial witnesses -- acvm_batch_solve is ACVM_E_STATE until another import. Nothing per instance comes back: a few words.
 *   - Refused on the host with ACVM_E_INVALID, nothing enqueued, the handle as it was: a null batch or descriptor; an unknown container; a
 *     pitch that is 0 or not a multiple of 16; a misaligned d_bytes; a null buffer with B > 0.
 *   - Synchronous, like every import.
 * acvm_batch_set_initial_witness_maps_wire is the host form: row j is bytes[j * pitch, + lengths[j]), pitch and alignment of any kind. A row
 * starting 1f 8b is inflated with zlib -- real deflate streams, what compressWitness writes, not only stored blocks; any other row is the raw
 * bincode body. A row in canonical shape (every length word 64, no 0x prefix, keys strictly ascending) is staged as it is; any other row goes
 * through the reader and the writer of acvm_witness_map_decode / _encode, so everything WitnessMap::try_from accepts is accepted with the same
 * meaning: strings of another length, prefixes, unordered and repeated keys, last one wins. A row the reader rejects -- a corrupt gzip stream, bad hex,
 * trailing bytes -- a key that is not an initial witness, or a map with more entries than fit is refused before anything is enqueued, the
 * message naming the instance and the reader's text; the handle stays as it was. Then the bodies go through the staging buffer as
 * ACVM_WIRE_BINCODE slots and the device path runs.
 * Not here: a node form, an acvm_batch_solve_then_import form, an asynchronous variant (compressed deflate is inflated on the device by
 * acvm_batch_import_device_wire_gzip, below; these two calls are as they were), keys
 * outside the handle's initial id set (the reference's ACVM::new would take them; here the plan is keyed by the initial ids). A per-row offset
 * column instead of a pitch is acvm_batch_import_device_wire_packed, below.
 */
typedef struct {
    uint32_t container;   /* ACVM_WIRE_BINCODE or ACVM_WIRE_GZIP_STORED: what every slot holds */
    uint64_t pitch;       /* bytes from one instance's slot to the next; a multiple of 16 */
} acvm_wire_in_desc_t;
int acvm_batch_import_device_wire(acvm_batch_t *b, const acvm_wire_in_desc_t *d, const void *d_bytes /* DEVICE, 16-byte aligned */,
                                  const uint64_t *d_lengths /* DEVICE [B] or NULL */);
int acvm_batch_set_initial_witness_maps_wire(acvm_batch_t *b, const uint8_t *bytes /* host */, uint64_t pitch /* any */,
                                             const uint64_t *lengths /* host [B], required */);
/*
 * The gzip import: every instance's map as one gzip member (RFC 1952) around its bincode body, INFLATED ON THE DEVICE -- one row per lane, every
 * row of the batch in flight together. What acvm_batch_witness_maps_wire_device(ACVM_WIRE_GZIP_DEFLATE) or (ACVM_WIRE_GZIP_STORED) left in device
 * memory is this call's input with no pass in between, and so is what compressWitness writes (GzEncoder, Compression::best(): dynamic-Huffman
 * blocks, witness_map.rs:109-146) or any other deflater: the inflater reads every RFC 1951 stream.
 *   - The slot at d_bytes + j * pitch holds instance j's member; row j reads only bytes [0, min(d_lengths[j], pitch)) of its slot (NULL
 *     lengths: pitch). Any mix and number of stored, fixed and dynamic blocks, distances up to 32 768. FLG may carry FEXTRA, FNAME, FCOMMENT
 *     and FHCRC (checked as zlib checks it); MTIME, XFL and OS are not looked at; bytes behind the trailer are ignored, as GzDecoder ignores
 *     them. The acceptance rules are zlib's.
 *   - The inflated body must be a canonical body of the handle: it is read as an ACVM_WIRE_BINCODE slot by acvm_batch_import_device_wire's
 *     kernels, the inflater's own output length serving as that row's d_lengths -- so trailing body bytes are a class-1 finding there. When every
 *     row passes the handle is left bit for bit as acvm_batch_import_device_wire(ACVM_WIRE_BINCODE) leaves it for the same bodies.
 *   - Two stages with one host synchronisation between them. Stage 1 inflates into scratch and writes nothing of the handle. Its findings are a
 *     class space of their own; a row's reader is sequential and stops at its first, so a row has at most one, and with it goes the number of
 *     block headers read so far (0 inside the head):
 *       1  HEAD      bytes 0..2 are not 1f 8b 08; a reserved FLG bit is set; FHCRC is not the header's CRC-32 mod 2^16
 *       2  BLOCK     BTYPE 3
 *       3  STORED    LEN is not ~NLEN
 *       4  CODES     a dynamic block's description that zlib refuses: HLIT > 29 or HDIST > 29; a code-length code that is over-subscribed or
 *                    incomplete; repeat 16 with no length before it; a repeat past HLIT + HDIST + 258; symbol 256 without a code; a
 *                    literal/length or distance set that is over-subscribed, or incomplete unless its longest code has 1 bit (an all-zero
 *                    distance set is legal)
 *       5  SYMBOL    bits that are no code of an incomplete set; literal/length symbols 286 / 287; distance symbols 30 / 31
 *       6  DISTANCE  a distance beyond the bytes written so far
 *       7  INPUT     the row's readable bytes end before the head, the final block or the 8 trailer bytes do
 *       8  OUTPUT    more output than the handle's longest body, 8 + 76 * n_initial
 *       9  CRC       the trailer's CRC-32 is not the output's
 *       10 ISIZE     the trailer's ISIZE is not the output's length mod 2^32 (checked after the CRC, as zlib does)
 *     Any of them is ACVM_E_INVALID: the message ("wire inflate: ...") gives the number of findings and the smallest (instance, class, block),
 *     and the handle stays AS IT WAS -- a previous import still solves. Stage 2 is the body import over the scratch; its findings, its message
 *     ("wire import: ...") and its "left without initial witnesses" rule are acvm_batch_import_device_wire's.
 *   - Refused on the host with ACVM_E_INVALID, nothing enqueued, the handle as it was: a null batch or descriptor; a container other than
 *     ACVM_WIRE_GZIP_DEFLATE; a pitch that is 0 or not a multiple of 16; a misaligned d_bytes; a null buffer with B > 0; more than 2^27 instances.
 *   - Host-to-device traffic: the body import's tables and 736 bytes of fixed code table; nothing per instance either way. The staging arena
 *     holds the scratch slots (the handle's longest body each, rounded up to 16) and 900 bytes of code tables per instance. Synchronous.
 * acvm_batch_set_initial_witness_maps_gzip is the host form: row j is bytes[j * pitch, + lengths[j]), pitch and alignment of any kind. The rows go up
 * as they are, COMPRESSED, at a 16-aligned pitch, then the device form runs: no host thread inflates anything. Also refused on the host: null
 * lengths, a row that does not start 1f 8b. A body that is not in canonical shape is a finding here;
 * acvm_batch_set_initial_witness_maps_wire, which inflates on the host and rewrites such bodies, remains the route for those.
 * acvm_debug_inflate_rows runs the shipped inflater through its launcher on n rows of the caller's, no handle: bytes that need not be witness
 * maps. out ([n][out_cap], out_cap a multiple of 4) goes up as it is and comes back with row i's bytes in front, so what the kernel leaves
 * alone is seen to be left alone; out_lengths[i] the bytes stored, findings[2 i], [2 i + 1] the class (0: none) and the block count, crcs
 * (may be NULL) the CRC-32 of the bytes stored. lengths may be NULL (pitch).
 * Not here: a node form, an acvm_batch_solve_then_import form, an asynchronous variant, raw-deflate or zlib wrappers, multi-member files
 * within one row (a packed buffer of one member per row is acvm_batch_import_device_wire_packed, below),
 * bodies outside canonical shape on the device, parallel decoding within one row.
 */
int acvm_batch_import_device_wire_gzip(acvm_batch_t *b, const acvm_wire_in_desc_t *d /* container must be ACVM_WIRE_GZIP_DEFLATE */,
                                       const void *d_bytes /* DEVICE, 16-byte aligned */, const uint64_t *d_lengths /* DEVICE [B] or NULL */);
int acvm_batch_set_initial_witness_maps_gzip(acvm_batch_t *b, const uint8_t *bytes /* host */, uint64_t pitch /* any */,
                                             const uint64_t *lengths /* host [B], required */);
int acvm_debug_inflate_rows(const uint8_t *rows /* host */, uint64_t pitch, const uint64_t *lengths, uint32_t n, uint64_t out_cap,
                            uint8_t *out /* host [n][out_cap] */, uint64_t *out_lengths, uint32_t *findings /* [n][2]: class, block */, uint32_t *crcs);
/*
 * PACKED wire buffers: an offsets column in place of the pitch. Row i occupies bytes [offsets[i], offsets[i + 1]) of one buffer, offsets[0] = 0,
 * no byte between rows -- memory in proportion to what is written, not to acvm_batch_wire_bound. A packed buffer of gzip members is, byte for
 * byte, one multi-member .gz file (gzip.decompress reads it in one call).
 * acvm_batch_witness_maps_wire_packed_device: the export. The descriptor is acvm_wire_desc_t with pitch == 0; all three containers, range and
 * list form; the rows are byte for byte those of acvm_batch_witness_maps_wire_device, whose kernels make them in the handle's staging arena in
 * chunks -- whole blocks of 64 rows, at most 64 MiB of slots -- behind which each chunk's lengths are scanned into the offsets (the running
 * base stays in a device word) and its rows packed into d_bytes. Device memory taken is the chunk and the tables, never n * bound.
 *   - What is written: d_offsets[0 .. n], always; *total = offsets[n]; *n_fit = the leading rows with offsets[i + 1] <= capacity; rows below
 *     n_fit complete.
 *   - What is never written or loaded: a byte of d_bytes at or behind offsets[n_fit], a byte in front of d_bytes; no byte of d_bytes is loaded,
 *     none is read-modify-written, and rows that share a dword each store their own bytes.
 *   - d_bytes == NULL with capacity == 0 is the sizing call: the offsets, total, nothing else. It costs a full encode -- for
 *     ACVM_WIRE_GZIP_DEFLATE a member's length is known only once it is made; the other containers run the same launches. A caller whose
 *     buffer was too small continues with the list form on the remaining instances.
 *   - States, refusals and host-to-device traffic: those of acvm_batch_witness_maps_wire_device; nothing per instance crosses the bus. Also
 *     refused with ACVM_E_INVALID, nothing enqueued: a descriptor pitch other than 0; null offsets; a null buffer with a capacity.
 *   - acvm_batch_witness_maps_wire_packed: the same into host memory, range form; out needs no alignment (NULL with capacity 0: sizing). Per
 *     chunk the rows are packed on the device and the chunk's packed range comes down in one copy straight to out + its base: no slot bytes
 *     behind a row's length cross the bus and no row is moved on the host.
 * acvm_batch_import_device_wire_packed: the way back in. d->container: any of the three (ACVM_WIRE_GZIP_DEFLATE takes
 * acvm_batch_import_device_wire_gzip's path, the others acvm_batch_import_device_wire's); d->pitch: the staging pitch, a nonzero multiple of 16
 * and so the longest row accepted. The call needs B * pitch bytes of staging in device memory, which the handle keeps.
 *   - The offsets are untrusted device data. They are judged and the rows unpacked into the staging slots first, which writes nothing of the
 *     handle; no load touches a byte outside [d_bytes, d_bytes + n_bytes) -- a buffer may end in mid-dword -- and there is one host
 *     synchronisation. Findings, a class space of their own:
 *       1  offsets[j + 1] < offsets[j]
 *       2  offsets[j + 1] > n_bytes
 *       3  a row longer than the pitch
 *     A row with a finding is not copied. Any finding is ACVM_E_INVALID: the message ("wire offsets: ...") gives the number of findings and the
 *     smallest (instance, class), and the handle stays AS IT WAS -- a previous import still solves.
 *   - Then the device import of the container runs over the slots with the rows' lengths as its d_lengths; its findings, its messages and its
 *     "left without initial witnesses" rule are unchanged, and on success the handle is bit for bit what the pitched import leaves for the
 *     same rows (acvm_debug_import_state).
 *   - Refused on the host, nothing enqueued, the handle as it was: what the pitched import of the container refuses; null offsets with B > 0.
 * acvm_debug_wire_repitch runs the shipped scan and repitch kernels through their launchers on host rows of the caller's, any bytes at any
 * lengths, zero included; no handle. unpack == 0: rows ([n][pitch], any pitch) and lengths give packed and offsets [n + 1], the scan run in
 * chunks of scan_chunk rows (0: one chunk), a row copied when it ends at or in front of capacity (<= packed_bytes); result = {total, n_fit}.
 * unpack != 0: packed and offsets give rows, lengths (0 for a row with a finding) and findings [n] (the class, 0: none); result = {the count
 * of findings, the key of the smallest (instance, class): ~(instance << 4 | class)}. displacement 0 .. 15: the packed buffer's device address
 * mod 16. Both buffers go up as given and come back whole, so that what the kernels leave alone is seen to be left alone.
 * Not here: a host form of the packed import, a node form, an acvm_batch_solve_then_import form, an asynchronous variant.
 */
int acvm_batch_witness_maps_wire_packed_device(acvm_batch_t *b, const acvm_wire_desc_t *d, const uint32_t *d_instances /* DEVICE or NULL */,
                                               void *d_bytes /* DEVICE, 16-byte aligned, may be NULL */, uint64_t capacity, uint64_t *d_offsets /* DEVICE [n + 1] */,
                                               uint64_t *total, uint32_t *n_fit /* either may be NULL */);
int acvm_batch_witness_maps_wire_packed(acvm_batch_t *b, const acvm_wire_desc_t *d, uint8_t *out /* host, may be NULL */, uint64_t capacity,
                                        uint64_t *offsets /* host [n + 1] */, uint64_t *total, uint32_t *n_fit);
int acvm_batch_import_device_wire_packed(acvm_batch_t *b, const acvm_wire_in_desc_t *d, const void *d_bytes /* DEVICE, 16-byte aligned */,
                                         uint64_t n_bytes, const uint64_t *d_offsets /* DEVICE [B + 1] */);
int acvm_debug_wire_repitch(uint32_t unpack, uint32_t n, uint64_t pitch, uint8_t *rows /* host [n][pitch] */, uint64_t *lengths /* [n] */,
                            uint8_t *packed /* host [packed_bytes] */, uint64_t packed_bytes, uint32_t displacement, uint64_t *offsets /* [n + 1] */,
                            uint64_t capacity, uint32_t scan_chunk, uint32_t *findings /* [n], unpack only */, uint64_t *result /* [2] */);


/*
 * The Rust call shape for ONE instance: struct ACVM (acvm/src/pwg/mod.rs:129-143) as a handle over a batch of one,
 * so that an `impl` of ACVM in Rust forwards method by method.
 *   acvm_new                      ACVM::new(backend, opcodes, initial_witness)  mod.rs:146-156 (opcodes = the circuit's)
 *   acvm_solve / acvm_solve_opcode  ACVM::solve :236-241 / ::solve_opcode :243-303; both return the ACVM_STATUS_* reached
 *   acvm_get_status               the ACVMStatus incl. the OpcodeResolutionError (acvm_result_t)
 *   acvm_instruction_pointer      :171
 *   acvm_witness_map              ACVM::witness_map :161: up to cap (index, 32-byte big-endian value) pairs ascending; returns the map's size
 *   acvm_finalize                 ACVM::finalize :176-181: the same, but ACVM_E_STATE unless the status is Solved (the reference panics)
 *   acvm_get_pending_foreign_call / acvm_resolve_pending_foreign_call   :203-228, same conventions as the batch calls
 */
typedef struct acvm_instance acvm_t;
acvm_t *acvm_new(const acvm_circuit_t *c, const acvm_bb_solver_t *backend, const uint32_t *initial_ids, const uint8_t *values_be32,
                 uint32_t n_initial);
void acvm_free(acvm_t *a);
int acvm_solve(acvm_t *a);
int acvm_solve_opcode(acvm_t *a);
int acvm_get_status(acvm_t *a, acvm_result_t *out);
uint32_t acvm_instruction_pointer(acvm_t *a);
long long acvm_witness_map(acvm_t *a, uint32_t *ids, uint8_t *values_be32, uint32_t cap);
long long acvm_finalize(acvm_t *a, uint32_t *ids, uint8_t *values_be32, uint32_t cap);
int acvm_get_pending_foreign_call(acvm_t *a, acvm_foreign_call_info_t *info);
int acvm_pending_foreign_call_inputs(acvm_t *a, uint32_t *lens, uint8_t *values_be32);
int acvm_resolve_pending_foreign_call(acvm_t *a, uint32_t n_values, const uint8_t *is_array, const uint32_t *lens, const uint8_t *values_be32);

/*
 * ACVM::new takes ANY WitnessMap (mod.rs:146); acvm_batch_new wants one id set for all instances because the circuit is
 * levelised against it. acvm_multi_* lifts that: instance i assigns the ids[offsets[i] .. offsets[i + 1]) (values_be32 in the
 * same order, 32 bytes each); instances with the same id SET share one levelised batch, results come back in the caller's
 * instance order. Everything else is the batch API with an instance index.
 */
typedef struct acvm_multi acvm_multi_t;
acvm_multi_t *acvm_multi_new(const acvm_circuit_t *c, const acvm_bb_solver_t *solver, uint32_t n_instances, const uint64_t *offsets /*[n + 1]*/,
                             const uint32_t *ids, const uint8_t *values_be32);
void acvm_multi_free(acvm_multi_t *m);
uint32_t acvm_multi_num_groups(const acvm_multi_t *m);
int acvm_multi_solve(acvm_multi_t *m); /* number of instances not Solved */
int acvm_multi_results(acvm_multi_t *m, acvm_result_t *out /*[n_instances]*/);
/* witness map of one instance: assigned [n_witnesses], values_be32 [n_witnesses][32]; n_witnesses = acvm_multi_num_witnesses */
uint32_t acvm_multi_num_witnesses(const acvm_multi_t *m);
int acvm_multi_witness_map(acvm_multi_t *m, uint32_t instance, uint8_t *assigned, uint8_t *values_be32);
/* the batch handle and the index inside it that serve `instance` (foreign calls, digests, ... go through the batch API) */
acvm_batch_t *acvm_multi_locate(acvm_multi_t *m, uint32_t instance, uint32_t *index_in_batch);


/*
 * The node-level driver: ONE call solves a global batch of instances of one circuit on every GPU of the node. It stands
 * for the loop a caller of the reference runs once per instance -- ACVM::new, solve, finalize or the error string, the return
 * witnesses (acvm_js/src/execute.rs:60-119, public_witness.rs:10-21) -- and owns what that loop needs on this hardware: the split of the
 * batch over the devices (contiguous, no exchange step), tiles inside a device (a 10k-gate circuit at 2^20 instances is 335 GB of
 * witness table), pinned staging with the upload of tile k + 1 beside the solve of tile k, the exact re-solve of diverging instances
 * beside the next tile, one host thread + one handle + one stream set per device.
 *   acvm_node_new    one batch handle of tile_instances instances per listed device (a device may be listed twice: two handles driven by
 *                    two host threads). keep_ids: the witnesses returned per instance (normally ACVM_SET_RETURN_VALUES).
 *   acvm_node_solve  values_be32 [n_instances][n_initial][32] in host memory (pageable is fine); any of the outputs may be NULL:
 *                    results [n_instances], kept_be32 [n_instances][n_keep][32] (zeros where unassigned), kept_assigned [n_instances][n_keep],
 *                    digests32 [n_instances][32] (acvm_batch_digest's definition). Returns the number of instances not Solved, or a
 *                    negative error. The handle is reusable: call it again with the next global batch.
 */
typedef struct acvm_node acvm_node_t;
typedef struct {
    uint32_t n_devices;       /* 0 = every visible device */
    const int *devices;       /* n_devices indices, NULL = 0 .. n_devices - 1 */
    uint32_t tile_instances;  /* instances per handle; 0 = the largest power of two <= 2^17 whose tables fit the device */
    uint32_t batch_flags;     /* ACVM_BATCH_* of the handles */
} acvm_node_opts_t;
typedef struct {
    uint32_t n_devices, tile_instances;
    uint64_t n_instances;
    double total_ms;            /* wall clock of the last acvm_node_solve / acvm_node_solve_device */
    int device[16];
    uint32_t async_exact[16];   /* 1: the handle re-solves diverging instances beside the next tile */
    uint32_t tiles[16], exact_instances[16];
    double lane_ms[16];         /* wall clock of the device's thread */
    double solve_device_ms[16]; /* HIP-event time of its solves */
    double h2d_wait_ms[16];     /* what of the uploads the solves did not cover */
    double export_ms[16];       /* results, kept witnesses and digests leaving the device */
    /* host placement (ABI 5): the device's NUMA node (/sys/bus/pci/devices/<bus id>/numa_node, -1 unknown) and the CPUs its lane's two host
     * threads are pinned to (local_cpulist: how many, and the first one; 0 / -1 = not pinned) */
    int numa_node[16];
    uint32_t n_cpus_pinned[16];
    int first_cpu[16];
    /* creation (ABI 6): how often acvm_node_new levelised the circuit (1, or 0 when the circuit's plan cache already held this plan -- the plan
     * is immutable and shared by every lane's handle), its wall clock, the planner's own time, and the process's resident set at the call */
    uint32_t plans_built;
    double create_ms, plan_ms;
    uint64_t host_rss_bytes;
} acvm_node_stats_t;
acvm_node_t *acvm_node_new(const acvm_circuit_t *c, const acvm_bb_solver_t *solver, const uint32_t *initial_ids, uint32_t n_initial,
                           const uint32_t *keep_ids, uint32_t n_keep, const acvm_node_opts_t *opts);
void acvm_node_free(acvm_node_t *n);
uint32_t acvm_node_tile_instances(const acvm_node_t *n);
uint32_t acvm_node_num_devices(const acvm_node_t *n);
long long acvm_node_solve(acvm_node_t *n, uint64_t n_instances, const uint8_t *values_be32, acvm_result_t *results, uint8_t *kept_be32,
                          uint8_t *kept_assigned, uint8_t *digests32);
/* acvm_node_solve with the inputs as host records (acvm_batch_import_device_records): n_instances records at in->pitch. The upload thread stages
 * and uploads m * pitch bytes per tile in place of m * n_initial * 32 and the tile is imported through the record plan; outputs, the exact path
 * beside the next tile, the foreign-call handler and the stats are those of acvm_node_solve. The descriptor is checked once, before any lane
 * starts: a refused call (ACVM_E_INVALID) starts nothing and leaves the node usable. A pitch above 32 * n_initial is refused too: the staging
 * slots are sized for the 32-byte form at acvm_node_new, and a wider record gains nothing. */
long long acvm_node_solve_records(acvm_node_t *n, uint64_t n_instances, const acvm_record_desc_t *in, const void *records /* host */,
                                  acvm_result_t *results, uint8_t *kept_be32, uint8_t *kept_assigned, uint8_t *digests32);
int acvm_node_stats(acvm_node_t *n, acvm_node_stats_t *out);
/*
 * acvm_node_solve for a producer and a consumer that live on the GPUs: every lane (one per handle of the node, in the order of the device list)
 * reads its initial witnesses from, and writes its outcomes into, DEVICE memory of its own device. No value crosses PCIe in either direction.
 *   - The caller decides the split: lane l solves rows 0 .. n - 1 of ITS buffers, in tiles of acvm_node_tile_instances. n == 0: the lane idles and
 *     none of its pointers is read. There is no global numbering: d_selected holds row numbers of the lane's own buffers.
 *   - d_values / in: read per tile as acvm_batch_import_device reads them; row i runs over the lane's n, a stride of 0 is dense over n.
 *   - d_kept / d_kept_assigned: element (i, k), k = position in the node's keep_ids, in any ACVM_ENC_* and either layout, kept_stride in elements
 *     (0 = dense over n): what acvm_batch_export_device of a plain batch writes, mask bytes 0 / 1 / 2 and zero bytes for unassigned elements
 *     included. BE32, instance-major, dense is byte for byte the lane's slice of acvm_node_solve's kept_be32 / kept_assigned.
 *   - d_status / d_err / d_opcode_index [n]: the columns of acvm_batch_outcomes_device; d_digests32 [n][32]: acvm_batch_digest's definition.
 *   - select_mask / d_selected ([n] capacity): the ascending row numbers whose status is in the mask; n_selected is counted whether or not
 *     d_selected is given. not_solved: the lane's rows that did not reach Solved. Both are written by the call.
 *   - Every output may be NULL. Bytes outside the described elements are never written. The buffers must not be touched during the call; the call
 *     returns after every lane's streams are synchronised, and every call reads the inputs anew.
 *   - Every lane gets the checks of acvm_batch_import_device and acvm_batch_export_device (shape, alignment, stride against n, column range)
 *     before ANY lane starts; also refused (ACVM_E_INVALID, the message names the lane): null inputs with n > 0 and initial witnesses, a mask
 *     without d_kept, n >= 2^32, n_lanes != acvm_node_num_devices. A refused call starts nothing and leaves the node usable.
 *   - The exact path of tile k still runs beside tile k + 1 (acvm_node_stats async_exact); its rows are written into the caller's buffers on the
 *     device when its outcome is collected, one tile later.
 *   - Returns the total number of rows not Solved, or a negative error. acvm_node_stats describes the last call of either form.
 * acvm_debug_node_io_bytes: the cumulative bytes the device form's own code copied for that lane, host to device (column list, the lanes and
 * records of the instances of the exact path) and back (the selection's count): nothing of it grows with n. The solve's own bookkeeping (the
 * event words of a tile that flagged instances, the exact lanes' result records) is the batch's and is not counted.
 * Not here: an asynchronous (caller-stream) variant, parts and broadcast columns for the inputs, whole-map outputs (keep_ids only), dense
 * compaction of the solved rows across tiles.
 */
typedef struct {
    uint64_t n;                  /* instances of this lane = rows 0 .. n-1 of every buffer below; 0: the lane idles. n < 2^32 */
    const void *d_values;        /* initial witnesses on the lane's device, read as acvm_batch_import_device reads them */
    acvm_import_desc_t in;       /* encoding, layout, columns, n_columns, stride; row i runs over the lane's n; stride 0 = dense over n */
    void *d_kept; uint8_t *d_kept_assigned;                    /* element (i, k), k = position in the node's keep_ids; may be NULL */
    uint32_t kept_encoding, kept_layout; uint64_t kept_stride; /* any ACVM_ENC_*, instance- or witness-major, 0 = dense over n */
    uint8_t *d_status, *d_err; uint32_t *d_opcode_index;       /* [n] each, may be NULL: the columns of acvm_batch_outcomes_device */
    uint8_t *d_digests32;        /* [n][32], acvm_batch_digest's definition; may be NULL */
    uint32_t select_mask; uint32_t *d_selected;                /* [n] capacity: ascending ROW numbers i whose status is in the mask; may be NULL */
    uint64_t n_selected, not_solved;                           /* written by the call */
} acvm_node_lane_io_t;
long long acvm_node_solve_device(acvm_node_t *n, acvm_node_lane_io_t *lanes, uint32_t n_lanes); /* n_lanes == acvm_node_num_devices */
int acvm_debug_node_io_bytes(const acvm_node_t *n, uint32_t lane, uint64_t *h2d, uint64_t *d2h);
/*
 * A foreign-call handler of the node: the round trip of acvm_js/src/execute.rs:109-113 -- while the status is RequiresForeignCall, ask the handler,
 * resolve_pending_foreign_call (pwg/mod.rs:203-228), solve again -- once per TILE and site instead of once per instance. Both node forms run the
 * same loop behind a tile's solve and before anything of that tile is exported:
 *   while the tile's handle lists sites (acvm_batch_foreign_call_sites) and the round is below max_rounds: for every site ascending, the inputs of
 *   its waiting list are written into scratch of the lane (acvm_batch_foreign_call_inputs_device, in the handler's in_encoding / in_layout, dense:
 *   n_rows x max_values), the handler is called, and its answer is resolved through acvm_batch_resolve_foreign_calls_device_rows; after all sites
 *   of the round the tile is solved again. The tile's results, kept witnesses, outcome columns and digests are then those of the last solve.
 *   - The handler returns 0: answered (optionally per row: row_lens as d_lens, answered as d_answered of the per-row call; a row whose `answered`
 *     byte is 0 keeps waiting and is listed again in the next round). 1: the site is declined for this tile -- its rows stay RequiresForeignCall
 *     (a reference status: the caller stopped answering) and the site is not asked about again in this tile. A negative value aborts the node
 *     call: it returns that value and the error text names lane, tile and site; the node stays usable. Any other value is ACVM_E_INVALID.
 *   - A round that resumed no row (every site declined or fully masked out) ends the loop: no further solve runs. Rows that still wait when
 *     max_rounds rounds have run are counted in rows_left_waiting.
 *   - ACVM_SPACE_DEVICE: every pointer of `in` and values / row_lens / answered of `out` are memory of the lane's device, which is the current
 *     device of the calling thread. The handler's own GPU work must be complete when it returns (the resolve runs on the batch's stream), and its
 *     answer buffers must stay valid until it is next called on that lane or the node call returns. No value crosses PCIe: per site and round
 *     the round trip moves the 8 bytes per waiting row of the batch-wide calls, the mask bytes when `answered` is given, and a few words.
 *     ACVM_SPACE_HOST: the node copies rows, lens, values and mask down into host buffers of its own (valid during the handler's call) and
 *     uploads the answer's values, row_lens and answered into its scratch; the same device calls follow.
 *   - The handler runs on the lane's host thread; different lanes call it concurrently: it must be thread-safe. It must not start a node call.
 *   - Scratch is grown on demand; a failed allocation ends the lane with ACVM_E_NOMEM and leaves the handle reusable.
 *   - acvm_node_set_foreign_call_handler(n, NULL): no handler, the node returns rows in RequiresForeignCall as without this call. Refused, nothing
 *     changed: ACVM_E_INVALID for a null fn, an unknown space, in_encoding or in_layout; ACVM_E_UNSUPPORTED for a node created with a caller's
 *     BlackBoxFunctionSolver (the device resolve refuses such handles); ACVM_E_STATE while a node call runs.
 *   - acvm_node_foreign_stats: the lane's loop during the last node call. The bytes are those of the batch-wide calls
 *     (acvm_debug_foreign_call_stats) plus the node's own copies in host space.
 * Not here: an asynchronous variant; parking a waiting tile beside the next one (a tile waits for its handler); a handler on a node with a
 * black-box solver.
 */
enum { ACVM_SPACE_DEVICE = 0, ACVM_SPACE_HOST = 1 };
typedef struct {
    uint32_t lane; int device;          /* index in the node's device list, its HIP device (current on the calling thread) */
    uint32_t tile, round;               /* tile of the lane, 0-based round of that tile */
    acvm_foreign_call_site_t site;      /* n_waiting == n_rows */
    uint32_t n_rows, max_values;        /* rows of the site's list in this tile, the longest row */
    uint64_t row_base;                  /* caller's number of row i = row_base + rows[i]:
                                           acvm_node_solve: global instance number, acvm_node_solve_device: the lane's row number */
    const uint32_t *rows;               /* [n_rows] ascending */
    const uint32_t *lens;               /* [n_rows][n_inputs] */
    const void *values; const uint8_t *mask;   /* n_rows x max_values, in the handler's in_encoding / in_layout, dense */
} acvm_node_foreign_round_t;
typedef struct {                        /* filled by the handler (zeroed before the call) */
    uint32_t n_values; const uint8_t *is_array; const uint32_t *lens;   /* HOST, as in acvm_foreign_call_answers_desc_t */
    uint32_t encoding, layout, n_columns; uint64_t stride;
    const void *values;                 /* in the handler's memory space */
    const uint32_t *row_lens;           /* optional [n_rows][n_values], same space */
    const uint8_t *answered;            /* optional [n_rows], same space */
} acvm_node_foreign_answer_t;
typedef int (*acvm_node_foreign_fn)(void *user, const acvm_node_foreign_round_t *in, acvm_node_foreign_answer_t *out);
typedef struct {
    acvm_node_foreign_fn fn; void *user;
    uint32_t space;                     /* ACVM_SPACE_DEVICE: every pointer of `in` and the three data pointers of `out` are memory of the lane's device;
                                           ACVM_SPACE_HOST: host memory (the node copies inputs down and answers up) */
    uint32_t in_encoding, in_layout;
    uint32_t max_rounds;                /* per tile; 0 = 256 */
} acvm_node_foreign_handler_t;
typedef struct {                        /* one lane, the last node call */
    uint32_t rounds;                    /* rounds in which the handler was asked, over all tiles */
    uint32_t handler_calls;
    uint64_t rows_answered;             /* rows resumed by an answer */
    uint64_t rows_declined;             /* rows of declined sites, and rows an `answered` column left out */
    uint64_t rows_left_waiting;         /* rows still waiting when a tile reached max_rounds */
    double handler_ms;                  /* wall clock inside the handler */
    uint64_t h2d_bytes, d2h_bytes;      /* of the round trips */
} acvm_node_foreign_stats_t;
int acvm_node_set_foreign_call_handler(acvm_node_t *n, const acvm_node_foreign_handler_t *h);   /* NULL: none */
int acvm_node_foreign_stats(acvm_node_t *n, uint32_t lane, acvm_node_foreign_stats_t *out);
/* host-only probes of the lanes' placement logic: a sysfs cpulist ("0-15,32-47") into CPU numbers (returns how many; the first `cap` are
 * written), and the NUMA node + local CPUs of PCI device `bus_id` under `pci_root` (normally /sys/bus/pci/devices) */
int acvm_debug_cpulist(const char *text, uint32_t *cpus, uint32_t cap);
int acvm_debug_device_locality(const char *pci_root, const char *bus_id, int *numa_node, uint32_t *cpus, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
