// kernels.hpp -- host-visible launchers of the gfx950 kernels (kernels*.hip).
#pragma once
#include "grumpkin_host.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acvm {

// per-instance outcome of the exact in-order kernels. status 1 (InProgress) while the instance is still running.
struct SlowResult {
    uint32_t status, err, opcode_index, aux0, aux1;
    uint32_t msg, x0, x1;  // DevMsg code + payload for the host-side message text
    uint32_t n_call_stack;
    uint32_t call_stack[16];
    uint32_t val[8];       // a canonical field value quoted by the message (Brillig black-box limb checks)
};

// Brillig foreign-call round trip (ACVM::get_pending_foreign_call / resolve_pending_foreign_call, pwg/mod.rs:203-228).
// Results the host resolved live in a batch-wide store, one slot per Brillig opcode that holds a ForeignCall, keyed by the
// INSTANCE (so the level kernels and the exact kernels read the same tables): descriptor words
// [n_results, (n_values, (is_array, n) x n_values) x n_results] of instance j at desc[w * Bp + j], values laid out like W.
struct FcStoreSlot {
    const uint32_t *desc;  // null: nothing resolved for this opcode yet
    const uint4 *vals;
};
// Inputs of a pending call of the exact lanes: pend_desc [n_inputs, len x n_inputs], values in pend_vals, laid out like W with
// stride n_slow.
struct FcLanes {
    uint32_t *pend_desc;
    uint32_t pend_desc_words;
    uint4 *pend_vals;
    uint32_t pend_vals_cap;
};

// limits of the Brillig VM for one launch (ops_brillig.hpp; batch.cpp retry_device_limits raises them on the exact path)
struct BrilligLimits {
    uint32_t steps;       // instructions one VM run may execute
    uint32_t call_depth;  // call-stack words
    uint32_t mem_cap;     // memory cells per lane; 0 = the record's own (planner estimate)
    uint64_t stride;      // retry passes: lanes of the compact scratch (ExactLanes::br_lane indexes them)
};

// lanes of the exact path: flagged instances gathered through slow_ids
struct ExactLanes {
    const uint32_t *slow_ids;
    uint32_t n_slow;
    uint32_t *assigned;              // bit w of lane t at assigned[(w >> 5) * n_slow + t]
    const uint32_t *start_opcode;    // first opcode the lane executes (its event)
    SlowResult *results;
    FcLanes fc;
    const uint32_t *br_lane = nullptr;  // Brillig retry pass: column of lane t in the compact VM scratch (0xFFFFFFFF: not retried); null otherwise
    uint32_t br_max_regs = 0;           // brillig_resume: the registers of the circuit's largest Brillig record -- the scratch's word region lies behind that many slots
    // brillig_resume (null otherwise): the lanes' checkpoint records [n_slow][BR_CKPT_WORDS]; per lane 1 = "the record is valid for the opcode
    // the lane starts at", written by the HOST before every pass; VM steps lane t executed in this pass (the host zeroes it before the pass)
    uint32_t *br_ckpt = nullptr;
    const uint32_t *br_resume = nullptr;
    unsigned long long *br_pass_steps = nullptr;
    uint64_t br_total = 0;  // ... VM steps one run of an opcode may execute over all its passes; BrilligLimits::steps is the slice of this pass
    // (these live here and not in BrilligLimits: DeviceProgram is copied into every level kernel's private memory, the exact kernel alone reads these)
};

// everything a record needs besides the witness table
struct DeviceProgram {
    const uint32_t *prog;         // in-order program (one record per opcode)
    const uint32_t *prog_offset;  // per opcode
    const uint32_t *consts;       // circuit constants, 8 x u32 Montgomery each
    const uint32_t *bytecode;     // Brillig programs
    uint4 *Mem;                   // per-instance memory blocks, laid out like W
    GrumpkinTables grumpkin;      // device lookup tables (null pointers if the circuit has no Grumpkin opcode)
    const uint32_t *ecdsa_g;      // generator tables of secp256k1 / secp256r1 (kernels_ecdsa.hip; null: the circuit has no ECDSA call)
    const uint32_t *ped_seed;     // per Pedersen record: hash_single(x of hash_pair(IV[domain separator], n), 0), affine, 16 x u32
    const FcStoreSlot *fc_store;  // device array, one entry per Brillig opcode with a ForeignCall (null: the circuit has none)
    const uint32_t *slot_of;      // witness -> row of the table for the level kernels (null: row = witness index; plan.cpp slot reuse)
    BrilligLimits brillig;        // limits of the Brillig VM for this launch
    const uint32_t *byte_plane_of; // witness -> its byte plane or NONE (null: the circuit has none; plan.hpp "Byte planes")
    const uint32_t *byte_plane;    // [plane][instance]: low 29 bits of the canonical value | is-byte << 31, written by the import
};

// projective witnesses (plan.cpp): device tables behind the export and the hand-over to the exact path
struct Unscale {
    const uint32_t *index;       // per witness: row of consts, 0xFFFFFFFF = stored as is (null: no witness is scaled)
    const uint32_t *consts;      // 1 / scale, 8 x u32 each (device Montgomery form)
    const uint32_t *consts_plain; // 1 / scale as a canonical integer: the Montgomery product with it is the canonical VALUE (unscale and leave Montgomery form in one)
    const uint32_t *scaled_ids;  // the scaled witnesses, in row order
    uint32_t n_scaled;
    const uint32_t *event;       // per instance: 0xFFFFFFFF = solved by the level kernels (its column is still scaled)
};

// gridDim.y is limited to 65535: launch(first, count) over [0, n) in chunks of at most that many
template <class Launch>
static inline void for_grid_y_chunks(uint32_t n, Launch launch) {
    for (uint32_t done = 0; done < n; done += 65535u) launch(done, n - done > 65535u ? 65535u : n - done);
}

// plane_of_input / plane: per input its byte plane or NONE, and the planes (both null: the circuit has none)
// event_reset: null, or the batch's event words: the import also leaves them "nobody flagged" (returns true when it did: the solve behind it needs no reset launch)
bool launch_import(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const uint8_t *in, const uint32_t *ids, uint32_t n_in, const uint32_t *gate = nullptr,
                   const uint32_t *plane_of_input = nullptr, uint32_t *plane = nullptr, uint32_t *event_reset = nullptr);
// acvm_batch_import_device: the initial witnesses from the caller's device buffer in any encoding, layout, stride and column list of the device export
// (import_decode.hpp). The other arguments and the return value as launch_import.
struct ImportDevice {
    uint32_t encoding, layout;
    const uint32_t *columns;  // device array, one column per input; null: input k is column k
    uint64_t stride;          // in elements, >= the layout's dense stride
    const void *in;           // 16-byte aligned (launch_import_typed: aligned to the element size)
};
bool launch_import_device(hipStream_t s, const ImportDevice &x, uint4 *W, uint64_t Bp, uint32_t B, const uint32_t *ids, uint32_t n_in, const uint32_t *gate = nullptr,
                          const uint32_t *plane_of_input = nullptr, uint32_t *plane = nullptr, uint32_t *event_reset = nullptr);
void launch_export(hipStream_t s, const uint4 *W, uint64_t Bp, uint32_t first, uint32_t n, const uint32_t *sel, uint32_t n_sel,
                   uint8_t *out, const Unscale &u, const uint32_t *row_of = nullptr);
// acvm_batch_export_device: the map of instances [first, first + n) x the witness list into the caller's device buffer (export_encode.hpp:
// encodings, layouts, where element (i, k) goes). sel: device array, or null = position k is witness k.
struct ExportDevice {
    uint32_t encoding, layout, first, n;
    const uint32_t *sel;
    uint32_t n_sel, n_witnesses;
    uint64_t stride;  // in elements, >= the layout's dense stride
    void *out;        // 16-byte aligned
    uint8_t *mask;    // one byte per element, same layout and stride; may be null
};
// every lane of the range read as a generic instance (u_factor: Unscale::consts_plain, or its Montgomery-256 twin for that encoding) ...
void launch_export_device(hipStream_t s, const ExportDevice &x, const uint4 *W, uint64_t Bp, const uint32_t *row_of, const uint32_t *producer, const Unscale &u,
                          const uint32_t *u_factor);
// ... then the instances of the exact path over their elements: lanes = n_lanes pairs (lane of the assigned bitmap, index in the range), values in
// column `lane` of W (side) or in column first + index
void launch_export_device_lanes(hipStream_t s, const ExportDevice &x, const uint4 *W, uint64_t Bp, bool side, const uint32_t *lanes, uint32_t n_lanes,
                                const uint32_t *assigned_bits, uint32_t n_slow);
// ---- kernels_typed_io.hip: the narrow encodings (export_encode.hpp EXPORT_ENC_U8 .. U128: elements of 1 .. 16 bytes, `in` / `out` aligned to
// the element size) and the broadcast layout of an import part (EXPORT_LAYOUT_BROADCAST, any encoding; 32-byte elements 16-byte aligned).
// Arguments and return value as launch_import_device / launch_export_device(_lanes); the mask byte of a narrow element is 0 / 1 / 2.
bool launch_import_typed(hipStream_t s, const ImportDevice &x, uint4 *W, uint64_t Bp, uint32_t B, const uint32_t *ids, uint32_t n_in, const uint32_t *gate = nullptr,
                         const uint32_t *plane_of_input = nullptr, uint32_t *plane = nullptr, uint32_t *event_reset = nullptr);
// ---- kernels_records.hip (acvm_batch_import_device_records): instance i reads its fields from the record at in + i * pitch, any alignment.
// windows / fields: the device tables of record_plan.hpp (rows and planes per field inside). The other arguments and the return value as
// launch_import.
bool launch_import_records(hipStream_t s, const void *in, uint64_t pitch, const uint32_t *windows, uint32_t n_windows, const uint32_t *fields, uint4 *W, uint64_t Bp,
                           uint32_t B, const uint32_t *gate, uint32_t *plane, uint32_t *event_reset);
// ---- kernels_records_masked.hip (acvm_batch_import_device_records_masked): launch_import_records over the masked tables of record_plan.hpp. In
// front of the kernel the words of the missing set of the live instances are zeroed on the stream, behind it the instances with an absent input
// are counted into result (import_mask.hpp: three words, zero before the call). Never gated. Returns what launch_import returns.
bool launch_import_records_masked(hipStream_t s, const void *in, uint64_t pitch, const uint32_t *windows, uint32_t n_windows, const uint32_t *fields, uint4 *W, uint64_t Bp,
                                  uint32_t B, uint32_t n_in, uint32_t *plane, uint32_t *event_reset, uint32_t *missing, uint64_t *result);
// ---- kernels_import_mask.hip (acvm_batch_import_device_masked; import_mask.hpp: where a mask byte lies, the missing set, the result words)
struct ImportMaskSource {
    const uint8_t *mask;      // the caller's d_assigned: one byte per element in the values' layout, stride and column list; any alignment
    uint32_t layout;
    const uint32_t *columns;  // device array, one column per input; null: input k is column k
    uint64_t stride;          // in elements, >= the layout's dense stride
};
// The mask pass, behind the value import of all n_in inputs: missing ([words][Bp]) is written for instances [0, B), the rows (and plane words) of
// absent elements are zeroed, result (IMPORT_MASK_RESULT_WORDS device words, zeroed by the caller) gathers what the host reads back.
void launch_import_mask(hipStream_t s, const ImportMaskSource &x, uint4 *W, uint64_t Bp, uint32_t B, const uint32_t *rows, uint32_t n_in, const uint32_t *plane_of_input,
                        uint32_t *plane, uint32_t *missing, uint64_t *result);
// the flag pass: every instance of [0, B) with an absent input leaves the generic path at opcode 0 (ops_common.hpp flag_instance)
void launch_import_missing_flag(hipStream_t s, const uint32_t *missing, uint32_t n_in, uint64_t Bp, uint32_t B, uint32_t *event);
// the clear pass behind launch_init_assigned: exact lane t drops the initial witnesses instance slow_ids[t] lacks from its assigned set
void launch_import_missing_clear(hipStream_t s, const uint32_t *missing, uint32_t n_in, uint64_t Bp, const uint32_t *init_ids, const uint32_t *slow_ids, uint32_t n_slow,
                                 uint32_t *assigned);
void launch_export_narrow(hipStream_t s, const ExportDevice &x, const uint4 *W, uint64_t Bp, const uint32_t *row_of, const uint32_t *producer, const Unscale &u);
void launch_export_narrow_lanes(hipStream_t s, const ExportDevice &x, const uint4 *W, uint64_t Bp, bool side, const uint32_t *lanes, uint32_t n_lanes,
                                const uint32_t *assigned_bits, uint32_t n_slow);
// ---- acvm_batch_export_device_list: row i of the output is instance list[i] of the batch (ExportDevice::first is 0, n the list's length). The host
// cannot see the list, so the kernels tell a generic instance from one of the exact path themselves: lane_of[j] is the instance's lane or -1.
struct ExportListSource {
    const uint32_t *list;           // device, n absolute instance numbers; an entry >= B reads as an instance that assigned nothing
    uint32_t B;                     // live instances
    const int32_t *lane_of;         // device, one word per instance of the handle
    const uint4 *Wx;                // the exact lanes' values: column `lane` of the side table (side), or the instance's own column of the level table
    uint64_t Bpx;
    bool side;
    const uint32_t *assigned_bits;  // bit w of lane t at assigned_bits[(w >> 5) * n_slow + t]
    uint32_t n_slow;
};
void launch_export_device_list(hipStream_t s, const ExportDevice &x, const uint4 *W, uint64_t Bp, const uint32_t *row_of, const uint32_t *producer, const Unscale &u,
                               const uint32_t *u_factor, const ExportListSource &src);
void launch_export_narrow_list(hipStream_t s, const ExportDevice &x, const uint4 *W, uint64_t Bp, const uint32_t *row_of, const uint32_t *producer, const Unscale &u,
                               const ExportListSource &src);
// ---- kernels_records_out.hip (acvm_batch_export_device_records): output row i writes its fields into the record at out + i * pitch, any
// alignment; row i is instance src.list[i], or first + i where src.list is null (the rest of src as for the list export: the exact lanes are
// found through lane_of either way). windows / fields: the device tables of record_out_plan.hpp, the encoding per field. u_plain / u_m256: the
// factor rows of the scaled witnesses for every encoding but Montgomery-256 / for it (null where no field takes it).
struct RecordExport {
    const uint4 *W;
    uint64_t Bp;
    uint32_t first, n;
    ExportListSource src;
    uint32_t n_witnesses;  // a field's witness >= n_witnesses is unassigned
    const uint32_t *row_of, *producer;
    const uint32_t *u_index, *u_plain, *u_m256;
    uint8_t *out;
    uint64_t pitch;
    const uint32_t *windows, *fields;
};
void launch_export_records(hipStream_t s, const RecordExport &x, uint32_t n_windows);
// ---- kernels_wire.hip (acvm_batch_witness_maps_wire_device): output row i writes the serialised WitnessMap of its instance into the slot at
// out + i * pitch (16-aligned, pitch a multiple of 16); row i is instance src.list[i], or first + i where src.list is null. sel: the device
// copy of the witness list (n_positions entries) or null = position k is witness k; rank / list_mask / crc_pow / crc_x64: wire_plan.hpp's
// tables; lane_prefix: [(n_witnesses + 31) / 32 + 1][n_slow], made by launch_wire_lane_prefix (null while no instance left the generic path);
// crc: n zeroed words (GZIP_STORED; else unused); lengths: n device words or null; deflate / deflate_prefix_bits: wire_plan.hpp's code table
// and the bits of its prefix (GZIP_DEFLATE; else null).
struct WireExport {
    const uint4 *W;
    uint64_t Bp;
    uint32_t first, n;
    ExportListSource src;
    uint32_t n_witnesses;
    const uint32_t *row_of, *producer;
    const uint32_t *u_index, *u_plain;
    const uint32_t *sel;
    uint32_t n_positions;
    const uint32_t *rank, *list_mask, *lane_prefix, *crc_pow;
    uint32_t crc_x64;
    uint32_t *crc;
    uint32_t container;
    uint8_t *out;
    uint64_t pitch;
    uint64_t *lengths;
    const uint32_t *deflate;
    uint32_t deflate_prefix_bits;
};
// per lane of the exact path and 32-witness word: its assigned list positions in the words below, and behind the last word their total
void launch_wire_lane_prefix(hipStream_t s, const uint32_t *assigned_bits, uint32_t n_slow, uint32_t n_words, const uint32_t *list_mask, uint32_t *lane_prefix);
void launch_wire_export(hipStream_t s, const WireExport &x, uint32_t n_windows);
// ---- kernels_wire_deflate.hip: the GZIP_DEFLATE container of the same call, what launch_wire_export dispatches to
void launch_wire_deflate(hipStream_t s, const WireExport &x, uint32_t n_windows);
// ---- kernels_wire_in.hip (acvm_batch_import_device_wire): instance j reads the serialised WitnessMap in the slot at in + j * pitch (16-aligned,
// pitch a multiple of 16) as its initial witnesses; what the row does not name is absent (import_mask.hpp: the missing set). keys / positions /
// crc_pow / crc_x64 / rank_bits: wire_in_plan.hpp's tables (crc_pow null for BINCODE); rows / plane_of_input: per position of initial_ids, as
// launch_import_mask takes them; crc: B words of scratch (GZIP_STORED; else unused); lengths: B device words or null; result: three words,
// zero before the call -- [IMPORT_MASK_BAD] the findings, [IMPORT_MASK_BAD_KEY] the smallest wire_in_key, [IMPORT_MASK_MISSING] the instances
// with an absent input. Every row of the live instances, every plane word of an input that has one, every missing word and the event words
// are written exactly once. Returns what launch_import returns: whether the event words were reset.
struct WireImport {
    const uint8_t *in;
    uint64_t pitch;
    const uint64_t *lengths;
    uint32_t container, B, n_in;
    const uint32_t *keys, *positions, *rows, *plane_of_input;
    uint32_t *plane;
    uint4 *W;
    uint64_t Bp;
    uint32_t *event_reset, *missing, *crc;
    const uint32_t *crc_pow;
    uint32_t crc_x64, rank_bits;
    uint64_t *result;
};
bool launch_wire_import(hipStream_t s, const WireImport &x, uint32_t n_windows);
// ---- kernels_wire_inflate.hip (acvm_batch_import_device_wire_gzip, stage 1): row j's gzip member in [in + j * pitch, + min(lengths[j], pitch))
// (lengths null: pitch) inflated into out + j * out_pitch (a multiple of 4; at most out_cap bytes, nothing at or behind the row's length is
// written). tables: n x INFLATE_PLAN_ROW_WORDS dwords of scratch for the rows' code tables. out_lengths: n words; findings: n x {class, block} (wire_inflate.hpp); crcs: n words or null; fixed: wire_inflate_plan.hpp's
// table; result: null, or two words, zero before the call -- the findings' count and the smallest inflate_key.
struct WireInflate {
    const uint8_t *in;
    uint64_t pitch;
    const uint64_t *lengths;
    uint32_t n;
    uint8_t *out;
    uint64_t out_pitch, out_cap;
    uint32_t *tables;
    uint64_t *out_lengths;
    uint32_t *findings, *crcs;
    const uint16_t *fixed;
    uint64_t *result;
};
void launch_wire_inflate(hipStream_t s, const WireInflate &x);
// ---- kernels_wire_pack.hip (acvm_batch_witness_maps_wire_packed_device, acvm_batch_import_device_wire_packed): wire_repitch.hpp's pieces.
// launch_wire_scan: offsets[0 .. m] of a chunk of m rows from its lengths, offsets[0] = state[REPITCH_STATE_BASE], which is left at offsets[m];
// state[REPITCH_STATE_FIT] grows by the rows with offsets[i + 1] <= capacity. One block; state is two device words, zero before the first chunk.
// launch_wire_repitch: the copy wire_repitch.hpp describes. launch_wire_offsets: an untrusted offsets column [n + 1] judged against n_bytes and
// the longest row accepted -- lengths[j] (0 for a row with a finding) and findings[j] (either may be null), result[0] += the findings,
// result[1] = max(wire_offsets_key): two device words, zero before the call.
struct WireRepitch;
void launch_wire_scan(hipStream_t s, const uint64_t *lengths, uint32_t m, uint64_t *offsets, uint64_t capacity, uint64_t *state);
void launch_wire_repitch(hipStream_t s, const WireRepitch &x);
void launch_wire_offsets(hipStream_t s, const uint64_t *offsets, uint32_t n, uint64_t n_bytes, uint64_t longest, uint64_t *lengths, uint32_t *findings, uint64_t *result);
// ---- kernels_select.hip (acvm_batch_outcomes_device): the outcome columns of n instances -- every one Solved, then the exact lanes' records
// {status, err, opcode index, index in the range} over them; any column may be null
void launch_outcomes_fill(hipStream_t s, uint32_t n, uint8_t *status, uint8_t *err, uint32_t *opcode_index);
void launch_outcomes_lanes(hipStream_t s, const uint32_t *records, uint32_t n_lanes, uint32_t n, uint8_t *status, uint8_t *err, uint32_t *opcode_index);
// lane_of[ids[t]] = t for t < n_slow (the map filled with -1 before: launch_fill_u32)
void launch_lane_map_scatter(hipStream_t s, int32_t *lane_of, uint32_t n_instances, const uint32_t *ids, uint32_t n_slow);
// rows of 32 bytes to where their instances are: out[i] = rows[t] for the n_lanes pairs (t, i) of `lanes` with i < n -- the digests of the side
// table's lanes into a column of the caller (any alignment)
void launch_scatter_rows32(hipStream_t s, const uint32_t *rows, const uint32_t *lanes, uint32_t n_lanes, uint32_t n, uint8_t *out);
// The ordered selection (select_scan.hpp): out[0 .. *count) = first + i for the i < n, ascending, whose status byte has its bit set in select_mask; what lies
// behind *count is not written. scratch: select_scratch_words(n) words; out may be null (the count alone); count: one device word.
size_t select_scratch_words(uint32_t n);
void launch_select(hipStream_t s, const uint8_t *status, uint32_t first, uint32_t n, uint32_t select_mask, uint32_t *scratch, uint32_t *out, uint32_t *count);
void launch_gather_initial(hipStream_t s, uint4 *Wx, uint64_t Bpx, const uint4 *W, uint64_t Bp, const uint32_t *init_ids, const uint32_t *init_rows, uint32_t n_init,
                           const uint32_t *slow_ids, uint32_t n_slow);
void launch_gather_columns(hipStream_t s, uint4 *Wx, uint64_t Bpx, const uint4 *W, uint64_t Bp, uint32_t n_rows, const uint32_t *slow_ids, uint32_t n_slow,
                           const uint32_t *unscale_index, const uint32_t *unscale_consts, const uint32_t *producer, const uint32_t *start_opcode);
void launch_unscale_slow(hipStream_t s, uint4 *W, uint64_t Bp, const uint32_t *slow_ids, uint32_t n_slow, const Unscale &u, const uint32_t *producer,
                         const uint32_t *start_opcode);
// The bundles of one gate launch (plan.hpp Plan::bundle_*) as the driver composes them for the device (batch.cpp upload_bundles; ops_common.hpp
// arith_level_body): tab = the launch's first (first program entry, shared row) pair of `count`; progs = the plan's whole list of (offset in gate_stream,
// first linear table | GATE_BUNDLE_LAST) pairs, grouped by bundle. grid.y counts the launch's bundles.
struct GateBundles {
    const uint2 *progs, *tab;
    uint32_t count;
};
void launch_arith_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const uint32_t *gate_stream, const uint32_t *consts, uint32_t *event, const uint4 *inv,
                        const uint32_t *lin_tables, const GateBundles &bundles);
void launch_inverse_batch(hipStream_t s, const uint4 *W, uint4 *inv, uint64_t Bp, uint32_t B, const uint32_t *gate_stream,
                          const uint32_t *job_offset, uint32_t n_jobs, uint32_t *event, uint32_t inv_chunk, uint32_t inv_share);
// waves that share one field inversion (tuning.hpp inv_share): 1, 2, 4 or 8; anything else is the next lower of those
inline uint32_t inverse_share_clamp(int64_t v) { return v >= 8 ? 8u : v >= 4 ? 4u : v >= 2 ? 2u : 1u; }
// the bundles of a level's gates and n_light light records of the same level in one launch (bundles + n_light <= 65535)
void launch_arith_light_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const uint32_t *gate_stream, const uint4 *inv, const DeviceProgram &dp,
                              const uint32_t *light_offsets, uint32_t n_light, uint32_t *event, const uint32_t *lin_tables, const GateBundles &bundles);
void launch_modmul_rate(hipStream_t s, uint32_t *out, uint32_t blocks, uint32_t iters);
void launch_secp_rate(hipStream_t s, uint32_t curve, uint32_t *out, uint32_t blocks, uint32_t iters);  // kernels_ecdsa.hip
void launch_stream_rate(hipStream_t s, const uint4 *a, const uint4 *b, uint4 *out, uint64_t n);  // n: multiple of 256
void launch_fr_selftest(hipStream_t s, uint64_t seed, uint32_t n, uint32_t *mismatches);
// acvm_debug_fr (fr_probe.hpp): words per item of `what` going in / coming out (0: no such routine); one lane per item, in / out on the device,
// uniform18: host memory, the two wave-uniform working-form factors of the "U" forms (null: zeros)
// acvm_debug_lin_add: fr29_lin_add<1 / 2> per lane; n_terms, tables (2 x 81 words) per wave of 64 items; rows 2 x 8, hs 9, out 9 words per item; all on the device
void launch_lin_add_probe(hipStream_t s, const uint32_t *n_terms, const uint32_t *tables, const uint32_t *rows, const uint32_t *hs, uint32_t n_items, uint32_t *out);
uint32_t fr_probe_words(uint32_t what, bool out);
void launch_fr_probe(hipStream_t s, uint32_t what, const uint32_t *in, uint32_t n_items, const uint32_t *uniform18, uint32_t *out);
void launch_fill_u32(hipStream_t s, uint32_t *p, uint32_t v, uint64_t n);
// event words [0, B) <- 0xFFFFFFFF, the count of flagged instances in front of them (event[-4], ops_common.hpp flag_instance) <- 0
void launch_event_reset(hipStream_t s, uint32_t *event, uint32_t B);
// event words <- min(event, opcode), the count <- B: a plan the level kernels do not cover entirely
void launch_event_truncate(hipStream_t s, uint32_t *event, uint32_t B, uint32_t opcode);
void launch_min_u32(hipStream_t s, uint32_t *p, uint32_t v, uint64_t n);
void launch_init_assigned(hipStream_t s, uint32_t *assigned, uint32_t n_slow, uint32_t n_words, uint32_t n_witnesses,
                          const uint32_t *producer, const uint32_t *start_opcode);

// ---- level kernels of the non-arithmetic record classes (FastPolicy): grid.y = records of the level.
// offsets: device array of record offsets into prog; scratch_off: per record, u32-word offset (per instance) into scratch
void launch_light_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const DeviceProgram &dp, const uint32_t *offsets, uint32_t n,
                        uint32_t *event);
// the straight-line Brillig records of a level (PK_BRILLIG_SL, ops_light.hpp op_brillig_sl)
void launch_light_sl_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const DeviceProgram &dp, const uint32_t *offsets, uint32_t n,
                           uint32_t *event);
void launch_hash_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const DeviceProgram &dp, const uint32_t *offsets,
                       const uint32_t *scratch_off, uint32_t n, uint32_t *event, uint32_t *scratch);
// records flagged HASH_COOP_FLAG (ops_hash.hpp): four waves per 64 instances, the byte message in LDS
// lds_words: 32-bit message words per instance of the longest record of the launch
void launch_hash_coop_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const DeviceProgram &dp, const uint32_t *offsets, uint32_t n, uint32_t *event, uint32_t lds_words);
void launch_grumpkin_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const DeviceProgram &dp, const uint32_t *offsets,
                           const uint32_t *scratch_off, uint32_t n, uint32_t *event, uint32_t *scratch);
// Pedersen records: 4 waves per group of 64 instances, one accumulator chain each (kernels_grumpkin.hip)
void launch_pedersen_seeds(hipStream_t s, const GrumpkinTables &T, const uint32_t *keys, uint32_t n, uint32_t *out);
void launch_pedersen_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const DeviceProgram &dp, const uint32_t *offsets, uint32_t n,
                           uint32_t *event, const uint32_t *scratch_off = nullptr, uint32_t *scratch = nullptr);
void launch_brillig_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const DeviceProgram &dp, const uint32_t *offsets,
                          const uint32_t *scratch_off, uint32_t n, uint32_t *event, uint32_t *scratch);

// ---- exact in-order kernels (ExactPolicy): one lane per flagged instance
void launch_exact_init(hipStream_t s, const ExactLanes &L);
// opcodes [op_begin, op_end) of EVERY class but CLS_HOSTBB in one launch (kernels_brillig.hip exact_run_kernel); prog_class: device
// array, OpClass per opcode; the class scratch buffers as the per-opcode kernels take them
struct ExactScratch { uint32_t *hash, *grumpkin, *brillig; };
// brillig_resume: the continuing lanes' registers, live cells and call-stack words from the old compact scratch into the new one
// (kernels_brillig_resume.hip; d_lanes: n_lanes BrRelocLane records on the device)
struct BrLayout;
struct BrRelocLane;
void launch_brillig_relocate(hipStream_t s, const BrRelocLane *d_lanes, uint32_t n_lanes, uint64_t max_items, const BrLayout &from, const uint32_t *old_scratch,
                             const BrLayout &to, uint32_t *new_scratch);
void launch_exact_run(hipStream_t s, uint4 *W, uint64_t Bp, const DeviceProgram &dp, const ExactLanes &L, uint32_t op_begin, uint32_t op_end, bool replay_memory,
                      const uint8_t *prog_class, const ExactScratch &sc);
void launch_grumpkin_probe(hipStream_t s, const GrumpkinTables &T, uint32_t what, uint32_t param, const uint32_t *in, uint32_t n_in, uint32_t *out);
// one lane per item (acvm_debug_grumpkin_items); scratch: Bp x GRUMPKIN_VARBASE_SCRATCH_WORDS words for what = 6, Bp a multiple of 64 that covers n_items
uint32_t grumpkin_items_words(uint32_t what, bool out);
void launch_grumpkin_items(hipStream_t s, const GrumpkinTables &T, uint32_t what, uint32_t param, const uint32_t *in, uint32_t n_items, uint32_t *out, uint32_t *scratch,
                           uint64_t Bp);
void launch_table_gather(hipStream_t s, const uint4 *table, const uint64_t *entries, uint32_t n, uint4 *out);  // (acvm_debug_table_read)
// ECDSA (kernels_ecdsa.hip; the generator tables d * 2^(16 j) * G of both curves: grumpkin_host.hpp ecdsa_generator_tables)
void launch_secp_probe(hipStream_t s, uint32_t curve, uint32_t what, const uint32_t *in, uint32_t n_items, uint32_t words_in, uint32_t words_out, uint32_t *out,
                       const uint32_t *gtabs);
void launch_ecdsa_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t B, const DeviceProgram &dp, const uint32_t *offsets, uint32_t n, uint32_t *event);
// caller-supplied BlackBoxFunctionSolver (kernels_ops.hip)
void launch_hostbb_precheck(hipStream_t s, const ExactLanes &L, uint32_t opcode, const uint32_t *sel, uint32_t n_sel, uint8_t *active);
void launch_hostbb_gather(hipStream_t s, const uint4 *W, uint64_t Bp, const uint32_t *ids, uint32_t first, uint32_t n_lanes, const uint32_t *sel,
                          uint32_t n_sel, uint8_t *out, const uint32_t *slot_of = nullptr);
void launch_hostbb_apply_level(hipStream_t s, uint4 *W, uint64_t Bp, uint32_t first, uint32_t n_lanes, uint32_t opcode, uint32_t func, const uint32_t *outs,
                               uint32_t n_out, const uint8_t *rc, const uint8_t *vals, uint32_t *event, const uint32_t *slot_of = nullptr);
void launch_hostbb_apply_exact(hipStream_t s, uint4 *W, uint64_t Bp, const ExactLanes &L, uint32_t first, uint32_t n_lanes, uint32_t opcode, uint32_t func,
                               const uint32_t *outs, uint32_t n_out, const uint8_t *active, const uint8_t *rc, const uint8_t *vals);
// per-instance digest of the witness map (kernels_hash.hip; definition: include/acvm_amd.h acvm_batch_digest). Device tables of the
// polynomial fingerprint, 8 x u32 per entry in the device's Montgomery form:
struct DigestTables {
    const uint32_t *g_pow;     // [n_witnesses]: g^(w+1)
    const uint32_t *g_scaled;  // [scaled witnesses, rows of Unscale]: g^(w+1) / scale_w
    const uint32_t *h_pow;     // [n_witnesses]: h^(w+1)
    const uint32_t *h_generic; // [1]: the sum of h^(w+1) over the witnesses the planner saw assigned
};
// the witness map hashed as bytes, in tree form (kernels_hash.hip; include/acvm_amd.h acvm_batch_digest_blake2s): leaves = scratch of
// digest_b2s_leaves(n_witnesses) x 8 x n words
uint32_t digest_b2s_leaves(uint32_t n_witnesses);
void launch_digest_blake2s(hipStream_t s, const uint4 *W, uint64_t Bp, uint32_t first, uint32_t n, uint32_t n_witnesses, const uint32_t *producer, const Unscale &u,
                           const int32_t *slow_index, const uint32_t *assigned, uint32_t n_slow, uint32_t *leaves, uint8_t *out);
uint32_t digest_chunks(uint32_t n_witnesses);  // rows of the partial-sum scratch of launch_digest: digest_chunks x n x 32 bytes
void launch_digest(hipStream_t s, const uint4 *W, uint64_t Bp, uint32_t first, uint32_t n, uint32_t n_witnesses, const uint32_t *producer, const Unscale &u,
                   const DigestTables &T, const int32_t *slow_index, const uint32_t *assigned, uint32_t n_slow, uint4 *partial, uint8_t *out);
// the digest folded into the solve (PlanOpts::fold_digest): partial = [records][2][Bp] x 16 B
void launch_digest_fold_level(hipStream_t s, const uint4 *W, uint64_t Bp, uint32_t B, const DeviceProgram &dp, const uint32_t *offsets, uint32_t n,
                              const DigestTables &T, uint4 *partial);
void launch_digest_final(hipStream_t s, const uint4 *partial, uint32_t n_rows, uint64_t stride, uint32_t first, uint32_t n, const uint32_t *event, const DigestTables &T,
                         uint8_t *out);
// ---- kernels_foreign.hip: the foreign-call round trip of a whole batch on the device (foreign_store.hpp). rows: device pairs (exact lane,
// instance) of the listed rows of a site's waiting list; row r of the launch is element row r of the caller's buffer.
struct FcInputsOut {
    const uint32_t *rows;
    uint32_t n_rows, n_inputs;      // n_inputs: words per row of lens
    uint32_t encoding, layout, n_columns;
    uint64_t stride;                // in elements, >= the layout's dense stride
    uint32_t *instances, *lens;     // each may be null
    uint8_t *values, *mask;         // each may be null; values aligned to the element size (16 bytes for the 32-byte encodings)
};
// the largest number of pending values among the rows, max-ed into *max_values (one device word, zeroed by the caller)
void launch_fc_inputs_max(hipStream_t s, const FcLanes &fc, uint32_t n_slow, const uint32_t *rows, uint32_t n_rows, uint32_t *max_values);
void launch_fc_inputs(hipStream_t s, const FcLanes &fc, uint32_t n_slow, const FcInputsOut &o);
struct FcAppend {
    uint32_t *desc;                 // the slot's tables (FcStoreSlot, writable) and their capacities
    uint4 *vals;
    uint64_t Bp;
    uint32_t desc_words, vals_cap;
    const uint32_t *rows;
    uint32_t n_rows;
    const uint32_t *shape;          // device: [n_values, (is_array, n) x n_values], the same for every row
    uint32_t shape_total;           // values of one result
    uint32_t encoding, layout;
    uint64_t stride;
    const void *values;             // the caller's buffer: the row's values back to back in columns 0 .. shape_total - 1
    uint32_t *refused;              // one device word, zeroed by the caller: rows whose result did not fit (nothing of them is written)
};
void launch_fc_append(hipStream_t s, const FcAppend &a);
// The per-row form (acvm_batch_resolve_foreign_calls_device_rows): a.shape gives n_values and which outputs are arrays, a.shape_total is not used.
struct FcAppendRows {
    FcAppend a;
    const uint32_t *lens;           // device [n_rows][n_values] row-major: values of array output k of row r (null: a.shape's own lengths)
    const uint8_t *answered;        // device [n_rows]: 0 = the row is left out (null: every row is answered)
    uint32_t n_columns;             // values per row of the caller's buffer: a row whose lengths sum to more is refused
};
// the largest total among the answered rows, max-ed into *max_values (one device word, zeroed by the caller); 0xFFFFFFFF: a total of 2^31 or more
void launch_fc_answers_max(hipStream_t s, const uint32_t *shape, const uint32_t *lens, const uint8_t *answered, uint32_t n_rows, uint32_t *max_values);
void launch_fc_append_rows(hipStream_t s, const FcAppendRows &ar);
// InProgress -> Solved after the last opcode
void launch_exact_finish(hipStream_t s, const ExactLanes &L, uint32_t min_ip = 0);

}  // namespace acvm
