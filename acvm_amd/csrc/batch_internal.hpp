// batch_internal.hpp -- what the translation units of the batch handle share (batch.cpp, batch_import.cpp, batch_schedule.cpp, batch_exact.cpp, batch_export.cpp,
// batch_messages.cpp, probes.cpp): staging, the exact path's building blocks, result formatting. Internal to the library; the node driver sees batch.hpp only.
#pragma once
#include "assigned_view.hpp"
#include "batch.hpp"

template <class T>
static int upload(T **dst, const std::vector<T> &src) {
    size_t bytes = (src.size() ? src.size() : 1) * sizeof(T);
    HIPCHK(hipMalloc((void **)dst, bytes));
    if (!src.empty()) HIPCHK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- batch.cpp
// staging arena: `bytes` of device memory valid until the next stage_reserve of this batch (256-byte aligned carving by the caller)
int stage_reserve(acvm_batch *b, size_t bytes);
// forget every resolved foreign-call result (a new ACVM: set_initial_witness / reset)
void clear_fc_store(acvm_batch *b);
void plan_stats(const Plan &p, acvm_stats_t *out);
// the event words of B instances (*event) behind their four-word header (*base, the allocation: the count of flagged instances at event[-4], the device
// address of *h_flag_count, pinned and device-mapped, at event[-2..-1]); the words themselves are left for launch_event_reset
int event_words_new(uint32_t B, uint32_t **base, uint32_t **event, uint32_t **h_flag_count);

// ---- batch_import.cpp
// an acvm_import_desc_t checked against the handle and the pointer (import_plan.cpp import_plan_desc): 0 and *out, or ACVM_E_INVALID and the error text
// (d_assigned: the mask of acvm_batch_import_device_masked, import_plan_desc_masked; null: none)
int import_plan_of(const acvm_batch *b, const acvm_import_desc_t *d, const void *d_values, ImportPlan *out, const uint8_t *d_assigned = nullptr);
// the plan's lists are on the device, in the handle's one list buffer (nothing to do for a plan without lists, or for the lists of the last upload)
int import_lists_ready(acvm_batch *b, const ImportPlan &plan);
// THE launch of an import on the handle's stream, whatever the entry point, and the only place that chooses among launch_import (the plain plan),
// launch_import_device and launch_import_typed and that hands out the event reset: exactly one launch of the call gets it. A plan with lists
// needs import_lists_ready first. gate: null, or the device word that must be zero for the import to happen. Returns whether a launch wrote the
// event words (events_fresh's rule).
bool batch_launch_import(acvm_batch *b, const ImportPlan &plan, const uint32_t *gate);
// any checked import without the wait (batch.hpp batch_import_async is this with the plain plan): lists, launches, the handle's state.
// *already (may be null): the import had run behind the last solve and nothing was enqueued.
int batch_import_plan_async(acvm_batch *b, const ImportPlan &plan, hipEvent_t imported, bool *already);

// ---- batch_schedule.cpp
// ACVM::solve for the batch; next: the plan of acvm_batch_solve_then_import(_ex) -- one resident part, whose d_values is the next tile's buffer --
// or null: nothing is imported behind the solve
int batch_solve_impl(acvm_batch *b, const ImportPlan *next);

// ---- batch_exact.cpp
int ensure_slow_capacity(acvm_batch *b, uint32_t n);
ExactLanes exact_lanes(acvm_batch *b, uint32_t n_slow);
int upload_fc_tables(acvm_batch *b, uint32_t n_slow);
int run_host_blackbox(acvm_batch *b, uint32_t opcode, bool exact, uint32_t n_slow);
int resolve_internal_calls(acvm_batch *b);  // the caller's BlackBoxFunctionSolver inside Brillig programs: answers the lanes waiting at one; > 0: solve again
// the exact in-order kernels over the current lanes from opcode min_start on (stepping: only opcodes [min_start, end_opcode), nothing replayed)
int run_exact_segments(acvm_batch *b, uint32_t n_slow, uint32_t min_start, bool replay = true, uint32_t end_opcode = 0xFFFFFFFFu);
int retry_device_limits(acvm_batch *b, uint32_t n_slow, bool replay, uint32_t end_opcode);
int count_not_solved(acvm_batch *b);
int solve_resume(acvm_batch *b);
int solve_stepping(acvm_batch *b, bool one);
int ensure_side_table(acvm_batch *b, uint32_t n_lanes, bool own_scratch);
int side_table_outcome(acvm_batch *b, ExactOutcome *out);

// ---- batch_foreign.cpp
// acvm_batch_resolve_foreign_call for exact lane t whose opcode's results (slot si) live on the device: the values are staged and appended by
// fc_append_kernel as a list of one row; sets the lane's resolved_new
int fc_append_one_instance(acvm_batch *b, uint32_t t, size_t si, uint32_t n_values, const uint8_t *is_array, const uint32_t *lens, const uint8_t *values_be32);

// a solve is about to consume the answers of the round (the lanes' resolved_new are cleared): the round's largest result joins every device-owned slot's bounds
static inline void fc_round_consumed(acvm_batch *b) {
    for (auto &sl : b->fc_slots) foreign_bounds_fold(&sl.bounds);
}

// ---- the table a host read or a digest is made from: where the values lie, how they are unscaled, witness -> row (null: row = witness index)
struct TableView { const uint4 *W; uint64_t Bp; Unscale u; const uint32_t *row_of; };
// the table of the level kernels: scaled columns leave through 1 / scale unless the lane's event word says it took the exact path
static inline TableView level_table(const acvm_batch *b) { return {b->d_W, b->Bp, b->unscale, b->d_slot_of}; }
// The side table (slot reuse, asynchronous exact jobs): lane t = the t-th flagged instance, row = witness index, nothing is scaled. The export and
// digest kernels unscale a lane whose event word is 0xFFFFFFFF ("solved by the level kernels"); d_slow_start holds opcode indices, which never
// are, so handing it over as the event words makes every lane read as "an instance of the exact path": plain values.
static inline TableView side_table(const acvm_batch *b) {
    Unscale plain = b->unscale;
    plain.event = b->d_slow_start;
    return {b->d_Wx, b->x_cap, plain, nullptr};
}

// ---- what every read-back entry point begins with: the exact job in flight is waited for (its outcome kept for the caller), an unsolved batch refused
static inline int finish_pending_and_require_solved(acvm_batch *b) {
    if (b->pending)
        if (int rc = batch_finish_pending(b, &b->last_outcome)) return rc;
    return b->solved ? 0 : set_err(ACVM_E_STATE, "batch not solved");
}
static inline int require_instance_range(const acvm_batch *b, uint32_t first, uint32_t n) {
    return (uint64_t)first + n > b->B ? set_err(ACVM_E_INVALID, "instance range out of bounds") : 0;
}

// ---- batch_export.cpp
int ensure_digest_tables(acvm_batch *b);
int digest_range(acvm_batch *b, hipStream_t s, const TableView &t, uint32_t first, uint32_t n, const int32_t *d_slow_index, bool use_host_index, uint32_t n_slow,
                 uint8_t *out32);
// THE host read: witnesses sel[0 .. n_sel) (a host list) of lanes [first, first + n) of the table as canonical big-endian values into out_be32
// ([n][n_sel][32], host), on stream s and waited for. Arena = the list | at most 64 MiB of values: a larger read takes several launches.
int read_witnesses(acvm_batch *b, hipStream_t s, const TableView &t, uint32_t first, uint32_t n, const uint32_t *sel, uint32_t n_sel, uint8_t *out_be32);
// one witness of one instance as 32 canonical big-endian bytes (message texts only; rare)
bool fetch_one(acvm_batch *b, uint32_t j, uint32_t w, uint8_t out[32]);
// the assigned set of the last solve (assigned_view.hpp) over the handle's bookkeeping; rows of the exact lanes' bitmap are copied when asked
// for (the blocking copy: not while an exact job is pending), a failing copy leaves its error in *err (if given) and the row unassigned
AssignedView batch_assigned(const acvm_batch *b, hipError_t *err = nullptr);
// the outcome of the pending exact job into b->exact_sink, on the job's stream and waited for (the side table is the next job's afterwards);
// *out (may be null): the instances and the heads of their results
int side_table_to_sink(acvm_batch *b, ExactOutcome *out);

// ---- batch_messages.cpp
// status, error, opcode index, aux words and call stack of an exact lane's outcome (r zeroed first); the message text is format_message's
void result_head(const SlowResult &sr, acvm_result_t &r);
void format_message(acvm_batch *b, uint32_t j, const SlowResult &sr, acvm_result_t &r);
void fill_result(acvm_batch *b, uint32_t j, acvm_result_t &r);
