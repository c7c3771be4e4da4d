// batch_import.cpp -- ACVM::new's initial WitnessMap (pwg/mod.rs:146-156) for the batch: every entry point that imports initial witnesses. Each
// of them has its arguments checked into an ImportPlan (import_plan.cpp: pure host code) and hands the plan to batch_import_plan_async, which
// sits on four helpers with one definition each: the list buffer (import_lists_ready), the launch (batch_launch_import), the question whether
// the import already ran behind the last solve (import_is_behind_solve) and the handle's state afterwards (import_epilogue).
#include "batch_internal.hpp"
#include "export_encode.hpp"
#include "import_mask.hpp"
#include "record_plan.hpp"
#include "wire_decode.hpp"
#include "wire_in_plan.hpp"
#include "wire_inflate.hpp"
#include "wire_inflate_plan.hpp"
#include "wire_repitch.hpp"

static_assert(EXPORT_ENC_BE32 == ACVM_ENC_BE32 && EXPORT_ENC_MONT256_LE == ACVM_ENC_MONT256_LE && EXPORT_ENC_U8 == ACVM_ENC_U8 && EXPORT_ENC_U128 == ACVM_ENC_U128 &&
                  EXPORT_INSTANCE_MAJOR == ACVM_LAYOUT_INSTANCE_MAJOR && EXPORT_WITNESS_MAJOR == ACVM_LAYOUT_WITNESS_MAJOR && EXPORT_LAYOUT_BROADCAST == ACVM_LAYOUT_BROADCAST,
              "the kernels (export_encode.hpp) and the checks (import_plan.cpp: include/acvm_amd.h) number encodings and layouts alike");
static_assert(IMPORT_MASK_INSTANCE_MAJOR == ACVM_LAYOUT_INSTANCE_MAJOR && IMPORT_MASK_WITNESS_MAJOR == ACVM_LAYOUT_WITNESS_MAJOR, "import_mask.hpp numbers the layouts as the ABI does");

static ImportView import_view(const acvm_batch *b) {
    const Plan &p = b->plan();
    return ImportView{b->B, (uint32_t)p.initial_ids.size(), p.initial_ids.data(), b->reuse() ? b->init_rows.data() : p.initial_ids.data(),
                      p.n_byte_planes ? b->plane_of_input.data() : nullptr};
}
int import_plan_of(const acvm_batch *b, const acvm_import_desc_t *d, const void *d_values, ImportPlan *out, const uint8_t *d_assigned) {
    const ImportView view = b ? import_view(b) : ImportView{};
    std::string err;
    const int rc = import_plan_desc_masked(b ? &view : nullptr, d, d_values, d_assigned, out, &err);
    return rc ? set_err(rc, err) : 0;
}

// One small host-to-device copy when the plan's lists differ from the last upload's, none otherwise (or for a plan without lists). The stream is
// waited for first: an import enqueued behind the last solve may still be reading the old lists.
int import_lists_ready(acvm_batch *b, const ImportPlan &plan) {
    const std::vector<uint32_t> &lists = plan.lists;
    if (lists.empty() || (b->d_import_lists && b->import_lists == lists)) return 0;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    b->import_lists.clear();
    if (lists.size() > b->import_lists_cap) {
        if (b->d_import_lists) { hipFree(b->d_import_lists); b->d_import_lists = nullptr; b->import_lists_cap = 0; }
        HIPCHK(hipMalloc((void **)&b->d_import_lists, lists.size() * 4));
        b->import_lists_cap = lists.size();
    }
    HIPCHK(hipMemcpy(b->d_import_lists, lists.data(), lists.size() * 4, hipMemcpyHostToDevice));
    b->import_lists = lists;
    b->n_import_list_copies++;
    return 0;
}
uint64_t acvm_debug_import_list_copies(const acvm_batch_t *b) { return b ? b->n_import_list_copies : 0; }

// The parts one after the other, each with the rows, planes and columns of ITS inputs: from the list buffer, or -- a descriptor -- the handle's
// resident tables.
bool batch_launch_import(acvm_batch *b, const ImportPlan &plan, const uint32_t *gate) {
    if (plan.record_masks) {  // (the masked tables and the masked kernel; import_masked_and_wait made the missing set ready and is never gated)
        const uint32_t *windows = b->d_import_lists, *fields = windows + (size_t)plan.record_windows * RECORD_MWINDOW_WORDS;
        return launch_import_records_masked(b->stream, plan.d_records, plan.record_pitch, windows, plan.record_windows, fields, b->d_W, b->Bp, b->B,
                                            (uint32_t)b->plan().initial_ids.size(), b->d_byte_plane, b->d_event, b->d_missing, b->d_mask_result);
    }
    if (plan.records) {  // (no parts: one launch over the window and field tables of the list buffer)
        const uint32_t *windows = b->d_import_lists, *fields = windows + (size_t)plan.record_windows * RECORD_WINDOW_WORDS;
        return launch_import_records(b->stream, plan.d_records, plan.record_pitch, windows, plan.record_windows, fields, b->d_W, b->Bp, b->B, gate, b->d_byte_plane, b->d_event);
    }
    bool reset_written = false;
    for (const ImportPlanPart &pt : plan.parts) {
        if (!pt.n) continue;
        const uint32_t *lists = b->d_import_lists;
        const uint32_t *rows = pt.resident ? (b->reuse() ? b->d_init_rows : b->d_init_ids) : lists + pt.rows_at;
        const uint32_t *planes = pt.resident ? b->d_byte_plane_of_input : pt.planes_at != IMPORT_NO_LIST ? lists + pt.planes_at : nullptr;
        const uint32_t *columns = pt.columns_at != IMPORT_NO_LIST ? lists + pt.columns_at : nullptr;
        uint32_t *reset = reset_written ? nullptr : b->d_event;
        bool did;
        if (plan.plain) did = launch_import(b->stream, b->d_W, b->Bp, b->B, (const uint8_t *)pt.d_values, rows, pt.n, gate, planes, b->d_byte_plane, reset);
        else {
            const ImportDevice x{pt.encoding, pt.layout, columns, pt.stride, pt.d_values};
            const bool typed = pt.elem_size != 32u || pt.layout == EXPORT_LAYOUT_BROADCAST;
            did = (typed ? launch_import_typed : launch_import_device)(b->stream, x, b->d_W, b->Bp, b->B, rows, pt.n, gate, planes, b->d_byte_plane, reset);
        }
        reset_written = reset_written || did;
    }
    return reset_written;
}

// acvm_batch_solve_then_import(_ex) put exactly this import behind the previous solve, and it ran: the rows are there, in stream order. (Only a
// plan of one resident part rides behind a solve: the plan of parts never compares equal to it, and a record plan has no parts.)
static bool import_is_behind_solve(const acvm_batch *b, const ImportPlan &plan) {
    return b->next_imported && !plan.records && plan.parts.size() == 1 && b->next_inputs == plan.parts[0].d_values && b->next_plan == plan;
}
// The handle's state after an import. enqueued: by this call, and reset_written is batch_launch_import's answer (events_fresh's rule: batch.hpp);
// otherwise the import is the one behind the last solve, which set events_fresh itself.
static void import_epilogue(acvm_batch *b, bool enqueued, bool reset_written) {
    b->next_imported = false;
    b->next_inputs = nullptr;
    if (enqueued) b->events_fresh = reset_written;
    b->n_missing = 0;  // (every instance holds every input; a masked import says otherwise behind its mask pass: import_masked_and_wait)
    b->inputs_set = true;
    b->solved = false;
    b->stepping = false;
    clear_fc_store(b);
}

int batch_import_plan_async(acvm_batch *b, const ImportPlan &plan, hipEvent_t imported, bool *already) {
    HIPCHK(hipSetDevice(b->device));
    const bool behind = import_is_behind_solve(b, plan);
    if (already) *already = behind;
    if (!behind)
        if (int rc = import_lists_ready(b, plan)) return rc;
    const bool reset_written = !behind && batch_launch_import(b, plan, nullptr);
    import_epilogue(b, !behind, reset_written);
    HIPCHK(hipGetLastError());
    if (imported) HIPCHK(hipEventRecord(imported, b->stream));
    return 0;
}
int batch_import_async(acvm_batch *b, const void *d_values_be32, hipEvent_t imported) {
    return batch_import_plan_async(b, import_plan_plain((uint32_t)b->plan().initial_ids.size(), d_values_be32), imported, nullptr);
}
int batch_import_desc_async(acvm_batch *b, const acvm_import_desc_t *d, const void *d_values) {
    ImportPlan plan;
    if (int rc = import_plan_of(b, d, d_values, &plan)) return rc;
    return batch_import_plan_async(b, plan, nullptr, nullptr);
}
// the import and the wait of the public entry points: the caller may reuse its buffers as soon as the call returns (an import that ran behind
// the previous solve left the buffer alone since: nothing to wait for)
static int import_and_wait(acvm_batch *b, const ImportPlan &plan) {
    bool already = false;
    if (int rc = batch_import_plan_async(b, plan, nullptr, &already)) return rc;
    if (!already) HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}

int acvm_batch_set_initial_witness_device(acvm_batch_t *b, const void *d_values_be32) try {
    if (!b) return set_err(ACVM_E_INVALID, "null batch");
    return import_and_wait(b, import_plan_plain((uint32_t)b->plan().initial_ids.size(), d_values_be32));
} ABI_CATCH
int acvm_batch_set_initial_witness(acvm_batch_t *b, const uint8_t *values_be32) try {
    if (!b) return set_err(ACVM_E_INVALID, "null batch");
    size_t bytes = (size_t)b->B * b->plan().initial_ids.size() * 32;
    if (bytes && !values_be32) return set_err(ACVM_E_INVALID, "null values");
    HIPCHK(hipSetDevice(b->device));
    if (int rc = stage_reserve(b, bytes)) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(b->d_stage, values_be32, bytes, hipMemcpyHostToDevice, b->stream));
    return acvm_batch_set_initial_witness_device(b, b->d_stage);
} ABI_CATCH
// The import as the mirror image of acvm_batch_export_device: any encoding, layout, stride and column list (include/acvm_amd.h).
int acvm_batch_import_device(acvm_batch_t *b, const acvm_import_desc_t *d, const void *d_values) try {
    ImportPlan plan;
    if (int rc = import_plan_of(b, d, d_values, &plan)) return rc;
    return import_and_wait(b, plan);
} ABI_CATCH
// ---- the masked import (include/acvm_amd.h acvm_batch_import_device_masked): the value import as any other, the mask pass behind it on the
// batch's stream, and the few words it reports read back behind the wait the call makes anyway.
static int missing_set_ready(acvm_batch *b) {
    const size_t words = (size_t)import_missing_words((uint32_t)b->plan().initial_ids.size()) * b->Bp;
    if (!b->d_missing) {  // (zeroed once: a word no mask pass has written -- an instance beyond the live count -- says "holds everything")
        HIPCHK(hipMalloc((void **)&b->d_missing, (words ? words : 1) * 4));
        HIPCHK(hipMemset(b->d_missing, 0, (words ? words : 1) * 4));
    }
    if (!b->h_mask_result) HIPCHK(hipHostMalloc((void **)&b->h_mask_result, IMPORT_MASK_RESULT_WORDS * 8, hipHostMallocDefault));
    if (!b->d_mask_result) {
        HIPCHK(hipMalloc((void **)&b->d_mask_result, IMPORT_MASK_RESULT_WORDS * 8));
        HIPCHK(hipMemset(b->d_mask_result, 0, IMPORT_MASK_RESULT_WORDS * 8));
    }
    return 0;
}
// what: whose bytes a refusal speaks of ("d_assigned", "record mask bytes"). A masked record plan carries its masks inside the import's own launch
// (batch_launch_import); a descriptor's mask pass follows the value import here. Both end in the same wait, refusal and bookkeeping.
static int import_masked_and_wait(acvm_batch *b, const ImportPlan &plan, const char *what = "d_assigned") {
    if (!plan.masked() && !plan.record_masks) return import_and_wait(b, plan);
    HIPCHK(hipSetDevice(b->device));
    if (int rc = missing_set_ready(b)) return rc;  // (in front of everything: a refusal so far leaves the handle as it was)
    if (int rc = batch_import_plan_async(b, plan, nullptr, nullptr)) return rc;
    // (d_mask_result is zero here: since its allocation, or since the memset the previous masked import left behind on the stream)
    if (plan.masked()) {
        const ImportPlanPart &pt = plan.parts[0];  // (a descriptor's plan: one resident part)
        const uint32_t *columns = pt.columns_at != IMPORT_NO_LIST ? b->d_import_lists + pt.columns_at : nullptr;
        launch_import_mask(b->stream, ImportMaskSource{plan.d_assigned, pt.layout, columns, pt.stride}, b->d_W, b->Bp, b->B, b->reuse() ? b->d_init_rows : b->d_init_ids, pt.n,
                           b->d_byte_plane_of_input, b->d_byte_plane, b->d_missing, b->d_mask_result);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b->h_mask_result, b->d_mask_result, IMPORT_MASK_RESULT_WORDS * 8, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    const uint64_t result[IMPORT_MASK_RESULT_WORDS] = {b->h_mask_result[0], b->h_mask_result[1], b->h_mask_result[2]};
    // the words are zeroed for the next masked import behind this one's wait: not waited for, so the memset costs the caller nothing
    HIPCHK(hipMemsetAsync(b->d_mask_result, 0, IMPORT_MASK_RESULT_WORDS * 8, b->stream));
    if (result[IMPORT_MASK_BAD]) {
        // The host could not see the bytes beforehand and the rows are written: the handle is left without initial witnesses.
        b->inputs_set = false;
        const uint32_t j = import_mask_key_instance(result[IMPORT_MASK_BAD_KEY]), k = import_mask_key_position(result[IMPORT_MASK_BAD_KEY]);
        return set_err(ACVM_E_INVALID, std::string(what) + ": " + std::to_string(result[IMPORT_MASK_BAD]) + " elements are neither 0 nor 1, the first of them instance " + std::to_string(j) +
                                           ", position " + std::to_string(k) + " (initial witness " + std::to_string(b->plan().initial_ids[k]) +
                                           "); the handle is left without initial witnesses");
    }
    b->n_missing = result[IMPORT_MASK_MISSING];
    return 0;
}
int acvm_batch_import_device_masked(acvm_batch_t *b, const acvm_import_desc_t *d, const void *d_values, const uint8_t *d_assigned) try {
    ImportPlan plan;
    if (int rc = import_plan_of(b, d, d_values, &plan, d_assigned)) return rc;
    return import_masked_and_wait(b, plan);
} ABI_CATCH
// the host form: values and mask bytes through the staging buffer, then the device path -- BE32, instance-major, dense
int acvm_batch_set_initial_witness_masked(acvm_batch_t *b, const uint8_t *values_be32, const uint8_t *assigned) try {
    if (!b) return set_err(ACVM_E_INVALID, "null batch");
    const size_t elements = (size_t)b->B * b->plan().initial_ids.size(), bytes = elements * 32;
    if (bytes && !values_be32) return set_err(ACVM_E_INVALID, "null values");
    if (bytes && !assigned) return set_err(ACVM_E_INVALID, "null assigned");
    HIPCHK(hipSetDevice(b->device));
    if (int rc = stage_reserve(b, align256(bytes) + elements)) return rc;
    if (bytes) {
        HIPCHK(hipMemcpyAsync(b->d_stage, values_be32, bytes, hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(b->d_stage + align256(bytes), assigned, elements, hipMemcpyHostToDevice, b->stream));
    }
    ImportPlan plan = import_plan_plain((uint32_t)b->plan().initial_ids.size(), b->d_stage);
    if (bytes) plan.d_assigned = b->d_stage + align256(bytes);
    return import_masked_and_wait(b, plan);
} ABI_CATCH
uint64_t acvm_debug_import_missing(const acvm_batch_t *b) { return b ? b->n_missing : 0; }

// One import from several buffers (include/acvm_amd.h): every part is checked like a descriptor, nothing is enqueued before all have passed. The
// event reset is given to exactly one launch. A plan of parts never rides behind a solve, so this call always waits.
int acvm_batch_import_device_parts(acvm_batch_t *b, const acvm_import_part_t *parts, uint32_t n_parts) try {
    const ImportView view = b ? import_view(b) : ImportView{};
    ImportPlan plan;
    std::string err;
    if (int rc = import_plan_parts(b ? &view : nullptr, parts, n_parts, &plan, &err)) return set_err(rc, err);
    return import_and_wait(b, plan);
} ABI_CATCH

// ---- the record import (include/acvm_amd.h acvm_batch_import_device_records): the field list is checked and cut into windows by
// record_plan.cpp, the tables travel in the handle's one list buffer, one launch reads them. A record plan never rides behind a solve.
static int import_plan_records_of(const acvm_batch *b, const acvm_record_desc_t *d, const void *d_records, ImportPlan *out) {
    const ImportView view = b ? import_view(b) : ImportView{};
    std::string err;
    const int rc = import_plan_records(b ? &view : nullptr, d, d_records, out, &err);
    return rc ? set_err(rc, err) : 0;
}
int batch_import_records_async(acvm_batch *b, const acvm_record_desc_t *d, const void *d_records, hipEvent_t imported) {
    ImportPlan plan;
    if (int rc = import_plan_records_of(b, d, d_records, &plan)) return rc;
    return batch_import_plan_async(b, plan, imported, nullptr);
}
int acvm_batch_import_device_records(acvm_batch_t *b, const acvm_record_desc_t *d, const void *d_records) try {
    ImportPlan plan;
    if (int rc = import_plan_records_of(b, d, d_records, &plan)) return rc;
    return import_and_wait(b, plan);
} ABI_CATCH
// the host form: the records through the staging buffer, then the device path. The descriptor is judged first (with the caller's pointer: the
// null rule), so a refused call copies nothing.
int acvm_batch_set_initial_witness_records(acvm_batch_t *b, const acvm_record_desc_t *d, const void *records) try {
    ImportPlan plan;
    if (int rc = import_plan_records_of(b, d, records, &plan)) return rc;
    const size_t bytes = d->n_fields ? (size_t)b->B * d->pitch : 0;
    HIPCHK(hipSetDevice(b->device));
    if (int rc = stage_reserve(b, bytes)) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(b->d_stage, records, bytes, hipMemcpyHostToDevice, b->stream));
    plan.d_records = b->d_stage;
    return import_and_wait(b, plan);
} ABI_CATCH

// ---- the masked record import (include/acvm_amd.h acvm_batch_import_device_records_masked): record_plan.cpp checks and cuts, the masked kernel
// reads values and presence bytes in one pass, and the call ends as the masked column import ends (import_masked_and_wait). No field with a mask:
// the plan is the unmasked call's, and so is everything behind it.
static int import_plan_records_masked_of(const acvm_batch *b, const acvm_record_masked_desc_t *d, const void *d_records, ImportPlan *out) {
    const ImportView view = b ? import_view(b) : ImportView{};
    std::string err;
    const int rc = import_plan_records_masked(b ? &view : nullptr, d, d_records, out, &err);
    return rc ? set_err(rc, err) : 0;
}
// staged: the records lie in the caller's HOST memory and go through the staging buffer first (a refused descriptor copies nothing)
static int import_records_masked(acvm_batch_t *b, const acvm_record_masked_desc_t *d, const void *records, bool staged) {
    ImportPlan plan;
    if (int rc = import_plan_records_masked_of(b, d, records, &plan)) return rc;
    if (staged) {
        const size_t bytes = d->n_fields ? (size_t)b->B * d->pitch : 0;
        HIPCHK(hipSetDevice(b->device));
        if (int rc = stage_reserve(b, bytes)) return rc;
        if (bytes) HIPCHK(hipMemcpyAsync(b->d_stage, records, bytes, hipMemcpyHostToDevice, b->stream));
        plan.d_records = b->d_stage;
    }
    return import_masked_and_wait(b, plan, "record mask bytes");
}
int acvm_batch_import_device_records_masked(acvm_batch_t *b, const acvm_record_masked_desc_t *d, const void *d_records) try {
    return import_records_masked(b, d, d_records, false);
} ABI_CATCH
int acvm_batch_set_initial_witness_records_masked(acvm_batch_t *b, const acvm_record_masked_desc_t *d, const void *records) try {
    return import_records_masked(b, d, records, true);
} ABI_CATCH

// ---- the wire import (include/acvm_amd.h acvm_batch_import_device_wire): wire_in_plan.cpp checks the descriptor and makes the sorted id table
// and the CRC power table, which go up into the staging arena (nothing per instance); kernels_wire_in.hip reads the slots. It ends as the masked
// import ends (import_masked_and_wait): the same wait, the same few words read back, the same fail-closed refusal and bookkeeping. A wire import
// never rides behind a solve.
static const char *wire_in_class_text(uint32_t cls) {
    static const char *const text[WIRE_IN_CLASSES] = {"", "the count word cannot be a map of this slot", "an entry's length word is not 64", "a character that is not a hex digit",
                                                      "a key that is not an initial witness of this handle", "keys not strictly ascending",
                                                      "a framing word of the gzip member is not the pinned one", "the trailer's CRC-32 is not the body's"};
    return text[cls < WIRE_IN_CLASSES ? cls : 0];
}
// host_slots: the host form's staged BINCODE slots (B * plan.pitch bytes), which go up behind the tables; else d_bytes is the caller's.
// front: the bytes at the arena's start that are the caller's (the gzip import's scratch, which d_bytes and d_lengths then lie in: that caller
// has reserved front + wire_in_arena_bytes already, so the reservation here moves nothing).
static size_t wire_in_arena_bytes(const WireInPlan &plan, uint32_t B, size_t host_slot_bytes) {
    return align256(plan.keys.size() * 4) + align256(plan.positions.size() * 4) + align256(plan.crc_pow.size() * 4) +
           align256(plan.container == ACVM_WIRE_GZIP_STORED ? (size_t)B * 4 : 0) + align256(host_slot_bytes);
}
static int import_wire_and_wait(acvm_batch *b, const WireInPlan &plan, const void *d_bytes, const uint64_t *d_lengths, const std::vector<uint8_t> *host_slots,
                                size_t front = 0) {
    HIPCHK(hipSetDevice(b->device));
    if (int rc = missing_set_ready(b)) return rc;  // (in front of everything: a refusal so far leaves the handle as it was)
    const bool gzip = plan.container == ACVM_WIRE_GZIP_STORED;
    // the arena: [the caller's front][keys][positions][crc powers][crc words][host form: slots]
    size_t at = front;
    auto carve = [&](size_t n_bytes) { const size_t begin = at; at += align256(n_bytes); return begin; };
    const size_t at_keys = carve(plan.keys.size() * 4), at_positions = carve(plan.positions.size() * 4), at_pow = carve(plan.crc_pow.size() * 4);
    const size_t at_crc = carve(gzip ? (size_t)b->B * 4 : 0), at_slots = carve(host_slots ? host_slots->size() : 0);
    if (int rc = stage_reserve(b, at)) return rc;
    hipStream_t s = b->stream;
    auto put = [&](size_t where, const void *from, size_t n_bytes) -> hipError_t {
        return n_bytes ? hipMemcpyAsync(b->d_stage + where, from, n_bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIPCHK(put(at_keys, plan.keys.data(), plan.keys.size() * 4));
    HIPCHK(put(at_positions, plan.positions.data(), plan.positions.size() * 4));
    HIPCHK(put(at_pow, plan.crc_pow.data(), plan.crc_pow.size() * 4));
    if (host_slots) HIPCHK(put(at_slots, host_slots->data(), host_slots->size()));
    // (d_mask_result is zero here: since its allocation, or since the memset the previous masked or wire import left behind on the stream)
    const WireImport x{host_slots ? b->d_stage + at_slots : (const uint8_t *)d_bytes, plan.pitch, d_lengths, plan.container, b->B, plan.n_initial,
                       (const uint32_t *)(b->d_stage + at_keys), (const uint32_t *)(b->d_stage + at_positions), b->reuse() ? b->d_init_rows : b->d_init_ids,
                       b->d_byte_plane_of_input, b->d_byte_plane, b->d_W, b->Bp, b->d_event, b->d_missing, (uint32_t *)(b->d_stage + at_crc),
                       gzip ? (const uint32_t *)(b->d_stage + at_pow) : nullptr, plan.crc_x64, plan.rank_bits, b->d_mask_result};
    const bool reset_written = launch_wire_import(s, x, plan.n_windows);
    import_epilogue(b, true, reset_written);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b->h_mask_result, b->d_mask_result, IMPORT_MASK_RESULT_WORDS * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // (also what keeps the plan's tables and the staged slots alive for their copies)
    const uint64_t result[IMPORT_MASK_RESULT_WORDS] = {b->h_mask_result[0], b->h_mask_result[1], b->h_mask_result[2]};
    HIPCHK(hipMemsetAsync(b->d_mask_result, 0, IMPORT_MASK_RESULT_WORDS * 8, s));
    if (result[IMPORT_MASK_BAD]) {
        // The host could not see the bytes beforehand and rows are written: the handle is left without initial witnesses.
        b->inputs_set = false;
        const uint64_t key = result[IMPORT_MASK_BAD_KEY];
        const uint32_t cls = wire_in_key_class(key, plan.rank_bits);
        return set_err(ACVM_E_INVALID, "wire import: " + std::to_string(result[IMPORT_MASK_BAD]) + " findings, the first of them instance " +
                                           std::to_string(wire_in_key_instance(key, plan.rank_bits)) + ", class " + std::to_string(cls) + " (" + wire_in_class_text(cls) + "), entry " +
                                           std::to_string(wire_in_key_rank(key, plan.rank_bits)) + "; the handle is left without initial witnesses");
    }
    b->n_missing = result[IMPORT_MASK_MISSING];
    return 0;
}
static int wire_in_plan_of(const acvm_batch *b, const acvm_wire_in_desc_t *d, const void *bytes, bool device, WireInPlan *out) {
    std::string err;
    const int rc = wire_in_plan(b ? &b->B : nullptr, b ? b->plan().initial_ids.data() : nullptr, b ? (uint32_t)b->plan().initial_ids.size() : 0u, d, bytes, device, out, &err);
    return rc ? set_err(rc, err) : 0;
}
int acvm_batch_import_device_wire(acvm_batch_t *b, const acvm_wire_in_desc_t *d, const void *d_bytes, const uint64_t *d_lengths) try {
    WireInPlan plan;
    if (int rc = wire_in_plan_of(b, d, d_bytes, true, &plan)) return rc;
    return import_wire_and_wait(b, plan, d_bytes, d_lengths, nullptr);
} ABI_CATCH
// The host form: every row judged on the host (wire_in_plan.cpp) -- inflated where it is a gzip member, staged as it is where the device form
// reads it, through the reader and the writer where not -- and nothing enqueued before every row has passed.
int acvm_batch_set_initial_witness_maps_wire(acvm_batch_t *b, const uint8_t *bytes, uint64_t pitch, const uint64_t *lengths) try {
    const acvm_wire_in_desc_t d{ACVM_WIRE_BINCODE, pitch};
    WireInPlan plan;
    if (int rc = wire_in_plan_of(b, &d, bytes, false, &plan)) return rc;
    if (b->B && !lengths) return set_err(ACVM_E_INVALID, "null lengths");
    plan.pitch = wire_in_stage_pitch(plan.n_initial);
    std::vector<uint8_t> slots((size_t)b->B * plan.pitch), inflated, body, values;
    std::vector<uint32_t> ids;
    for (uint32_t j = 0; j < b->B; j++) {
        const uint8_t *row = bytes + (size_t)j * pitch;
        size_t len = (size_t)lengths[j];
        auto refuse = [&](const std::string &text) { return set_err(ACVM_E_INVALID, "instance " + std::to_string(j) + ": " + text); };
        if (len >= 2 && row[0] == 0x1f && row[1] == 0x8b) {
            if (!witness_map_inflate(row, len, inflated)) return refuse("gzip stream is corrupt");
            row = inflated.data();
            len = inflated.size();
        }
        if (!wire_in_body_canonical(plan, row, len)) {
            std::string err;
            if (!witness_map_from_bytes(row, len, ids, values, err)) return refuse(err);
            if (wire_in_body_of_map(plan, ids.data(), values.data(), ids.size(), &body, &err)) return refuse(err);
            row = body.data();
            len = body.size();
        }
        memcpy(&slots[(size_t)j * plan.pitch], row, len);
    }
    return import_wire_and_wait(b, plan, nullptr, nullptr, &slots);
} ABI_CATCH

// ---- the gzip import (include/acvm_amd.h acvm_batch_import_device_wire_gzip). Stage 1: kernels_wire_inflate.hip inflates every row into the
// arena's scratch and writes nothing of the handle; its two result words come back behind the one wait between the stages, and any finding
// ends the call with the handle as it was. Stage 2 is the body import above over the scratch, the inflater's lengths its d_lengths. The arena
// is reserved ONCE for both (wire_inflate_plan.hpp): a second reservation that grew it would free the scratch under stage 2.
static const char *inflate_class_text(uint32_t cls) {
    static const char *const text[INFLATE_CLASSES] = {"", "the head is not a gzip head", "block type 3", "a stored block's LEN is not ~NLEN", "a dynamic block's code description is invalid",
                                                      "bits that are no symbol of the block's code", "a distance beyond the bytes written", "the readable bytes end inside the member",
                                                      "more output than the handle's longest body", "the trailer's CRC-32 is not the output's", "the trailer's ISIZE is not the output's length"};
    return text[cls < INFLATE_CLASSES ? cls : 0];
}
// device: bytes / lengths are the caller's device memory; else host rows at `pitch`, staged compressed
static int import_wire_gzip(acvm_batch *b, const acvm_wire_in_desc_t *d, const void *bytes, const uint64_t *lengths, bool device) {
    uint64_t longest = 0;
    // (the host form's rows are looked at before the plan is made: it wants the longest of them. A pitch the plan will refuse is not walked.)
    if (!device && b && d && bytes && (unsigned __int128)b->B * d->pitch <= ((unsigned __int128)1 << 57)) {
        if (b->B && !lengths) return set_err(ACVM_E_INVALID, "null lengths");
        for (uint32_t j = 0; j < b->B; j++) {
            const uint8_t *row = (const uint8_t *)bytes + (size_t)j * d->pitch;
            const uint64_t n = std::min<uint64_t>(lengths[j], d->pitch);
            if (n < 2 || row[0] != 0x1f || row[1] != 0x8b) return set_err(ACVM_E_INVALID, "instance " + std::to_string(j) + ": the row does not start 1f 8b");
            longest = std::max(longest, n);
        }
    }
    WireInflatePlan plan;
    {
        std::string err;
        const int rc = wire_inflate_plan(b ? &b->B : nullptr, b ? b->plan().initial_ids.data() : nullptr, b ? (uint32_t)b->plan().initial_ids.size() : 0u, d, bytes, device,
                                         longest, &plan, &err);
        if (rc) return set_err(rc, err);
    }
    if (!b->B) return import_wire_and_wait(b, plan.body, nullptr, nullptr, nullptr);
    HIPCHK(hipSetDevice(b->device));
    if (int rc = missing_set_ready(b)) return rc;
    if (int rc = stage_reserve(b, plan.front + wire_in_arena_bytes(plan.body, b->B, 0))) return rc;
    hipStream_t s = b->stream;
    uint8_t *arena = b->d_stage;
    std::vector<uint8_t> staged;
    std::vector<uint64_t> staged_lengths;
    HIPCHK(hipMemsetAsync(arena + plan.at_result, 0, 16, s));
    HIPCHK(hipMemcpyAsync(arena + plan.at_fixed, plan.fixed.data(), plan.fixed.size() * 2, hipMemcpyHostToDevice, s));
    if (!device) {  // the rows as they are, compressed, at the staged pitch; their readable lengths beside them
        staged.assign((size_t)b->B * plan.pitch, 0);
        staged_lengths.resize(b->B);
        for (uint32_t j = 0; j < b->B; j++) {
            staged_lengths[j] = std::min<uint64_t>(lengths[j], d->pitch);
            memcpy(&staged[(size_t)j * plan.pitch], (const uint8_t *)bytes + (size_t)j * d->pitch, (size_t)staged_lengths[j]);
        }
        HIPCHK(hipMemcpyAsync(arena + plan.at_rows, staged.data(), staged.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(arena + plan.at_row_lengths, staged_lengths.data(), staged_lengths.size() * 8, hipMemcpyHostToDevice, s));
    }
    uint64_t *d_body_lengths = (uint64_t *)(arena + plan.at_lengths);
    const WireInflate x{device ? (const uint8_t *)bytes : arena + plan.at_rows, plan.pitch, device ? lengths : (const uint64_t *)(arena + plan.at_row_lengths), b->B,
                        arena + plan.at_scratch, plan.out_pitch, plan.out_cap, (uint32_t *)(arena + plan.at_tables), d_body_lengths, (uint32_t *)(arena + plan.at_findings), nullptr,
                        (const uint16_t *)(arena + plan.at_fixed), (uint64_t *)(arena + plan.at_result)};
    launch_wire_inflate(s, x);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b->h_mask_result, arena + plan.at_result, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // (the one wait between the stages; also what keeps the staged rows alive for their copy)
    const uint64_t n_findings = b->h_mask_result[0], key = b->h_mask_result[1];
    if (n_findings) {
        const uint32_t cls = inflate_key_class(key);
        return set_err(ACVM_E_INVALID, "wire inflate: " + std::to_string(n_findings) + " findings, the first of them instance " + std::to_string(inflate_key_instance(key)) + ", class " +
                                           std::to_string(cls) + " (" + inflate_class_text(cls) + "), block " + std::to_string(inflate_key_block(key)) + "; the handle stays as it was");
    }
    return import_wire_and_wait(b, plan.body, arena + plan.at_scratch, d_body_lengths, nullptr, plan.front);
}
int acvm_batch_import_device_wire_gzip(acvm_batch_t *b, const acvm_wire_in_desc_t *d, const void *d_bytes, const uint64_t *d_lengths) try {
    return import_wire_gzip(b, d, d_bytes, d_lengths, true);
} ABI_CATCH
int acvm_batch_set_initial_witness_maps_gzip(acvm_batch_t *b, const uint8_t *bytes, uint64_t pitch, const uint64_t *lengths) try {
    const acvm_wire_in_desc_t d{ACVM_WIRE_GZIP_DEFLATE, pitch};
    return import_wire_gzip(b, &d, bytes, lengths, false);
} ABI_CATCH

// ---- the packed import (include/acvm_amd.h acvm_batch_import_device_wire_packed): row j is bytes [offsets[j], offsets[j + 1]) of one buffer.
// kernels_wire_pack.hip judges the offsets -- untrusted device data -- and unpacks the rows that pass into pitched slots of the handle's own
// (d_unpack: d_stage is the import's behind it, which may move it); nothing of the handle is written before the one wait, and any finding ends
// the call there. Then the device import of the container runs over the slots, the rows' lengths its d_lengths.
static const char *offsets_class_text(uint32_t cls) {
    static const char *const text[REPITCH_CLASSES] = {"", "the row's end lies in front of its start", "the row ends beyond the buffer", "the row is longer than the pitch"};
    return text[cls < REPITCH_CLASSES ? cls : 0];
}
int acvm_batch_import_device_wire_packed(acvm_batch_t *b, const acvm_wire_in_desc_t *d, const void *d_bytes, uint64_t n_bytes, const uint64_t *d_offsets) try {
    // the descriptor and the buffer are judged by the plan of the import that will read the slots
    const bool deflate = d && d->container == ACVM_WIRE_GZIP_DEFLATE;
    WireInPlan plan;
    if (deflate) {
        WireInflatePlan inflate;
        std::string err;
        if (int rc = wire_inflate_plan(b ? &b->B : nullptr, b ? b->plan().initial_ids.data() : nullptr, b ? (uint32_t)b->plan().initial_ids.size() : 0u, d, d_bytes, true, 0, &inflate, &err))
            return set_err(rc, err);
    } else if (int rc = wire_in_plan_of(b, d, d_bytes, true, &plan)) return rc;
    if (b->B && !d_offsets) return set_err(ACVM_E_INVALID, "null offsets");
    if (!b->B) return deflate ? import_wire_gzip(b, d, d_bytes, nullptr, true) : import_wire_and_wait(b, plan, d_bytes, nullptr, nullptr);
    HIPCHK(hipSetDevice(b->device));
    // d_unpack: [result: 2 words][lengths][slots]
    const size_t at_lengths = 256, at_slots = at_lengths + align256((size_t)b->B * 8), need = at_slots + (size_t)b->B * d->pitch;
    if (need > b->unpack_cap) {
        HIPCHK(hipStreamSynchronize(b->stream));
        if (b->d_unpack) { hipFree(b->d_unpack); b->d_unpack = nullptr; b->unpack_cap = 0; }
        HIPCHK(hipMalloc((void **)&b->d_unpack, need));
        b->unpack_cap = need;
    }
    hipStream_t s = b->stream;
    uint64_t *d_result = (uint64_t *)b->d_unpack, *d_lengths = (uint64_t *)(b->d_unpack + at_lengths);
    uint8_t *d_slots = b->d_unpack + at_slots;
    HIPCHK(hipMemsetAsync(d_result, 0, 16, s));
    launch_wire_offsets(s, d_offsets, b->B, n_bytes, d->pitch, d_lengths, nullptr, d_result);
    launch_wire_repitch(s, WireRepitch{b->B, (const uint8_t *)d_bytes, 0u, d_offsets, n_bytes, 0u, nullptr, d_slots, d->pitch, nullptr, 0u, 0u, 0u, wire_repitch_units(d->pitch)});
    HIPCHK(hipGetLastError());
    uint64_t result[2] = {0u, 0u};
    HIPCHK(hipMemcpyAsync(result, d_result, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // (the one wait in front of the import)
    if (result[0]) {
        const uint32_t cls = wire_offsets_key_class(result[1]);
        return set_err(ACVM_E_INVALID, "wire offsets: " + std::to_string(result[0]) + " findings, the first of them instance " + std::to_string(wire_offsets_key_instance(result[1])) +
                                           ", class " + std::to_string(cls) + " (" + offsets_class_text(cls) + "); the handle stays as it was");
    }
    return deflate ? import_wire_gzip(b, d, d_slots, d_lengths, true) : import_wire_and_wait(b, plan, d_slots, d_lengths, nullptr);
} ABI_CATCH

// The shipped scan, offsets check and repitch kernel through their launchers on rows of the caller's, no handle (include/acvm_amd.h). Both
// buffers start on the device as the caller's, so that what the kernels leave alone comes back as it went in.
int acvm_debug_wire_repitch(uint32_t unpack, uint32_t n, uint64_t pitch, uint8_t *rows, uint64_t *lengths, uint8_t *packed, uint64_t packed_bytes, uint32_t displacement,
                            uint64_t *offsets, uint64_t capacity, uint32_t scan_chunk, uint32_t *findings, uint64_t *result) try {
    if (!offsets || !result || (n && !lengths) || (n && pitch && !rows) || (packed_bytes && !packed) || (unpack && n && !findings)) return set_err(ACVM_E_INVALID, "null argument");
    if (displacement > 15u) return set_err(ACVM_E_INVALID, "displacement " + std::to_string(displacement) + " is above 15");
    if ((unsigned __int128)n * pitch > ((unsigned __int128)1 << 36) || packed_bytes > ((uint64_t)1 << 36)) return set_err(ACVM_E_INVALID, "too large for this probe");
    if (!unpack) {
        if (capacity > packed_bytes) return set_err(ACVM_E_INVALID, "capacity " + std::to_string(capacity) + " is above the packed buffer's " + std::to_string(packed_bytes) + " bytes");
        for (uint32_t i = 0; i < n; i++)
            if (lengths[i] > pitch) return set_err(ACVM_E_INVALID, "row " + std::to_string(i) + ": length " + std::to_string(lengths[i]) + " is above the pitch " + std::to_string(pitch));
    }
    struct Mem {
        void *p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Mem() {
            for (void *q : p)
                if (q) hipFree(q);
        }
    } m;
    const size_t row_bytes = (size_t)n * pitch;
    const size_t sizes[5] = {row_bytes + 16, (size_t)packed_bytes + 32, ((size_t)n + 1) * 8, ((size_t)n + 1) * 8, REPITCH_STATE_WORDS * 8 + (size_t)n * 4 + 4};
    for (int k = 0; k < 5; k++) HIPCHK(hipMalloc(&m.p[k], sizes[k]));
    uint8_t *d_rows = (uint8_t *)m.p[0], *d_packed = (uint8_t *)m.p[1] + displacement;
    uint64_t *d_lengths = (uint64_t *)m.p[2], *d_offsets = (uint64_t *)m.p[3], *d_state = (uint64_t *)m.p[4];
    uint32_t *d_findings = (uint32_t *)(d_state + REPITCH_STATE_WORDS);
    if (row_bytes) HIPCHK(hipMemcpy(d_rows, rows, row_bytes, hipMemcpyHostToDevice));
    if (packed_bytes) HIPCHK(hipMemcpy(d_packed, packed, packed_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_state, 0, REPITCH_STATE_WORDS * 8));
    if (!unpack) {
        if (n) HIPCHK(hipMemcpy(d_lengths, lengths, (size_t)n * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(d_offsets, 0, 8));
        const uint32_t chunk = scan_chunk ? scan_chunk : std::max(n, 1u);
        for (uint32_t done = 0; done < n; done += chunk) {
            const uint32_t rows_now = std::min(chunk, n - done);
            const uint8_t *from = d_rows + (size_t)done * pitch;
            launch_wire_scan(nullptr, d_lengths + done, rows_now, d_offsets + done, capacity, d_state);
            launch_wire_repitch(nullptr, WireRepitch{rows_now, from, pitch, nullptr, (uint64_t)rows_now * pitch, (uint32_t)((uintptr_t)from & 15u), d_lengths + done, d_packed, 0u,
                                                     d_offsets + done, 0u, capacity, (uint32_t)((uintptr_t)d_packed & 15u), wire_repitch_units(pitch)});
        }
    } else {
        HIPCHK(hipMemcpy(d_offsets, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
        launch_wire_offsets(nullptr, d_offsets, n, packed_bytes, pitch, d_lengths, d_findings, d_state);
        launch_wire_repitch(nullptr, WireRepitch{n, d_packed, 0u, d_offsets, packed_bytes, (uint32_t)((uintptr_t)d_packed & 15u), nullptr, d_rows, pitch, nullptr, 0u, 0u,
                                                 (uint32_t)((uintptr_t)d_rows & 15u), wire_repitch_units(pitch)});
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (row_bytes) HIPCHK(hipMemcpy(rows, d_rows, row_bytes, hipMemcpyDeviceToHost));
    if (packed_bytes) HIPCHK(hipMemcpy(packed, d_packed, packed_bytes, hipMemcpyDeviceToHost));
    if (!unpack) HIPCHK(hipMemcpy(offsets, d_offsets, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
    if (unpack && n) {
        HIPCHK(hipMemcpy(lengths, d_lengths, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(findings, d_findings, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(result, d_state, REPITCH_STATE_WORDS * 8, hipMemcpyDeviceToHost));
    return 0;
} ABI_CATCH

// The shipped inflater through its launcher on rows of the caller's, no handle (include/acvm_amd.h). The device's output starts as the caller's
// `out`, so that what the kernel leaves alone comes back as it went in.
int acvm_debug_inflate_rows(const uint8_t *rows, uint64_t pitch, const uint64_t *lengths, uint32_t n, uint64_t out_cap, uint8_t *out, uint64_t *out_lengths,
                            uint32_t *findings, uint32_t *crcs) try {
    if (n && (!rows || (!out && out_cap) || !out_lengths || !findings)) return set_err(ACVM_E_INVALID, "null argument");
    if (n && !pitch) return set_err(ACVM_E_INVALID, "pitch 0");
    if (out_cap % 4) return set_err(ACVM_E_INVALID, "out_cap " + std::to_string(out_cap) + " is not a multiple of 4");
    if ((unsigned __int128)n * pitch > ((unsigned __int128)1 << 40) || (unsigned __int128)n * out_cap > ((unsigned __int128)1 << 40)) return set_err(ACVM_E_INVALID, "too large for this probe");
    if (!n) return 0;
    struct Mem {
        void *p[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Mem() {
            for (void *q : p)
                if (q) hipFree(q);
        }
    } m;
    const std::vector<uint16_t> fixed = wire_inflate_fixed_tables();
    const size_t in_bytes = (size_t)n * pitch, out_bytes = (size_t)n * out_cap;
    const size_t sizes[8] = {in_bytes, (size_t)n * 8, out_bytes ? out_bytes : 4, (size_t)n * 8, (size_t)n * 8, (size_t)n * 4, fixed.size() * 2, (size_t)n * INFLATE_PLAN_ROW_WORDS * 4};
    for (int k = 0; k < 8; k++) HIPCHK(hipMalloc(&m.p[k], sizes[k]));
    HIPCHK(hipMemcpy(m.p[0], rows, in_bytes, hipMemcpyHostToDevice));
    if (lengths) HIPCHK(hipMemcpy(m.p[1], lengths, (size_t)n * 8, hipMemcpyHostToDevice));
    if (out_bytes) HIPCHK(hipMemcpy(m.p[2], out, out_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(m.p[6], fixed.data(), fixed.size() * 2, hipMemcpyHostToDevice));
    const WireInflate x{(const uint8_t *)m.p[0], pitch, lengths ? (const uint64_t *)m.p[1] : nullptr, n, (uint8_t *)m.p[2], out_cap, out_cap, (uint32_t *)m.p[7], (uint64_t *)m.p[3], (uint32_t *)m.p[4],
                        (uint32_t *)m.p[5], (const uint16_t *)m.p[6], nullptr};
    launch_wire_inflate(nullptr, x);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (out_bytes) HIPCHK(hipMemcpy(out, m.p[2], out_bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_lengths, m.p[3], (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(findings, m.p[4], (size_t)n * 8, hipMemcpyDeviceToHost));
    if (crcs) HIPCHK(hipMemcpy(crcs, m.p[5], (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
} ABI_CATCH

// What the last import left (include/acvm_amd.h): rows, planes, event words and missing set of the live instances, for the tests that compare two
// import entry points bit for bit.
int acvm_debug_import_state(acvm_batch_t *b, uint32_t *rows, uint32_t *planes, uint32_t *events, uint32_t *missing) try {
    if (!b) return set_err(ACVM_E_INVALID, "null batch");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    const Plan &p = b->plan();
    const uint32_t n_in = (uint32_t)p.initial_ids.size(), B = b->B;
    for (uint32_t k = 0; k < n_in && B; k++) {
        const uint32_t row = b->reuse() ? b->init_rows[k] : p.initial_ids[k];
        if (rows)
            for (uint32_t half = 0; half < 2; half++)
                HIPCHK(hipMemcpy(rows + ((size_t)k * 2 + half) * B * 4, b->d_W + ((uint64_t)row * 2 + half) * b->Bp, (size_t)B * 16, hipMemcpyDeviceToHost));
        if (planes) {
            const uint32_t pl = p.n_byte_planes ? b->plane_of_input[k] : 0xFFFFFFFFu;
            if (pl == 0xFFFFFFFFu) std::fill(planes + (size_t)k * B, planes + (size_t)(k + 1) * B, 0u);
            else HIPCHK(hipMemcpy(planes + (size_t)k * B, b->d_byte_plane + (uint64_t)pl * b->Bp, (size_t)B * 4, hipMemcpyDeviceToHost));
        }
    }
    if (events) {
        HIPCHK(hipMemcpy(events, b->d_event - 4, 8, hipMemcpyDeviceToHost));
        if (B) HIPCHK(hipMemcpy(events + 2, b->d_event, (size_t)B * 4, hipMemcpyDeviceToHost));
    }
    if (missing)
        for (uint32_t word = 0; word < import_missing_words(n_in) && B; word++) {
            if (!b->d_missing) std::fill(missing + (size_t)word * B, missing + (size_t)(word + 1) * B, 0u);
            else HIPCHK(hipMemcpy(missing + (size_t)word * B, b->d_missing + (uint64_t)word * b->Bp, (size_t)B * 4, hipMemcpyDeviceToHost));
        }
    return 0;
} ABI_CATCH
