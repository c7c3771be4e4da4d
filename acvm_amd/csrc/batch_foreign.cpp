// batch_foreign.cpp -- the Brillig foreign-call round trip for the whole batch (include/acvm_amd.h acvm_batch_foreign_call_sites,
// acvm_batch_foreign_call_inputs_device, acvm_batch_resolve_foreign_calls_device, acvm_batch_resolve_foreign_calls_device_rows): the pending inputs of
// the waiting instances leave as device columns and the answers are appended to the result store where it lives (kernels_foreign.hip). Every check of what the caller hands over is foreign_plan.cpp's;
// this file owns the store: a slot starts host-built (FcSlot::inst, batch_exact.cpp upload_fc_tables) and becomes device-owned at the first batch-wide
// resolve into it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "batch_internal.hpp"
#include "foreign_plan.hpp"

static std::vector<FcLaneRecord> lane_records(const acvm_batch *b) {
    std::vector<FcLaneRecord> lanes;
    if (!b->solved) return lanes;
    lanes.resize(std::min(b->slow_ids.size(), b->slow_res.size()));
    for (size_t t = 0; t < lanes.size(); t++) {
        const SlowResult &sr = b->slow_res[t];
        lanes[t].instance = b->slow_ids[t];
        lanes[t].status = sr.status;
        lanes[t].opcode_index = sr.opcode_index;
        lanes[t].brillig_index = sr.x0;
        lanes[t].resolved_new = t < b->fc_lane.size() && b->fc_lane[t].resolved_new;
    }
    return lanes;
}
static bool is_internal(const std::string &function) { return function.compare(0, strlen(PLAN_FC_INTERNAL_PREFIX), PLAN_FC_INTERNAL_PREFIX) == 0; }
static std::vector<FcSiteDecl> site_decls(const Plan &p) {
    std::vector<FcSiteDecl> decls;
    for (auto &kv : p.fc_function) {
        FcSiteDecl d;
        d.opcode_index = (uint32_t)(kv.first >> 32);
        d.brillig_index = (uint32_t)kv.first;
        auto n = p.fc_n_inputs.find(kv.first);
        d.n_inputs = n == p.fc_n_inputs.end() ? 0u : n->second;
        d.function = kv.second;
        d.internal = is_internal(kv.second);
        decls.push_back(std::move(d));
    }
    return decls;
}
static FcHandleView handle_view(const acvm_batch *b, uint32_t opcode_index, uint32_t brillig_index) {
    FcHandleView v;
    v.solved = b->solved;
    v.has_solver = b->has_solver;
    auto it = b->plan().fc_function.find(((uint64_t)opcode_index << 32) | brillig_index);
    v.site_internal = it != b->plan().fc_function.end() && is_internal(it->second);
    return v;
}
// device time between the two events of the last batch-wide kernel (recorded around it on the batch's stream, which has been waited for)
static int fc_events(acvm_batch *b) {
    for (hipEvent_t &e : b->ev_fc)
        if (!e) HIPCHK(hipEventCreate(&e));
    return 0;
}

// The (lane, instance) pairs of rows [first_row, first_row + n_rows) of a site on the device, in a buffer of the handle's own. A waiting list is fixed from
// one solve to the next, so the pairs of the last range stay valid until the lanes change (acvm_batch::fc_epoch: any solve or step, new
// inputs) and the sizing call, the inputs call and the resolve of one range upload them once -- 8 bytes per row and round, not per call.
static int rows_on_device(acvm_batch *b, const std::vector<FcRow> &list, uint32_t opcode_index, uint32_t brillig_index, uint32_t first_row, uint32_t n_rows, bool *cached) {
    const uint64_t key[4] = {b->fc_epoch, ((uint64_t)opcode_index << 32) | brillig_index, first_row, n_rows};
    *cached = b->fc_rows_valid && !memcmp(key, b->fc_rows_key, sizeof key);
    if (*cached) return 0;
    b->fc_rows_valid = false;
    b->fc_rows_longest_valid = false;
    b->fc_rows_host.resize((size_t)n_rows * 2);
    for (uint32_t r = 0; r < n_rows; r++) {
        b->fc_rows_host[2 * (size_t)r] = list[first_row + r].lane;
        b->fc_rows_host[2 * (size_t)r + 1] = list[first_row + r].instance;
    }
    if (b->fc_rows_host.size() > b->fc_rows_cap) {
        if (b->d_fc_rows) hipFree(b->d_fc_rows);
        b->d_fc_rows = nullptr;
        b->fc_rows_cap = 0;
        const size_t cap = b->fc_rows_host.size() + b->fc_rows_host.size() / 4 + 64;
        HIPCHK(hipMalloc((void **)&b->d_fc_rows, cap * 4));
        b->fc_rows_cap = cap;
    }
    // (fc_rows_host lives in the handle: the copy may read it until the stream is next waited for, which every caller does before it returns)
    HIPCHK(hipMemcpyAsync(b->d_fc_rows, b->fc_rows_host.data(), b->fc_rows_host.size() * 4, hipMemcpyHostToDevice, b->stream));
    b->n_fc_h2d_bytes += b->fc_rows_host.size() * 4;
    memcpy(b->fc_rows_key, key, sizeof key);
    b->fc_rows_valid = true;
    return 0;
}

int acvm_batch_foreign_call_sites(acvm_batch_t *b, acvm_foreign_call_site_t *out, uint32_t cap) try {
    if (!b || (cap && !out)) return set_err(ACVM_E_INVALID, "null argument");
    const std::vector<FcLaneRecord> lanes = lane_records(b);
    const std::vector<acvm_foreign_call_site_t> sites = foreign_sites(site_decls(b->plan()), lanes.data(), lanes.size());
    for (size_t i = 0; i < sites.size() && i < cap; i++) out[i] = sites[i];
    return (int)sites.size();
} ABI_CATCH

int acvm_batch_foreign_call_inputs_device(acvm_batch_t *b, const acvm_foreign_call_inputs_desc_t *d, uint32_t *max_values) try {
    if (!b || !d) return set_err(ACVM_E_INVALID, "null argument");
    const std::vector<FcLaneRecord> lanes = lane_records(b);
    const std::vector<FcRow> list = foreign_waiting_list(lanes.data(), lanes.size(), d->opcode_index, d->brillig_index);
    const FcHandleView view = handle_view(b, d->opcode_index, d->brillig_index);
    uint64_t stride = 0;
    std::string refusal;
    if (int rc = foreign_check_inputs(&view, d, list, &stride, &refusal)) return set_err(rc, refusal);
    if (max_values) *max_values = 0;
    const uint32_t n_rows = d->n_rows, n_slow = (uint32_t)b->slow_ids.size();
    if (!n_rows) return 0;
    HIPCHK(hipSetDevice(b->device));
    if (int rc = fc_events(b)) return rc;
    hipStream_t s = b->stream;
    bool cached = false;
    if (int rc = rows_on_device(b, list, d->opcode_index, d->brillig_index, d->first_row, n_rows, &cached)) return rc;
    const uint32_t *d_rows = b->d_fc_rows;
    const FcLanes fc{b->d_fc_pend_desc, b->fc_pend_desc_words, b->d_fc_pend_vals, b->fc_pend_vals_cap};
    // the longest row: found on the device once per range and round (the sizing call; the inputs call behind it finds it here)
    if (!b->fc_rows_longest_valid) {
        if (int rc = stage_reserve(b, 256)) return rc;
        uint32_t *d_max = (uint32_t *)b->d_stage;
        HIPCHK(hipMemsetAsync(d_max, 0, 4, s));
        launch_fc_inputs_max(s, fc, n_slow, d_rows, n_rows, d_max);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&b->fc_rows_longest, d_max, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        b->n_fc_d2h_bytes += 4;
        b->fc_rows_longest_valid = true;
    }
    const uint32_t longest = b->fc_rows_longest;
    if (max_values) *max_values = longest;
    if (int rc = foreign_check_width(d, longest, &refusal)) return set_err(rc, refusal);  // (nothing of the caller's has been written)
    if (!d->d_instances && !d->d_lens && !d->d_values && !d->d_mask) return 0;
    auto n_in = b->plan().fc_n_inputs.find(((uint64_t)d->opcode_index << 32) | d->brillig_index);
    const FcInputsOut o{d_rows, n_rows, n_in == b->plan().fc_n_inputs.end() ? 0u : n_in->second, d->encoding, d->layout, d->n_columns, stride,
                        d->d_instances, d->d_lens, (uint8_t *)d->d_values, d->d_mask};
    HIPCHK(hipEventRecord(b->ev_fc[0], s));
    launch_fc_inputs(s, fc, n_slow, o);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(b->ev_fc[1], s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, b->ev_fc[0], b->ev_fc[1]));
    b->fc_inputs_ms = ms;
    return 0;
} ABI_CATCH

// ---- the store
// the kernels reach the tables through d_fc_store: refreshed when a slot's pointers moved
static int refresh_fc_store(acvm_batch *b, hipStream_t s) {
    if (!b->d_fc_store) return 0;
    std::vector<FcStoreSlot> tab(b->fc_slots.size());
    for (size_t si = 0; si < tab.size(); si++) tab[si] = FcStoreSlot{b->fc_slots[si].d_desc, b->fc_slots[si].d_vals};
    HIPCHK(hipMemcpyAsync(b->d_fc_store, tab.data(), tab.size() * sizeof(FcStoreSlot), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // (`tab` lives until here)
    b->n_fc_h2d_bytes += tab.size() * sizeof(FcStoreSlot);
    return 0;
}
// host-built -> device-owned: what the host holds of the slot goes up once (if it changed since its last upload), then only the bounds are kept
static int slot_to_device(acvm_batch *b, acvm_batch::FcSlot &sl) {
    if (sl.device_owned) return 0;
    uint32_t words = 1, vals = 0;
    for (auto &kv : sl.inst) {
        uint32_t dw = 1, nv = 0;
        for (auto &res : kv.second) {
            dw += 1 + 2 * (uint32_t)res.size();
            for (auto &v : res) nv += (uint32_t)v.vals.size();
        }
        words = std::max(words, dw);
        vals = std::max(vals, nv);
    }
    if (sl.dirty)
        if (int rc = upload_fc_tables(b, (uint32_t)b->slow_ids.size())) return rc;
    sl.inst.clear();
    sl.bounds = FcBounds();
    sl.bounds.words = words;
    sl.bounds.vals = vals;
    sl.device_owned = true;
    return 0;
}
// the slot's tables hold one more result of `add_words` words and `add_vals` values in every column: they grow by allocating, copying the prefix device
// to device -- the layouts [w][Bp] and [2 v + h][Bp] make a prefix copy sufficient -- and zeroing the rest
static int slot_reserve(acvm_batch *b, acvm_batch::FcSlot &sl, uint32_t add_words, uint32_t add_vals) {
    const FcCapacity have{sl.d_desc ? sl.desc_words : 0u, sl.d_vals ? sl.vals_cap : 0u};
    FcCapacity want;
    bool grow = false;
    std::string refusal;
    if (int rc = foreign_capacity(sl.bounds, add_words, add_vals, have, &grow, &want, &refusal)) return set_err(rc, refusal);
    if (!grow) return 0;
    hipStream_t s = b->stream;
    const size_t old_desc = (size_t)have.desc_words * b->Bp * 4, new_desc = (size_t)want.desc_words * b->Bp * 4;
    const size_t old_vals = (size_t)have.vals_cap * 2 * b->Bp * sizeof(uint4), new_vals = (size_t)want.vals_cap * 2 * b->Bp * sizeof(uint4);
    uint32_t *desc = nullptr;
    uint4 *vals = nullptr;
    HIPCHK(hipMalloc((void **)&desc, new_desc));
    if (hipMalloc((void **)&vals, new_vals) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(desc);
        return set_err(ACVM_E_DEVICE, "no device memory for the foreign-call results of " + std::to_string(want.vals_cap) + " values per instance");
    }
    hipError_t e = hipSuccess;
    if (old_desc) e = hipMemcpyAsync(desc, sl.d_desc, old_desc, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)desc + old_desc, 0, new_desc - old_desc, s);
    if (e == hipSuccess && old_vals) e = hipMemcpyAsync(vals, sl.d_vals, old_vals, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)vals + old_vals, 0, new_vals - old_vals, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        hipFree(desc);
        hipFree(vals);
        return set_err(ACVM_E_DEVICE, std::string("growing the foreign-call result store: ") + hipGetErrorString(e));
    }
    for (void *q : {(void *)sl.d_desc, (void *)sl.d_vals})
        if (q) hipFree(q);
    sl.d_desc = desc;
    sl.d_vals = vals;
    sl.desc_words = want.desc_words;
    sl.vals_cap = want.vals_cap;
    return refresh_fc_store(b, s);
}

// the per-row form of an append: only the rows of `resumed` are answered
struct FcRowsForm {
    const uint32_t *d_lens;
    const uint8_t *d_answered;
    uint32_t n_columns;
    const std::vector<uint32_t> *resumed;  // pairs (lane, instance) of the answered rows (foreign_mask_resumes)
};
// what one append is given
struct FcAppendCall {
    size_t si = 0;                                 // the slot
    const std::vector<uint32_t> *pairs = nullptr;  // (lane, instance) per listed row
    const uint32_t *d_rows_ready = nullptr;        // the pairs on the device already, or null
    const std::vector<uint32_t> *words = nullptr;  // the shape words
    uint32_t total = 0;                            // values per row: the shape's total -- with rows_form the LARGEST total of an answered row
    uint32_t encoding = 0, layout = 0;
    uint64_t stride = 0;
    const void *d_values = nullptr;                // the caller's device buffer, or
    const uint8_t *h_values = nullptr;             // host values staged here (h_bytes of them)
    size_t h_bytes = 0;
    const FcRowsForm *rows_form = nullptr;         // the per-row form, or null
};
// One result of the shape `words` appended for the listed rows from a device buffer -- the caller's, or h_values staged here (fc_append_one_instance).
// Marks the lanes answered.
static int append_rows(acvm_batch *b, const FcAppendCall &c) {
    const size_t si = c.si, h_bytes = c.h_bytes;
    const std::vector<uint32_t> &pairs = *c.pairs, &words = *c.words;
    const uint32_t *d_rows_ready = c.d_rows_ready;
    const uint32_t total = c.total, encoding = c.encoding, layout = c.layout;
    const uint64_t stride = c.stride;
    const void *d_values = c.d_values;
    const uint8_t *h_values = c.h_values;
    const FcRowsForm *rows_form = c.rows_form;
    const uint32_t n_rows = (uint32_t)(pairs.size() / 2);
    if (!n_rows) return 0;
    HIPCHK(hipSetDevice(b->device));
    if (int rc = fc_events(b)) return rc;
    acvm_batch::FcSlot &sl = b->fc_slots[si];
    if (int rc = slot_to_device(b, sl)) return rc;
    if (int rc = slot_reserve(b, sl, (uint32_t)words.size(), total)) return rc;
    hipStream_t s = b->stream;
    // arena: rows | shape words | the refused count | staged values
    const size_t o_shape = align256(pairs.size() * 4), o_refused = o_shape + align256(words.size() * 4), o_values = o_refused + 256;
    if (int rc = stage_reserve(b, o_values + align256(h_bytes))) return rc;
    const uint32_t *d_rows = d_rows_ready ? d_rows_ready : (const uint32_t *)b->d_stage;
    uint32_t *d_shape = (uint32_t *)(b->d_stage + o_shape), *d_refused = (uint32_t *)(b->d_stage + o_refused);
    if (!d_rows_ready) HIPCHK(hipMemcpyAsync(b->d_stage, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_shape, words.data(), words.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_refused, 0, 4, s));
    if (h_values && h_bytes) {
        HIPCHK(hipMemcpyAsync(b->d_stage + o_values, h_values, h_bytes, hipMemcpyHostToDevice, s));
        d_values = b->d_stage + o_values;
    }
    b->n_fc_h2d_bytes += ((d_rows_ready ? 0 : pairs.size()) + words.size()) * 4 + h_bytes;
    const FcAppend a{sl.d_desc, sl.d_vals, b->Bp, sl.desc_words, sl.vals_cap, d_rows, n_rows, d_shape, total, encoding, layout, stride, d_values, d_refused};
    HIPCHK(hipEventRecord(b->ev_fc[0], s));
    if (rows_form) launch_fc_append_rows(s, FcAppendRows{a, rows_form->d_lens, rows_form->d_answered, rows_form->n_columns});
    else launch_fc_append(s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(b->ev_fc[1], s));
    uint32_t refused = 0;
    HIPCHK(hipMemcpyAsync(&refused, d_refused, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    b->n_fc_d2h_bytes += 4;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, b->ev_fc[0], b->ev_fc[1]));
    b->fc_append_ms = ms;
    // (the bounds make room for every column before the launch: a refused row means they no longer describe the tables)
    if (refused) return set_err(ACVM_E_DEVICE, "the foreign-call result store refused " + std::to_string(refused) + " rows: its capacity bounds are broken");
    foreign_bounds_add(&sl.bounds, (uint32_t)words.size(), total);  // (per round, not per call: fc_round_consumed folds it in)
    if (b->fc_lane.size() < b->slow_ids.size()) b->fc_lane.resize(b->slow_ids.size());
    const std::vector<uint32_t> &answered = rows_form ? *rows_form->resumed : pairs;
    for (size_t r = 0; r < answered.size() / 2; r++) b->fc_lane[answered[2 * r]].resolved_new = true;
    return 0;
}

int acvm_batch_resolve_foreign_calls_device(acvm_batch_t *b, const acvm_foreign_call_answers_desc_t *d) try {
    if (!b || !d) return set_err(ACVM_E_INVALID, "null argument");
    const std::vector<FcLaneRecord> lanes = lane_records(b);
    const std::vector<FcRow> list = foreign_waiting_list(lanes.data(), lanes.size(), d->opcode_index, d->brillig_index);
    const FcHandleView view = handle_view(b, d->opcode_index, d->brillig_index);
    uint64_t stride = 0;
    std::vector<uint32_t> words;
    uint32_t total = 0;
    std::string refusal;
    if (int rc = foreign_check_answers(&view, d, list, &stride, &words, &total, &refusal)) return set_err(rc, refusal);
    if (!d->n_rows) return 0;
    const auto &slots = b->plan().fc_slot_opcode;
    const size_t si = (size_t)(std::find(slots.begin(), slots.end(), d->opcode_index) - slots.begin());
    if (si >= b->fc_slots.size()) return set_err(ACVM_E_STATE, "the rows do not wait at a Brillig opcode with a foreign call");
    HIPCHK(hipSetDevice(b->device));
    bool cached = false;
    if (int rc = rows_on_device(b, list, d->opcode_index, d->brillig_index, d->first_row, d->n_rows, &cached)) return rc;
    FcAppendCall call;
    call.si = si;
    call.pairs = &b->fc_rows_host;
    call.d_rows_ready = b->d_fc_rows;
    call.words = &words;
    call.total = total;
    call.encoding = d->encoding;
    call.layout = d->layout;
    call.stride = stride;
    call.d_values = d->d_values;
    return append_rows(b, call);
} ABI_CATCH

int acvm_batch_resolve_foreign_calls_device_rows(acvm_batch_t *b, const acvm_foreign_call_answers_rows_desc_t *d) try {
    if (!b || !d) return set_err(ACVM_E_INVALID, "null argument");
    const std::vector<FcLaneRecord> lanes = lane_records(b);
    const std::vector<FcRow> list = foreign_waiting_list(lanes.data(), lanes.size(), d->opcode_index, d->brillig_index);
    const FcHandleView view = handle_view(b, d->opcode_index, d->brillig_index);
    uint64_t stride = 0;
    std::vector<uint32_t> words;
    uint32_t total = 0;
    std::string refusal;
    if (int rc = foreign_check_answers_rows(&view, d, list, &stride, &words, &total, &refusal)) return set_err(rc, refusal);
    if (!d->n_rows) return 0;
    const auto &slots = b->plan().fc_slot_opcode;
    const size_t si = (size_t)(std::find(slots.begin(), slots.end(), d->opcode_index) - slots.begin());
    if (si >= b->fc_slots.size()) return set_err(ACVM_E_STATE, "the rows do not wait at a Brillig opcode with a foreign call");
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    // the host must know which lanes resume: the mask comes down, one byte per row. It is read ONCE: a copy in the handle's own device memory is what
    // comes down and what both kernels read, so that the lanes marked answered and the rows appended are the same whatever happens to the caller's column
    std::vector<uint8_t> mask;
    const uint8_t *d_answered = nullptr;
    if (d->d_answered) {
        if (d->n_rows > b->fc_mask_cap) {
            if (b->d_fc_mask) hipFree(b->d_fc_mask);
            b->d_fc_mask = nullptr;
            b->fc_mask_cap = 0;
            const size_t cap = (size_t)d->n_rows + d->n_rows / 4 + 256;
            HIPCHK(hipMalloc((void **)&b->d_fc_mask, cap));
            b->fc_mask_cap = cap;
        }
        HIPCHK(hipMemcpyAsync(b->d_fc_mask, d->d_answered, d->n_rows, hipMemcpyDeviceToDevice, s));
        d_answered = b->d_fc_mask;
        mask.resize(d->n_rows);
        HIPCHK(hipMemcpyAsync(mask.data(), d_answered, d->n_rows, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        b->n_fc_d2h_bytes += d->n_rows;
    }
    std::vector<uint32_t> resumed;
    if (int rc = foreign_mask_resumes(list, d->first_row, d->n_rows, d->d_answered ? mask.data() : nullptr, &resumed, &refusal)) return set_err(rc, refusal);
    if (resumed.empty()) return 0;  // (every row is left out: nothing is appended, nobody resumes)
    // the largest total among the answered rows, found on the device before anything is written: it sizes the store and judges n_columns
    if (d->d_lens) {
        if (int rc = stage_reserve(b, 256 + align256(words.size() * 4))) return rc;
        uint32_t *d_max = (uint32_t *)b->d_stage, *d_shape = (uint32_t *)(b->d_stage + 256);
        uint32_t longest = 0;
        HIPCHK(hipMemsetAsync(d_max, 0, 4, s));
        HIPCHK(hipMemcpyAsync(d_shape, words.data(), words.size() * 4, hipMemcpyHostToDevice, s));
        launch_fc_answers_max(s, d_shape, d->d_lens, d_answered, d->n_rows, d_max);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&longest, d_max, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        b->n_fc_h2d_bytes += words.size() * 4;
        b->n_fc_d2h_bytes += 4;
        if (int rc = foreign_check_rows_width(d->n_columns, longest, d->d_values != nullptr, &total, &refusal)) return set_err(rc, refusal);
    }
    bool cached = false;
    if (int rc = rows_on_device(b, list, d->opcode_index, d->brillig_index, d->first_row, d->n_rows, &cached)) return rc;
    const FcRowsForm form{d->d_lens, d_answered, d->n_columns, &resumed};
    FcAppendCall call;
    call.si = si;
    call.pairs = &b->fc_rows_host;
    call.d_rows_ready = b->d_fc_rows;
    call.words = &words;
    call.total = total;  // (the largest total of an answered row)
    call.encoding = d->encoding;
    call.layout = d->layout;
    call.stride = stride;
    call.d_values = d->d_values;
    call.rows_form = &form;
    return append_rows(b, call);
} ABI_CATCH

int fc_append_one_instance(acvm_batch *b, uint32_t t, size_t si, uint32_t n_values, const uint8_t *is_array, const uint32_t *lens, const uint8_t *values_be32) {
    std::vector<uint32_t> words;
    uint32_t total = 0;
    std::string refusal;
    if (int rc = foreign_shape(n_values, is_array, lens, &words, &total, &refusal)) return set_err(rc, refusal);
    const std::vector<uint32_t> pairs = {t, b->slow_ids[t]};
    // (canonical big-endian values back to back: one instance-major row; the arena is 256-byte aligned)
    FcAppendCall call;
    call.si = si;
    call.pairs = &pairs;
    call.words = &words;
    call.total = total;
    call.encoding = ACVM_ENC_BE32;
    call.layout = ACVM_LAYOUT_INSTANCE_MAJOR;
    call.stride = std::max<uint32_t>(total, 1);
    call.h_values = values_be32;
    call.h_bytes = (size_t)total * 32;
    return append_rows(b, call);
}

int acvm_debug_foreign_call_stats(const acvm_batch_t *b, uint64_t *h2d_bytes, uint64_t *d2h_bytes, double *inputs_kernel_ms, double *append_kernel_ms,
                                  uint64_t *store_bytes) {
    if (!b) return set_err(ACVM_E_INVALID, "null batch");
    if (h2d_bytes) *h2d_bytes = b->n_fc_h2d_bytes;
    if (d2h_bytes) *d2h_bytes = b->n_fc_d2h_bytes;
    if (inputs_kernel_ms) *inputs_kernel_ms = b->fc_inputs_ms;
    if (append_kernel_ms) *append_kernel_ms = b->fc_append_ms;
    if (store_bytes) {
        *store_bytes = 0;
        for (auto &sl : b->fc_slots) *store_bytes += (sl.d_desc ? (uint64_t)sl.desc_words * b->Bp * 4 : 0) + (sl.d_vals ? (uint64_t)sl.vals_cap * 2 * b->Bp * sizeof(uint4) : 0);
    }
    return 0;
}
