// batch_export.cpp -- the values that leave the device after a solve: witnesses and witness maps (ACVM::witness_map / finalize,
// acvm/src/pwg/mod.rs:161,176-181), the per-instance map digest, public-witness extraction (acvm_js/src/public_witness.rs), the export into a
// caller's device buffer. Results and texts: batch_messages.cpp.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>
#include "batch_internal.hpp"
#include "export_encode.hpp"
#include "record_out_plan.hpp"
#include "wire_pack_plan.hpp"
#include "wire_plan.hpp"
#include "wire_repitch.hpp"

static const uint8_t DIGEST_G[32] = {0x23, 0x35, 0x53, 0x18, 0xdb, 0xff, 0xab, 0x2f, 0xb7, 0x72, 0x11, 0x7c, 0x57, 0x5c, 0x61, 0xb1,
                                     0x79, 0xf8, 0xc9, 0x83, 0x3c, 0x83, 0xba, 0x65, 0x59, 0x7e, 0x17, 0x3c, 0x35, 0xc4, 0xbb, 0xe3};
static const uint8_t DIGEST_H[32] = {0x28, 0x25, 0x78, 0x33, 0xe7, 0x23, 0x7f, 0xbd, 0x29, 0x7c, 0x55, 0x74, 0x6b, 0xe0, 0xa3, 0xa9,
                                     0x8a, 0x2a, 0x89, 0x8d, 0x8a, 0xb1, 0x0b, 0xe0, 0x05, 0xaa, 0x2f, 0xdf, 0x9c, 0x60, 0x11, 0xa4};
// device tables of the digest: g^(w+1), g^(w+1) / scale_w for the scaled witnesses, h^(w+1), and the h-sum of the planner's assigned set
int ensure_digest_tables(acvm_batch *b) {
    if (b->d_fp_g) return 0;
    const Plan &p = b->plan();
    const uint32_t nw = p.n_witnesses;
    const FrH g = frh::from_be_bytes32_reduce(DIGEST_G, 32), h = frh::from_be_bytes32_reduce(DIGEST_H, 32);
    std::vector<uint32_t> tg((size_t)std::max<uint32_t>(nw, 1) * 8), th((size_t)std::max<uint32_t>(nw, 1) * 8), tgs(std::max<size_t>(p.unscale.size(), 1) * 8), hgen(8);
    FrH gp = g, hp = h, hsum = frh::zero();
    auto put = [](std::vector<uint32_t> &v, size_t i, const FrH &x) {
        const FrH d = frh::to_device_form(x);
        memcpy(&v[8 * i], d.l, 32);
    };
    for (uint32_t w = 0; w < nw; w++) {
        put(tg, w, gp);
        put(th, w, hp);
        if (p.unscale_index[w] != 0xFFFFFFFFu) put(tgs, p.unscale_index[w], frh::mul(gp, p.unscale[p.unscale_index[w]]));
        if (p.producer[w] != 0xFFFFFFFFu) hsum = frh::add(hsum, hp);
        gp = frh::mul(gp, g);
        hp = frh::mul(hp, h);
    }
    put(hgen, 0, hsum);
    if (int rc = upload(&b->d_fp_g, tg)) return rc;
    if (int rc = upload(&b->d_fp_h, th)) return rc;
    if (int rc = upload(&b->d_fp_gs, tgs)) return rc;
    if (int rc = upload(&b->d_fp_hgen, hgen)) return rc;
    b->fp = DigestTables{b->d_fp_g, b->d_fp_gs, b->d_fp_h, b->d_fp_hgen};
    return 0;
}

// digests of lanes [first, first + n) of a witness table into host memory out32 ([n][32]), staged through the arena on stream s:
// arena = (slow_index) | partial sums | digests. The per-instance lane of `assigned` comes from a device array (d_slow_index) or from the
// batch's host vector (use_host_index: uploaded here); neither is needed when t.u.event is null (every lane read as an instance of the
// level kernels).
int digest_range(acvm_batch *b, hipStream_t s, const TableView &t, uint32_t first, uint32_t n, const int32_t *d_slow_index, bool use_host_index, uint32_t n_slow,
                 uint8_t *out32) {
    const Plan &p = b->plan();
    if (!n) return 0;
    if (int rc = ensure_digest_tables(b)) return rc;
    const size_t idx_bytes = use_host_index ? align256((size_t)b->B * 4) : 0;
    const size_t part_bytes = align256((size_t)digest_chunks(p.n_witnesses) * n * 32);
    if (int rc = stage_reserve(b, idx_bytes + part_bytes + (size_t)n * 32)) return rc;
    if (use_host_index) {
        HIPCHK(hipMemcpyAsync(b->d_stage, b->slow_index.data(), (size_t)b->B * 4, hipMemcpyHostToDevice, s));
        d_slow_index = (const int32_t *)b->d_stage;
    }
    uint4 *d_part = (uint4 *)(b->d_stage + idx_bytes);
    uint8_t *d_out = b->d_stage + idx_bytes + part_bytes;
    launch_digest(s, t.W, t.Bp, first, n, p.n_witnesses, b->d_producer, t.u, b->fp, d_slow_index, b->d_assigned, n_slow, d_part, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out32, d_out, (size_t)n * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int read_witnesses(acvm_batch *b, hipStream_t s, const TableView &t, uint32_t first, uint32_t n, const uint32_t *sel, uint32_t n_sel, uint8_t *out_be32) {
    if (!n || !n_sel) return 0;
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)n_sel * 32)));
    const size_t sel_bytes = align256((size_t)n_sel * 4);
    if (int rc = stage_reserve(b, sel_bytes + (size_t)chunk * n_sel * 32)) return rc;
    uint32_t *d_sel = (uint32_t *)b->d_stage;
    uint8_t *d_out = b->d_stage + sel_bytes;
    HIPCHK(hipMemcpyAsync(d_sel, sel, (size_t)n_sel * 4, hipMemcpyHostToDevice, s));
    for (uint32_t done = 0; done < n; done += chunk) {
        const uint32_t m = std::min(chunk, n - done);
        launch_export(s, t.W, t.Bp, first + done, m, d_sel, n_sel, d_out, t.u, t.row_of);
        HIPCHK(hipMemcpyAsync(out_be32 + (size_t)done * n_sel * 32, d_out, (size_t)m * n_sel * 32, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));  // (also what keeps a list on the caller's stack alive for its copy)
    }
    return 0;
}

AssignedView batch_assigned(const acvm_batch *b, hipError_t *err) {  // (err may be null: for views that never copy a row)
    const uint32_t n_slow = (uint32_t)b->slow_ids.size();
    return AssignedView(b->plan().producer.data(), b->plan().n_witnesses, b->slow_index.data(), n_slow, [b, n_slow, err](uint32_t word, uint32_t *row) {
        const hipError_t e = hipMemcpy(row, b->d_assigned + (size_t)word * n_slow, (size_t)n_slow * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess && err) *err = e;
        return e == hipSuccess;
    });
}

// after acvm_batch_solve_then_import the rows of the INITIAL witnesses hold the next tile's values: whatever reads them back is refused
int refuse_if_next_imported(const acvm_batch *b, const uint32_t *ws, uint32_t n, bool whole_map) {
    if (!b->next_imported) return 0;
    bool hit = whole_map;
    for (uint32_t k = 0; k < n && !hit; k++) hit = std::find(b->plan().initial_ids.begin(), b->plan().initial_ids.end(), ws[k]) != b->plan().initial_ids.end();
    if (!hit) return 0;
    return set_err(ACVM_E_STATE, "the initial witnesses of this solve are gone: acvm_batch_solve_then_import put the next tile's inputs into the table behind the solve "
                                 "(read results, non-initial witnesses and nothing else; or use acvm_batch_solve)");
}

// ---- slot reuse (ACVM_BATCH_REUSE_SLOTS): what can be read back
static bool reuse_kept(const acvm_batch *b, uint32_t w) {
    const Plan &p = b->plan();
    if (w >= p.n_witnesses) return false;
    if (std::find(p.initial_ids.begin(), p.initial_ids.end(), w) != p.initial_ids.end()) return true;
    return std::find(b->opts.keep.begin(), b->opts.keep.end(), w) != b->opts.keep.end();
}
static int reuse_check_kept(const acvm_batch *b, const uint32_t *ws, uint32_t n) {
    if (!b->reuse()) return 0;
    for (uint32_t k = 0; k < n; k++)
        if (ws[k] < b->plan().n_witnesses && !reuse_kept(b, ws[k]))
            return set_err(ACVM_E_STATE, "witness " + std::to_string(ws[k]) + " was not kept: the batch recycles witness rows (ACVM_BATCH_REUSE_SLOTS); "
                                         "only the initial witnesses and keep_ids can be read back");
    return 0;
}
// the instances of the exact path have their values in the table of their own: overwrite their rows of an export (values_be32 [n][n_sel][32] of
// instances [first, first + n)). slow_ids ascends with the instance, so the exact lanes of a range are consecutive lanes of the side table: one
// read, then scattered
static int reuse_patch_exact(acvm_batch *b, const uint32_t *sel, uint32_t n_sel, uint32_t first, uint32_t n, uint8_t *values_be32) {
    if (!b->side()) return 0;
    std::vector<uint32_t> at;  // the exact lanes' positions in the range
    for (uint32_t i = 0; i < n; i++)
        if (b->slow_index[first + i] >= 0) at.push_back(i);
    if (at.empty()) return 0;
    const size_t row = (size_t)n_sel * 32;
    std::vector<uint8_t> lanes(at.size() * row);
    if (int rc = read_witnesses(b, b->stream, side_table(b), (uint32_t)b->slow_index[first + at[0]], (uint32_t)at.size(), sel, n_sel, lanes.data())) return rc;
    for (size_t k = 0; k < at.size(); k++) memcpy(values_be32 + at[k] * row, &lanes[k * row], row);
    return 0;
}

bool fetch_one(acvm_batch *b, uint32_t j, uint32_t w, uint8_t out[32]) {
    // While an exact job is pending its lanes live in the side table and the caller's NEXT tile may already be enqueued on the handle's
    // stream: the fetch goes through the job's stream (and a staging slot of its own, not read_witnesses' arena), so that a failing
    // instance's message does not wait for a whole level schedule.
    const bool side_lane = b->side() && b->slow_index[j] >= 0;
    hipStream_t s = b->pending && side_lane ? b->stream_x : b->stream;
    if (!b->d_fetch && hipMalloc((void **)&b->d_fetch, 512) != hipSuccess) return false;
    uint32_t *d_sel = (uint32_t *)b->d_fetch;
    uint8_t *d_out = b->d_fetch + 256;
    if (hipMemcpyAsync(d_sel, &w, 4, hipMemcpyHostToDevice, s) != hipSuccess) return false;
    if (hipStreamSynchronize(s) != hipSuccess) return false;  // &w is a stack address
    const TableView t = side_lane ? side_table(b) : level_table(b);
    launch_export(s, t.W, t.Bp, side_lane ? (uint32_t)b->slow_index[j] : j, 1, d_sel, 1, d_out, t.u, t.row_of);
    return hipMemcpyAsync(out, d_out, 32, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
}

// results, kept witnesses and digests of instances [0, n) for the node driver (batch.hpp)
int batch_export_tile(acvm_batch *b, uint32_t n, const uint32_t *keep, uint32_t n_keep, acvm_result_t *results, uint8_t *kept_values, uint8_t *kept_assigned,
                      uint8_t *digests) {
    const Plan &p = b->plan();
    if (!b->solved || n > b->B) return set_err(ACVM_E_STATE, "batch not solved");
    HIPCHK(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    const bool defer = b->pending;  // the instances of the exact path arrive with the job's outcome
    if (results)
        for (uint32_t j = 0; j < n; j++)
            if (!(defer && b->slow_index[j] >= 0)) fill_result(b, j, results[j]);
    if (n_keep && kept_values) {
        if (int rc = read_witnesses(b, s, level_table(b), 0, n, keep, n_keep, kept_values)) return rc;
        if (!defer)  // synchronous exact lanes: their values from where they live, their flags from the bitmap
            if (int rc = reuse_patch_exact(b, keep, n_keep, 0, n, kept_values)) return rc;
        hipError_t herr = hipSuccess;
        batch_assigned(b, &herr).fill(0, n, keep, n_keep, kept_assigned, kept_values, defer ? AssignedView::LEVEL_ONLY : AssignedView::ALL);
        HIPCHK(herr);
    }
    if (digests) {
        if (defer || b->slow_ids.empty()) {
            // (the table-wide kernels: flagged columns hold leftovers and are overwritten by the outcome)
            if (p.n_digest_segments && b->d_leaves) {
                if (int rc = stage_reserve(b, (size_t)n * 32)) return rc;
                launch_digest_final(s, b->d_leaves, p.n_digest_segments, b->Bp, 0, n, nullptr, b->fp, b->d_stage);
                HIPCHK(hipMemcpyAsync(digests, b->d_stage, (size_t)n * 32, hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
            } else {
                // every lane is read as a generic instance here: an event word that is set would send the kernel to the assigned bitmap of a
                // job that is still running
                TableView t = level_table(b);
                t.u.event = nullptr;
                if (int rc = digest_range(b, s, t, 0, n, nullptr, false, 0, digests)) return rc;
            }
        } else if (int rc = acvm_batch_digest(b, 0, n, digests)) return rc;
    }
    return 0;
}

int acvm_batch_witness_map(acvm_batch_t *b, uint32_t first, uint32_t n, uint8_t *assigned, uint8_t *values_be32) try {
    if (!b || !assigned || !values_be32) return set_err(ACVM_E_INVALID, "null argument");
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (int rc = require_instance_range(b, first, n)) return rc;
    if (b->side()) return set_err(ACVM_E_STATE, "the batch recycles witness rows (ACVM_BATCH_REUSE_SLOTS) or solved its exact lanes in the side table: full maps are not kept; read the kept witnesses and the digest");
    if (int rc = refuse_if_next_imported(b, nullptr, 0, true)) return rc;
    HIPCHK(hipSetDevice(b->device));
    const uint32_t nw = b->plan().n_witnesses;
    if (!n || !nw) return 0;
    std::vector<uint32_t> sel(nw);
    for (uint32_t w = 0; w < nw; w++) sel[w] = w;
    // (level_table's row map is null here: only a plan that recycles rows has one -- plan.cpp assign_rows, batch.cpp -- and that is side(), refused above)
    if (int rc = read_witnesses(b, b->stream, level_table(b), first, n, sel.data(), nw, values_be32)) return rc;
    bool any_exact = false;
    for (uint32_t i = 0; i < n; i++) any_exact |= b->slow_index[first + i] >= 0;
    const uint32_t n_slow = (uint32_t)b->slow_ids.size();
    std::vector<uint32_t> bitmap(any_exact ? (size_t)n_slow * b->n_words : 1);  // every witness is asked for: the whole bitmap in one copy
    if (any_exact) HIPCHK(hipMemcpy(bitmap.data(), b->d_assigned, bitmap.size() * 4, hipMemcpyDeviceToHost));
    AssignedView(b->plan().producer.data(), nw, b->slow_index.data(), n_slow, bitmap.data()).fill(first, n, nullptr, nw, assigned, values_be32);
    return 0;
} ABI_CATCH

// digests of the instances of the exact path listed in `flagged` (instance indices >= first), from their own witness maps, into
// out32[(instance - first) * 32]
static int digest_exact_instances(acvm_batch *b, const std::vector<uint32_t> &flagged, uint32_t first, uint8_t *out32) {
    const uint32_t n_slow = (uint32_t)b->slow_ids.size();
    if (b->side()) {  // all lanes of the side table at once (lane t = the t-th flagged instance), then scattered to their instances
        std::vector<uint8_t> lanes((size_t)n_slow * 32);
        if (int rc = digest_range(b, b->stream, side_table(b), 0, n_slow, (const int32_t *)b->d_ids_x, false, n_slow, lanes.data())) return rc;
        for (uint32_t j : flagged) memcpy(out32 + (size_t)(j - first) * 32, &lanes[(size_t)b->slow_index[j] * 32], 32);
        return 0;
    }
    // plain table: the instance's own column, one launch each (few by construction: acvm_batch_digest takes the table-wide kernel otherwise)
    for (uint32_t j : flagged)
        if (int rc = digest_range(b, b->stream, level_table(b), j, 1, nullptr, true, n_slow, out32 + (size_t)(j - first) * 32)) return rc;
    return 0;
}

// per-instance digest of the solved witness map (definition: kernels_hash.hip, include/acvm_amd.h)
int acvm_batch_digest(acvm_batch_t *b, uint32_t first, uint32_t n, uint8_t *out32) try {
    if (!b || (n && !out32)) return set_err(ACVM_E_INVALID, "null argument");
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (int rc = require_instance_range(b, first, n)) return rc;
    if (!n) return 0;
    if (int rc = refuse_if_next_imported(b, nullptr, 0, !(b->plan().n_digest_segments && b->d_leaves))) return rc;  // (a folded digest was summed during the solve)
    HIPCHK(hipSetDevice(b->device));
    const Plan &p = b->plan();
    if (int rc = ensure_digest_tables(b)) return rc;
    std::vector<uint32_t> flagged;
    for (uint32_t i = 0; i < n; i++)
        if (b->slow_index[first + i] >= 0) flagged.push_back(first + i);
    if (p.n_digest_segments && b->d_leaves && !b->force_slow && !b->stepping) {
        // folded into the solve: the partial sums of the generic instances are there; only their total is left (and the instances of the
        // exact path, whose sums come from their own maps below)
        if (int rc = stage_reserve(b, (size_t)n * 32)) return rc;
        launch_digest_final(b->stream, b->d_leaves, p.n_digest_segments, b->Bp, first, n, b->d_event, b->fp, b->d_stage);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out32, b->d_stage, (size_t)n * 32, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (flagged.empty()) return 0;
        if (b->side() || flagged.size() <= 64) return digest_exact_instances(b, flagged, first, out32);
        // (plain table with many instances of the exact path -- a whole batch waiting at a foreign call, a batch of failures: the
        // table-wide kernel below serves generic and exact lanes alike through slow_index)
    }
    if (b->side()) {  // the level table does not hold the maps of the exact path's instances
        TableView t = level_table(b);
        t.u.event = nullptr;  // (their columns are read as leftovers and overwritten below)
        if (int rc = digest_range(b, b->stream, t, first, n, nullptr, false, 0, out32)) return rc;
        return flagged.empty() ? 0 : digest_exact_instances(b, flagged, first, out32);
    }
    return digest_range(b, b->stream, level_table(b), first, n, nullptr, true, (uint32_t)b->slow_ids.size(), out32);
} ABI_CATCH

// SURVEY 8d's digest as written -- Blake2s over the witness vector's bytes -- in tree form (definition: include/acvm_amd.h). The whole table must be
// there: not with recycled rows, not while an asynchronous exact job holds instances in its side table.
int acvm_batch_digest_blake2s(acvm_batch_t *b, uint32_t first, uint32_t n, uint8_t *out32) try {
    if (!b || (n && !out32)) return set_err(ACVM_E_INVALID, "null argument");
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (int rc = require_instance_range(b, first, n)) return rc;
    if (!n) return 0;
    if (b->side()) return set_err(ACVM_E_STATE, "the byte-wise digest hashes every witness row: not with ACVM_BATCH_REUSE_SLOTS (rows are recycled) nor while instances of "
                                                "the exact path live in a side table; acvm_batch_digest serves those");
    if (int rc = refuse_if_next_imported(b, nullptr, 0, true)) return rc;
    HIPCHK(hipSetDevice(b->device));
    const Plan &p = b->plan();
    hipStream_t s = b->stream;
    const size_t idx_bytes = align256((size_t)b->B * 4);
    const size_t leaf_bytes = align256((size_t)digest_b2s_leaves(p.n_witnesses) * 32 * n);
    if (int rc = stage_reserve(b, idx_bytes + leaf_bytes + (size_t)n * 32)) return rc;
    HIPCHK(hipMemcpyAsync(b->d_stage, b->slow_index.data(), (size_t)b->B * 4, hipMemcpyHostToDevice, s));
    uint32_t *d_leaves = (uint32_t *)(b->d_stage + idx_bytes);
    uint8_t *d_out = b->d_stage + idx_bytes + leaf_bytes;
    launch_digest_blake2s(s, b->d_W, b->Bp, first, n, p.n_witnesses, b->d_producer, b->unscale, (const int32_t *)b->d_stage, b->d_assigned, (uint32_t)b->slow_ids.size(), d_leaves, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out32, d_out, (size_t)n * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
} ABI_CATCH

int acvm_batch_extract_witnesses(acvm_batch_t *b, const uint32_t *witnesses, uint32_t n_witnesses, uint32_t first, uint32_t n,
                                 uint8_t *values_be32) try {
    if (!b || (n_witnesses && (!witnesses || !values_be32))) return set_err(ACVM_E_INVALID, "null argument");
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (int rc = require_instance_range(b, first, n)) return rc;
    if (!n || !n_witnesses) return 0;
    if (int rc = refuse_if_next_imported(b, witnesses, n_witnesses, false)) return rc;
    HIPCHK(hipSetDevice(b->device));
    const uint32_t nw = b->plan().n_witnesses;
    char text[160];
    for (uint32_t k = 0; k < n_witnesses; k++)
        if (witnesses[k] >= nw) {
            snprintf(text, sizeof text, "Failed to extract witness %u from witness map. Witness not found. (instance %u)", witnesses[k], first);
            return set_err(ACVM_E_STATE, text);
        }
    // assigned? Only the listed witnesses are looked at (assigned_view.hpp): O(n + n_slow x n_witnesses), not O(n x all witnesses)
    hipError_t herr = hipSuccess;
    uint32_t bad_j, bad_w;
    const bool missing = batch_assigned(b, &herr).first_missing(first, n, witnesses, n_witnesses, &bad_j, &bad_w);
    HIPCHK(herr);
    if (missing) {
        snprintf(text, sizeof text, "Failed to extract witness %u from witness map. Witness not found. (instance %u)", bad_w, bad_j);
        return set_err(ACVM_E_STATE, text);
    }
    if (int rc = reuse_check_kept(b, witnesses, n_witnesses)) return rc;
    if (int rc = read_witnesses(b, b->stream, level_table(b), first, n, witnesses, n_witnesses, values_be32)) return rc;
    return reuse_patch_exact(b, witnesses, n_witnesses, first, n, values_be32);
} ABI_CATCH

// ---------------------------------------------------------------------------------------------- the map for a consumer on the device
// 2^256 / scale mod p as canonical integers, one row per scaled witness like Unscale::consts_plain: the planner's representative (R = 2^256,
// fr_host.hpp) of 1 / scale IS that integer. Built when the first Montgomery-256 export asks for it.
static int ensure_mont256_table(acvm_batch *b) {
    const Plan &p = b->plan();
    if (b->d_unscale_m256 || p.scaled_ids.empty()) return 0;
    std::vector<uint32_t> uc(p.unscale.size() * 8);
    for (size_t i = 0; i < p.unscale.size(); i++) memcpy(&uc[8 * i], p.unscale[i].l, 32);
    return upload(&b->d_unscale_m256, uc);
}

// What the range export and the list export check alike, in one order: the descriptor's shape, the pointers, the batch's state, the range (list: the
// list's length against nothing -- its entries are the device's to judge), the stride, what the batch kept. 0 and *n_sel / *stride, or the refusal.
static int export_device_checks(acvm_batch *b, const acvm_export_desc_t *d, const void *d_values, const uint32_t *d_instances, bool list, uint32_t *n_sel_out,
                                uint64_t *stride_out) {
    if (!d) return set_err(ACVM_E_INVALID, "null argument");
    // (the buffer checks of import_plan.hpp, shared with the imports)
    std::string refusal = buffer_check_shape(d->encoding, d->layout, false);
    if (!refusal.empty()) return set_err(ACVM_E_INVALID, refusal);
    if (list && d->first != 0) return set_err(ACVM_E_INVALID, "first must be 0 for a list export: the list holds absolute instance numbers");
    if (!b || !d_values || (list && d->n && !d_instances)) return set_err(ACVM_E_INVALID, "null argument");
    refusal = buffer_check_pointer(d->encoding, d_values);
    if (!refusal.empty()) return set_err(ACVM_E_INVALID, refusal);
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (!list)
        if (int rc = require_instance_range(b, d->first, d->n)) return rc;
    const bool whole = d->witnesses == nullptr;
    const uint32_t n_sel = whole ? b->plan().n_witnesses : d->n_witnesses;
    uint64_t stride = d->stride;
    refusal = buffer_check_stride(d->layout, d->n, n_sel, &stride);
    if (!refusal.empty()) return set_err(ACVM_E_INVALID, refusal);
    if (whole) {
        if (b->side()) return set_err(ACVM_E_STATE, "the batch recycles witness rows (ACVM_BATCH_REUSE_SLOTS) or solved its exact lanes in the side table: full maps are not kept; read the kept witnesses and the digest");
        if (int rc = refuse_if_next_imported(b, nullptr, 0, true)) return rc;
    } else {
        if (int rc = refuse_if_next_imported(b, d->witnesses, n_sel, false)) return rc;
        if (int rc = reuse_check_kept(b, d->witnesses, n_sel)) return rc;
    }
    *n_sel_out = n_sel;
    *stride_out = stride;
    return 0;
}

// The launches of a range export without the wait (as batch_enqueue_kept stands to read_witnesses): every lane of the range as a generic
// instance (scaled columns, the planner's assigned set), then the exact lanes -- d_lanes: n_lanes device pairs (lane, index in the range) --
// from where they live (their own columns of the level table, or the side table), scattered into their elements.
static int enqueue_export_device(acvm_batch *b, hipStream_t s, const ExportDevice &x, const uint32_t *d_lanes, uint32_t n_lanes) {
    const bool narrow = export_enc_is_narrow(x.encoding);  // elements of 1 .. 16 bytes, aligned to their size; mask bytes 0 / 1 / 2
    if (x.encoding == EXPORT_ENC_MONT256_LE)
        if (int rc = ensure_mont256_table(b)) return rc;
    if (n_lanes < x.n) {
        if (narrow) launch_export_narrow(s, x, b->d_W, b->Bp, b->d_slot_of, b->d_producer, b->unscale);
        else launch_export_device(s, x, b->d_W, b->Bp, b->d_slot_of, b->d_producer, b->unscale, x.encoding == EXPORT_ENC_MONT256_LE ? b->d_unscale_m256 : b->unscale.consts_plain);
    }
    if (n_lanes)
        (narrow ? launch_export_narrow_lanes : launch_export_device_lanes)(s, x, b->side() ? b->d_Wx : b->d_W, b->side() ? b->x_cap : b->Bp, b->side(), d_lanes, n_lanes, b->d_assigned,
                                                                           (uint32_t)b->slow_ids.size());
    HIPCHK(hipGetLastError());
    return 0;
}

int acvm_batch_export_device(acvm_batch_t *b, const acvm_export_desc_t *d, void *d_values, uint8_t *d_assigned) try {
    uint32_t n_sel = 0;
    uint64_t stride = 0;
    if (int rc = export_device_checks(b, d, d_values, nullptr, false, &n_sel, &stride)) return rc;
    const uint32_t first = d->first, n = d->n;
    const uint32_t nw = b->plan().n_witnesses;
    const bool whole = d->witnesses == nullptr;
    if (!n || !n_sel) return 0;
    HIPCHK(hipSetDevice(b->device));
    // the instances of the exact path among the range: (lane, index in the range) pairs for the second launch
    std::vector<uint32_t> lanes;
    for (uint32_t i = 0; i < n; i++)
        if (b->slow_index[first + i] >= 0) { lanes.push_back((uint32_t)b->slow_index[first + i]); lanes.push_back(i); }
    const uint32_t n_lanes = (uint32_t)(lanes.size() / 2);
    const size_t sel_bytes = whole ? 0 : align256((size_t)n_sel * 4);
    if (sel_bytes + lanes.size() * 4)
        if (int rc = stage_reserve(b, sel_bytes + lanes.size() * 4)) return rc;
    hipStream_t s = b->stream;
    uint32_t *d_sel = whole ? nullptr : (uint32_t *)b->d_stage, *d_lanes = (uint32_t *)(b->d_stage + sel_bytes);
    if (!whole) HIPCHK(hipMemcpyAsync(d_sel, d->witnesses, (size_t)n_sel * 4, hipMemcpyHostToDevice, s));
    if (n_lanes) HIPCHK(hipMemcpyAsync(d_lanes, lanes.data(), lanes.size() * 4, hipMemcpyHostToDevice, s));
    b->n_export_h2d_bytes += (whole ? 0 : (uint64_t)n_sel * 4) + (uint64_t)lanes.size() * 4;
    const ExportDevice x{d->encoding, d->layout, first, n, d_sel, n_sel, nw, stride, d_values, d_assigned};
    if (int rc = enqueue_export_device(b, s, x, d_lanes, n_lanes)) return rc;
    HIPCHK(hipStreamSynchronize(s));  // (also what keeps `lanes` and the caller's list alive for their copies)
    return 0;
} ABI_CATCH

// ---- the map of LISTED instances (include/acvm_amd.h acvm_batch_export_device_list). The list lives on the device, so which of its rows are exact lanes
// is the kernels' to find out: through the handle's instance -> lane map, which is made on the device from slow_ids (n_slow words go up, once per change
// of slow_index; none while no instance left the generic path). ids_stage: room for those words in the arena the caller reserved.
static int lane_map_ready(acvm_batch *b, hipStream_t s, uint32_t *ids_stage) {
    if (b->d_lane_map && b->lane_map_epoch == b->slow_epoch) return 0;
    if (!b->d_lane_map) HIPCHK(hipMalloc((void **)&b->d_lane_map, (size_t)std::max<uint32_t>(b->capacity, 1) * 4));
    launch_fill_u32(s, (uint32_t *)b->d_lane_map, 0xFFFFFFFFu, b->capacity);
    const uint32_t n_slow = (uint32_t)b->slow_ids.size();
    if (n_slow) {
        HIPCHK(hipMemcpyAsync(ids_stage, b->slow_ids.data(), (size_t)n_slow * 4, hipMemcpyHostToDevice, s));
        b->n_export_h2d_bytes += (uint64_t)n_slow * 4;
        launch_lane_map_scatter(s, b->d_lane_map, b->capacity, ids_stage, n_slow);
    }
    HIPCHK(hipGetLastError());
    b->lane_map_epoch = b->slow_epoch;
    return 0;
}

int acvm_batch_export_device_list(acvm_batch_t *b, const acvm_export_desc_t *d, const uint32_t *d_instances, void *d_values, uint8_t *d_assigned) try {
    uint32_t n_sel = 0;
    uint64_t stride = 0;
    if (int rc = export_device_checks(b, d, d_values, d_instances, true, &n_sel, &stride)) return rc;
    const uint32_t n = d->n, nw = b->plan().n_witnesses;
    const bool whole = d->witnesses == nullptr;
    if (!n || !n_sel) return 0;
    HIPCHK(hipSetDevice(b->device));
    if (d->encoding == EXPORT_ENC_MONT256_LE)
        if (int rc = ensure_mont256_table(b)) return rc;
    const uint32_t n_slow = (uint32_t)b->slow_ids.size();
    const bool map_stale = !(b->d_lane_map && b->lane_map_epoch == b->slow_epoch);
    const size_t sel_bytes = whole ? 0 : align256((size_t)n_sel * 4), ids_bytes = map_stale ? (size_t)n_slow * 4 : 0;
    if (sel_bytes + ids_bytes)
        if (int rc = stage_reserve(b, sel_bytes + ids_bytes)) return rc;
    hipStream_t s = b->stream;
    uint32_t *d_sel = whole ? nullptr : (uint32_t *)b->d_stage;
    if (!whole) {
        HIPCHK(hipMemcpyAsync(d_sel, d->witnesses, (size_t)n_sel * 4, hipMemcpyHostToDevice, s));
        b->n_export_h2d_bytes += (uint64_t)n_sel * 4;
    }
    if (int rc = lane_map_ready(b, s, (uint32_t *)(b->d_stage + sel_bytes))) return rc;
    const ExportDevice x{d->encoding, d->layout, 0u, n, d_sel, n_sel, nw, stride, d_values, d_assigned};
    const ExportListSource src{d_instances, b->B, b->d_lane_map, b->side() ? b->d_Wx : b->d_W, b->side() ? b->x_cap : b->Bp, b->side(), b->d_assigned, n_slow};
    if (export_enc_is_narrow(d->encoding)) launch_export_narrow_list(s, x, b->d_W, b->Bp, b->d_slot_of, b->d_producer, b->unscale, src);
    else launch_export_device_list(s, x, b->d_W, b->Bp, b->d_slot_of, b->d_producer, b->unscale, d->encoding == EXPORT_ENC_MONT256_LE ? b->d_unscale_m256 : b->unscale.consts_plain, src);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));  // (also what keeps the caller's witness list and slow_ids alive for their copies)
    return 0;
} ABI_CATCH

// ---- the map as packed records (include/acvm_amd.h acvm_batch_export_device_records): the field list is checked, cut into windows and given its
// cover bitmaps by record_out_plan.cpp, the tables live in a device buffer of their own that is uploaded when they change, one launch writes the
// records. Range and list are the same kernel, and both find the exact lanes through the lane map.
static int record_out_tables_ready(acvm_batch *b, const RecordOutPlan &plan) {
    const std::vector<uint32_t> &tables = plan.tables;
    if (tables.empty() || (b->d_record_out_tables && b->record_out_tables == tables)) return 0;
    HIPCHK(hipStreamSynchronize(b->stream));  // (nothing reads the old tables any more)
    b->record_out_tables.clear();
    if (tables.size() > b->record_out_tables_cap) {
        if (b->d_record_out_tables) { hipFree(b->d_record_out_tables); b->d_record_out_tables = nullptr; b->record_out_tables_cap = 0; }
        HIPCHK(hipMalloc((void **)&b->d_record_out_tables, tables.size() * 4));
        b->record_out_tables_cap = tables.size();
    }
    HIPCHK(hipMemcpy(b->d_record_out_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice));
    b->record_out_tables = tables;
    b->n_export_h2d_bytes += (uint64_t)tables.size() * 4;
    return 0;
}
// Both forms. records: the caller's buffer, device or host (host: the records are made in the staging buffer, zero-filled first, and copied down).
static int export_records(acvm_batch *b, const acvm_record_out_desc_t *d, const uint32_t *d_instances, void *records, bool host) {
    RecordOutPlan plan;
    std::string refusal;
    if (int rc = record_out_plan(b ? &b->B : nullptr, d, d_instances != nullptr, records, &plan, &refusal)) return set_err(rc, refusal);
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (int rc = refuse_if_next_imported(b, plan.witnesses.data(), (uint32_t)plan.witnesses.size(), false)) return rc;
    if (int rc = reuse_check_kept(b, plan.witnesses.data(), (uint32_t)plan.witnesses.size())) return rc;
    if (!plan.n || !plan.n_entries) return 0;
    HIPCHK(hipSetDevice(b->device));
    if (plan.mont256)
        if (int rc = ensure_mont256_table(b)) return rc;
    const uint32_t n_slow = (uint32_t)b->slow_ids.size();
    const bool map_stale = !(b->d_lane_map && b->lane_map_epoch == b->slow_epoch);
    const size_t ids_bytes = map_stale ? align256((size_t)n_slow * 4) : 0, bytes = host ? (size_t)plan.n * plan.pitch : 0;
    if (ids_bytes + bytes)
        if (int rc = stage_reserve(b, ids_bytes + bytes)) return rc;
    hipStream_t s = b->stream;
    if (int rc = record_out_tables_ready(b, plan)) return rc;
    if (int rc = lane_map_ready(b, s, (uint32_t *)b->d_stage)) return rc;
    uint8_t *out = host ? b->d_stage + ids_bytes : (uint8_t *)records;
    if (host) HIPCHK(hipMemsetAsync(out, 0, bytes, s));
    const uint32_t *windows = b->d_record_out_tables, *fields = windows + (size_t)plan.n_windows * RECORD_OUT_WINDOW_WORDS;
    const RecordExport x{b->d_W, b->Bp, plan.first, plan.n,
                         ExportListSource{d_instances, b->B, b->d_lane_map, b->side() ? b->d_Wx : b->d_W, b->side() ? b->x_cap : b->Bp, b->side(), b->d_assigned, n_slow},
                         b->plan().n_witnesses, b->d_slot_of, b->d_producer, b->unscale.index, b->unscale.consts_plain, b->d_unscale_m256,
                         out, plan.pitch, windows, fields};
    launch_export_records(s, x, plan.n_windows);
    HIPCHK(hipGetLastError());
    if (host) HIPCHK(hipMemcpyAsync(records, out, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // (also what keeps slow_ids alive for its copy)
    return 0;
}
int acvm_batch_export_device_records(acvm_batch_t *b, const acvm_record_out_desc_t *d, const uint32_t *d_instances, void *d_records) try {
    return export_records(b, d, d_instances, d_records, false);
} ABI_CATCH
int acvm_batch_witness_records(acvm_batch_t *b, const acvm_record_out_desc_t *d, void *records) try {
    return export_records(b, d, nullptr, records, true);
} ABI_CATCH

// ---- the map in the reference's wire format for many instances (include/acvm_amd.h acvm_batch_witness_maps_wire_device): wire_plan.cpp checks
// the descriptor and makes the generic instance's rank table and the CRC power table, which go up with the witness list into the staging arena
// (nothing per instance); a pre-pass makes the exact lanes' ranks from their assigned bitmap; kernels_wire.hip writes the slots. Range and list
// are the same kernels, and both find the exact lanes through the lane map. Host form: the slots are made in the staging arena in chunks of
// instances, one copy down per chunk, and row i's bytes [0, lengths[i]) reach the caller's buffer.
//
// The packed forms (acvm_batch_witness_maps_wire_packed_device): the same slots, made chunk by chunk in the arena by the same launches; behind
// each chunk kernels_wire_pack.hip scans its lengths into the offsets column -- the running base stays in a device word -- and packs its rows
// into the caller's buffer. Host form: the chunk is packed into a second region of the arena and its packed range comes down in one copy,
// straight to out + the chunk's base.
struct WirePacked {
    uint64_t capacity;
    uint64_t *offsets;  // [n + 1], where the buffer is: device or host
    uint64_t *total;
    uint32_t *n_fit;
};
static WireRepitch wire_pack_call(const uint8_t *slots, uint64_t pitch, const uint64_t *lengths, uint32_t m, uint8_t *dst, const uint64_t *dst_offsets, uint64_t rebase, uint64_t capacity) {
    return WireRepitch{m, slots, pitch, nullptr, (uint64_t)m * pitch, (uint32_t)((uintptr_t)slots & 15u), lengths, dst, 0u, dst_offsets, rebase, capacity,
                       (uint32_t)((uintptr_t)dst & 15u), wire_repitch_units(pitch)};
}
static int export_wire(acvm_batch *b, const acvm_wire_desc_t *d, const uint32_t *d_instances, void *bytes, uint64_t *lengths, bool host, const WirePacked *packed = nullptr) {
    WirePlan plan;
    std::string refusal;
    const uint32_t *live = b ? &b->B : nullptr, *producer = b ? b->plan().producer.data() : nullptr;
    const uint32_t n_witnesses = b ? b->plan().n_witnesses : 0u;
    if (int rc = packed ? wire_pack_plan(live, producer, n_witnesses, d, d_instances != nullptr, bytes, packed->capacity, packed->offsets, !host, &plan, &refusal)
                        : wire_plan(live, producer, n_witnesses, d, d_instances != nullptr, bytes, !host, &plan, &refusal))
        return set_err(rc, refusal);
    if (host && !packed && plan.n && !lengths) return set_err(ACVM_E_INVALID, "null lengths");
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (plan.whole) {
        if (b->side()) return set_err(ACVM_E_STATE, "the batch recycles witness rows (ACVM_BATCH_REUSE_SLOTS) or solved its exact lanes in the side table: full maps are not kept; read the kept witnesses and the digest");
        if (int rc = refuse_if_next_imported(b, nullptr, 0, true)) return rc;
    } else {
        if (int rc = refuse_if_next_imported(b, plan.witnesses.data(), plan.n_positions, false)) return rc;
        if (int rc = reuse_check_kept(b, plan.witnesses.data(), plan.n_positions)) return rc;
    }
    if (!plan.n && !packed) return 0;
    HIPCHK(hipSetDevice(b->device));
    if (!plan.n) {  // (the offsets column is always written)
        if (host) packed->offsets[0] = 0u;
        else HIPCHK(hipMemset(packed->offsets, 0, 8));
        if (packed->total) *packed->total = 0u;
        if (packed->n_fit) *packed->n_fit = 0u;
        return 0;
    }
    const bool gzip = plan.container == ACVM_WIRE_GZIP_STORED;
    const uint32_t n_slow = (uint32_t)b->slow_ids.size(), n_words = (uint32_t)plan.list_mask.size();
    const bool map_stale = !(b->d_lane_map && b->lane_map_epoch == b->slow_epoch);
    // the rows of one pass: all of them into the caller's device buffer, or what fits the chunk of the staging arena (whole blocks of 64 rows)
    uint32_t chunk = plan.n;
    const bool staged = host || packed;  // the slots are made in the arena
    if (staged) chunk = wire_chunk_rows(plan.n, plan.pitch);
    // the arena: [witness list][rank][list mask][crc powers][slow ids][lane prefix][deflate table][crc words][host: lengths, slots], or behind
    // the crc words [packed: wire_pack_arena's pieces]
    size_t at = 0;
    auto carve = [&](size_t n_bytes) { const size_t begin = at; at += align256(n_bytes); return begin; };
    const size_t at_sel = carve(plan.whole ? 0 : (size_t)plan.n_positions * 4), at_rank = carve(plan.rank.size() * 4), at_mask = carve((size_t)n_words * 4);
    const size_t at_pow = carve(plan.crc_pow.size() * 4), at_ids = carve(map_stale ? (size_t)n_slow * 4 : 0), at_prefix = carve(((size_t)n_words + 1) * n_slow * 4);
    const size_t at_deflate = carve(plan.deflate.size() * 4);
    const size_t at_crc = carve(gzip ? (size_t)chunk * 4 : 0);
    const WirePackArena pack = wire_pack_arena(at, chunk, plan.pitch, host);
    const size_t at_lengths = packed ? (size_t)pack.at_lengths : carve(host ? (size_t)chunk * 8 : 0), at_slots = packed ? (size_t)pack.at_slots : carve(host ? (size_t)chunk * plan.pitch : 0);
    if (packed) at = (size_t)pack.end;
    if (int rc = stage_reserve(b, at)) return rc;
    hipStream_t s = b->stream;
    auto put = [&](size_t where, const std::vector<uint32_t> &v) -> hipError_t {
        if (v.empty()) return hipSuccess;
        b->n_export_h2d_bytes += (uint64_t)v.size() * 4;
        return hipMemcpyAsync(b->d_stage + where, v.data(), v.size() * 4, hipMemcpyHostToDevice, s);
    };
    HIPCHK(put(at_sel, plan.witnesses));
    HIPCHK(put(at_rank, plan.rank));
    HIPCHK(put(at_mask, plan.list_mask));
    HIPCHK(put(at_pow, plan.crc_pow));
    HIPCHK(put(at_deflate, plan.deflate));
    if (int rc = lane_map_ready(b, s, (uint32_t *)(b->d_stage + at_ids))) return rc;
    uint32_t *d_prefix = n_slow ? (uint32_t *)(b->d_stage + at_prefix) : nullptr;
    launch_wire_lane_prefix(s, b->d_assigned, n_slow, n_words, (const uint32_t *)(b->d_stage + at_mask), d_prefix);
    std::vector<uint8_t> slots;
    if (host && !packed) slots.resize((size_t)chunk * plan.pitch);
    uint64_t *d_state = (uint64_t *)(b->d_stage + pack.at_state);
    if (packed) HIPCHK(hipMemsetAsync(d_state, 0, REPITCH_STATE_WORDS * 8, s));
    for (uint32_t done = 0; done < plan.n; done += chunk) {
        const uint32_t m = std::min(chunk, plan.n - done);
        uint32_t *d_crc = gzip ? (uint32_t *)(b->d_stage + at_crc) : nullptr;
        if (gzip) launch_fill_u32(s, d_crc, 0u, m);
        const WireExport x{b->d_W, b->Bp, plan.first + done, m,
                           ExportListSource{d_instances, b->B, b->d_lane_map, b->side() ? b->d_Wx : b->d_W, b->side() ? b->x_cap : b->Bp, b->side(), b->d_assigned, n_slow},
                           b->plan().n_witnesses, b->d_slot_of, b->d_producer, b->unscale.index, b->unscale.consts_plain,
                           plan.whole ? nullptr : (const uint32_t *)(b->d_stage + at_sel), plan.n_positions,
                           (const uint32_t *)(b->d_stage + at_rank), (const uint32_t *)(b->d_stage + at_mask), d_prefix, (const uint32_t *)(b->d_stage + at_pow), plan.crc_x64, d_crc,
                           plan.container, staged ? b->d_stage + at_slots : (uint8_t *)bytes, plan.pitch, staged ? (uint64_t *)(b->d_stage + at_lengths) : lengths,
                           plan.deflate.empty() ? nullptr : (const uint32_t *)(b->d_stage + at_deflate), plan.deflate_prefix_bits};
        launch_wire_export(s, x, plan.n_windows);
        HIPCHK(hipGetLastError());
        if (packed && !host) {
            launch_wire_scan(s, x.lengths, m, packed->offsets + done, packed->capacity, d_state);
            if (bytes) launch_wire_repitch(s, wire_pack_call(x.out, plan.pitch, x.lengths, m, (uint8_t *)bytes, packed->offsets + done, 0u, packed->capacity));
            HIPCHK(hipGetLastError());
        } else if (packed) {
            // the chunk's offsets come down first: they say which of its rows fit and how many bytes those are
            uint64_t *d_offsets = (uint64_t *)(b->d_stage + pack.at_offsets), *offsets = packed->offsets + done;
            launch_wire_scan(s, x.lengths, m, d_offsets, packed->capacity, d_state);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(offsets, d_offsets, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            uint32_t fit = 0;
            uint64_t end = 0;
            wire_pack_fit(offsets, m, packed->capacity, &fit, &end);
            if (bytes && fit) {
                uint8_t *d_packed = b->d_stage + pack.at_packed;
                launch_wire_repitch(s, wire_pack_call(x.out, plan.pitch, x.lengths, fit, d_packed, d_offsets, offsets[0], packed->capacity));
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync((uint8_t *)bytes + offsets[0], d_packed, (size_t)(offsets[fit] - offsets[0]), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
            }
        } else if (host) {
            HIPCHK(hipMemcpyAsync(lengths + done, x.lengths, (size_t)m * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(slots.data(), x.out, (size_t)m * plan.pitch, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (uint32_t i = 0; i < m; i++) memcpy((uint8_t *)bytes + (size_t)(done + i) * plan.pitch, &slots[(size_t)i * plan.pitch], (size_t)lengths[done + i]);
        }
    }
    uint64_t state[REPITCH_STATE_WORDS] = {0u, 0u};
    if (packed && !host) HIPCHK(hipMemcpyAsync(state, d_state, sizeof state, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // (also what keeps the plan's tables and slow_ids alive for their copies)
    if (packed) {
        uint32_t fit = (uint32_t)state[REPITCH_STATE_FIT];
        uint64_t total = state[REPITCH_STATE_BASE];
        if (host) wire_pack_fit(packed->offsets, plan.n, packed->capacity, &fit, &total);
        if (packed->total) *packed->total = total;
        if (packed->n_fit) *packed->n_fit = fit;
    }
    return 0;
}
long long acvm_batch_wire_bound(const acvm_batch_t *b, const acvm_wire_desc_t *d) try {
    if (!d) return set_err(ACVM_E_INVALID, "null argument");
    if (!b) return set_err(ACVM_E_INVALID, "null batch");
    if (d->container != ACVM_WIRE_BINCODE && d->container != ACVM_WIRE_GZIP_STORED && d->container != ACVM_WIRE_GZIP_DEFLATE)
        return set_err(ACVM_E_INVALID, "unknown container " + std::to_string(d->container));
    return (long long)wire_plan_bound(d->container, d->witnesses ? d->n_witnesses : b->plan().n_witnesses);
} ABI_CATCH
int acvm_batch_witness_maps_wire_device(acvm_batch_t *b, const acvm_wire_desc_t *d, const uint32_t *d_instances, void *d_bytes, uint64_t *d_lengths) try {
    return export_wire(b, d, d_instances, d_bytes, d_lengths, false);
} ABI_CATCH
int acvm_batch_witness_maps_wire(acvm_batch_t *b, const acvm_wire_desc_t *d, uint8_t *out, uint64_t *lengths) try {
    return export_wire(b, d, nullptr, out, lengths, true);
} ABI_CATCH
int acvm_batch_witness_maps_wire_packed_device(acvm_batch_t *b, const acvm_wire_desc_t *d, const uint32_t *d_instances, void *d_bytes, uint64_t capacity, uint64_t *d_offsets,
                                               uint64_t *total, uint32_t *n_fit) try {
    const WirePacked packed{capacity, d_offsets, total, n_fit};
    return export_wire(b, d, d_instances, d_bytes, nullptr, false, &packed);
} ABI_CATCH
int acvm_batch_witness_maps_wire_packed(acvm_batch_t *b, const acvm_wire_desc_t *d, uint8_t *out, uint64_t capacity, uint64_t *offsets, uint64_t *total, uint32_t *n_fit) try {
    const WirePacked packed{capacity, offsets, total, n_fit};
    return export_wire(b, d, nullptr, out, nullptr, true, &packed);
} ABI_CATCH

uint64_t acvm_debug_export_h2d_bytes(const acvm_batch_t *b) { return b ? b->n_export_h2d_bytes : 0; }

// ---- per-instance outcomes where the witnesses are (include/acvm_amd.h acvm_batch_outcomes_device). The host's slow_res is the authority (Brillig retries
// and host callbacks finalise lanes there): every instance of the range is written as a generic one -- Solved -- and the records of the exact lanes of
// the range go over them, one small list like the range export's `lanes`. The selection runs on the status column (a scratch one when the caller wants none).
// the two launches of the columns without the wait: n instances Solved, then n_lanes records (device) over them
static void enqueue_outcomes(hipStream_t s, uint32_t n, const uint32_t *d_records, uint32_t n_lanes, uint8_t *d_status, uint8_t *d_err, uint32_t *d_opcode_index) {
    launch_outcomes_fill(s, n, d_status, d_err, d_opcode_index);
    launch_outcomes_lanes(s, d_records, n_lanes, n, d_status, d_err, d_opcode_index);
}

// ---- the tile sinks of the node's device form (batch.hpp TileSink)
static int sink_reserve(acvm_batch *b, int which, size_t bytes) {
    if (bytes <= b->sink_cap[which]) return 0;
    if (b->d_sink[which]) { hipFree(b->d_sink[which]); b->d_sink[which] = nullptr; b->sink_cap[which] = 0; }
    const size_t cap = std::max<size_t>(bytes + bytes / 4, (size_t)64 << 10);
    HIPCHK(hipMalloc((void **)&b->d_sink[which], cap));
    b->sink_cap[which] = cap;
    return 0;
}
// digests of ALL lanes of the side table (lane t = the t-th flagged instance) into the rows of the pairs' instances: out[i] for the pairs (t, i).
// d_part / d_rows: digest_chunks x n_slow x 32 and n_slow x 32 bytes of scratch the caller reserved
static void enqueue_side_digests(acvm_batch *b, hipStream_t s, const uint32_t *d_lanes, uint32_t n_lanes, uint32_t n, uint4 *d_part, uint8_t *d_rows, uint8_t *out) {
    const uint32_t n_slow = (uint32_t)b->slow_ids.size();
    const TableView t = side_table(b);
    launch_digest(s, t.W, t.Bp, 0, n_slow, b->plan().n_witnesses, b->d_producer, t.u, b->fp, (const int32_t *)b->d_ids_x, b->d_assigned, n_slow, d_part, d_rows);
    launch_scatter_rows32(s, (const uint32_t *)d_rows, d_lanes, n_lanes, n, out);
}
static size_t side_digest_bytes(const acvm_batch *b, uint32_t n_slow) { return align256((size_t)digest_chunks(b->plan().n_witnesses) * n_slow * 32) + align256((size_t)n_slow * 32); }

int batch_enqueue_tile_outcomes(acvm_batch *b, const TileSink *k) try {
    if (!b || !k) return set_err(ACVM_E_INVALID, "null argument");
    if (!b->solved || k->n != b->B) return set_err(ACVM_E_STATE, "batch not solved");
    HIPCHK(hipSetDevice(b->device));
    const Plan &p = b->plan();
    hipStream_t s = b->stream;
    const uint32_t n = k->n, n_slow = (uint32_t)b->slow_ids.size();
    const bool defer = b->pending;  // the instances of the exact path arrive with the job's outcome (side_table_to_sink)
    // the lanes of a synchronous exact path are final: their (lane, instance) pairs and their records {status, err, opcode index, instance}
    std::vector<uint32_t> &lanes = b->sink_lanes, &records = b->sink_records;
    lanes.clear();
    records.clear();
    if (!defer)
        for (uint32_t t = 0; t < n_slow; t++) {
            const uint32_t j = b->slow_ids[t];
            if (j >= n) continue;
            lanes.insert(lanes.end(), {t, j});
            if (p.n_opcodes != 0 && t < b->slow_res.size()) records.insert(records.end(), {b->slow_res[t].status, b->slow_res[t].err, b->slow_res[t].opcode_index, j});
        }
    const uint32_t n_lanes = (uint32_t)(lanes.size() / 2);
    const bool side_digests = k->d_digests && n_lanes && b->side(), map_digests = k->d_digests && n_lanes && !b->side();
    const bool map_stale = map_digests && !(b->d_lane_map && b->lane_map_epoch == b->slow_epoch);
    const size_t lanes_bytes = align256(lanes.size() * 4), rec_bytes = align256(records.size() * 4), ids_bytes = map_stale ? align256((size_t)n_slow * 4) : 0;
    if (int rc = sink_reserve(b, 0, lanes_bytes + rec_bytes + ids_bytes + (side_digests ? side_digest_bytes(b, n_slow) : 0))) return rc;
    uint32_t *d_lanes = (uint32_t *)b->d_sink[0], *d_records = (uint32_t *)(b->d_sink[0] + lanes_bytes), *d_ids = (uint32_t *)(b->d_sink[0] + lanes_bytes + rec_bytes);
    uint8_t *d_digest_scratch = b->d_sink[0] + lanes_bytes + rec_bytes + ids_bytes;
    // (the host lists are the handle's: they live until the next solve has waited for this stream)
    if (n_lanes) HIPCHK(hipMemcpyAsync(d_lanes, lanes.data(), lanes.size() * 4, hipMemcpyHostToDevice, s));
    if (!records.empty()) HIPCHK(hipMemcpyAsync(d_records, records.data(), records.size() * 4, hipMemcpyHostToDevice, s));
    if (k->h2d) *k->h2d += (uint64_t)(lanes.size() + records.size()) * 4;
    if (k->d_kept && k->n_keep) {
        const ExportDevice x{k->encoding, k->layout, 0u, n, k->d_keep, k->n_keep, p.n_witnesses, k->stride, k->d_kept, k->d_kept_assigned};
        if (int rc = enqueue_export_device(b, s, x, d_lanes, n_lanes)) return rc;
    }
    enqueue_outcomes(s, n, d_records, (uint32_t)(records.size() / 4), k->d_status, k->d_err, k->d_opcode_index);
    if (k->d_digests) {
        if (int rc = ensure_digest_tables(b)) return rc;
        const bool folded = p.n_digest_segments && b->d_leaves;
        // every lane read as a generic instance (batch_export_tile's rule: an event word that is set would send the kernel to the assigned
        // bitmap of a job that is still running; the exact lanes' rows are leftovers and are overwritten)
        auto generic = [&]() -> int {
            const size_t part_bytes = align256((size_t)digest_chunks(p.n_witnesses) * n * 32);
            if (int rc = stage_reserve(b, part_bytes)) return rc;
            TableView t = level_table(b);
            t.u.event = nullptr;
            launch_digest(s, t.W, t.Bp, 0, n, p.n_witnesses, b->d_producer, t.u, b->fp, nullptr, b->d_assigned, 0, (uint4 *)b->d_stage, k->d_digests);
            return 0;
        };
        if (map_digests) {
            // a plain table with final exact lanes: the table-wide kernel serves generic and exact lanes alike (acvm_batch_digest) through the
            // instance -> lane map, which is made on the device
            const size_t part_bytes = align256((size_t)digest_chunks(p.n_witnesses) * n * 32);
            if (int rc = stage_reserve(b, part_bytes)) return rc;
            const uint64_t before = b->n_export_h2d_bytes;
            if (int rc = lane_map_ready(b, s, d_ids)) return rc;
            if (k->h2d) *k->h2d += b->n_export_h2d_bytes - before;
            const TableView t = level_table(b);
            launch_digest(s, t.W, t.Bp, 0, n, p.n_witnesses, b->d_producer, t.u, b->fp, b->d_lane_map, b->d_assigned, n_slow, (uint4 *)b->d_stage, k->d_digests);
        } else {
            if (folded && (defer || !n_lanes || (!b->force_slow && !b->stepping))) launch_digest_final(s, b->d_leaves, p.n_digest_segments, b->Bp, 0, n, side_digests ? b->d_event : nullptr, b->fp, k->d_digests);
            else if (int rc = generic()) return rc;
            if (side_digests) enqueue_side_digests(b, s, d_lanes, n_lanes, n, (uint4 *)d_digest_scratch, d_digest_scratch + align256((size_t)digest_chunks(p.n_witnesses) * n_slow * 32), k->d_digests);
        }
    }
    HIPCHK(hipGetLastError());
    if (!b->ev_sink) HIPCHK(hipEventCreateWithFlags(&b->ev_sink, hipEventDisableTiming));
    HIPCHK(hipEventRecord(b->ev_sink, s));
    return 0;
} ABI_CATCH

void batch_set_exact_sink(acvm_batch *b, const TileSink *sink) {
    if (!b->pending) return;
    b->exact_sink = *sink;
    b->exact_sink_set = true;
}
int batch_stream_synchronize(acvm_batch *b) {
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}

int side_table_to_sink(acvm_batch *b, ExactOutcome *out) {
    const TileSink &k = b->exact_sink;
    hipStream_t s = b->xstream();
    const uint32_t n_slow = (uint32_t)b->slow_ids.size();
    if (out) {
        out->instance = b->slow_ids;
        out->results.resize(n_slow);
        for (uint32_t t = 0; t < n_slow; t++) result_head(b->slow_res[t], out->results[t]);
    }
    std::vector<uint32_t> lanes, records;
    for (uint32_t t = 0; t < n_slow; t++) {
        const uint32_t j = b->slow_ids[t];
        if (j >= k.n) continue;
        lanes.insert(lanes.end(), {t, j});
        records.insert(records.end(), {b->slow_res[t].status, b->slow_res[t].err, b->slow_res[t].opcode_index, j});
    }
    const uint32_t n_lanes = (uint32_t)(lanes.size() / 2);
    if (!n_lanes) return 0;
    const size_t lanes_bytes = align256(lanes.size() * 4), rec_bytes = align256(records.size() * 4);
    if (int rc = sink_reserve(b, 1, lanes_bytes + rec_bytes + (k.d_digests ? side_digest_bytes(b, n_slow) : 0))) return rc;
    uint32_t *d_lanes = (uint32_t *)b->d_sink[1], *d_records = (uint32_t *)(b->d_sink[1] + lanes_bytes);
    uint8_t *d_digest_scratch = b->d_sink[1] + lanes_bytes + rec_bytes;
    if (k.d_digests)
        if (int rc = ensure_digest_tables(b)) return rc;
    // the level kernels' leftovers for these rows were written on the handle's stream: these writes go over them
    if (b->ev_sink) HIPCHK(hipStreamWaitEvent(s, b->ev_sink, 0));
    HIPCHK(hipMemcpyAsync(d_lanes, lanes.data(), lanes.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_records, records.data(), records.size() * 4, hipMemcpyHostToDevice, s));
    if (k.h2d) *k.h2d += (uint64_t)(lanes.size() + records.size()) * 4;
    if (k.d_kept && k.n_keep) {  // from the side table while it still holds them: the next job's gather overwrites it
        const ExportDevice x{k.encoding, k.layout, 0u, k.n, k.d_keep, k.n_keep, b->plan().n_witnesses, k.stride, k.d_kept, k.d_kept_assigned};
        (export_enc_is_narrow(k.encoding) ? launch_export_narrow_lanes : launch_export_device_lanes)(s, x, b->d_Wx, b->x_cap, true, d_lanes, n_lanes, b->d_assigned, n_slow);
    }
    launch_outcomes_lanes(s, d_records, n_lanes, k.n, k.d_status, k.d_err, k.d_opcode_index);
    if (k.d_digests) enqueue_side_digests(b, s, d_lanes, n_lanes, k.n, (uint4 *)d_digest_scratch, d_digest_scratch + align256((size_t)digest_chunks(b->plan().n_witnesses) * n_slow * 32), k.d_digests);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));  // (also what keeps the two lists alive for their copies)
    return 0;
}

int acvm_batch_outcomes_device(acvm_batch_t *b, const acvm_outcomes_desc_t *d, uint32_t *n_selected) try {
    if (!d) return set_err(ACVM_E_INVALID, "null argument");
    if (!d->d_status && !d->d_err && !d->d_opcode_index && !d->d_selected && !n_selected)
        return set_err(ACVM_E_INVALID, "nothing to write: every column, the selection and its count are null");
    if (!b) return set_err(ACVM_E_INVALID, "null argument");
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    const uint32_t first = d->first, n = d->n;
    if (int rc = require_instance_range(b, first, n)) return rc;
    if (n_selected) *n_selected = 0;
    if (!n) return 0;
    HIPCHK(hipSetDevice(b->device));
    // {status, err, opcode index, index in the range} of the exact lanes of the range (slow_ids ascends with the instance); fill_result's rule
    std::vector<uint32_t> records;
    if (b->plan().n_opcodes != 0) {
        const auto lo = std::lower_bound(b->slow_ids.begin(), b->slow_ids.end(), first);
        for (auto it = lo; it != b->slow_ids.end() && (uint64_t)*it < (uint64_t)first + n; ++it) {
            const SlowResult &sr = b->slow_res[(size_t)(it - b->slow_ids.begin())];
            records.insert(records.end(), {sr.status, sr.err, sr.opcode_index, *it - first});
        }
    }
    const uint32_t n_lanes = (uint32_t)(records.size() / 4);
    const bool select = d->d_selected || n_selected;
    const size_t rec_bytes = align256(records.size() * 4), status_bytes = select && !d->d_status ? align256(n) : 0;
    const size_t scan_bytes = select ? align256((select_scratch_words(n) + 1) * 4) : 0;
    if (rec_bytes + status_bytes + scan_bytes)
        if (int rc = stage_reserve(b, rec_bytes + status_bytes + scan_bytes)) return rc;
    hipStream_t s = b->stream;
    uint32_t *d_records = (uint32_t *)b->d_stage;
    uint8_t *d_status = d->d_status ? d->d_status : select ? b->d_stage + rec_bytes : nullptr;
    uint32_t *d_scan = (uint32_t *)(b->d_stage + rec_bytes + status_bytes), *d_count = d_scan + select_scratch_words(n);
    if (n_lanes) {
        HIPCHK(hipMemcpyAsync(d_records, records.data(), records.size() * 4, hipMemcpyHostToDevice, s));
        b->n_export_h2d_bytes += (uint64_t)records.size() * 4;
    }
    enqueue_outcomes(s, n, d_records, n_lanes, d_status, d->d_err, d->d_opcode_index);
    uint32_t count = 0;
    if (select) {
        launch_select(s, d_status, first, n, d->select_mask, d_scan, d->d_selected, d_count);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));  // (also what keeps `records` and `count` alive for their copies)
    if (n_selected) *n_selected = count;
    return 0;
} ABI_CATCH

int acvm_device_download(void *dst_host, const void *src_device, size_t bytes) {
    if (bytes && (!dst_host || !src_device)) return set_err(ACVM_E_INVALID, "null argument");
    if (bytes) HIPCHK(hipMemcpy(dst_host, src_device, bytes, hipMemcpyDeviceToHost));
    return 0;
}

long long acvm_batch_witness_map_bytes(acvm_batch_t *b, uint32_t instance, uint8_t *out, size_t cap) try {
    if (!b) return set_err(ACVM_E_INVALID, "null argument");
    if (!b->solved) return set_err(ACVM_E_STATE, "batch not solved");
    if (instance >= b->B) return set_err(ACVM_E_INVALID, "instance out of range");
    const uint32_t nw = b->plan().n_witnesses;
    std::vector<uint8_t> assigned(nw ? nw : 1), values((size_t)(nw ? nw : 1) * 32);
    if (int rc = acvm_batch_witness_map(b, instance, 1, assigned.data(), values.data())) return rc;
    std::vector<uint32_t> ids;
    std::vector<uint8_t> vals;
    for (uint32_t w = 0; w < nw; w++)
        if (assigned[w]) {
            ids.push_back(w);
            vals.insert(vals.end(), values.begin() + (size_t)w * 32, values.begin() + (size_t)w * 32 + 32);
        }
    return acvm_witness_map_encode(ids.data(), vals.data(), (uint32_t)ids.size(), out, cap);
} ABI_CATCH

int acvm_batch_witness(acvm_batch_t *b, uint32_t witness, uint8_t *out_be32, uint8_t *assigned) try {
    if (!b || !out_be32 || !assigned) return set_err(ACVM_E_INVALID, "null argument");
    if (int rc = finish_pending_and_require_solved(b)) return rc;
    if (witness >= b->plan().n_witnesses) { memset(assigned, 0, b->B); memset(out_be32, 0, (size_t)b->B * 32); return 0; }
    if (int rc = refuse_if_next_imported(b, &witness, 1, false)) return rc;
    HIPCHK(hipSetDevice(b->device));
    if (!b->B) return 0;
    if (int rc = reuse_check_kept(b, &witness, 1)) return rc;
    if (int rc = read_witnesses(b, b->stream, level_table(b), 0, b->B, &witness, 1, out_be32)) return rc;
    if (int rc = reuse_patch_exact(b, &witness, 1, 0, b->B, out_be32)) return rc;
    hipError_t herr = hipSuccess;
    batch_assigned(b, &herr).fill(0, b->B, &witness, 1, assigned, out_be32);
    HIPCHK(herr);
    return 0;
} ABI_CATCH
