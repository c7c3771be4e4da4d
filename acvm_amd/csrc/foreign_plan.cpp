// foreign_plan.cpp -- the site list, the waiting lists, the refusals, the shape words and the capacity rule of the batch-wide foreign-call round trip
// (foreign_plan.hpp). Everything the caller controls is judged here. Nothing here knows a device.
#include "foreign_plan.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>

namespace acvm {

static bool waits(const FcLaneRecord &l) { return l.status == ACVM_STATUS_REQUIRES_FOREIGN_CALL; }

std::vector<acvm_foreign_call_site_t> foreign_sites(const std::vector<FcSiteDecl> &decls, const FcLaneRecord *lanes, size_t n_lanes) {
    std::map<uint64_t, const FcSiteDecl *> known;
    for (const FcSiteDecl &d : decls) known[((uint64_t)d.opcode_index << 32) | d.brillig_index] = &d;
    std::map<uint64_t, acvm_foreign_call_site_t> sites;  // (ordered by (opcode, brillig index))
    for (size_t t = 0; t < n_lanes; t++) {
        const FcLaneRecord &l = lanes[t];
        if (!waits(l)) continue;
        const uint64_t key = ((uint64_t)l.opcode_index << 32) | l.brillig_index;
        auto decl = known.find(key);
        if (decl != known.end() && decl->second->internal) continue;
        auto it = sites.find(key);
        if (it == sites.end()) {
            acvm_foreign_call_site_t s;
            memset(&s, 0, sizeof s);
            s.opcode_index = l.opcode_index;
            s.brillig_index = l.brillig_index;
            if (decl != known.end()) {
                s.n_inputs = decl->second->n_inputs;
                snprintf(s.function, sizeof s.function, "%s", decl->second->function.c_str());
            }
            it = sites.emplace(key, s).first;
        }
        it->second.n_waiting++;
        it->second.n_resolved += l.resolved_new ? 1u : 0u;
    }
    std::vector<acvm_foreign_call_site_t> out;
    for (auto &kv : sites) out.push_back(kv.second);
    return out;
}

std::vector<FcRow> foreign_waiting_list(const FcLaneRecord *lanes, size_t n_lanes, uint32_t opcode_index, uint32_t brillig_index) {
    std::vector<FcRow> list;
    for (size_t t = 0; t < n_lanes; t++) {
        const FcLaneRecord &l = lanes[t];
        if (!waits(l) || l.opcode_index != opcode_index || l.brillig_index != brillig_index) continue;
        FcRow r;
        r.lane = (uint32_t)t;
        r.instance = l.instance;
        r.resolved = l.resolved_new;
        list.push_back(r);
    }
    // (the lanes of a solve are ascending in their instance already; a list is ascending whatever order they come in)
    std::stable_sort(list.begin(), list.end(), [](const FcRow &a, const FcRow &b) { return a.instance < b.instance; });
    return list;
}

static constexpr uint64_t FC_MAX_WORDS = 1ull << 31;

int foreign_shape(uint32_t n_values, const uint8_t *is_array, const uint32_t *lens, std::vector<uint32_t> *words, uint32_t *total, std::string *err) {
    if (n_values && (!is_array || !lens)) { *err = "null argument"; return ACVM_E_INVALID; }
    if (1ull + 2ull * n_values > FC_MAX_WORDS) { *err = "n_values " + std::to_string(n_values) + " is beyond any result"; return ACVM_E_INVALID; }
    std::vector<uint32_t> w;
    w.reserve(1 + 2 * (size_t)n_values);
    w.push_back(n_values);
    uint64_t sum = 0;
    for (uint32_t k = 0; k < n_values; k++) {
        const uint32_t n = is_array[k] ? lens[k] : 1u;
        w.push_back(is_array[k] ? 1u : 0u);
        w.push_back(n);
        sum += n;
        if (sum > FC_MAX_WORDS) { *err = "the result's " + std::to_string(sum) + " values are beyond any result"; return ACVM_E_INVALID; }
    }
    *words = std::move(w);
    *total = (uint32_t)sum;
    return 0;
}

static std::string range_refusal(uint32_t first_row, uint32_t n_rows, size_t list_size, uint32_t opcode_index, uint32_t brillig_index) {
    if ((uint64_t)first_row + n_rows <= list_size) return std::string();
    return "rows [" + std::to_string(first_row) + ", " + std::to_string((uint64_t)first_row + n_rows) + ") are outside the " + std::to_string(list_size) +
           " rows waiting at opcode " + std::to_string(opcode_index) + ", brillig index " + std::to_string(brillig_index);
}
// the buffer of n_rows x n_columns elements: stride against the layout, the offset of its last element, the pointer
static std::string buffer_refusal(uint32_t encoding, uint32_t layout, uint32_t n_rows, uint32_t n_columns, const void *d_values, uint64_t *stride) {
    std::string err = buffer_check_stride(layout, n_rows, n_columns, stride);
    if (!err.empty()) return err;
    const unsigned __int128 rows = layout == ACVM_LAYOUT_WITNESS_MAJOR ? n_columns : n_rows;
    if (rows * *stride > ((unsigned __int128)1 << 57)) return "stride " + std::to_string(*stride) + " is beyond any device buffer";
    return d_values ? buffer_check_pointer(encoding, d_values) : std::string();
}

int foreign_check_inputs(const FcHandleView *view, const acvm_foreign_call_inputs_desc_t *d, const std::vector<FcRow> &list, uint64_t *stride, std::string *err) {
    if (!view || !d) { *err = "null argument"; return ACVM_E_INVALID; }
    *err = buffer_check_shape(d->encoding, d->layout, false);
    if (!err->empty()) return ACVM_E_INVALID;
    if (!view->solved) { *err = "batch not solved"; return ACVM_E_STATE; }
    if (view->site_internal) { *err = "the calls of this site are answered by the library (the caller's BlackBoxFunctionSolver)"; return ACVM_E_INVALID; }
    *err = range_refusal(d->first_row, d->n_rows, list.size(), d->opcode_index, d->brillig_index);
    if (!err->empty()) return ACVM_E_INVALID;
    uint64_t s = d->stride;
    *err = buffer_refusal(d->encoding, d->layout, d->n_rows, d->n_columns, d->d_values, &s);
    if (!err->empty()) return ACVM_E_INVALID;
    *stride = s;
    return 0;
}

int foreign_check_width(const acvm_foreign_call_inputs_desc_t *d, uint32_t max_values, std::string *err) {
    if ((!d->d_values && !d->d_mask) || d->n_columns >= max_values) return 0;
    *err = "n_columns " + std::to_string(d->n_columns) + " is below the " + std::to_string(max_values) + " values of the longest row";
    return ACVM_E_INVALID;
}

// what both resolve calls check before a device is touched; per_row_lens: the lengths are a device column (the host shape's total and the width are
// judged behind the sizing launch, foreign_check_rows_width); masked: which rows are answered is a device column (foreign_mask_resumes judges them)
static int check_answers(const FcHandleView *view, const acvm_foreign_call_answers_desc_t *d, bool per_row_lens, bool masked, const std::vector<FcRow> &list, uint64_t *stride,
                         std::vector<uint32_t> *words, uint32_t *total, std::string *err) {
    *err = buffer_check_shape(d->encoding, d->layout, false);
    if (!err->empty()) return ACVM_E_INVALID;
    if (!view->solved) { *err = "batch not solved"; return ACVM_E_STATE; }
    if (view->has_solver) {
        *err = "a handle with a caller's BlackBoxFunctionSolver keeps its foreign-call results on the host: resolve per instance (acvm_batch_resolve_foreign_call)";
        return ACVM_E_UNSUPPORTED;
    }
    *err = range_refusal(d->first_row, d->n_rows, list.size(), d->opcode_index, d->brillig_index);
    if (!err->empty()) return ACVM_E_INVALID;
    std::vector<uint32_t> w;
    uint32_t sum = 0;
    if (per_row_lens) {
        // (the host lens are not read: an array output's words carry length 0 here, the row's own length on the device)
        if (d->n_values && !d->is_array) { *err = "null argument"; return ACVM_E_INVALID; }
        const std::vector<uint32_t> none(d->n_values, 0u);
        if (int rc = foreign_shape(d->n_values, d->is_array, none.data(), &w, &sum, err)) return rc;
    } else {
        if (int rc = foreign_shape(d->n_values, d->is_array, d->lens, &w, &sum, err)) return rc;
        if (d->n_columns < sum) {
            *err = "n_columns " + std::to_string(d->n_columns) + " is below the " + std::to_string(sum) + " values of the result's shape";
            return ACVM_E_INVALID;
        }
        if (sum && d->n_rows && !d->d_values) { *err = "null values"; return ACVM_E_INVALID; }
    }
    uint64_t s = d->stride;
    *err = buffer_refusal(d->encoding, d->layout, d->n_rows, d->n_columns, d->d_values, &s);
    if (!err->empty()) return ACVM_E_INVALID;
    if (!masked) {
        std::vector<uint32_t> pairs;
        if (int rc = foreign_mask_resumes(list, d->first_row, d->n_rows, nullptr, &pairs, err)) return rc;
    }
    *stride = s;
    *words = std::move(w);
    *total = sum;
    return 0;
}

int foreign_check_answers(const FcHandleView *view, const acvm_foreign_call_answers_desc_t *d, const std::vector<FcRow> &list, uint64_t *stride, std::vector<uint32_t> *words,
                          uint32_t *total, std::string *err) {
    if (!view || !d) { *err = "null argument"; return ACVM_E_INVALID; }
    return check_answers(view, d, false, false, list, stride, words, total, err);
}

int foreign_check_answers_rows(const FcHandleView *view, const acvm_foreign_call_answers_rows_desc_t *d, const std::vector<FcRow> &list, uint64_t *stride,
                               std::vector<uint32_t> *words, uint32_t *total, std::string *err) {
    if (!view || !d) { *err = "null argument"; return ACVM_E_INVALID; }
    const acvm_foreign_call_answers_desc_t base{d->opcode_index, d->brillig_index, d->first_row, d->n_rows, d->n_values, d->is_array, d->lens, d->encoding, d->layout,
                                                d->n_columns, d->stride, d->d_values};
    return check_answers(view, &base, d->d_lens != nullptr, d->d_answered != nullptr, list, stride, words, total, err);
}

int foreign_mask_resumes(const std::vector<FcRow> &list, uint32_t first_row, uint32_t n_rows, const uint8_t *answered, std::vector<uint32_t> *pairs, std::string *err) {
    std::vector<uint32_t> out;
    for (uint32_t i = 0; i < n_rows; i++) {
        if (answered && !answered[i]) continue;  // (left out: it may have been answered before, or be answered later in the round)
        const uint32_t r = first_row + i;
        if (list[r].resolved) {
            *err = "row " + std::to_string(r) + " (instance " + std::to_string(list[r].instance) + ") was already answered since the last solve; call acvm_batch_solve";
            return ACVM_E_STATE;
        }
        out.push_back(list[r].lane);
        out.push_back(list[r].instance);
    }
    *pairs = std::move(out);
    return 0;
}

int foreign_check_rows_width(uint32_t n_columns, uint32_t longest, bool has_values, uint32_t *total, std::string *err) {
    if (longest >= FC_MAX_WORDS) { *err = "a row's lengths sum to 2^31 values or more: beyond any result"; return ACVM_E_INVALID; }
    if (n_columns < longest) {
        *err = "n_columns " + std::to_string(n_columns) + " is below the " + std::to_string(longest) + " values of the longest answered row";
        return ACVM_E_INVALID;
    }
    if (longest && !has_values) { *err = "null values"; return ACVM_E_INVALID; }
    *total = longest;
    return 0;
}

void foreign_bounds_add(FcBounds *b, uint32_t add_words, uint32_t add_vals) {
    b->round_words = std::max(b->round_words, add_words);
    b->round_vals = std::max(b->round_vals, add_vals);
}
void foreign_bounds_fold(FcBounds *b) {
    // (foreign_capacity refused what would pass 2^31: the sums fit)
    b->words += b->round_words;
    b->vals += b->round_vals;
    b->round_words = b->round_vals = 0;
}

int foreign_capacity(const FcBounds &bounds, uint32_t add_words, uint32_t add_vals, const FcCapacity &have, bool *grow, FcCapacity *want, std::string *err) {
    const uint64_t need_words = (uint64_t)bounds.words + std::max(bounds.round_words, add_words), need_vals = (uint64_t)bounds.vals + std::max(bounds.round_vals, add_vals);
    if (need_words > FC_MAX_WORDS || need_vals > FC_MAX_WORDS) {
        *err = "the results of one opcode would exceed 2^31 descriptor words or values per instance";
        return ACVM_E_INVALID;
    }
    *grow = need_words > have.desc_words || need_vals > have.vals_cap || !have.vals_cap;
    *want = have;
    if (*grow) {
        want->desc_words = (uint32_t)std::max<uint64_t>(have.desc_words, need_words + need_words / 2 + 8);
        want->vals_cap = (uint32_t)std::max<uint64_t>(have.vals_cap, need_vals + need_vals / 2 + 8);
    }
    return 0;
}

}  // namespace acvm
