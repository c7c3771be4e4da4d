// import_plan.cpp -- the checks and the list layout of a device import (import_plan.hpp). Everything the caller controls is judged here: encodings,
// layouts, pointers, strides, column lists, position lists. Nothing here knows a device.
#include "import_plan.hpp"

namespace acvm {

static bool enc_is_narrow(uint32_t e) { return e >= ACVM_ENC_U8 && e <= ACVM_ENC_U128; }
uint32_t buffer_element_size(uint32_t encoding) { return enc_is_narrow(encoding) ? 1u << (encoding - ACVM_ENC_U8) : 32u; }

std::string buffer_check_shape(uint32_t encoding, uint32_t layout, bool broadcast) {
    if (encoding > ACVM_ENC_MONT256_LE && !enc_is_narrow(encoding)) return "unknown encoding " + std::to_string(encoding);
    if (layout > ACVM_LAYOUT_WITNESS_MAJOR && !(broadcast && layout == ACVM_LAYOUT_BROADCAST)) return "unknown layout " + std::to_string(layout);
    return std::string();
}
std::string buffer_check_pointer(uint32_t encoding, const void *d_values) {
    const uint32_t size = buffer_element_size(encoding), align = size < 16u ? size : 16u;
    if (!((uintptr_t)d_values & (align - 1u))) return std::string();
    return size == 32u ? std::string("d_values must be 16-byte aligned") : "d_values must be aligned to the element size, " + std::to_string(size) + " bytes";
}
std::string buffer_check_stride(uint32_t layout, uint32_t n, uint32_t n_sel, uint64_t *stride) {
    const uint64_t dense = layout == ACVM_LAYOUT_WITNESS_MAJOR ? n : n_sel;
    if (!*stride) *stride = dense;
    if (*stride < dense) return "stride " + std::to_string(*stride) + " is below the dense stride " + std::to_string(dense) + " of the layout";
    return std::string();
}

// The checks every described buffer gets, for the n inputs it supplies (all initial witnesses for a descriptor, a part's positions for a part).
// part: the broadcast layout is allowed, and the plain shape's exemption from the alignment rule is not. Leaves *plain and the part's shape;
// the lists are laid out by the callers once every check has passed.
static std::string check_buffer(const ImportView *view, uint32_t encoding, uint32_t layout, const uint32_t *columns, uint32_t n, uint32_t n_columns, uint64_t stride,
                                const void *d_values, bool part, ImportPlanPart *out, bool *plain) {
    std::string err = buffer_check_shape(encoding, layout, part);
    if (!err.empty()) return err;
    if (!view) return "null batch";
    if (n && !d_values) return "null values";
    if (!columns) n_columns = n;
    else
        for (uint32_t k = 0; k < n; k++)
            if (columns[k] >= n_columns)
                return "column " + std::to_string(columns[k]) + " of initial witness " + std::to_string(k) + " is not below n_columns " + std::to_string(n_columns);
    if (layout == ACVM_LAYOUT_BROADCAST) stride = 1;  // (ignored: element c lies at c * size)
    else {
        err = buffer_check_stride(layout, view->B, n_columns, &stride);
        if (!err.empty()) return err;
        // (the byte offset of the last element fits 63 bits)
        const unsigned __int128 rows = layout == ACVM_LAYOUT_WITNESS_MAJOR ? n_columns : view->B;
        if (rows * stride > ((unsigned __int128)1 << 57)) return "stride " + std::to_string(stride) + " is beyond any device buffer";
    }
    *plain = !part && encoding == ACVM_ENC_BE32 && layout == ACVM_LAYOUT_INSTANCE_MAJOR && !columns && stride == view->n_in;
    // (the plain shape IS acvm_batch_set_initial_witness_device, which reads any pointer: import_witness_kernel<false>)
    if (!*plain) {
        err = buffer_check_pointer(encoding, d_values);
        if (!err.empty()) return err;
    }
    out->encoding = encoding;
    out->layout = layout;
    out->elem_size = buffer_element_size(encoding);
    out->stride = stride;
    out->n = n;
    out->d_values = d_values;
    return std::string();
}

ImportPlan import_plan_plain(uint32_t n_in, const void *d_values) {
    ImportPlan plan;
    plan.plain = true;
    plan.parts.resize(1);
    ImportPlanPart &pt = plan.parts[0];
    pt.encoding = ACVM_ENC_BE32;
    pt.layout = ACVM_LAYOUT_INSTANCE_MAJOR;
    pt.stride = pt.n = n_in;
    pt.d_values = d_values;
    pt.resident = true;
    return plan;
}

int import_plan_desc(const ImportView *view, const acvm_import_desc_t *d, const void *d_values, ImportPlan *out, std::string *err) {
    if (!d) { *err = "null argument"; return ACVM_E_INVALID; }
    ImportPlan plan;
    plan.parts.resize(1);
    ImportPlanPart &pt = plan.parts[0];
    const uint32_t n_in = view ? view->n_in : 0u;
    *err = check_buffer(view, d->encoding, d->layout, d->columns, n_in, d->n_columns, d->stride, d_values, false, &pt, &plan.plain);
    if (!err->empty()) return ACVM_E_INVALID;
    pt.resident = true;
    if (d->columns) {
        pt.columns_at = 0;
        plan.lists.assign(d->columns, d->columns + n_in);
    }
    *out = std::move(plan);
    return 0;
}

int import_plan_desc_masked(const ImportView *view, const acvm_import_desc_t *d, const void *d_values, const uint8_t *d_assigned, ImportPlan *out, std::string *err) {
    ImportPlan plan;
    if (int rc = import_plan_desc(view, d, d_values, &plan, err)) return rc;
    plan.d_assigned = d_assigned;
    *out = std::move(plan);
    return 0;
}

int import_plan_parts(const ImportView *view, const acvm_import_part_t *parts, uint32_t n_parts, ImportPlan *out, std::string *err) {
    if (n_parts && !parts) { *err = "null argument"; return ACVM_E_INVALID; }
    ImportPlan plan;
    plan.parts.resize(n_parts);
    for (uint32_t q = 0; q < n_parts; q++) {
        const acvm_import_part_t &pt = parts[q];
        bool plain = false;
        *err = check_buffer(view, pt.encoding, pt.layout, pt.columns, pt.n, pt.n_columns, pt.stride, pt.d_values, true, &plan.parts[q], &plain);
        if (err->empty() && pt.n && !pt.positions) *err = "null positions";
        if (!err->empty()) { *err = "part " + std::to_string(q) + ": " + *err; return ACVM_E_INVALID; }
    }
    if (!view) { *err = "null batch"; return ACVM_E_INVALID; }
    const uint32_t n_in = view->n_in;
    std::vector<int32_t> owner(n_in, -1);
    for (uint32_t q = 0; q < n_parts; q++)
        for (uint32_t k = 0; k < parts[q].n; k++) {
            const uint32_t pos = parts[q].positions[k];
            if (pos >= n_in) { *err = "part " + std::to_string(q) + ": position " + std::to_string(pos) + " is not below n_initial " + std::to_string(n_in); return ACVM_E_INVALID; }
            if (owner[pos] >= 0) {
                *err = "position " + std::to_string(pos) + " is supplied twice (parts " + std::to_string(owner[pos]) + " and " + std::to_string(q) + ")";
                return ACVM_E_INVALID;
            }
            owner[pos] = (int32_t)q;
        }
    for (uint32_t pos = 0; pos < n_in; pos++)
        if (owner[pos] < 0) { *err = "position " + std::to_string(pos) + " (initial witness " + std::to_string(view->ids[pos]) + ") is supplied by no part"; return ACVM_E_INVALID; }
    // every part has passed: the lists
    for (uint32_t q = 0; q < n_parts; q++) {
        const acvm_import_part_t &pt = parts[q];
        ImportPlanPart &pp = plan.parts[q];
        pp.rows_at = plan.lists.size();
        for (uint32_t k = 0; k < pt.n; k++) plan.lists.push_back(view->rows[pt.positions[k]]);
        if (view->planes) {
            pp.planes_at = plan.lists.size();
            for (uint32_t k = 0; k < pt.n; k++) plan.lists.push_back(view->planes[pt.positions[k]]);
        }
        if (pt.columns) {
            pp.columns_at = plan.lists.size();
            plan.lists.insert(plan.lists.end(), pt.columns, pt.columns + pt.n);
        }
    }
    *out = std::move(plan);
    return 0;
}

}  // namespace acvm
