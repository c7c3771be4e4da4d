// record_plan.cpp -- the checks, the field table and the window cut of the record import and of its masked form (record_plan.hpp). Everything
// the caller controls is judged here. Nothing here knows a device.
#include "record_plan.hpp"
#include <algorithm>

namespace acvm {

int import_plan_records(const ImportView *view, const acvm_record_desc_t *d, const void *d_records, ImportPlan *out, std::string *err) {
    auto refuse = [&](const std::string &text) { *err = text; return ACVM_E_INVALID; };
    if (!d) return refuse("null argument");
    if (d->n_fields && !d->fields) return refuse("null fields");
    if (!view) return refuse("null batch");
    const uint32_t n_in = view->n_in, n_fields = d->n_fields;
    const uint64_t pitch = d->pitch;
    std::vector<int64_t> owner(n_in, -1);
    for (uint32_t f = 0; f < n_fields; f++) {
        const acvm_record_field_t &fd = d->fields[f];
        auto who = [&] { return "field " + std::to_string(f) + " (position " + std::to_string(fd.position) + "): "; };  // (a refusal's text only)
        if (fd.encoding > ACVM_ENC_MONT256_LE && !(fd.encoding >= ACVM_ENC_U8 && fd.encoding <= ACVM_ENC_U128)) return refuse(who() + "unknown encoding " + std::to_string(fd.encoding));
        if (fd.position >= n_in) return refuse(who() + "position " + std::to_string(fd.position) + " is not below n_initial " + std::to_string(n_in));
        const uint64_t size = buffer_element_size(fd.encoding);
        // (offset + size may wrap 2^64: judged by differences)
        if (fd.offset > pitch || size > pitch - fd.offset)
            return refuse(who() + "offset " + std::to_string(fd.offset) + " + size " + std::to_string(size) + " is beyond the pitch " + std::to_string(pitch));
        if (owner[fd.position] >= 0)
            return refuse("position " + std::to_string(fd.position) + " is supplied twice (fields " + std::to_string(owner[fd.position]) + " and " + std::to_string(f) + ")");
        owner[fd.position] = (int64_t)f;
    }
    for (uint32_t pos = 0; pos < n_in; pos++)
        if (owner[pos] < 0) return refuse("position " + std::to_string(pos) + " (initial witness " + std::to_string(view->ids[pos]) + ") is supplied by no field");
    if (n_fields && view->B && !d_records) return refuse("null records");
    // (the byte offset of the last record fits 63 bits)
    if (n_fields && (unsigned __int128)view->B * pitch > ((unsigned __int128)1 << 57)) return refuse("pitch " + std::to_string(pitch) + " is beyond any device buffer");

    // ---- every check has passed: the windows, each with the indices of its fields
    struct Cut { uint64_t offset; uint32_t length; std::vector<uint32_t> fields; };
    std::vector<Cut> cuts;
    if (n_fields && pitch <= RECORD_PLAN_WINDOW_CAP) {
        cuts.push_back(Cut{0, (uint32_t)pitch, {}});
        for (uint32_t f = 0; f < n_fields; f++) cuts[0].fields.push_back(f);
    } else if (n_fields) {
        std::vector<uint32_t> order(n_fields);
        for (uint32_t f = 0; f < n_fields; f++) order[f] = f;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return d->fields[a].offset < d->fields[b].offset; });
        for (uint32_t f : order) {
            const uint64_t begin = d->fields[f].offset, end = begin + buffer_element_size(d->fields[f].encoding);  // (end <= pitch: no wrap)
            if (cuts.empty() || end - cuts.back().offset > RECORD_PLAN_WINDOW_CAP) cuts.push_back(Cut{begin, 0, {}});
            Cut &c = cuts.back();
            c.length = std::max<uint32_t>(c.length, (uint32_t)(end - c.offset));
            c.fields.push_back(f);
        }
    }
    ImportPlan plan;
    plan.records = true;
    plan.record_pitch = pitch;
    plan.record_windows = (uint32_t)cuts.size();
    plan.d_records = d_records;
    plan.lists.reserve(cuts.size() * RECORD_WINDOW_WORDS + (size_t)n_fields * RECORD_FIELD_WORDS);
    uint32_t first = 0;
    for (const Cut &c : cuts) {
        plan.lists.insert(plan.lists.end(), {(uint32_t)c.offset, (uint32_t)(c.offset >> 32), c.length, first, (uint32_t)c.fields.size()});
        first += (uint32_t)c.fields.size();
    }
    for (const Cut &c : cuts)
        for (uint32_t f : c.fields) {
            const acvm_record_field_t &fd = d->fields[f];
            plan.lists.insert(plan.lists.end(), {view->rows[fd.position], view->planes ? view->planes[fd.position] : 0xFFFFFFFFu, fd.encoding, (uint32_t)(fd.offset - c.offset)});
        }
    *out = std::move(plan);
    return 0;
}

int import_plan_records_masked(const ImportView *view, const acvm_record_masked_desc_t *d, const void *d_records, ImportPlan *out, std::string *err) {
    auto refuse = [&](const std::string &text) { *err = text; return ACVM_E_INVALID; };
    if (!d) return refuse("null argument");
    if (d->n_fields && !d->fields) return refuse("null fields");
    // ---- the unmasked call's checks, by the unmasked call: the same order and the same texts, and -- no field with a mask -- its plan
    const uint32_t n_fields = d->n_fields;
    const uint64_t pitch = d->pitch;
    std::vector<acvm_record_field_t> plain(n_fields);
    bool any_mask = false;
    for (uint32_t f = 0; f < n_fields; f++) {
        plain[f] = acvm_record_field_t{d->fields[f].position, d->fields[f].encoding, d->fields[f].offset};
        any_mask = any_mask || d->fields[f].mask_offset != ACVM_RECORD_NO_MASK;
    }
    const acvm_record_desc_t pd{pitch, plain.data(), n_fields};
    ImportPlan unmasked;
    if (int rc = import_plan_records(view, &pd, d_records, &unmasked, err)) return rc;
    for (uint32_t f = 0; f < n_fields; f++) {
        const acvm_record_masked_field_t &fd = d->fields[f];
        if (fd.mask_offset != ACVM_RECORD_NO_MASK && fd.mask_offset >= pitch)
            return refuse("field " + std::to_string(f) + " (position " + std::to_string(fd.position) + "): mask_offset " + std::to_string(fd.mask_offset) +
                          " is not below the pitch " + std::to_string(pitch));
    }
    if (!any_mask) {
        *out = std::move(unmasked);
        return 0;
    }

    // ---- the units: a field with its mask byte where the two span at most a window, the element alone where they do not (or there is no mask)
    struct Unit { uint64_t begin, end; bool far; };
    std::vector<Unit> units(n_fields);
    for (uint32_t f = 0; f < n_fields; f++) {
        const acvm_record_masked_field_t &fd = d->fields[f];
        Unit u{fd.offset, fd.offset + buffer_element_size(fd.encoding), false};  // (end <= pitch: no wrap)
        if (fd.mask_offset != ACVM_RECORD_NO_MASK) {
            const uint64_t begin = std::min(u.begin, fd.mask_offset), end = std::max(u.end, fd.mask_offset + 1);
            if (end - begin <= RECORD_PLAN_WINDOW_CAP) { u.begin = begin; u.end = end; }
            else u.far = true;
        }
        units[f] = u;
    }
    struct Cut { uint64_t offset; uint32_t length; std::vector<uint32_t> fields; };
    std::vector<Cut> cuts;
    if (pitch <= RECORD_PLAN_WINDOW_CAP) {  // (the record is the window: every unit is near)
        cuts.push_back(Cut{0, (uint32_t)pitch, {}});
        for (uint32_t f = 0; f < n_fields; f++) cuts[0].fields.push_back(f);
    } else {
        std::vector<uint32_t> order(n_fields);
        for (uint32_t f = 0; f < n_fields; f++) order[f] = f;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return units[a].begin < units[b].begin; });
        for (uint32_t f : order) {
            if (cuts.empty() || units[f].end - cuts.back().offset > RECORD_PLAN_WINDOW_CAP) cuts.push_back(Cut{units[f].begin, 0, {}});
            Cut &c = cuts.back();
            c.length = std::max<uint32_t>(c.length, (uint32_t)(units[f].end - c.offset));
            c.fields.push_back(f);
        }
    }
    ImportPlan plan;
    plan.records = true;
    plan.record_masks = true;
    plan.record_pitch = pitch;
    plan.record_windows = (uint32_t)cuts.size();
    plan.d_records = d_records;
    plan.lists.reserve(cuts.size() * RECORD_MWINDOW_WORDS + (size_t)n_fields * RECORD_MFIELD_WORDS);
    uint32_t first = 0;
    for (const Cut &c : cuts) {
        uint32_t base = 0xFFFFFFFFu;
        for (uint32_t f : c.fields) base = std::min(base, d->fields[f].position >> 5);
        plan.lists.insert(plan.lists.end(), {(uint32_t)c.offset, (uint32_t)(c.offset >> 32), c.length, first, (uint32_t)c.fields.size(), base});
        first += (uint32_t)c.fields.size();
    }
    for (const Cut &c : cuts)
        for (uint32_t f : c.fields) {
            const acvm_record_masked_field_t &fd = d->fields[f];
            const bool none = fd.mask_offset == ACVM_RECORD_NO_MASK, far = units[f].far;
            plan.lists.insert(plan.lists.end(), {view->rows[fd.position], view->planes ? view->planes[fd.position] : 0xFFFFFFFFu, fd.encoding, (uint32_t)(fd.offset - c.offset),
                                                 fd.position, none ? RECORD_MASK_NONE : far ? RECORD_MASK_FAR : (uint32_t)(fd.mask_offset - c.offset),
                                                 far ? (uint32_t)fd.mask_offset : 0u, far ? (uint32_t)(fd.mask_offset >> 32) : 0u});
        }
    *out = std::move(plan);
    return 0;
}

}  // namespace acvm
