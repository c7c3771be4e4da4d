// record_out_plan.cpp -- the checks, the window cut, the cover bitmaps and the field table of the record export (record_out_plan.hpp).
// Everything the caller controls is judged here. Nothing here knows a device.
#include "record_out_plan.hpp"
#include <algorithm>

namespace acvm {

int record_out_plan(const uint32_t *live, const acvm_record_out_desc_t *d, bool list, const void *records, RecordOutPlan *out, std::string *err) {
    auto refuse = [&](const std::string &text) { *err = text; return ACVM_E_INVALID; };
    if (!d) return refuse("null argument");
    if (d->n_fields && !d->fields) return refuse("null fields");
    if (!live) return refuse("null batch");
    const uint32_t n_fields = d->n_fields;
    const uint64_t pitch = d->pitch;
    // a covered range [begin, end) of the record: the element of field f, or its mask byte
    struct Range { uint64_t begin, end; uint32_t field; bool mask; uint32_t window; };
    std::vector<Range> ranges;
    ranges.reserve((size_t)n_fields * 2);
    for (uint32_t f = 0; f < n_fields; f++) {
        const acvm_record_out_field_t &fd = d->fields[f];
        auto who = [&] { return "field " + std::to_string(f) + " (witness " + std::to_string(fd.witness) + "): "; };  // (a refusal's text only)
        if (fd.encoding > ACVM_ENC_MONT256_LE && !(fd.encoding >= ACVM_ENC_U8 && fd.encoding <= ACVM_ENC_U128)) return refuse(who() + "unknown encoding " + std::to_string(fd.encoding));
        const uint64_t size = buffer_element_size(fd.encoding);
        // (offset + size may wrap 2^64: judged by differences)
        if (fd.offset > pitch || size > pitch - fd.offset)
            return refuse(who() + "offset " + std::to_string(fd.offset) + " + size " + std::to_string(size) + " is beyond the pitch " + std::to_string(pitch));
        ranges.push_back(Range{fd.offset, fd.offset + size, f, false, 0});
        if (fd.mask_offset != ACVM_RECORD_NO_MASK) {
            if (fd.mask_offset >= pitch) return refuse(who() + "mask offset " + std::to_string(fd.mask_offset) + " is beyond the pitch " + std::to_string(pitch));
            ranges.push_back(Range{fd.mask_offset, fd.mask_offset + 1, f, true, 0});
        }
    }
    // a store has one owner per byte: no two covered ranges may share one (every end is at most the pitch: nothing wraps)
    std::stable_sort(ranges.begin(), ranges.end(), [](const Range &a, const Range &b) { return a.begin < b.begin; });
    for (size_t r = 1; r < ranges.size(); r++)
        if (ranges[r].begin < ranges[r - 1].end) {
            const Range &a = ranges[r - 1], &b = ranges[r];
            auto what = [&](const Range &x) { return std::string(x.mask ? "the mask byte" : "the element") + " of field " + std::to_string(x.field) + " (witness " + std::to_string(d->fields[x.field].witness) + ")"; };
            return refuse(what(b) + " at offset " + std::to_string(b.begin) + " overlaps " + what(a) + " at [" + std::to_string(a.begin) + ", " + std::to_string(a.end) + ")");
        }
    if (list && d->first != 0) return refuse("first must be 0 for a list export: the list holds absolute instance numbers");
    if (!list && (d->first > *live || d->n > *live - d->first))
        return refuse("instances [" + std::to_string(d->first) + ", " + std::to_string((uint64_t)d->first + d->n) + ") are beyond the " + std::to_string(*live) + " live instances");
    if (n_fields && d->n && !records) return refuse("null records");
    // (the byte offset of the last record fits 63 bits)
    if (n_fields && (unsigned __int128)d->n * pitch > ((unsigned __int128)1 << 57)) return refuse("pitch " + std::to_string(pitch) + " is beyond any device buffer");

    // ---- every check has passed: the windows over the covered ranges (ascending and disjoint already)
    struct Cut { uint64_t offset; uint32_t length; std::vector<uint32_t> entries; uint32_t bitmap[RECORD_OUT_BITMAP_WORDS]; };
    std::vector<Cut> cuts;
    for (Range &r : ranges) {
        if (cuts.empty()) cuts.push_back(Cut{pitch <= RECORD_PLAN_WINDOW_CAP ? 0 : r.begin, pitch <= RECORD_PLAN_WINDOW_CAP ? (uint32_t)pitch : 0u, {}, {}});
        else if (pitch > RECORD_PLAN_WINDOW_CAP && r.end - cuts.back().offset > RECORD_PLAN_WINDOW_CAP) cuts.push_back(Cut{r.begin, 0, {}, {}});
        Cut &c = cuts.back();
        c.length = std::max<uint32_t>(c.length, (uint32_t)(r.end - c.offset));
        r.window = (uint32_t)cuts.size() - 1u;
        for (uint64_t at = r.begin - c.offset; at < r.end - c.offset; at++) c.bitmap[at >> 5] |= 1u << (at & 31u);
    }
    // the entries: a record that is one window keeps the caller's order, a cut one takes the ranges' order; element and mask byte of a field
    // that share a window are one entry, at the place of whichever comes first
    std::vector<const Range *> value_of(n_fields, nullptr), mask_of(n_fields, nullptr);
    for (const Range &r : ranges) (r.mask ? mask_of : value_of)[r.field] = &r;
    uint32_t n_entries = 0;
    auto emit = [&](uint32_t f, const Range *value, const Range *mask) {
        Cut &c = cuts[(value ? value : mask)->window];
        const acvm_record_out_field_t &fd = d->fields[f];
        const uint32_t kind = (value ? RECORD_OUT_KIND_VALUE : 0u) | (mask ? RECORD_OUT_KIND_MASK : 0u);
        c.entries.insert(c.entries.end(), {fd.witness, fd.encoding, value ? (uint32_t)(value->begin - c.offset) : 0u, kind | (mask ? (uint32_t)(mask->begin - c.offset) << 8 : 0u)});
        n_entries++;
    };
    auto emit_field = [&](uint32_t f, const Range *at) {  // at: the range the walk stands on (null: both)
        const Range *value = value_of[f], *mask = mask_of[f];
        if (mask && mask->window == value->window) {
            if (!at || at == std::min(value, mask)) emit(f, value, mask);  // (ranges is sorted: the lower address is the earlier range)
        } else {
            if (!at || at == value) emit(f, value, nullptr);
            if (mask && (!at || at == mask)) emit(f, nullptr, mask);
        }
    };
    if (pitch <= RECORD_PLAN_WINDOW_CAP)
        for (uint32_t f = 0; f < n_fields; f++) emit_field(f, nullptr);
    else
        for (const Range &r : ranges) emit_field(r.field, &r);

    RecordOutPlan plan;
    plan.pitch = pitch;
    plan.first = d->first;
    plan.n = d->n;
    plan.n_windows = (uint32_t)cuts.size();
    plan.n_entries = n_entries;
    for (uint32_t f = 0; f < n_fields; f++) {
        (d->fields[f].encoding == ACVM_ENC_MONT256_LE ? plan.mont256 : plan.plain) = true;
        plan.witnesses.push_back(d->fields[f].witness);
    }
    std::sort(plan.witnesses.begin(), plan.witnesses.end());
    plan.witnesses.erase(std::unique(plan.witnesses.begin(), plan.witnesses.end()), plan.witnesses.end());
    plan.tables.reserve(cuts.size() * RECORD_OUT_WINDOW_WORDS + (size_t)n_entries * RECORD_OUT_FIELD_WORDS);
    uint32_t first_entry = 0;
    for (const Cut &c : cuts) {
        const uint32_t n = (uint32_t)(c.entries.size() / RECORD_OUT_FIELD_WORDS);
        plan.tables.insert(plan.tables.end(), {(uint32_t)c.offset, (uint32_t)(c.offset >> 32), c.length, first_entry, n});
        plan.tables.insert(plan.tables.end(), c.bitmap, c.bitmap + RECORD_OUT_BITMAP_WORDS);
        first_entry += n;
    }
    for (const Cut &c : cuts) plan.tables.insert(plan.tables.end(), c.entries.begin(), c.entries.end());
    *out = std::move(plan);
    return 0;
}

}  // namespace acvm
