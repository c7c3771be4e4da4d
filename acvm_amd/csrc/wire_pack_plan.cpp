// wire_pack_plan.cpp -- see wire_pack_plan.hpp. Pure host code: no HIP call, no handle.
#include "wire_pack_plan.hpp"

#include <algorithm>

namespace acvm {

uint32_t wire_chunk_rows(uint32_t n, uint64_t pitch) { return (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(64, WIRE_HOST_CHUNK_BYTES / pitch / 64 * 64)); }

int wire_pack_plan(const uint32_t *live, const uint32_t *producer, uint32_t n_witnesses, const acvm_wire_desc_t *d, bool list, const void *bytes, uint64_t capacity,
                   const void *offsets, bool device, WirePlan *out, std::string *err) {
    auto refuse = [&](const std::string &text) { *err = text; return ACVM_E_INVALID; };
    if (!d) return refuse("null argument");
    if (!live) return refuse("null batch");
    if (d->pitch) return refuse("pitch " + std::to_string(d->pitch) + ": a packed export has no pitch, the descriptor's must be 0");
    if (!offsets) return refuse("null offsets");
    if (!bytes && capacity) return refuse("null buffer with a capacity of " + std::to_string(capacity));
    if (device && ((uintptr_t)bytes & 15u)) return refuse("the buffer is not aligned to 16 bytes");
    // (wire_plan judges the buffer for null only: the sizing call has none, so it sees the offsets column, which is not null)
    return wire_plan(live, producer, n_witnesses, d, list, bytes ? bytes : offsets, false, out, err);
}

WirePackArena wire_pack_arena(uint64_t front, uint32_t chunk, uint64_t pitch, bool host) {
    auto align256 = [](uint64_t x) { return (x + 255u) & ~(uint64_t)255; };
    WirePackArena a;
    uint64_t at = align256(front);
    auto carve = [&](uint64_t n_bytes) { const uint64_t begin = at; at += align256(n_bytes); return begin; };
    a.at_state = carve(16);
    a.at_lengths = carve((uint64_t)chunk * 8);
    a.at_slots = carve((uint64_t)chunk * pitch);
    a.at_packed = carve(host ? (uint64_t)chunk * pitch : 0);
    a.at_offsets = carve(host ? ((uint64_t)chunk + 1) * 8 : 0);
    a.end = at;
    return a;
}

void wire_pack_fit(const uint64_t *offsets, uint32_t n, uint64_t capacity, uint32_t *n_fit, uint64_t *total) {
    uint32_t fit = 0;
    while (fit < n && offsets[fit + 1] <= capacity) fit++;
    *n_fit = fit;
    *total = offsets[n];
}

}  // namespace acvm
