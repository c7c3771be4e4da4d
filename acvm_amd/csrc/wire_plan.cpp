// wire_plan.cpp -- see wire_plan.hpp. Pure host code: no HIP call, no handle.
#include "wire_plan.hpp"
#include "assigned_view.hpp"

namespace acvm {

static constexpr uint32_t CRC_POLY = 0xEDB88320u;
static uint32_t crc_mul(uint32_t a, uint32_t b) {  // a * b mod P, bit 31 = x^0 (zlib's multmodp)
    uint32_t p = 0;
    for (int k = 31; k >= 0; k--) {
        if ((a >> k) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return p;
}
static uint32_t crc_xpow_bytes(uint64_t bytes) {  // x^(8 bytes) mod P
    uint32_t r = 0x80000000u, sq = 0x00800000u;
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
    }
    return r;
}

std::vector<uint32_t> wire_plan_crc_powers(uint32_t n_positions, uint32_t *x64) {
    std::vector<uint32_t> pow((size_t)n_positions + 1);
    const uint32_t step = crc_xpow_bytes(WIRE_PLAN_ENTRY_BYTES);
    pow[0] = 0x80000000u;
    for (uint32_t k = 1; k <= n_positions; k++) pow[k] = crc_mul(pow[k - 1], step);
    *x64 = crc_xpow_bytes(8);
    return pow;
}

uint64_t wire_plan_body_offset(uint32_t container, uint64_t k) { return container == ACVM_WIRE_GZIP_STORED ? 16 + k + 20 * (k / WIRE_PLAN_BLOCK_BYTES) : k; }
uint64_t wire_plan_length(uint32_t container, uint64_t n_entries) {
    const uint64_t L = 8 + (uint64_t)WIRE_PLAN_ENTRY_BYTES * n_entries;
    return container == ACVM_WIRE_GZIP_STORED ? 16 + L + 20 * ((L + WIRE_PLAN_BLOCK_BYTES - 1) / WIRE_PLAN_BLOCK_BYTES - 1) + 8 : L;
}
uint64_t wire_plan_bound(uint32_t container, uint64_t n_positions) { return (wire_plan_length(container, n_positions) + 15) / 16 * 16; }

int wire_plan(const uint32_t *live, const uint32_t *producer, uint32_t n_witnesses, const acvm_wire_desc_t *d, bool list, const void *bytes, bool device,
              WirePlan *out, std::string *err) {
    auto refuse = [&](const std::string &text) { *err = text; return ACVM_E_INVALID; };
    if (!d) return refuse("null argument");
    if (!live) return refuse("null batch");
    if (d->container != ACVM_WIRE_BINCODE && d->container != ACVM_WIRE_GZIP_STORED) return refuse("unknown container " + std::to_string(d->container));
    const bool whole = d->witnesses == nullptr;
    if (!whole)
        for (uint32_t k = 1; k < d->n_witnesses; k++)
            if (d->witnesses[k] <= d->witnesses[k - 1])
                return refuse("the witness list is not strictly ascending: entry " + std::to_string(k) + " (witness " + std::to_string(d->witnesses[k]) + ") follows witness " +
                              std::to_string(d->witnesses[k - 1]));
    if (list && d->first != 0) return refuse("first must be 0 for a list export: the list holds absolute instance numbers");
    if (!list && (uint64_t)d->first + d->n > *live)
        return refuse("instances [" + std::to_string(d->first) + ", " + std::to_string((uint64_t)d->first + d->n) + ") are beyond the " + std::to_string(*live) + " live instances");
    const uint32_t n_positions = whole ? n_witnesses : d->n_witnesses;
    const uint64_t bound = wire_plan_bound(d->container, n_positions), pitch = d->pitch ? d->pitch : bound;
    if (pitch < bound) return refuse("pitch " + std::to_string(pitch) + " is below the bound " + std::to_string(bound) + " (acvm_batch_wire_bound)");
    if (pitch % 16) return refuse("pitch " + std::to_string(pitch) + " is not a multiple of 16");
    if ((unsigned __int128)d->n * pitch > ((unsigned __int128)1 << 57)) return refuse("pitch " + std::to_string(pitch) + " is beyond any device buffer");
    if (d->n && !bytes) return refuse("null buffer");
    if (device && ((uintptr_t)bytes & 15u)) return refuse("the buffer is not aligned to 16 bytes");

    WirePlan p;
    p.container = d->container;
    p.first = d->first;
    p.n = d->n;
    p.pitch = pitch;
    p.bound = bound;
    p.whole = whole;
    p.n_positions = n_positions;
    p.n_windows = (n_positions + WIRE_PLAN_WINDOW - 1) / WIRE_PLAN_WINDOW;
    if (!whole) p.witnesses.assign(d->witnesses, d->witnesses + d->n_witnesses);
    const AssignedView generic(producer, n_witnesses, nullptr, 0, (const uint32_t *)nullptr);
    p.rank.resize((size_t)n_positions + 1);
    p.list_mask.assign(((size_t)n_witnesses + 31) / 32, 0u);
    for (uint32_t k = 0; k < n_positions; k++) {
        const uint32_t w = whole ? k : d->witnesses[k];
        p.rank[k] = (uint32_t)p.entries.size();
        if (generic.produced(w)) p.entries.push_back(w);
        if (w < n_witnesses) p.list_mask[w >> 5] |= 1u << (w & 31);
    }
    p.rank[n_positions] = (uint32_t)p.entries.size();
    if (d->container == ACVM_WIRE_GZIP_STORED) p.crc_pow = wire_plan_crc_powers(n_positions, &p.crc_x64);
    *out = std::move(p);
    return 0;
}

}  // namespace acvm
