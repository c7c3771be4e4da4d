// wire_in_plan.cpp -- see wire_in_plan.hpp. Pure host code: no HIP call, no handle.
#include "wire_in_plan.hpp"

#include <algorithm>
#include <map>
#include <numeric>

namespace acvm {

static uint32_t bits_of(uint64_t v) {  // the bits that hold every value below v
    uint32_t n = 0;
    for (v = v ? v - 1 : 0; v; v >>= 1) n++;
    return n;
}

uint64_t wire_in_stage_pitch(uint32_t n_initial) { return wire_plan_bound(ACVM_WIRE_BINCODE, n_initial); }

int wire_in_plan(const uint32_t *live, const uint32_t *initial_ids, uint32_t n_initial, const acvm_wire_in_desc_t *d, const void *bytes, bool device, WireInPlan *out,
                 std::string *err) {
    auto refuse = [&](const std::string &text) { *err = text; return ACVM_E_INVALID; };
    if (!live) return refuse("null batch");
    if (!d) return refuse("null argument");
    if (d->container != ACVM_WIRE_BINCODE && d->container != ACVM_WIRE_GZIP_STORED) return refuse("unknown container " + std::to_string(d->container));
    if (device && !d->pitch) return refuse("pitch 0 is not a multiple of 16 above 0");
    if (device && d->pitch % 16) return refuse("pitch " + std::to_string(d->pitch) + " is not a multiple of 16");
    if ((unsigned __int128)*live * d->pitch > ((unsigned __int128)1 << 57)) return refuse("pitch " + std::to_string(d->pitch) + " is beyond any device buffer");
    if (*live && !bytes) return refuse("null buffer");
    if (device && ((uintptr_t)bytes & 15u)) return refuse("the buffer is not aligned to 16 bytes");
    WireInPlan p;
    p.container = d->container;
    p.pitch = d->pitch;
    p.n_initial = n_initial;
    p.n_windows = (n_initial + WIRE_PLAN_WINDOW - 1) / WIRE_PLAN_WINDOW;
    p.rank_bits = bits_of(n_initial);
    if (bits_of(*live) + 3 + p.rank_bits > 63) return refuse("instances and initial witnesses are beyond what a finding can name");
    p.positions.resize(n_initial);
    std::iota(p.positions.begin(), p.positions.end(), 0u);
    std::stable_sort(p.positions.begin(), p.positions.end(), [&](uint32_t x, uint32_t y) { return initial_ids[x] < initial_ids[y]; });
    p.keys.resize(n_initial);
    for (uint32_t k = 0; k < n_initial; k++) p.keys[k] = initial_ids[p.positions[k]];
    if (d->container == ACVM_WIRE_GZIP_STORED) p.crc_pow = wire_plan_crc_powers(n_initial, &p.crc_x64);
    *out = std::move(p);
    return 0;
}

static uint64_t le(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int k = n - 1; k >= 0; k--) v = v << 8 | p[k];
    return v;
}
static bool hex_digit(uint8_t c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'); }

bool wire_in_body_canonical(const WireInPlan &plan, const uint8_t *body, size_t len) {
    if (len < 8) return false;
    const uint64_t n = le(body, 8);
    if (n > plan.n_initial || len != 8 + (size_t)WIRE_PLAN_ENTRY_BYTES * n) return false;
    uint64_t previous = 0;
    for (uint64_t r = 0; r < n; r++) {
        const uint8_t *e = body + 8 + (size_t)WIRE_PLAN_ENTRY_BYTES * r;
        const uint32_t key = (uint32_t)le(e, 4);
        if (le(e + 4, 8) != 64) return false;
        for (int k = 0; k < 64; k++)
            if (!hex_digit(e[12 + k])) return false;
        if (r && key <= previous) return false;
        if (!std::binary_search(plan.keys.begin(), plan.keys.end(), key)) return false;
        previous = key;
    }
    return true;
}

int wire_in_body_of_map(const WireInPlan &plan, const uint32_t *ids, const uint8_t *values_be32, size_t n, std::vector<uint8_t> *body, std::string *err) {
    std::map<uint32_t, const uint8_t *> m;  // BTreeMap: ascending, a repeated key keeps its last value
    for (size_t i = 0; i < n; i++) {
        if (!std::binary_search(plan.keys.begin(), plan.keys.end(), ids[i])) {
            *err = "witness " + std::to_string(ids[i]) + " is not an initial witness of this handle";
            return ACVM_E_INVALID;
        }
        m[ids[i]] = values_be32 + 32 * i;
    }
    std::vector<uint8_t> out;
    out.reserve(8 + (size_t)WIRE_PLAN_ENTRY_BYTES * m.size());
    auto put = [&](uint64_t v, int bytes) { for (int k = 0; k < bytes; k++) out.push_back((uint8_t)(v >> (8 * k))); };
    put(m.size(), 8);
    static const char *hex = "0123456789abcdef";
    for (const auto &kv : m) {
        put(kv.first, 4);
        put(64, 8);
        for (int k = 0; k < 32; k++) { out.push_back((uint8_t)hex[kv.second[k] >> 4]); out.push_back((uint8_t)hex[kv.second[k] & 15]); }
    }
    *body = std::move(out);
    return 0;
}

}  // namespace acvm
