// wire_inflate_plan.cpp -- see wire_inflate_plan.hpp. Pure host code: no HIP call, no handle.
#include "wire_inflate_plan.hpp"

namespace acvm {

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

std::vector<uint16_t> wire_inflate_fixed_tables() {
    std::vector<uint16_t> t(INFLATE_PLAN_TAB_HALFWORDS, 0);
    // canonical order: by length, then by symbol -- 7 bits: 256 .. 279; 8 bits: 0 .. 143, 280 .. 287; 9 bits: 144 .. 255
    t[INFLATE_PLAN_LCNT + 7] = 24;
    t[INFLATE_PLAN_LCNT + 8] = 152;
    t[INFLATE_PLAN_LCNT + 9] = 112;
    uint32_t at = INFLATE_PLAN_LSYM;
    for (uint32_t s = 256; s < 280; s++) t[at++] = (uint16_t)s;
    for (uint32_t s = 0; s < 144; s++) t[at++] = (uint16_t)s;
    for (uint32_t s = 280; s < 288; s++) t[at++] = (uint16_t)s;
    for (uint32_t s = 144; s < 256; s++) t[at++] = (uint16_t)s;
    // all 32 codes of 5 bits are codes; 30 and 31 are symbols the reader refuses
    t[INFLATE_PLAN_DCNT + 5] = 32;
    for (uint32_t s = 0; s < 32; s++) t[INFLATE_PLAN_DSYM + s] = (uint16_t)s;
    return t;
}

int wire_inflate_plan(const uint32_t *live, const uint32_t *initial_ids, uint32_t n_initial, const acvm_wire_in_desc_t *d, const void *bytes, bool device,
                      uint64_t host_row_bytes, WireInflatePlan *out, std::string *err) {
    auto refuse = [&](const std::string &text) { *err = text; return ACVM_E_INVALID; };
    if (!live) return refuse("null batch");
    if (!d) return refuse("null argument");
    if (d->container != ACVM_WIRE_GZIP_DEFLATE) return refuse("container " + std::to_string(d->container) + " is not ACVM_WIRE_GZIP_DEFLATE");
    if (device && !d->pitch) return refuse("pitch 0 is not a multiple of 16 above 0");
    if (device && d->pitch % 16) return refuse("pitch " + std::to_string(d->pitch) + " is not a multiple of 16");
    if ((unsigned __int128)*live * d->pitch > ((unsigned __int128)1 << 57)) return refuse("pitch " + std::to_string(d->pitch) + " is beyond any device buffer");
    if (*live && !bytes) return refuse("null buffer");
    if (device && ((uintptr_t)bytes & 15u)) return refuse("the buffer is not aligned to 16 bytes");
    if (*live > (1u << 27)) return refuse("more instances than a finding can name");
    WireInflatePlan p;
    p.out_pitch = wire_in_stage_pitch(n_initial);
    p.out_cap = 8 + (uint64_t)WIRE_PLAN_ENTRY_BYTES * n_initial;
    p.pitch = device ? d->pitch : (host_row_bytes + 15) / 16 * 16;
    if (!p.pitch) p.pitch = 16;
    const acvm_wire_in_desc_t body{ACVM_WIRE_BINCODE, p.out_pitch};
    alignas(16) static const uint8_t aligned_somewhere[16] = {0};  // (stage 2 reads the arena, which is aligned: this stands in for it in the check)
    if (int rc = wire_in_plan(live, initial_ids, n_initial, &body, aligned_somewhere, true, &p.body, err)) return rc;
    p.fixed = wire_inflate_fixed_tables();
    const size_t B = *live;
    size_t at = 0;
    auto carve = [&](size_t n_bytes) { const size_t begin = at; at += up256(n_bytes); return begin; };
    p.at_scratch = carve(B * (size_t)p.out_pitch);
    p.at_lengths = carve(B * 8);
    p.at_findings = carve(B * 8);
    p.at_tables = carve(B * (size_t)INFLATE_PLAN_ROW_WORDS * 4);
    p.at_fixed = carve(p.fixed.size() * 2);
    p.at_result = carve(16);
    p.at_rows = carve(device ? 0 : B * (size_t)p.pitch);
    p.at_row_lengths = carve(device ? 0 : B * 8);
    p.front = at;
    *out = std::move(p);
    return 0;
}

}  // namespace acvm
