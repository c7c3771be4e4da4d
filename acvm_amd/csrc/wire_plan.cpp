// wire_plan.cpp -- see wire_plan.hpp. Pure host code: no HIP call, no handle.
#include "wire_plan.hpp"
#include "assigned_view.hpp"

#include <algorithm>
#include <stdexcept>

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
// ---- ACVM_WIRE_GZIP_DEFLATE
static const uint32_t LENGTH_BASE[21] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67};  // symbols 257 .. 277
static const uint32_t LENGTH_EXTRA[21] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4};
static const uint32_t CLEN_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
static constexpr uint32_t N_LITLEN = 278, N_DIST = 13, HCLEN = 14;

static uint32_t reverse_bits(uint32_t code, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < n; k++) r |= ((code >> k) & 1u) << (n - 1 - k);
    return r;
}
// RFC 1951 3.2.2; throws unless the Kraft sum is exactly 1
static std::vector<uint32_t> canonical(const std::vector<uint8_t> &lengths, const char *what) {
    uint32_t count[16] = {}, next[16] = {};
    uint64_t kraft = 0;
    for (uint8_t n : lengths)
        if (n) { count[n]++; kraft += 1u << (15 - n); }
    if (kraft != 1u << 15) throw std::logic_error(std::string("the ") + what + " code is not complete");
    uint32_t code = 0;
    for (uint32_t bits = 1; bits < 16; bits++) {
        code = (code + count[bits - 1]) << 1;
        next[bits] = code;
    }
    std::vector<uint32_t> out(lengths.size(), 0u);
    for (size_t s = 0; s < lengths.size(); s++)
        if (lengths[s]) out[s] = next[lengths[s]]++;
    return out;
}
namespace {
struct BitString {
    std::vector<uint32_t> words;
    uint32_t n = 0;
    void put(uint32_t value, uint32_t bits) {  // bits <= 32
        for (uint32_t k = 0; k < bits; k++, n++) {
            if (n / 32 == words.size()) words.push_back(0u);
            words[n / 32] |= ((value >> k) & 1u) << (n % 32);
        }
    }
};
}  // namespace

WireDeflateCode wire_deflate_code() {
    WireDeflateCode c;
    // the literal/length code: the 16 hex characters 5 bits, the length symbols 7, the other 241 in ascending order 9 (the first 103) or 10
    c.lengths.assign(N_LITLEN, 0);
    uint32_t others = 0;
    for (uint32_t s = 0; s <= 256; s++) {
        const bool hex = (s >= '0' && s <= '9') || (s >= 'a' && s <= 'f');
        c.lengths[s] = hex ? 5 : others++ < 103 ? 9 : 10;
    }
    for (uint32_t s = 257; s < N_LITLEN; s++) c.lengths[s] = 7;
    const std::vector<uint32_t> code = canonical(c.lengths, "literal/length");
    c.lit.resize(257);
    for (uint32_t s = 0; s <= 256; s++) c.lit[s] = reverse_bits(code[s], c.lengths[s]) | (uint32_t)c.lengths[s] << 16;
    c.match.assign(WIRE_PLAN_ENTRY_BYTES + 1, 0u);
    for (uint32_t n = 3; n <= WIRE_PLAN_ENTRY_BYTES; n++) {
        uint32_t k = 20;
        while (LENGTH_BASE[k] > n) k--;
        c.match[n] = reverse_bits(code[257 + k], 7) | (n - LENGTH_BASE[k]) << 7 | (7 + LENGTH_EXTRA[k]) << 16;
    }
    // the header. One sequence of 291 lengths in runs: zeros by 18 (11 .. 138) then 17 (3 .. 10), a length v by itself and then 16 (3 .. 6), the
    // longest repeat first; the code-length code is stated, not derived: 16 -> 1 bit, 9 -> 2, 7 -> 3, 1 5 10 18 -> 5.
    std::vector<uint8_t> seq(c.lengths);
    seq.resize(N_LITLEN + N_DIST, 0);
    seq[N_LITLEN + 0] = seq[N_LITLEN + 12] = 1;  // distance 1; distances 65 .. 96
    std::vector<uint8_t> clen(19, 0);
    clen[16] = 1, clen[9] = 2, clen[7] = 3, clen[1] = clen[5] = clen[10] = clen[18] = 5;
    const std::vector<uint32_t> clen_code = canonical(clen, "code-length");
    BitString b;
    b.put(1, 1);  // BFINAL
    b.put(2, 2);  // BTYPE = 10
    b.put(N_LITLEN - 257, 5);
    b.put(N_DIST - 1, 5);
    b.put(HCLEN, 4);
    for (uint32_t k = 0; k < HCLEN + 4; k++) b.put(clen[CLEN_ORDER[k]], 3);
    auto symbol = [&](uint32_t s, uint32_t extra_bits, uint32_t extra) {
        if (!clen[s]) throw std::logic_error("the code-length code lacks symbol " + std::to_string(s));
        b.put(reverse_bits(clen_code[s], clen[s]), clen[s]);
        b.put(extra, extra_bits);
    };
    for (size_t i = 0; i < seq.size();) {
        const uint8_t v = seq[i];
        size_t n = 1;
        while (i + n < seq.size() && seq[i + n] == v) n++;
        i += n;
        if (!v) {
            for (; n >= 11; n -= std::min<size_t>(n, 138)) symbol(18, 7, (uint32_t)std::min<size_t>(n, 138) - 11);
            for (; n >= 3; n -= std::min<size_t>(n, 10)) symbol(17, 3, (uint32_t)std::min<size_t>(n, 10) - 3);
            for (; n; n--) symbol(0, 0, 0);
        } else {
            symbol(v, 0, 0);
            for (n--; n >= 3; n -= std::min<size_t>(n, 6)) symbol(16, 2, (uint32_t)std::min<size_t>(n, 6) - 3);
            for (; n; n--) symbol(v, 0, 0);
        }
    }
    c.header = b.words;
    c.header_bits = b.n;
    return c;
}

uint32_t wire_deflate_match_bits(const WireDeflateCode &c, uint32_t length, uint32_t distance) { return (c.match[length] >> 16) + (distance == 1 ? 1u : 6u); }

std::vector<uint32_t> wire_deflate_device_table(const WireDeflateCode &c, uint32_t *prefix_bits) {
    std::vector<uint32_t> t(WIRE_PLAN_DEFLATE_WORDS, 0u);
    std::copy(c.lit.begin(), c.lit.end(), t.begin() + WIRE_PLAN_DEFLATE_LIT);
    std::copy(c.match.begin(), c.match.end(), t.begin() + WIRE_PLAN_DEFLATE_MATCH);
    BitString b;
    const uint8_t head[11] = {0x1f, 0x8b, 0x08, 0x08, 0, 0, 0, 0, 0, 0xff, 0};
    for (uint8_t x : head) b.put(x, 8);
    for (uint32_t k = 0; k < c.header_bits; k += 32) b.put(c.header[k / 32], std::min(32u, c.header_bits - k));
    if (b.words.size() > WIRE_PLAN_DEFLATE_PREFIX_WORDS) throw std::logic_error("the deflate prefix outgrew its table");
    std::copy(b.words.begin(), b.words.end(), t.begin() + WIRE_PLAN_DEFLATE_PREFIX);
    *prefix_bits = b.n;
    return t;
}

// the code and the device's table are constants: made once
namespace {
struct DeflateConstants {
    WireDeflateCode code;
    std::vector<uint32_t> table;
    uint32_t prefix_bits = 0;
    DeflateConstants() : code(wire_deflate_code()) { table = wire_deflate_device_table(code, &prefix_bits); }
};
const DeflateConstants &deflate_constants() {
    static const DeflateConstants c;
    return c;
}
}  // namespace
static uint64_t deflate_bound(uint64_t n_positions) {
    const uint32_t header_bits = deflate_constants().code.header_bits;
    // the block at its dearest: the header, 8 count literals of 10 bits, per entry 12 header literals of 10 and 64 characters of 5, end-of-block.
    // No match costs more than the literals it replaces (tools/wire_deflate_plan_host_test.cpp checks every length with both distances).
    const uint64_t bits = header_bits + 8u * 10u + n_positions * (12u * 10u + 64u * 5u) + 10u;
    return (11 + (bits + 7) / 8 + 8 + 15) / 16 * 16;
}
uint64_t wire_plan_bound(uint32_t container, uint64_t n_positions) {
    if (container == ACVM_WIRE_GZIP_DEFLATE) return deflate_bound(n_positions);
    return (wire_plan_length(container, n_positions) + 15) / 16 * 16;
}

int wire_plan(const uint32_t *live, const uint32_t *producer, uint32_t n_witnesses, const acvm_wire_desc_t *d, bool list, const void *bytes, bool device,
              WirePlan *out, std::string *err) {
    auto refuse = [&](const std::string &text) { *err = text; return ACVM_E_INVALID; };
    if (!d) return refuse("null argument");
    if (!live) return refuse("null batch");
    if (d->container != ACVM_WIRE_BINCODE && d->container != ACVM_WIRE_GZIP_STORED && d->container != ACVM_WIRE_GZIP_DEFLATE) return refuse("unknown container " + std::to_string(d->container));
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
    if (d->container != ACVM_WIRE_BINCODE) p.crc_pow = wire_plan_crc_powers(n_positions, &p.crc_x64);
    if (d->container == ACVM_WIRE_GZIP_DEFLATE) {
        p.deflate = deflate_constants().table;
        p.deflate_prefix_bits = deflate_constants().prefix_bits;
    }
    *out = std::move(p);
    return 0;
}

}  // namespace acvm
