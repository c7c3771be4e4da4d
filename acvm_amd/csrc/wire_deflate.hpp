// wire_deflate.hpp -- the deflating container of the batch-wide WitnessMap wire format (include/acvm_amd.h ACVM_WIRE_GZIP_DEFLATE,
// kernels_wire_deflate.hip): the parse of one 76-byte entry given its predecessor, its cost in bits, and the emission of its tokens at a bit
// offset. Everything here is __host__ __device__ and makes no HIP runtime call, so that the host runs what the kernel runs
// (tools/wire_deflate_host_test.hip, tests/test_wire_deflate_on_host.py). The code tables are wire_plan.cpp's (wire_deflate_device_table).
//
// The parse. A token never spans two entries. From p = 0: L76 = the run of positions from p on where the entry equals its predecessor (0 at
// rank 0), L1 = the run where a byte equals the byte before it in the entry (0 at p = 0). If max(L76, L1) >= 3, a match of that length with
// distance 76 if L76 >= L1, else distance 1; otherwise the literal. Both runs are read off two 76-bit equality masks made once per entry.
#pragma once
#include "wire_encode.hpp"

namespace acvm {

constexpr uint32_t WIRE_GZIP_DEFLATE = 8;  // (ACVM_WIRE_GZIP_DEFLATE)
// the table's layout (wire_plan.hpp WIRE_PLAN_DEFLATE_*; kernels_wire_deflate.hip asserts that the two agree)
constexpr uint32_t WIRE_DEFLATE_LIT = 0, WIRE_DEFLATE_EOB = 256, WIRE_DEFLATE_MATCH = 257, WIRE_DEFLATE_PREFIX = 334, WIRE_DEFLATE_PREFIX_WORDS = 12, WIRE_DEFLATE_WORDS = 346;
constexpr uint32_t WIRE_DEFLATE_MIN_MATCH = 3, WIRE_DEFLATE_GZIP_HEAD_BYTES = 11;
// distance 1: the bit 0. Distance 76: the bit 1, then 76 - 65 = 11 in five extra bits.
constexpr uint32_t WIRE_DEFLATE_DIST1_BITS = 1, WIRE_DEFLATE_DIST76 = 1u | 11u << 1, WIRE_DEFLATE_DIST76_BITS = 6;
// an entry at its dearest: 12 header literals of 10 bits, 64 characters of 5
constexpr uint32_t WIRE_DEFLATE_ENTRY_MAX_BITS = 12 * 10 + 64 * 5;

// bit q of {lo, hi} is position q of the entry (q < 76; the bits above are 0)
struct WireMask {
    uint64_t lo, hi;
};
struct WireDeflateMasks {
    WireMask far, near;  // cur[q] == prev[q]; cur[q] == cur[q - 1] (bit 0 is 0)
};
// the four bits "byte b of x is zero"
FR_HD __forceinline__ uint32_t wire_zero_bytes(uint32_t x) {
    const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}
// cur, prev: the entry and its predecessor as 19 dwords in memory order; prev may be null: rank 0
template <typename Words, typename Prev>
FR_HD __forceinline__ WireDeflateMasks wire_deflate_masks(const Words &cur, const Prev &prev, bool has_prev) {
    WireDeflateMasks m{{0u, 0u}, {0u, 0u}};
    uint32_t before = 0u;
#pragma unroll
    for (uint32_t x = 0; x < WIRE_ENTRY_WORDS; x++) {
        const uint32_t c = cur[x];
        const uint64_t far = has_prev ? wire_zero_bytes(c ^ prev[x]) : 0u;
        uint64_t near = wire_zero_bytes(c ^ ((c << 8) | (before >> 24)));
        if (x == 0) near &= ~(uint64_t)1;
        before = c;
        if (x < 16) {
            m.far.lo |= far << (4u * x);
            m.near.lo |= near << (4u * x);
        } else {
            m.far.hi |= far << (4u * (x - 16u));
            m.near.hi |= near << (4u * (x - 16u));
        }
    }
    return m;
}
// the run of set bits of m from position p (< 76) on
FR_HD __forceinline__ uint32_t wire_mask_run(const WireMask &m, uint32_t p) {
    uint64_t lo, hi;
    if (p >= 64u) {
        lo = m.hi >> (p - 64u);
        hi = 0u;
    } else if (p) {
        lo = (m.lo >> p) | (m.hi << (64u - p));
        hi = m.hi >> p;
    } else {
        lo = m.lo;
        hi = m.hi;
    }
    if (~lo) return (uint32_t)__builtin_ctzll(~lo);
    return 64u + (uint32_t)__builtin_ctzll(~hi);  // (hi has at most 12 set bits)
}
// the token at p: length 0 = the literal, else a match of `length` at `distance`
struct WireToken {
    uint32_t length, distance;
};
FR_HD __forceinline__ WireToken wire_deflate_token(const WireDeflateMasks &m, uint32_t p) {
    const uint32_t l76 = wire_mask_run(m.far, p), l1 = wire_mask_run(m.near, p);
    const uint32_t best = l76 >= l1 ? l76 : l1;
    if (best < WIRE_DEFLATE_MIN_MATCH) return WireToken{0u, 0u};
    return WireToken{best, l76 >= l1 ? 76u : 1u};
}
template <typename Words>
FR_HD __forceinline__ uint32_t wire_entry_byte(const Words &cur, uint32_t p) {
    return (cur[p >> 2] >> (8u * (p & 3u))) & 0xffu;
}
// what a token puts into the stream: its bits (LSB first) and their count (<= 17)
template <typename Table>
FR_HD __forceinline__ void wire_deflate_token_bits(const WireToken &t, uint32_t byte, const Table &table, uint32_t &bits, uint32_t &n) {
    if (!t.length) {
        const uint32_t e = table[WIRE_DEFLATE_LIT + byte];
        bits = e & 0xffffu;
        n = e >> 16;
        return;
    }
    const uint32_t e = table[WIRE_DEFLATE_MATCH + t.length];
    const uint32_t n_length = e >> 16;
    bits = (e & 0xffffu) | (t.distance == 1u ? 0u : WIRE_DEFLATE_DIST76 << n_length);
    n = n_length + (t.distance == 1u ? WIRE_DEFLATE_DIST1_BITS : WIRE_DEFLATE_DIST76_BITS);
}
// the parse into tokens (at most 76); returns their number
template <typename Words, typename Prev>
FR_HD inline uint32_t wire_deflate_parse(const Words &cur, const Prev &prev, bool has_prev, WireToken *tokens) {
    const WireDeflateMasks m = wire_deflate_masks(cur, prev, has_prev);
    uint32_t n = 0;
    for (uint32_t p = 0; p < WIRE_ENTRY_BYTES;) {
        const WireToken t = wire_deflate_token(m, p);
        tokens[n++] = t;
        p += t.length ? t.length : 1u;
    }
    return n;
}
// the bits of an entry
template <typename Words, typename Table>
FR_HD inline uint32_t wire_deflate_cost(const Words &cur, const WireDeflateMasks &m, const Table &table) {
    uint32_t cost = 0;
    for (uint32_t p = 0; p < WIRE_ENTRY_BYTES;) {
        const WireToken t = wire_deflate_token(m, p);
        uint32_t bits, n;
        wire_deflate_token_bits(t, t.length ? 0u : wire_entry_byte(cur, p), table, bits, n);
        cost += n;
        p += t.length ? t.length : 1u;
    }
    return cost;
}

// A bit writer over a zeroed word buffer shared with neighbours: bits gather in a 64-bit accumulator and leave as whole words. The writer's
// first word (its neighbour in front may own the low bits) and its last, partial one are OR-ed in by `shared`, the words between are this
// writer's alone and stored by `own`. Sink: void shared(uint32_t word_index, uint32_t bits), void own(uint32_t word_index, uint32_t bits).
template <typename Sink>
struct WireBitWriter {
    Sink sink;
    uint64_t acc;
    uint32_t n, word;  // the bits in acc, the word they start in
    bool first;
    FR_HD WireBitWriter(const Sink &s, uint64_t bit_offset) : sink(s), acc(0u), n((uint32_t)(bit_offset & 31u)), word((uint32_t)(bit_offset >> 5)), first(true) {}
    FR_HD __forceinline__ void put(uint32_t bits, uint32_t count) {  // count <= 32
        acc |= (uint64_t)bits << n;
        n += count;
        if (n >= 32u) {
            if (first) sink.shared(word, (uint32_t)acc);
            else sink.own(word, (uint32_t)acc);
            first = false;
            acc >>= 32;
            n -= 32u;
            word++;
        }
    }
    // the bit position behind the last bit
    FR_HD __forceinline__ uint64_t finish() {
        if (n && (uint32_t)acc) sink.shared(word, (uint32_t)acc);
        return (uint64_t)word * 32u + n;
    }
};
// the tokens of an entry at a bit offset; returns the bit position behind them
template <typename Words, typename Table, typename Sink>
FR_HD inline uint64_t wire_deflate_emit(const Words &cur, const WireDeflateMasks &m, const Table &table, const Sink &sink, uint64_t bit_offset) {
    WireBitWriter<Sink> w(sink, bit_offset);
    for (uint32_t p = 0; p < WIRE_ENTRY_BYTES;) {
        const WireToken t = wire_deflate_token(m, p);
        uint32_t bits, n;
        wire_deflate_token_bits(t, t.length ? 0u : wire_entry_byte(cur, p), table, bits, n);
        w.put(bits, n);
        p += t.length ? t.length : 1u;
    }
    return w.finish();
}

// the member's bytes at the most for n_positions list positions, rounded up to 16 (wire_plan.cpp wire_plan_bound)
FR_HD __forceinline__ uint64_t wire_deflate_bound(uint32_t header_bits, uint64_t n_positions) {
    const uint64_t bits = header_bits + 8u * 10u + n_positions * WIRE_DEFLATE_ENTRY_MAX_BITS + 10u;
    return (WIRE_DEFLATE_GZIP_HEAD_BYTES + (bits + 7u) / 8u + WIRE_TRAILER_BYTES + 15u) / 16u * 16u;
}

}  // namespace acvm
