// wire_decode.hpp -- the arithmetic of the batch-wide WitnessMap wire format READ on the device (include/acvm_amd.h
// acvm_batch_import_device_wire, kernels_wire_in.hip): the counterpart of wire_encode.hpp. Hex characters back to the bytes they spell, the
// judgement of a row's count word, the framing words a stored-block member must hold, an entry's share of the body's CRC-32 and the key that
// names a finding. Everything here is __host__ __device__ so that the host can run what the kernels run (tools/wire_decode_host_test.hip,
// tests/test_wire_decode_on_host.py).
#pragma once
#include "wire_encode.hpp"
#include "import_decode.hpp"

namespace acvm {

// ---- the findings of untrusted bytes, in the order a reader meets them (include/acvm_amd.h)
enum : uint32_t {
    WIRE_IN_COUNT = 1,    // the count word cannot be a map of this slot
    WIRE_IN_LENGTH = 2,   // an entry's length word is not 64
    WIRE_IN_HEX = 3,      // a character that is not a hex digit
    WIRE_IN_KEY = 4,      // a key that is not an initial witness of the handle
    WIRE_IN_ORDER = 5,    // keys not strictly ascending
    WIRE_IN_FRAMING = 6,  // GZIP_STORED: a head, joint, ISIZE or block-header word that is not the pinned one
    WIRE_IN_CRC = 7,      // GZIP_STORED: the trailer's CRC-32 is not the body's
    WIRE_IN_CLASSES = 8
};
constexpr uint32_t WIRE_IN_NO_MAP = 0xFFFFFFFFu;  // what a row with a WIRE_IN_COUNT finding has instead of an entry count

// ---- hex. Four characters, one per byte, to their four nibbles, one per byte; bad gets a bit for every byte that is no hex digit. Branch-free
// and the same for every lane: a byte with its top bit set is none; below 0x80 a digit is [0x30, 0x3a) and a letter, folded to lower case,
// [0x61, 0x67) -- both read from bit 7 of two sums that cannot carry into the next byte (0x7f + 0x50 < 0x100). A letter's low nibble is 1 .. 6.
FR_HD __forceinline__ uint32_t wire_unhex4(uint32_t chars, uint32_t &bad) {
    const uint32_t y = chars & 0x7f7f7f7fu;
    const uint32_t digit = (y + 0x50505050u) & ~(y + 0x46464646u);
    const uint32_t z = y | 0x20202020u;
    const uint32_t letter = (z + 0x1f1f1f1fu) & ~(z + 0x19191919u);
    bad |= ((digit | letter) & ~chars & 0x80808080u) ^ 0x80808080u;
    return (y & 0x0f0f0f0fu) + ((letter >> 7) & 0x01010101u) * 9u;
}
// Eight characters (lo = the first four in memory order) to the dword of the big-endian element they spell, its first byte the lowest: the
// inverse of wire_hex_dword.
FR_HD __forceinline__ uint32_t wire_unhex_dword(uint32_t lo, uint32_t hi, uint32_t &bad) {
    auto pack = [](uint32_t n) { return ((n & 0xfu) << 4) | ((n >> 8) & 0xfu) | (((n >> 16) & 0xfu) << 12) | (((n >> 24) & 0xfu) << 8); };
    return pack(wire_unhex4(lo, bad)) | (pack(wire_unhex4(hi, bad)) << 16);
}
// the 64 characters of an entry as 16 dwords to the lo / hi words import_limbs takes for EXPORT_ENC_BE32; false: a character is no hex digit
FR_HD __forceinline__ bool wire_unhex(const uint32_t chars[16], uint4 &lo, uint4 &hi) {
    uint32_t bad = 0u, v[8];
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) v[k] = wire_unhex_dword(chars[2u * k], chars[2u * k + 1u], bad);
    lo = make_uint4(v[0], v[1], v[2], v[3]);
    hi = make_uint4(v[4], v[5], v[6], v[7]);
    return bad == 0u;
}

// ---- the count word. A slot of `pitch` bytes holds one at all when its 8 bytes lie inside it; N is a map of the slot when it names no more
// entries than the handle has initial witnesses (so the sum below cannot wrap), its bytes fit the pitch and -- the caller gave a length -- are
// exactly that many.
FR_HD __forceinline__ bool wire_in_count_readable(uint32_t container, uint64_t pitch) { return wire_body_offset(container, 0) + WIRE_COUNT_BYTES <= pitch; }
FR_HD __forceinline__ bool wire_in_count_ok(uint32_t container, uint64_t pitch, uint32_t n_initial, uint64_t n, bool have_length, uint64_t length) {
    if (n > n_initial) return false;
    const uint64_t bytes = wire_length(container, n);
    return bytes <= pitch && (!have_length || length == bytes);
}

// ---- the framing of a GZIP_STORED row of n entries: where its words lie and what they must be (wire_head / wire_joint give head and joints)
FR_HD __forceinline__ uint64_t wire_in_joint_offset(uint64_t block) { return wire_body_offset(WIRE_GZIP_STORED, block * WIRE_BLOCK_BYTES) - WIRE_JOINT_BYTES; }  // block >= 1
FR_HD __forceinline__ uint64_t wire_in_trailer_offset(uint64_t n_entries) { return wire_length(WIRE_GZIP_STORED, n_entries) - WIRE_TRAILER_BYTES; }
FR_HD __forceinline__ uint32_t wire_in_isize(uint64_t n_entries) { return (uint32_t)wire_body_bytes(n_entries); }
// raw(u64le N) from the arithmetic alone: eight table-free byte steps are 64 shift steps
FR_HD __forceinline__ uint32_t wire_crc_raw_count(uint32_t n_entries) {
    uint32_t c = n_entries;
    for (int k = 0; k < 64; k++) c = (c >> 1) ^ (WIRE_CRC_POLY & (0u - (c & 1u)));
    return c;
}
// what the entry of rank r of a map of n entries adds to the XOR wire_crc_combine takes: raw(entry) * x^(8 * 76 * (n - 1 - r)); pow: that power
template <typename Table>
FR_HD __forceinline__ uint32_t wire_crc_entry(const uint32_t words[WIRE_ENTRY_WORDS], uint32_t pow, const Table &sliced) {
    return wire_crc_mul(pow, wire_crc_raw_sliced(words, WIRE_ENTRY_WORDS, sliced));
}
// the CRC-32 the trailer of a row must hold; entries: the XOR of its entries' shares
FR_HD __forceinline__ uint32_t wire_in_crc(uint32_t n_entries, uint32_t pow_n, uint32_t x64, uint32_t entries) {
    return wire_crc_combine(pow_n, x64, wire_crc_raw_count(n_entries), entries);
}

// ---- the finding key: ~(instance, class, entry rank) packed most significant first, kept with atomicMax so that zero means "none" and the
// word left is the smallest triple (import_mask.hpp import_mask_key). rank_bits: the width of the rank field, the plan's
// (wire_in_plan.hpp: instance, class and rank fit 63 bits together).
FR_HD __forceinline__ uint64_t wire_in_key(uint64_t instance, uint32_t cls, uint32_t rank, uint32_t rank_bits) { return ~((((instance << 3) | cls) << rank_bits) | rank); }
FR_HD __forceinline__ uint32_t wire_in_key_instance(uint64_t word, uint32_t rank_bits) { return (uint32_t)(~word >> (rank_bits + 3u)); }
FR_HD __forceinline__ uint32_t wire_in_key_class(uint64_t word, uint32_t rank_bits) { return (uint32_t)(~word >> rank_bits) & 7u; }
FR_HD __forceinline__ uint32_t wire_in_key_rank(uint64_t word, uint32_t rank_bits) { return (uint32_t)(~word & ((1ull << rank_bits) - 1u)); }

// the position of `key` in the handle's initial ids, or 0xFFFFFFFF: keys ascend, positions[k] is where keys[k] stands in initial_ids
FR_HD __forceinline__ uint32_t wire_in_position(const uint32_t *keys, const uint32_t *positions, uint32_t n, uint32_t key) {
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1u;
        else hi = mid;
    }
    return lo < n && keys[lo] == key ? positions[lo] : 0xFFFFFFFFu;
}

}  // namespace acvm
