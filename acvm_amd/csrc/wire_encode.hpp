// wire_encode.hpp -- the arithmetic of the batch-wide WitnessMap wire format (include/acvm_amd.h acvm_batch_witness_maps_wire_device,
// kernels_wire.hip): the hex expansion of an element, the 76 bytes of a map entry, the framing of a stored-block gzip member and the CRC-32 of a
// body accumulated entry by entry. Everything here is __host__ __device__ so that the host can run what the kernels run
// (tools/wire_encode_host_test.hip, tests/test_wire_encode_on_host.py); the lengths and the power table are also wire_plan.cpp's.
//
// The body (acir/src/native_types/witness_map.rs, circuit.cpp witness_map_to_bytes): u64le N, then per entry u32le witness, u64le 64 and 64
// lowercase hex characters of the canonical big-endian value: 8 + 76 N bytes, the entry of rank r at 8 + 76 r. Everything is a multiple of 4.
#pragma once
#include "export_encode.hpp"

namespace acvm {

enum : uint32_t { WIRE_BINCODE = 0, WIRE_GZIP_STORED = 1, WIRE_N_CONTAINERS = 2 };  // (ACVM_WIRE_* of include/acvm_amd.h)
constexpr uint32_t WIRE_COUNT_BYTES = 8, WIRE_ENTRY_BYTES = 76, WIRE_ENTRY_WORDS = WIRE_ENTRY_BYTES / 4;
// A stored block holds 65 532 body bytes (the largest multiple of 4 a 16-bit LEN can say); the member's head -- the 11-byte gzip header and the
// first block's 5-byte header -- is 16 bytes, every later block has 3 empty stored blocks and its own header, 20 bytes, in front; the trailer
// is CRC-32 and ISIZE. So body dwords stay aligned dwords of the member.
constexpr uint32_t WIRE_BLOCK_BYTES = 65532, WIRE_BLOCK_WORDS = WIRE_BLOCK_BYTES / 4, WIRE_HEAD_BYTES = 16, WIRE_JOINT_BYTES = 20, WIRE_TRAILER_BYTES = 8;
// the kernel's tile: 64 rows x WIRE_WINDOW list positions; a row's image is WIRE_WINDOW entries, the LDS pitch is odd (lane = row in phase 1:
// the 64 lanes of one store fall on 64 banks)
constexpr uint32_t WIRE_ROWS = 64, WIRE_WINDOW = 8, WIRE_IMAGE_WORDS = WIRE_WINDOW * WIRE_ENTRY_WORDS, WIRE_LDS_PITCH = WIRE_IMAGE_WORDS + 1;
static_assert(WIRE_LDS_PITCH % 2 == 1, "an odd pitch");

FR_HD __forceinline__ uint64_t wire_body_bytes(uint64_t n_entries) { return WIRE_COUNT_BYTES + (uint64_t)WIRE_ENTRY_BYTES * n_entries; }
FR_HD __forceinline__ uint64_t wire_blocks(uint64_t body_bytes) { return (body_bytes + WIRE_BLOCK_BYTES - 1) / WIRE_BLOCK_BYTES; }
// where body byte k lies in the slot
FR_HD __forceinline__ uint64_t wire_body_offset(uint32_t container, uint64_t k) {
    return container == WIRE_GZIP_STORED ? WIRE_HEAD_BYTES + k + (uint64_t)WIRE_JOINT_BYTES * (k / WIRE_BLOCK_BYTES) : k;
}
// the bytes of a map of n_entries entries
FR_HD __forceinline__ uint64_t wire_length(uint32_t container, uint64_t n_entries) {
    const uint64_t L = wire_body_bytes(n_entries);
    return container == WIRE_GZIP_STORED ? WIRE_HEAD_BYTES + L + (uint64_t)WIRE_JOINT_BYTES * (wire_blocks(L) - 1) + WIRE_TRAILER_BYTES : L;
}
// the 20 bytes in front of the data of stored block `block` >= 1 of a body of body_bytes, as 5 dwords: three empty non-final stored blocks
// (00 00 00 ff ff each), then BFINAL, LEN, ~LEN
FR_HD __forceinline__ void wire_joint(uint64_t body_bytes, uint64_t block, uint32_t out[5]) {
    const uint64_t left = body_bytes - block * WIRE_BLOCK_BYTES;
    const uint32_t final = left <= WIRE_BLOCK_BYTES ? 1u : 0u, len = final ? (uint32_t)left : WIRE_BLOCK_BYTES;
    out[0] = 0xff000000u;
    out[1] = 0x000000ffu;
    out[2] = 0x0000ffffu;
    out[3] = 0x00ffff00u | (final << 24);
    out[4] = len | ((~len & 0xffffu) << 16);
}
// the 16 bytes at the member's start: 1f 8b 08 08, MTIME 0, XFL 0, OS 255, the empty name's NUL, then the first block's header
FR_HD __forceinline__ void wire_head(uint64_t body_bytes, uint32_t out[4]) {
    const uint32_t final = body_bytes <= WIRE_BLOCK_BYTES ? 1u : 0u, len = final ? (uint32_t)body_bytes : WIRE_BLOCK_BYTES;
    out[0] = 0x08088b1fu;
    out[1] = 0u;
    out[2] = 0x0000ff00u | (final << 24);
    out[3] = len | ((~len & 0xffffu) << 16);
}

// ---- hex. The four nibbles of 16 bits, one per byte, to '0' .. '9', 'a' .. 'f' at once: a byte above 9 takes 39 more.
FR_HD __forceinline__ uint32_t wire_hex4(uint32_t nibbles) {
    return nibbles + 0x30303030u + (((nibbles + 0x06060606u) >> 4) & 0x01010101u) * 39u;
}
// One dword of an export_encode BE32 element (its bytes b0 b1 b2 b3 in memory order, b0 the lowest byte of v) as the eight characters they
// print as, high nibble first: lo = the characters of b0 b1, hi = those of b2 b3.
FR_HD __forceinline__ void wire_hex_dword(uint32_t v, uint32_t &lo, uint32_t &hi) {
    auto spread = [](uint32_t h) { return ((h >> 4) & 0xfu) | ((h & 0xfu) << 8) | (((h >> 12) & 0xfu) << 16) | (((h >> 8) & 0xfu) << 24); };
    lo = wire_hex4(spread(v & 0xffffu));
    hi = wire_hex4(spread(v >> 16));
}
// the 64 characters of an element as 16 dwords
FR_HD __forceinline__ void wire_hex(const ExportElement &e, uint32_t out[16]) {
    const uint32_t v[8] = {e.lo.x, e.lo.y, e.lo.z, e.lo.w, e.hi.x, e.hi.y, e.hi.z, e.hi.w};
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) wire_hex_dword(v[k], out[2u * k], out[2u * k + 1u]);
}
// the 76 bytes of the entry of `witness`: u32le witness, u64le 64, the characters
FR_HD __forceinline__ void wire_entry(uint32_t witness, const ExportElement &e, uint32_t out[WIRE_ENTRY_WORDS]) {
    out[0] = witness;
    out[1] = 64u;
    out[2] = 0u;
    wire_hex(e, out + 3);
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320) as a polynomial mod P: bit 31 of a register is x^0, a shift right multiplies by x.
// The RAW crc of bytes is the register after them from a zero register, without the final xor: it is linear, and
//   crc32(body) = 0xFFFFFFFF ^ shift(0xFFFFFFFF, |body|) ^ shift(raw(count), 76 N) ^ XOR_r shift(raw(entry_r), 76 (N - 1 - r)),
// shift(c, m) = c advanced over m zero bytes = c * x^(8 m).
constexpr uint32_t WIRE_CRC_POLY = 0xEDB88320u;
FR_HD __forceinline__ uint32_t wire_crc_table_entry(uint32_t byte) {
    uint32_t c = byte;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (WIRE_CRC_POLY & (0u - (c & 1u)));
    return c;
}
// the register advanced over the four bytes of a little-endian dword; table: the 256 entries above
template <typename Table>
FR_HD __forceinline__ uint32_t wire_crc_dword(uint32_t c, uint32_t v, const Table &table) {
    c ^= v;
#pragma unroll
    for (int k = 0; k < 4; k++) c = table[c & 0xffu] ^ (c >> 8);
    return c;
}
template <typename Table>
FR_HD __forceinline__ uint32_t wire_crc_raw(const uint32_t *words, uint32_t n, const Table &table) {
    uint32_t c = 0u;
    for (uint32_t k = 0; k < n; k++) c = wire_crc_dword(c, words[k], table);
    return c;
}
// The same step with four lookups that do not wait for each other (slicing by 4): entry 256 k + b of the sliced table is byte b advanced over
// k further zero bytes, so the dword's four bytes -- 3, 2, 1, 0 zero bytes in front of the dword's end -- are looked up at once.
constexpr uint32_t WIRE_CRC_SLICES = 4, WIRE_CRC_SLICED_WORDS = WIRE_CRC_SLICES * 256;
FR_HD __forceinline__ uint32_t wire_crc_sliced_entry(uint32_t index) {
    uint32_t c = wire_crc_table_entry(index & 0xffu);
    for (uint32_t k = index >> 8; k; k--) c = wire_crc_table_entry(c & 0xffu) ^ (c >> 8);
    return c;
}
template <typename Table>
FR_HD __forceinline__ uint32_t wire_crc_dword_sliced(uint32_t c, uint32_t v, const Table &sliced) {
    c ^= v;
    return sliced[768u + (c & 0xffu)] ^ sliced[512u + ((c >> 8) & 0xffu)] ^ sliced[256u + ((c >> 16) & 0xffu)] ^ sliced[c >> 24];
}
template <typename Table>
FR_HD __forceinline__ uint32_t wire_crc_raw_sliced(const uint32_t *words, uint32_t n, const Table &sliced) {
    uint32_t c = 0u;
    for (uint32_t k = 0; k < n; k++) c = wire_crc_dword_sliced(c, words[k], sliced);
    return c;
}
// a * b mod P
FR_HD __forceinline__ uint32_t wire_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0u;
#pragma unroll
    for (int k = 31; k >= 0; k--) {
        p ^= b & (0u - ((a >> k) & 1u));
        b = (b >> 1) ^ (WIRE_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 bytes) mod P
FR_HD inline uint32_t wire_crc_xpow_bytes(uint64_t bytes) {
    uint32_t r = 0x80000000u, sq = 0x00800000u;  // x^0, x^8
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) r = wire_crc_mul(r, sq);
        sq = wire_crc_mul(sq, sq);
    }
    return r;
}
// The combination. pow_n = x^(8 * 76 * N) (the power table's entry N), x64 = x^64, raw_count = raw(u64le N),
// entries = XOR_r raw(entry_r) * x^(8 * 76 * (N - 1 - r)).
FR_HD __forceinline__ uint32_t wire_crc_combine(uint32_t pow_n, uint32_t x64, uint32_t raw_count, uint32_t entries) {
    return 0xFFFFFFFFu ^ wire_crc_mul(wire_crc_mul(x64, pow_n), 0xFFFFFFFFu) ^ wire_crc_mul(pow_n, raw_count) ^ entries;
}

}  // namespace acvm
