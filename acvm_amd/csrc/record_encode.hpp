// record_encode.hpp -- what the record export (kernels_records_out.hip, include/acvm_amd.h acvm_batch_export_device_records) computes per element
// behind export_encode.hpp: the inverse of record_decode.hpp. An element of 1 .. 32 bytes is placed at an arbitrary byte of a record's word
// image (the block's staging image, record_decode.hpp's address map), and the image leaves for global memory under a byte-exact cover rule.
// Everything here is __host__ __device__ so that the host can run what the kernel runs (tools/record_encode_host_test.hip,
// tests/test_record_encode_on_host.py).
#pragma once
#include "export_encode.hpp"
#include "record_decode.hpp"

namespace acvm {

// The staging image is record_decode.hpp's: per record the ALIGNED dwords of global memory that hold a byte of its window, so every record
// keeps its byte phase and the write-out stores the words as they lie; RECORD_LDS_PITCH = 65 words apart, address map record_lds_word. The bank
// argument carries over unchanged: in phase 1 lane i writes word i * 65 + w_i, w_i = (phase_i + byte) / 4 in {w, w + 1} -- at most 2 lanes per
// bank, at least 32 banks, whatever the record pitch.

// The element of `size` bytes (1, 2, 4, 8, 16 or 32; lo = bytes [0, 16), hi = bytes [16, 32) as they lie in memory, every byte at and above
// `size` zero) goes to byte `byte` of a word image that was ZEROED before. Funnel shifts over aligned words, no byte loop.
//   - A word the element owns whole -- all four bytes inside [byte, byte + size) -- is a plain store: store(word index, value).
//   - The first and the last word, when the element owns only some of their bytes, may hold bytes of another field: they go through
//     or_into(word index, value), which must be ATOMIC where two waves share the image (an LDS atomicOr: two waves never do a plain
//     read-modify-write of one word). The element's bytes alone are set; the image was zero, so the OR places them.
// size is uniform where the caller is a wave; byte need not be.
template <class Store, class OrInto>
FR_HD __forceinline__ void record_scatter(uint32_t byte, uint32_t size, const uint4 &lo, const uint4 &hi, Store store, OrInto or_into) {
    const uint32_t w0 = byte / 4u, shift = 8u * (byte & 3u), n_words = (byte + size - 1u) / 4u - w0 + 1u;  // 1 .. 9
    const uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t n_in = (size + 3u) / 4u;
    uint32_t below = 0u;  // the word of the element under the one being placed
#pragma unroll
    for (uint32_t i = 0; i < 9u; i++) {
        if (i < n_words) {
            const uint32_t cur = i < n_in ? v[i & 7u] : 0u;  // (n_in <= 8)
            // bytes [4 i - (byte & 3), 4 i - (byte & 3) + 4) of the element: (cur : below) >> (32 - shift); shift 0 gives cur
            const uint32_t word = (uint32_t)((((uint64_t)cur << 32) | below) >> (32u - shift));
            below = cur;
            const bool whole = 4u * (w0 + i) >= byte && 4u * (w0 + i) + 4u <= byte + size;
            if (whole) store(w0 + i, word);
            else or_into(w0 + i, word);
        }
    }
}

// The four cover bits of ALIGNED dword k of the image of a record's window that begins at byte phase `phase` (0 .. 3) of dword 0: bit b is set
// when byte b of that dword is byte 4 k + b - phase of the window, lies in [0, length) and is covered -- bit (that byte) of `bitmap`
// (record_out_plan.hpp: RECORD_WINDOW_CAP bits, bit b of the window in word b >> 5). Bits outside [0, length) are zero whatever the bitmap
// holds. The write-out rule is this nibble and nothing else: 0xF is one dword store, any other value one byte store per set bit, 0 nothing --
// so a dword is written whole only when all four of its bytes are this record's covered bytes, and at a joint of two records, two blocks or
// two windows each side stores its own bytes.
FR_HD __forceinline__ uint32_t record_cover_nibble(const uint32_t *bitmap, uint32_t length, uint32_t phase, uint32_t k) {
    const int32_t pos = (int32_t)(4u * k) - (int32_t)phase;  // the window byte of the dword's byte 0: -3 .. length + 2
    uint32_t bits;
    if (pos < 0) bits = bitmap[0] << (uint32_t)(-pos);
    else {
        const uint32_t word = (uint32_t)pos >> 5, sh = (uint32_t)pos & 31u;
        const uint32_t lo = word < RECORD_WINDOW_CAP / 32u ? bitmap[word] : 0u, hi = word + 1u < RECORD_WINDOW_CAP / 32u ? bitmap[word + 1u] : 0u;
        bits = record_funnel(lo, hi, sh);
    }
    bits &= 0xFu;
    const int32_t room = (int32_t)length - pos;  // bytes of the window from the dword's byte 0 on
    if (room <= 0) return 0u;
    if (room < 4) bits &= (1u << room) - 1u;
    return bits;
}

}  // namespace acvm
