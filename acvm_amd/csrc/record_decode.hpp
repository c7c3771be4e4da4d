// record_decode.hpp -- what the record import (kernels_records.hip, include/acvm_amd.h acvm_batch_import_device_records) computes per element in
// front of import_decode.hpp: where a byte of a record lies in the block's staging image, and the element of 1 .. 32 bytes at an arbitrary byte
// offset of that image. Everything here is __host__ __device__ so that the host can run what the kernel runs (tools/record_decode_host_test.hip,
// tests/test_record_decode_on_host.py); record_plan.cpp takes the constants.
#pragma once
#include "import_decode.hpp"

namespace acvm {

// A block stages one WINDOW of 64 consecutive records: a byte range of the record that holds whole fields, at most RECORD_WINDOW_CAP bytes.
// A record of at most that many bytes is one window, the record itself.
constexpr uint32_t RECORD_WINDOW_CAP = 256u;
constexpr uint32_t RECORD_BLOCK_INSTANCES = 64u;
// The image of one record's window: the ALIGNED dwords of global memory that hold a byte of it, in order, so every record keeps its byte phase
// (address & 3) and phase 1 stores the words as loaded. Phase p and L bytes take (p + L + 3) / 4 words: at most (256 + 3 + 3) / 4 = 65.
constexpr uint32_t RECORD_IMAGE_WORDS = (RECORD_WINDOW_CAP + 6u) / 4u;
// The images lie RECORD_LDS_PITCH words apart. The bank argument (64 banks of 4 bytes; a dword read is served per half wave, i.e. modulus 32
// lanes, wider reads modulus 64): in phase 2 lane i reads word i * PITCH + w_i of the array, where w_i = (phase_i + byte) / 4 and the phases of
// the 64 records differ by less than a word, so w_i is w or w + 1. With PITCH = 65 = 1 (mod 64) lane i falls on bank (i + w_i) mod 64: the
// lanes with w_i = w take 64 different banks among themselves, so do those with w_i = w + 1, and a bank is asked by at most one lane of each
// kind -- at most 2 lanes per bank, at least 32 banks, whatever the record pitch. (A plain copy at a record pitch of 128 or 256 bytes would put
// all 64 lanes on one bank.) record_lds_word below is the whole address map; the host test counts the banks through it.
constexpr uint32_t RECORD_LDS_PITCH = 65u;
constexpr uint32_t RECORD_LDS_WORDS = RECORD_BLOCK_INSTANCES * RECORD_LDS_PITCH;  // 16 640 bytes per block: nine blocks fit a CU's 160 KiB
static_assert(RECORD_LDS_PITCH >= RECORD_IMAGE_WORDS && RECORD_LDS_PITCH % 64u == 1u, "the bank argument above");

// byte phase of a record's window: how far into its first aligned dword the window begins. window_address: the byte address in global memory
FR_HD __forceinline__ uint32_t record_phase(uint64_t window_address) { return (uint32_t)(window_address & 3u); }
// The staging image's address map: the word of the block's LDS array that holds byte `byte_in_window` of the window of the block's instance
// `instance_in_block`, whose window begins at phase `phase`; the byte is byte (phase + byte_in_window) & 3 of that word.
FR_HD __forceinline__ uint32_t record_lds_word(uint32_t instance_in_block, uint32_t phase, uint32_t byte_in_window) {
    return instance_in_block * RECORD_LDS_PITCH + (phase + byte_in_window) / 4u;
}

// bytes [at, at + 4) of the little-endian byte string whose aligned dwords are lo (bytes 0 .. 3) and hi (bytes 4 .. 7); shift = 8 * (at & 3)
FR_HD __forceinline__ uint32_t record_funnel(uint32_t lo, uint32_t hi, uint32_t shift) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> shift); }

// The element of `size` bytes (1, 2, 4, 8, 16 or 32) that begins at byte `byte` of the word image `words`, as import_decode.hpp takes it: lo =
// bytes [0, 16) and hi = bytes [16, 32) as they lie in memory, a narrow element zero-extended. Funnel shifts over aligned words, no byte loop.
// No word is read that holds no byte of the element: the upper operand of the last funnel is clamped to the element's last word (shifted out
// when it is not needed). size is uniform where the caller is a wave.
FR_HD __forceinline__ void record_assemble(const uint32_t *words, uint32_t byte, uint32_t size, uint4 &lo, uint4 &hi) {
    const uint32_t w0 = byte / 4u, shift = 8u * (byte & 3u), last = (byte + size - 1u) / 4u;
    const uint32_t n_out = (size + 3u) / 4u;
    uint32_t v[8];
    uint32_t cur = words[w0];
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) {
        v[i] = 0u;
        if (i < n_out) {
            const uint32_t at = w0 + i + 1u;
            const uint32_t next = words[at < last ? at : last];
            v[i] = record_funnel(cur, next, shift);
            cur = next;
        }
    }
    if (size < 4u) v[0] &= (1u << (8u * size)) - 1u;
    lo = make_uint4(v[0], v[1], v[2], v[3]);
    hi = make_uint4(v[4], v[5], v[6], v[7]);
}

// ---- the masked record import (kernels_records_masked.hip, include/acvm_amd.h acvm_batch_import_device_records_masked)
// The presence byte of a field whose mask byte lies in the block's window: byte `byte` (phase + offset in the window) of a record's word image.
FR_HD __forceinline__ uint32_t record_presence_byte(const uint32_t *words, uint32_t byte) { return (words[byte / 4u] >> (8u * (byte & 3u))) & 0xffu; }
// A block ORs the missing-set bits (import_mask.hpp) of its window's fields in LDS before anything goes to global memory: RECORD_MISS_SLOTS words
// per instance, slot s for the missing word `base + s`, base the lowest word a field of the window has (the window table carries it). A field
// whose word lies further up has no slot -- RECORD_MISS_NO_SLOT -- and its absent lanes go to global memory one by one. Slot-major: lane i of a
// wave falls on bank i, whatever the slot.
constexpr uint32_t RECORD_MISS_SLOTS = 8u;  // 8 x 64 words = 2 KiB beside the image's 16 640 bytes: eight blocks of 256 threads still fill a CU
constexpr uint32_t RECORD_MISS_LDS_WORDS = RECORD_MISS_SLOTS * RECORD_BLOCK_INSTANCES;
constexpr uint32_t RECORD_MISS_NO_SLOT = 0xFFFFFFFFu;
FR_HD __forceinline__ uint32_t record_miss_slot(uint32_t position, uint32_t base_word) {
    const uint32_t s = (position >> 5) - base_word;  // (position >> 5 >= base_word by the table's construction; a wrap is above the slots too)
    return s < RECORD_MISS_SLOTS ? s : RECORD_MISS_NO_SLOT;
}
FR_HD __forceinline__ uint32_t record_miss_lds_word(uint32_t slot, uint32_t instance_in_block) { return slot * RECORD_BLOCK_INSTANCES + instance_in_block; }

// One element of a record, everything (the kernel takes a wave of bytes from fr_mont_of_byte instead of the product: the same row)
FR_HD __forceinline__ ImportDecoded record_decode(const uint32_t *words, uint32_t byte, uint32_t encoding) {
    const uint32_t size = export_element_size(encoding);
    uint4 lo, hi;
    record_assemble(words, byte, size, lo, hi);
    return size == 32u ? import_decode(lo, hi, encoding) : import_decode_narrow(lo);
}

}  // namespace acvm
