// kernels_records_masked.hip -- the masked record import (include/acvm_amd.h acvm_batch_import_device_records_masked): the record import for
// instances that do not all hold every initial witness, the presence of an element a byte of the record itself.
//
//  import_records_masked_kernel   import_records_kernel (kernels_records.hip) over the masked tables of record_plan.hpp: the same phase 1
//                                 (record_stage.hpp), and in phase 2 a lane takes its presence byte from the LDS image -- or, a mask byte further
//                                 than a window from its element, with one byte load -- before it decodes. An absent lane decodes the element of
//                                 zero bytes: the zero row and the plane word 0x80000000 leave in the one store of the row every lane makes. Its
//                                 bit of the missing set (import_mask.hpp) is ORed per (word, instance) in LDS, and the block sends each nonzero
//                                 word to global memory with one atomicOr: blocks of other windows of the same instances hold other bits of it.
//  import_missing_count_kernel    behind it: the instances with at least one absent input, from the missing set -- what a field-wise kernel
//                                 cannot count without counting an instance once per absent field
//
// A translation unit of its own: kernels_records.hip and kernels_import_mask.hip compile to what they compiled to before these kernels existed.
#include "record_stage.hpp"
#include "import_mask.hpp"

namespace acvm {

struct RecordMaskArgs {
    uint32_t *missing;           // [import_missing_words(n_in)][Bp], the words of the live instances zeroed in front of the launch
    unsigned long long *result;  // IMPORT_MASK_RESULT_WORDS words (import_mask.hpp)
};

// blockIdx.x: the 64 instances, blockIdx.y (+ w0): the window
__global__ void __launch_bounds__(256) import_records_masked_kernel(const RecordImportArgs a, const RecordMaskArgs m, uint32_t w0) {
    __shared__ uint32_t image[RECORD_LDS_WORDS];
    __shared__ uint32_t miss[RECORD_MISS_LDS_WORDS];
    const uint32_t t = threadIdx.x;
    const uint64_t j0 = (uint64_t)blockIdx.x * RECORD_BLOCK_INSTANCES;
    const uint32_t nb = a.B - j0 < RECORD_BLOCK_INSTANCES ? (uint32_t)(a.B - j0) : RECORD_BLOCK_INSTANCES;  // (the grid has no block at or behind B)
    const uint32_t *win = a.windows + (size_t)(w0 + blockIdx.y) * RECORD_MWINDOW_WORDS;
    const uint64_t win_offset = ((uint64_t)win[RECORD_WINDOW_OFFSET_HI] << 32) | win[RECORD_WINDOW_OFFSET_LO];
    const uint32_t win_length = win[RECORD_WINDOW_LENGTH], first_field = win[RECORD_WINDOW_FIRST_FIELD], n_fields = win[RECORD_WINDOW_N_FIELDS];
    const uint32_t miss_base = win[RECORD_MWINDOW_MISS_BASE];
    const uint64_t S = (uint64_t)(uintptr_t)a.in + j0 * a.pitch + win_offset;
    // ---- phase 1: the window as the unmasked kernel stages it, and the block's missing words zeroed
    for (uint32_t q = t; q < RECORD_MISS_LDS_WORDS; q += 256u) miss[q] = 0u;
    record_stage(image, S, a.pitch, win_length, nb, t);
    __syncthreads();
    // ---- phase 2: one wave per field, lane = instance
    const uint32_t wave = t >> 6, i = t & 63u;
    const uint64_t j = j0 + i;
    const uint32_t phase = record_phase(S + (uint64_t)i * a.pitch);
    for (uint32_t f = wave; f < n_fields; f += 4u) {  // (wave-uniform: the field's words are scalar loads)
        const uint32_t *fd = a.fields + (size_t)(first_field + f) * RECORD_MFIELD_WORDS;
        const uint32_t row = fd[RECORD_FIELD_ROW], pl = fd[RECORD_FIELD_PLANE], encoding = fd[RECORD_FIELD_ENCODING], byte = fd[RECORD_FIELD_BYTE];
        const uint32_t position = fd[RECORD_MFIELD_POSITION], mask = fd[RECORD_MFIELD_MASK];
        if (j < a.B) {
            uint32_t presence = 1u;
            if (mask == RECORD_MASK_FAR) presence = a.in[j * a.pitch + (((uint64_t)fd[RECORD_MFIELD_FAR_HI] << 32) | fd[RECORD_MFIELD_FAR_LO])];  // (below the pitch)
            else if (mask != RECORD_MASK_NONE) presence = record_presence_byte(image + i * RECORD_LDS_PITCH, phase + mask);
            uint32_t word;
            const Fr v = record_element<true>(image + i * RECORD_LDS_PITCH, phase + byte, encoding, pl != 0xFFFFFFFFu, presence == 1u, word);
            fr_store_nt(a.W, row, a.Bp, j, v);
            if (pl != 0xFFFFFFFFu) a.plane[(uint64_t)pl * a.Bp + j] = word;
            if (a.event_reset && first_field + f == 0u) record_event_reset(a.event_reset, j);
            if (mask != RECORD_MASK_NONE) {  // (wave-uniform)
                // anything but 1 leaves the element absent (a refused import leaves the handle without initial witnesses anyway)
                if (presence != 1u) {
                    const uint32_t slot = record_miss_slot(position, miss_base);
                    if (slot != RECORD_MISS_NO_SLOT) atomicOr(&miss[record_miss_lds_word(slot, i)], import_missing_bit(position));
                    else atomicOr(&m.missing[import_missing_word(position, a.Bp, j)], import_missing_bit(position));
                }
                // the bytes other than 0 / 1: their number, and the smallest (instance, position) -- lanes hold ascending instances, so the lowest
                // lane with a bad byte holds the wave's smallest key for this field (kernels_import_mask.hip mask_results)
                const uint64_t bad = __builtin_amdgcn_ballot_w64(presence > 1u);
                if (bad) {
                    const uint32_t lowest = (uint32_t)__builtin_ctzll(bad);
                    if (i == lowest) {
                        atomicAdd(m.result + IMPORT_MASK_BAD, (unsigned long long)__builtin_popcountll(bad));
                        atomicMax(m.result + IMPORT_MASK_BAD_KEY, (unsigned long long)import_mask_key(j, position));
                    }
                }
            }
        }
    }
    // ---- the block's missing words: one global atomicOr per nonzero (word, instance)
    __syncthreads();
    for (uint32_t q = t; q < RECORD_MISS_LDS_WORDS; q += 256u) {
        const uint32_t slot = q / RECORD_BLOCK_INSTANCES, inst = q % RECORD_BLOCK_INSTANCES;  // (q = record_miss_lds_word(slot, inst))
        const uint32_t bits = miss[q];
        if (bits) atomicOr(&m.missing[(uint64_t)(miss_base + slot) * a.Bp + j0 + inst], bits);  // (bits of live instances only: inst < nb)
    }
}

// the instances with at least one absent input: one atomic per wave that has one (ballot, the lowest lane speaks)
__global__ void __launch_bounds__(256) import_missing_count_kernel(const uint32_t *__restrict__ missing, uint32_t n_words, uint64_t Bp, uint32_t B, unsigned long long *result) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t any = 0;
    if (j < B)
        for (uint32_t word = 0; word < n_words; word++) any |= missing[(uint64_t)word * Bp + j];
    const uint64_t lacking = __builtin_amdgcn_ballot_w64(any != 0u);
    if (lacking && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(lacking)) atomicAdd(result + IMPORT_MASK_MISSING, (unsigned long long)__builtin_popcountll(lacking));
}

bool launch_import_records_masked(hipStream_t s, const void *in, uint64_t pitch, const uint32_t *windows, uint32_t n_windows, const uint32_t *fields, uint4 *W, uint64_t Bp,
                                  uint32_t B, uint32_t n_in, uint32_t *plane, uint32_t *event_reset, uint32_t *missing, uint64_t *result) {
    if (!B || !n_windows) return false;
    const uint32_t n_words = import_missing_words(n_in);
    // every word of the live instances is rewritten: zero, then the bits of this call
    (void)hipMemset2DAsync(missing, Bp * 4, 0, (size_t)B * 4, n_words, s);
    const RecordImportArgs a{W, Bp, B, (const uint8_t *)in, pitch, windows, fields, nullptr, plane, event_reset};
    const RecordMaskArgs m{missing, (unsigned long long *)result};
    for_grid_y_chunks(n_windows, [&](uint32_t done, uint32_t chunk) {
        hipLaunchKernelGGL(import_records_masked_kernel, dim3((B + RECORD_BLOCK_INSTANCES - 1u) / RECORD_BLOCK_INSTANCES, chunk), dim3(256), 0, s, a, m, done);
    });
    hipLaunchKernelGGL(import_missing_count_kernel, dim3((B + 255u) / 256u), dim3(256), 0, s, missing, n_words, Bp, B, (unsigned long long *)result);
    return event_reset != nullptr;
}

}  // namespace acvm
