// kernels_records.hip -- the record import (include/acvm_amd.h acvm_batch_import_device_records): the initial witnesses as one packed record of
// mixed-width fields per instance, at any pitch, any field offset and any base alignment.
//
//  import_records_kernel   a block of 256 threads owns 64 consecutive instances and one window of the record (record_plan.hpp): phase 1 copies
//                          the window's aligned dwords of its 64 records into LDS, phase 2 is import_narrow_im_kernel's second phase -- one
//                          wave per field, lane = instance, the element assembled from LDS (record_decode.hpp), decoded (import_decode.hpp)
//                          and stored as two 1 KiB half rows per wave
//
// A translation unit of its own: the other code objects compile to what they compiled to before this kernel existed.
#include "ops_common.hpp"
#include "kernels.hpp"
#include "record_decode.hpp"
#include "record_plan.hpp"

namespace acvm {

static_assert(RECORD_WINDOW_CAP == RECORD_PLAN_WINDOW_CAP, "the kernel (record_decode.hpp) and the window cut (record_plan.cpp) agree on the window size");

struct RecordImportArgs {
    uint4 *W;
    uint64_t Bp;
    uint32_t B;
    const uint8_t *in;        // any alignment
    uint64_t pitch;
    const uint32_t *windows;  // [n_windows][RECORD_WINDOW_WORDS]
    const uint32_t *fields;   // [n_fields][RECORD_FIELD_WORDS], window by window
    const uint32_t *gate;
    uint32_t *plane, *event_reset;
};
// ACVM::new: nobody has left the generic path yet (kernels_import.hip import_event_reset)
__device__ __forceinline__ void record_event_reset(uint32_t *event_reset, uint64_t j) {
    event_reset[j] = 0xFFFFFFFFu;
    if (j == 0) { event_reset[-4] = 0u; event_reset[-3] = 0u; }
}

// One element from the block's image: the row and the plane word. encoding (and with it the size) is wave-uniform; every lane of the wave that
// is still active must arrive (the ballots): a wave of bytes -- message bytes, digits, flags -- takes the row from the closed form of
// ops_common.hpp fr_mont_of_byte instead of a product, and U8 always (kernels_typed_io.hip typed_narrow_row, kernels_import.hip import_element).
__device__ __forceinline__ Fr record_element(const uint32_t *image, uint32_t byte, uint32_t encoding, bool want_plane, uint32_t &plane_word) {
    const uint32_t size = export_element_size(encoding);
    uint4 lo, hi;
    record_assemble(image, byte, size, lo, hi);
    if (size == 1u) {
        plane_word = lo.x | 0x80000000u;
        return fr_mont_of_byte(lo.x);
    }
    if (size != 32u) {
        const Fr x = import_narrow_limbs(lo);
        plane_word = import_plane_word(x);
        if (__builtin_amdgcn_ballot_w64(!import_is_byte(x)) == 0) return fr_mont_of_byte(lo.x);
        return fr_mul(x, import_r522());
    }
    const Fr m = import_limbs(lo, hi, encoding);
    const bool have_canonical = encoding != EXPORT_ENC_MONT256_LE || want_plane;
    Fr x = m;
    if (have_canonical) x = import_canonical(m, encoding);
    const bool is_byte = have_canonical && import_is_byte(x);
    plane_word = (x.v[0] & 0x1fffffffu) | (is_byte ? 0x80000000u : 0u);  // (meaningless without a canonical value: nobody stores it then)
    if (__builtin_amdgcn_ballot_w64(!is_byte) == 0) return fr_mont_of_byte(x.v[0]);
    return import_row(m, x, encoding);
}

// blockIdx.x: the 64 instances, blockIdx.y (+ w0): the window. The LDS image and its bank argument: record_decode.hpp.
__global__ void __launch_bounds__(256) import_records_kernel(const RecordImportArgs a, uint32_t w0) {
    __shared__ uint32_t image[RECORD_LDS_WORDS];
    if (a.gate && *a.gate != 0u) return;  // (block-uniform)
    const uint32_t t = threadIdx.x;
    const uint64_t j0 = (uint64_t)blockIdx.x * RECORD_BLOCK_INSTANCES;
    const uint32_t nb = a.B - j0 < RECORD_BLOCK_INSTANCES ? (uint32_t)(a.B - j0) : RECORD_BLOCK_INSTANCES;  // (the grid has no block at or behind B)
    const uint32_t *win = a.windows + (size_t)(w0 + blockIdx.y) * RECORD_WINDOW_WORDS;
    const uint64_t win_offset = ((uint64_t)win[RECORD_WINDOW_OFFSET_HI] << 32) | win[RECORD_WINDOW_OFFSET_LO];
    const uint32_t win_length = win[RECORD_WINDOW_LENGTH], first_field = win[RECORD_WINDOW_FIRST_FIELD], n_fields = win[RECORD_WINDOW_N_FIELDS];
    // byte address of the window of the block's first record
    const uint64_t S = (uint64_t)(uintptr_t)a.in + j0 * a.pitch + win_offset;
    // ---- phase 1: record i takes the (phase_i + length + 3) / 4 aligned dwords that hold a byte of its window, consecutive lanes on consecutive
    // dwords: a group of G lanes per record, G the power of two that holds the most dwords a record of this block takes (no division anywhere).
    // Only dwords that hold a byte of a window of the block's records are loaded. For a pitch up to the window size the window is the record
    // and the nb records are one contiguous span: neighbouring groups then meet in the dword at the joint, which both load. Four loads are in
    // flight per lane before the first of them is stored: the phase is as long as one load's latency, not four. (Plain loads: the blocks of
    // the other windows of these records read the same lines again.)
    {
        // a pitch of whole dwords keeps the phase of the first record; any other takes every phase
        const uint32_t row_words = ((a.pitch & 3u) ? win_length + 6u : record_phase(S) + win_length + 3u) / 4u;  // 1 .. 65
        const uint32_t shift = row_words > 1u ? 32u - __builtin_clz(row_words - 1u) : 0u;                      // G = 1 << shift >= row_words, at most 128
        const uint32_t total = RECORD_BLOCK_INSTANCES << shift;
        for (uint32_t g0 = t; g0 < total; g0 += 1024u) {
            uint32_t v[4], at_lds[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) {
                const uint32_t g = g0 + 256u * u, i = g >> shift, k = g & ((1u << shift) - 1u);
                const uint64_t at = S + (uint64_t)i * a.pitch;
                const uint32_t phase = record_phase(at);
                const bool mine = g < total && i < nb && k < (phase + win_length + 3u) / 4u;
                at_lds[u] = mine ? i * RECORD_LDS_PITCH + k : 0xFFFFFFFFu;
                v[u] = mine ? *(const uint32_t *)(at - phase + 4u * (uint64_t)k) : 0u;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++)
                if (at_lds[u] != 0xFFFFFFFFu) image[at_lds[u]] = v[u];
        }
    }
    __syncthreads();
    // ---- phase 2: one wave per field, lane = instance
    const uint32_t wave = t >> 6, i = t & 63u;
    const uint64_t j = j0 + i;
    const uint32_t phase = record_phase(S + (uint64_t)i * a.pitch);
    for (uint32_t f = wave; f < n_fields; f += 4u) {  // (wave-uniform: the field's words are scalar loads)
        const uint32_t *fd = a.fields + (size_t)(first_field + f) * RECORD_FIELD_WORDS;
        const uint32_t row = fd[RECORD_FIELD_ROW], pl = fd[RECORD_FIELD_PLANE], encoding = fd[RECORD_FIELD_ENCODING], byte = fd[RECORD_FIELD_BYTE];
        if (j < a.B) {
            uint32_t word;
            const Fr m = record_element(image + i * RECORD_LDS_PITCH, phase + byte, encoding, pl != 0xFFFFFFFFu, word);
            fr_store_nt(a.W, row, a.Bp, j, m);
            if (pl != 0xFFFFFFFFu) a.plane[(uint64_t)pl * a.Bp + j] = word;
            // the event reset rides on exactly one field of the call: the first of the table
            if (a.event_reset && first_field + f == 0u) record_event_reset(a.event_reset, j);
        }
    }
}

bool launch_import_records(hipStream_t s, const void *in, uint64_t pitch, const uint32_t *windows, uint32_t n_windows, const uint32_t *fields, uint4 *W, uint64_t Bp,
                           uint32_t B, const uint32_t *gate, uint32_t *plane, uint32_t *event_reset) {
    if (!B || !n_windows) return false;
    const RecordImportArgs a{W, Bp, B, (const uint8_t *)in, pitch, windows, fields, gate, plane, event_reset};
    for_grid_y_chunks(n_windows, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(import_records_kernel, dim3((B + RECORD_BLOCK_INSTANCES - 1u) / RECORD_BLOCK_INSTANCES, m), dim3(256), 0, s, a, done);
    });
    return event_reset != nullptr;
}

}  // namespace acvm
