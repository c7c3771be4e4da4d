// kernels_records.hip -- the record import (include/acvm_amd.h acvm_batch_import_device_records): the initial witnesses as one packed record of
// mixed-width fields per instance, at any pitch, any field offset and any base alignment.
//
//  import_records_kernel   a block of 256 threads owns 64 consecutive instances and one window of the record (record_plan.hpp): phase 1 copies
//                          the window's aligned dwords of its 64 records into LDS, phase 2 is import_narrow_im_kernel's second phase -- one
//                          wave per field, lane = instance, the element assembled from LDS (record_decode.hpp), decoded (import_decode.hpp)
//                          and stored as two 1 KiB half rows per wave
//
// A translation unit of its own: the other code objects compile to what they compiled to before this kernel existed.
#include "record_stage.hpp"

namespace acvm {

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
    // ---- phase 1 (record_stage.hpp): the aligned dwords of the window of the block's records into LDS
    record_stage(image, S, a.pitch, win_length, nb, t);
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
            const Fr m = record_element<false>(image + i * RECORD_LDS_PITCH, phase + byte, encoding, pl != 0xFFFFFFFFu, true, word);
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
