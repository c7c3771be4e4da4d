// kernels_records_out.hip -- the record export (include/acvm_amd.h acvm_batch_export_device_records): the witness map as one packed record of
// mixed-width fields per output row, at any pitch, any field offset and any base alignment.
//
//  export_records_kernel   a block of 256 threads owns 64 consecutive output rows and one window of the record (record_out_plan.hpp): phase 0
//                          zeroes the block's image in LDS, phase 1 is one wave per field, lane = row -- the element from where the other exports
//                          take it, encoded (export_encode.hpp) and scattered into the row's image (record_encode.hpp) -- phase 2 stores the
//                          image under the cover rule: a dword whole only where all four bytes are this record's covered bytes, else byte by byte
//
// The write side is not the import kernel run backwards: a store may not touch the neighbouring bytes. No byte of the caller's buffer is loaded.
// A translation unit of its own: the other code objects compile to what they compiled to before this kernel existed.
#include "ops_common.hpp"
#include "kernels.hpp"
#include "export_source.hpp"
#include "record_encode.hpp"
#include "record_out_plan.hpp"

namespace acvm {

static_assert(RECORD_WINDOW_CAP == RECORD_PLAN_WINDOW_CAP, "the kernel (record_decode.hpp) and the window cut (record_out_plan.cpp) agree on the window size");

// The row of an element and the factor it is multiplied with, from where the other exports take them (export_source.hpp): as kernels.hip
// export_generic_element for a generic instance (scaled rows with 1 / scale or 2^256 / scale, by the FIELD's encoding), as export_list_element for
// an instance of the exact path (its column of the side table or its own column, nothing scaled), nothing for a row that names no instance.
// w and encoding are wave-uniform: the table lookups are scalar loads.
struct RecordOutRow {
    uint32_t j;    // the instance; >= B: no instance
    int32_t lane;  // its lane of the exact path, or -1
};
__device__ __forceinline__ bool record_out_source(const RecordExport &a, const RecordOutRow &r, uint32_t w, uint32_t encoding, Fr &row, Fr &factor) {
    const ExportListSource &L = a.src;
    if (r.j >= L.B) return false;
    if (r.lane < 0) {
        uint32_t at, ui;
        export_generic_source(w, a.n_witnesses, a.row_of, a.producer, a.u_index, at, ui);
        if (at == 0xFFFFFFFFu) return false;
        row = fr_load_nt(a.W, at, a.Bp, r.j);
        factor = ui != 0xFFFFFFFFu ? fr_const(encoding == EXPORT_ENC_MONT256_LE ? a.u_m256 : a.u_plain, ui) : export_plain_factor(encoding);
        return true;
    }
    if (!export_lane_assigned(L.assigned_bits, L.n_slow, (uint32_t)r.lane, w, a.n_witnesses)) return false;
    row = fr_load(L.Wx, w, L.Bpx, L.side ? (uint64_t)(uint32_t)r.lane : (uint64_t)r.j);
    factor = export_plain_factor(encoding);
    return true;
}

// blockIdx.x: the 64 output rows, blockIdx.y (+ w0): the window. The LDS image and its bank argument: record_decode.hpp, record_encode.hpp.
__global__ void __launch_bounds__(256) export_records_kernel(const RecordExport a, uint32_t w0) {
    __shared__ uint32_t image[RECORD_LDS_WORDS];
    __shared__ uint32_t cover[RECORD_OUT_BITMAP_WORDS];
    const uint32_t t = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * RECORD_BLOCK_INSTANCES;
    const uint32_t nb = a.n - i0 < RECORD_BLOCK_INSTANCES ? (uint32_t)(a.n - i0) : RECORD_BLOCK_INSTANCES;  // (the grid has no block at or behind n)
    const uint32_t *win = a.windows + (size_t)(w0 + blockIdx.y) * RECORD_OUT_WINDOW_WORDS;
    const uint64_t win_offset = ((uint64_t)win[RECORD_WINDOW_OFFSET_HI] << 32) | win[RECORD_WINDOW_OFFSET_LO];
    const uint32_t win_length = win[RECORD_WINDOW_LENGTH], first_field = win[RECORD_WINDOW_FIRST_FIELD], n_fields = win[RECORD_WINDOW_N_FIELDS];
    // byte address of the window of the block's first record
    const uint64_t S = (uint64_t)(uintptr_t)a.out + i0 * a.pitch + win_offset;
    // ---- phase 0: the image is zero, so that an OR places bytes; the window's cover bitmap beside it
    for (uint32_t x = t; x < RECORD_LDS_WORDS; x += 256u) image[x] = 0u;
    if (t < RECORD_OUT_BITMAP_WORDS) cover[t] = win[RECORD_OUT_WINDOW_BITMAP + t];
    __syncthreads();
    // ---- phase 1: one wave per field, lane = row. Row loads are 1 KiB per half row per wave for the generic instances of a range.
    {
        const uint32_t wave = t >> 6, i = t & 63u;
        const bool active = i < nb;
        RecordOutRow r{0xFFFFFFFFu, -1};
        if (active) {
            r.j = a.src.list ? a.src.list[i0 + i] : a.first + (uint32_t)(i0 + i);
            if (r.j < a.src.B) r.lane = a.src.lane_of[r.j];
        }
        const uint32_t phase = record_phase(S + (uint64_t)i * a.pitch);
        uint32_t *img = image + i * RECORD_LDS_PITCH;
        auto store = [&](uint32_t word, uint32_t v) { img[word] = v; };
        auto or_into = [&](uint32_t word, uint32_t v) { atomicOr(&img[word], v); };  // (another wave's field may own the word's other bytes)
        for (uint32_t f = wave; f < n_fields; f += 4u) {  // (wave-uniform: the field's words are scalar loads)
            const uint32_t *fd = a.fields + (size_t)(first_field + f) * RECORD_OUT_FIELD_WORDS;
            const uint32_t w = fd[RECORD_OUT_FIELD_WITNESS], encoding = fd[RECORD_OUT_FIELD_ENCODING], byte = fd[RECORD_OUT_FIELD_BYTE], kind = fd[RECORD_OUT_FIELD_KIND];
            if (!active) continue;
            const uint32_t size = export_element_size(encoding);
            Fr row = fr_zero(), factor = fr_zero();
            const bool assigned = record_out_source(a, r, w, encoding, row, factor);
            uint4 lo, hi = make_uint4(0u, 0u, 0u, 0u);
            uint32_t mask;
            if (size == 32u) {
                const ExportElement e = export_encode(row, factor, encoding, assigned);
                lo = e.lo;
                hi = e.hi;
                mask = assigned ? 1u : 0u;
            } else {
                const ExportNarrow e = export_encode_narrow(row, factor, size, assigned);
                lo = e.lo;
                mask = e.mask;
            }
            if (kind & RECORD_OUT_KIND_VALUE) record_scatter(phase + byte, size, lo, hi, store, or_into);
            if (kind & RECORD_OUT_KIND_MASK) record_scatter(phase + ((kind >> 8) & 0xFFu), 1u, make_uint4(mask, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u), store, or_into);
        }
    }
    __syncthreads();
    // ---- phase 2: record i leaves as the (phase_i + length + 3) / 4 aligned dwords that hold a byte of its window, consecutive lanes on
    // consecutive dwords: a group of G lanes per record, G the power of two that holds the most dwords a record of this block takes (the
    // import's phase 1). Each dword takes its cover nibble (record_encode.hpp): all ones is one dword store, otherwise every covered byte is a
    // byte store, none is nothing. Neighbouring groups meet in the dword at the joint of two records: each stores its own bytes of it. Stores
    // are nontemporal: somebody else's kernel reads them.
    {
        const uint32_t row_words = ((a.pitch & 3u) ? win_length + 6u : record_phase(S) + win_length + 3u) / 4u;  // 1 .. 65
        const uint32_t shift = row_words > 1u ? 32u - __builtin_clz(row_words - 1u) : 0u;                      // G = 1 << shift >= row_words, at most 128
        const uint32_t total = RECORD_BLOCK_INSTANCES << shift;
        for (uint32_t g = t; g < total; g += 256u) {
            const uint32_t i = g >> shift, k = g & ((1u << shift) - 1u);
            const uint64_t at = S + (uint64_t)i * a.pitch;
            const uint32_t phase = record_phase(at);
            if (i >= nb || k >= (phase + win_length + 3u) / 4u) continue;
            const uint32_t nibble = record_cover_nibble(cover, win_length, phase, k);
            if (nibble == 0u) continue;
            const uint32_t v = image[i * RECORD_LDS_PITCH + k];
            uint8_t *p = (uint8_t *)(uintptr_t)(at - phase + 4u * (uint64_t)k);  // aligned; only covered bytes of it are touched
            if (nibble == 0xFu) __builtin_nontemporal_store(v, (uint32_t *)p);
            else {
#pragma unroll
                for (uint32_t b = 0; b < 4u; b++)
                    if ((nibble >> b) & 1u) __builtin_nontemporal_store((uint8_t)(v >> (8u * b)), p + b);
            }
        }
    }
}

void launch_export_records(hipStream_t s, const RecordExport &x, uint32_t n_windows) {
    if (!x.n || !n_windows) return;
    for_grid_y_chunks(n_windows, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(export_records_kernel, dim3((x.n + RECORD_BLOCK_INSTANCES - 1u) / RECORD_BLOCK_INSTANCES, m), dim3(256), 0, s, x, done);
    });
}

}  // namespace acvm
