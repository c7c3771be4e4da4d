// kernels_foreign.hip -- the Brillig foreign-call round trip for a whole batch, on the device (include/acvm_amd.h acvm_batch_foreign_call_inputs_device,
// acvm_batch_resolve_foreign_calls_device; foreign_store.hpp holds what the host can run of it):
//
//  fc_inputs_max_kernel  one lane per listed row: the row's number of pending values, reduced to the maximum -- one atomic per wave
//  fc_inputs_kernel      one thread per (row, column): the pending inputs of the row's exact lane, encoded like a witness of the export
//  fc_append_kernel      one lane per listed row: one ForeignCallResult appended behind the instance's results of the opcode
//  fc_answers_max_kernel the twin of fc_inputs_max_kernel for per-row answers: the total of each answered row's lengths, reduced to the maximum
//  fc_append_rows_kernel fc_append_kernel with the row's own lengths and a mask of the rows that are answered
//
// Row r of a site's waiting list is exact lane rows[2 r], instance rows[2 r + 1]; the list is ascending in both, so consecutive rows are (mostly)
// consecutive lanes: the loads of pend_desc / pend_vals along t and the stores of the result store along j coalesce like the rows of W. The caller's
// buffer is touched once per element: coalesced when it is witness-major, at the caller's stride when it is instance-major. No LDS, plain vector
// loads and stores: the kernels move 32 bytes per value and are bound by launch latency at any batch a handle holds.
//
// A translation unit of its own: the other code objects compile to what they compiled to before these kernels existed.
#include "ops_common.hpp"
#include "kernels.hpp"
#include "foreign_store.hpp"

namespace acvm {

__global__ void __launch_bounds__(256) fc_inputs_max_kernel(const FcLanes fc, uint64_t n_slow, const uint32_t *__restrict__ rows, uint32_t n_rows, uint32_t *max_values) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    // (no early return: every lane of the wave takes part in the reduction)
    uint32_t total = r < n_rows ? fc_pending_total(fc.pend_desc, fc.pend_desc_words, n_slow, rows[2u * r]) : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)total, off, 64);
        total = other > total ? other : total;
    }
    if ((threadIdx.x & 63u) == 0u && total) atomicMax(max_values, total);
}

__device__ __forceinline__ void fc_narrow_write(uint8_t *p, const uint4 &v, uint32_t size) {
    switch (size) {
        case 1: *p = (uint8_t)v.x; break;
        case 2: *(uint16_t *)p = (uint16_t)v.x; break;
        case 4: *(uint32_t *)p = v.x; break;
        case 8: *(uint2 *)p = make_uint2(v.x, v.y); break;
        default: *(uint4 *)p = v; break;
    }
}

// blockIdx.y + c0 = column. The threads of column 0 also write the row's instance number and its lengths.
__global__ void __launch_bounds__(256) fc_inputs_kernel(const FcLanes fc, uint64_t n_slow, const FcInputsOut o, uint32_t c0) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const uint32_t c = c0 + blockIdx.y;
    if (r >= o.n_rows) return;
    const uint32_t t = o.rows[2u * r];
    if (c == 0u) {
        if (o.instances) o.instances[r] = o.rows[2u * r + 1u];
        if (o.lens) {
            const uint32_t n_in = fc_pending_inputs(fc.pend_desc, fc.pend_desc_words, t);
            for (uint32_t i = 0; i < o.n_inputs; i++) o.lens[(uint64_t)r * o.n_inputs + i] = i < n_in ? fc.pend_desc[(uint64_t)(1u + i) * n_slow + t] : 0u;
        }
    }
    if (c >= o.n_columns || (!o.values && !o.mask)) return;
    uint32_t total = fc_pending_total(fc.pend_desc, fc.pend_desc_words, n_slow, t);
    if (total > fc.pend_vals_cap) total = fc.pend_vals_cap;
    const bool exists = c < total;
    const Fr row = exists ? fr_load(fc.pend_vals, c, n_slow, t) : fr_zero();
    const uint64_t at = export_element_index(o.layout, o.stride, r, c);
    uint32_t mask;
    if (export_enc_is_narrow(o.encoding)) {
        const uint32_t size = export_element_size(o.encoding);
        const ExportNarrow e = export_encode_narrow(row, export_plain_factor(EXPORT_ENC_LE32), size, exists);
        if (o.values) fc_narrow_write(o.values + at * size, e.lo, size);
        mask = e.mask;
    } else {
        const ExportElement e = export_encode(row, export_plain_factor(o.encoding), o.encoding, exists);
        if (o.values) {
            uint4 *p = (uint4 *)(o.values + at * 32u);
            p[0] = e.lo;
            p[1] = e.hi;
        }
        mask = exists ? 1u : 0u;
    }
    if (o.mask) o.mask[at] = (uint8_t)mask;
}

// one lane per row; refused[0] counts the rows whose result did not fit their column (nothing of such a row is written)
__global__ void __launch_bounds__(256) fc_append_kernel(const FcAppend a) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.n_rows) return;
    const uint64_t j = a.rows[2u * r + 1u];
    if (j >= a.Bp) { atomicAdd(a.refused, 1u); return; }
    const FcAnswers ans{(const uint8_t *)a.values, a.encoding, a.layout, a.stride};
    if (!fc_store_append(a.desc, a.vals, a.Bp, j, a.desc_words, a.vals_cap, a.shape, a.shape_total, ans, r)) atomicAdd(a.refused, 1u);
}

// ---- per-row answers: the lengths of array outputs and the answered rows are device columns
__global__ void __launch_bounds__(256) fc_answers_max_kernel(const uint32_t *__restrict__ shape, const uint32_t *__restrict__ lens, const uint8_t *__restrict__ answered,
                                                             uint32_t n_rows, uint32_t *max_values) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const FcRowAnswers ra{lens, answered, 0u};
    // (no early return: every lane of the wave takes part in the reduction)
    uint32_t total = r < n_rows ? fc_row_total_saturated(shape, ra, r) : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)total, off, 64);
        total = other > total ? other : total;
    }
    if ((threadIdx.x & 63u) == 0u && total) atomicMax(max_values, total);
}

// one lane per row; a row that is left out returns at once; refused[0] counts the answered rows whose result did not fit (nothing of them is written)
__global__ void __launch_bounds__(256) fc_append_rows_kernel(const FcAppendRows ar) {
    const FcAppend &a = ar.a;
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.n_rows) return;
    const FcRowAnswers ra{ar.lens, ar.answered, ar.n_columns};
    if (!fc_row_answered(ra, r)) return;
    const uint64_t j = a.rows[2u * r + 1u];
    if (j >= a.Bp) { atomicAdd(a.refused, 1u); return; }
    const FcAnswers ans{(const uint8_t *)a.values, a.encoding, a.layout, a.stride};
    if (fc_store_append_row(a.desc, a.vals, a.Bp, j, a.desc_words, a.vals_cap, a.shape, ra, ans, r) == FC_ROW_REFUSED) atomicAdd(a.refused, 1u);
}

void launch_fc_inputs_max(hipStream_t s, const FcLanes &fc, uint32_t n_slow, const uint32_t *rows, uint32_t n_rows, uint32_t *max_values) {
    if (!n_rows) return;
    hipLaunchKernelGGL(fc_inputs_max_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, s, fc, (uint64_t)n_slow, rows, n_rows, max_values);
}
void launch_fc_inputs(hipStream_t s, const FcLanes &fc, uint32_t n_slow, const FcInputsOut &o) {
    if (!o.n_rows) return;
    const uint32_t n_y = (o.values || o.mask) && o.n_columns ? o.n_columns : 1u;
    for_grid_y_chunks(n_y, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(fc_inputs_kernel, dim3((o.n_rows + 255u) / 256u, m), dim3(256), 0, s, fc, (uint64_t)n_slow, o, done); });
}
void launch_fc_append(hipStream_t s, const FcAppend &a) {
    if (!a.n_rows) return;
    hipLaunchKernelGGL(fc_append_kernel, dim3((a.n_rows + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_fc_answers_max(hipStream_t s, const uint32_t *shape, const uint32_t *lens, const uint8_t *answered, uint32_t n_rows, uint32_t *max_values) {
    if (!n_rows) return;
    hipLaunchKernelGGL(fc_answers_max_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, s, shape, lens, answered, n_rows, max_values);
}
void launch_fc_append_rows(hipStream_t s, const FcAppendRows &ar) {
    if (!ar.a.n_rows) return;
    hipLaunchKernelGGL(fc_append_rows_kernel, dim3((ar.a.n_rows + 255u) / 256u), dim3(256), 0, s, ar);
}

}  // namespace acvm
