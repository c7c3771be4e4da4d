// kernels_typed_io.hip -- device I/O in the element's own width (include/acvm_amd.h ACVM_ENC_U8 .. ACVM_ENC_U128, ACVM_LAYOUT_BROADCAST):
//
//  import_narrow_wm_kernel      witness-major source: streaming, lane = instance, one natural-width load per lane
//  import_narrow_im_kernel      instance-major source: 64 instances x 4 inputs transposed through LDS (the VALUES: 16 bytes per element)
//  import_broadcast_kernel      one element for every instance, any encoding: a wave-uniform value stored to every lane's row
//  export_narrow_direct_kernel  witness-major (and short lists): lane = instance, a wave writes 64 x size contiguous bytes
//  export_narrow_im_kernel      instance-major: 64 instances x T positions transposed through LDS, a wave writes runs of T x size bytes
//  export_narrow_lanes_kernel   the instances of the exact path over their elements
//
// A translation unit of its own: kernels.hip and kernels_import.hip compile to the code objects they compiled to before these kernels existed.
#include "ops_common.hpp"
#include "kernels.hpp"
#include "import_decode.hpp"
#include "export_source.hpp"

namespace acvm {

// ------------------------------------------------------------------------------------------ import
struct TypedImportArgs {
    uint4 *W;
    uint64_t Bp;
    uint32_t B, n_in;
    const uint8_t *in;        // aligned to the element size
    const uint32_t *ids;      // rows of the inputs
    const uint32_t *columns;  // per input the column of `in` that holds it; null: input k is column k
    uint32_t encoding, size;
    uint64_t stride;          // in elements
    const uint32_t *gate, *plane_of_input;
    uint32_t *plane, *event_reset;
};
// ACVM::new: nobody has left the generic path yet (kernels_import.hip import_event_reset)
__device__ __forceinline__ void typed_event_reset(uint32_t *event_reset, uint64_t j) {
    event_reset[j] = 0xFFFFFFFFu;
    if (j == 0) { event_reset[-4] = 0u; event_reset[-3] = 0u; }
}
// One narrow element: the row and the plane word. U8 needs no ballot -- every element is a byte -- and takes the closed form; the wider ones
// take it when the whole wave holds bytes (every lane still active must call this), else the product with R^2.
__device__ __forceinline__ Fr typed_narrow_row(const uint4 &lo, uint32_t size, uint32_t &plane_word) {
    const Fr x = import_narrow_limbs(lo);
    if (size == 1u) {
        plane_word = lo.x | 0x80000000u;
        return fr_mont_of_byte(lo.x);
    }
    plane_word = import_plane_word(x);
    if (__builtin_amdgcn_ballot_w64(!import_is_byte(x)) == 0) return fr_mont_of_byte(lo.x);
    return fr_mul(x, import_r522());
}
__device__ __forceinline__ void typed_store(const TypedImportArgs &a, uint32_t k, uint64_t j, const Fr &row, uint32_t word) {
    fr_store_nt(a.W, a.ids[k], a.Bp, j, row);
    if (a.plane_of_input) {  // (wave-uniform per k: a scalar load)
        const uint32_t pl = a.plane_of_input[k];
        if (pl != 0xFFFFFFFFu) a.plane[(uint64_t)pl * a.Bp + j] = word;
    }
    if (a.event_reset && k == 0) typed_event_reset(a.event_reset, j);
}
// witness-major source: lane = instance, blockIdx.y = input. A wave reads 64 x size contiguous bytes and stores two 1 KiB half rows.
__global__ void __launch_bounds__(256) import_narrow_wm_kernel(const TypedImportArgs a, uint32_t k0) {
    if (a.gate && *a.gate != 0u) return;  // (block-uniform)
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t k = k0 + blockIdx.y;
    if (j >= a.B) return;
    const uint32_t c = a.columns ? a.columns[k] : k;
    const uint4 lo = import_narrow_read(a.in + export_element_offset(EXPORT_WITNESS_MAJOR, a.stride, j, c, a.size), a.size);
    uint32_t word;
    const Fr row = typed_narrow_row(lo, a.size, word);
    typed_store(a, k, j, row, word);
}
// instance-major source: a block converts 64 instances x 4 inputs. Phase 1 has four lanes on the four inputs of an instance (adjacent columns:
// 4 x size contiguous bytes per instance) and leaves the VALUES in LDS, rows of 65 units; phase 2 is the witness-major kernel's body: one wave
// per input, lane = instance, 1 KiB contiguous per half row.
__global__ void __launch_bounds__(256) import_narrow_im_kernel(const TypedImportArgs a, uint32_t g0) {
    __shared__ uint4 tile[4][65];
    if (a.gate && *a.gate != 0u) return;  // (block-uniform)
    const uint32_t t = threadIdx.x;
    const uint64_t j0 = (uint64_t)blockIdx.x * 64u;
    const uint32_t k0 = (g0 + blockIdx.y) * 4u;
    {
        const uint32_t ji = t >> 2, kk = t & 3u;
        const uint64_t j = j0 + ji;
        const uint32_t k = k0 + kk;
        if (j < a.B && k < a.n_in) {
            const uint32_t c = a.columns ? a.columns[k] : k;
            tile[kk][ji] = import_narrow_read(a.in + export_element_offset(EXPORT_INSTANCE_MAJOR, a.stride, j, c, a.size), a.size);
        }
    }
    __syncthreads();
    {
        const uint32_t kk = t >> 6, ji = t & 63u;
        const uint64_t j = j0 + ji;
        const uint32_t k = k0 + kk;
        if (j < a.B && k < a.n_in) {
            uint32_t word;
            const Fr row = typed_narrow_row(tile[kk][ji], a.size, word);
            typed_store(a, k, j, row, word);
        }
    }
}
// broadcast: element c lies at c * size and is the value of every instance. Every lane reads the same address (one request per wave) and the
// decoding is wave-uniform; any encoding.
__global__ void __launch_bounds__(256) import_broadcast_kernel(const TypedImportArgs a, uint32_t k0) {
    if (a.gate && *a.gate != 0u) return;  // (block-uniform)
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t k = k0 + blockIdx.y;
    if (j >= a.B) return;
    const uint32_t c = a.columns ? a.columns[k] : k;
    const uint8_t *p = a.in + (uint64_t)c * a.size;
    Fr row;
    uint32_t word;
    if (a.size == 32u) {
        const uint4 lo = *(const uint4 *)p, hi = *(const uint4 *)(p + 16);
        const Fr m = import_limbs(lo, hi, a.encoding);
        const Fr x = import_canonical(m, a.encoding);
        row = import_row(m, x, a.encoding);
        word = import_plane_word(x);
    } else {
        row = typed_narrow_row(import_narrow_read(p, a.size), a.size, word);
    }
    typed_store(a, k, j, row, word);
}

bool launch_import_typed(hipStream_t s, const ImportDevice &x, uint4 *W, uint64_t Bp, uint32_t B, const uint32_t *ids, uint32_t n_in, const uint32_t *gate,
                         const uint32_t *plane_of_input, uint32_t *plane, uint32_t *event_reset) {
    if (!B || !n_in) return false;
    const TypedImportArgs a{W, Bp, B, n_in, (const uint8_t *)x.in, ids, x.columns, x.encoding, export_element_size(x.encoding), x.stride, gate, plane_of_input, plane, event_reset};
    if (x.layout == EXPORT_INSTANCE_MAJOR)
        for_grid_y_chunks((n_in + 3u) / 4u, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(import_narrow_im_kernel, dim3((B + 63u) / 64u, m), dim3(256), 0, s, a, done); });
    else if (x.layout == EXPORT_LAYOUT_BROADCAST)
        for_grid_y_chunks(n_in, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(import_broadcast_kernel, dim3((B + 255u) / 256u, m), dim3(256), 0, s, a, done); });
    else
        for_grid_y_chunks(n_in, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(import_narrow_wm_kernel, dim3((B + 255u) / 256u, m), dim3(256), 0, s, a, done); });
    return event_reset != nullptr;
}

// ------------------------------------------------------------------------------------------ export
struct NarrowExportArgs {
    const uint4 *W;
    uint64_t Bp;
    uint32_t first, n;            // instances [first, first + n)
    const uint32_t *sel;          // the witness list; null: position k is witness k
    uint32_t n_sel, n_witnesses;  // a listed index >= n_witnesses is unassigned
    const uint32_t *row_of, *producer;
    const uint32_t *u_index, *u_factor;  // scaled witnesses: 1 / scale as canonical integers (Unscale::consts_plain)
    uint32_t size;
    uint64_t stride;
    uint8_t *out;
    uint8_t *mask;  // may be null
};
// the element's `size` bytes to p (aligned to size): one store of the natural width
__device__ __forceinline__ void narrow_write(uint8_t *p, const uint4 &v, uint32_t size) {
    switch (size) {
        case 1: *p = (uint8_t)v.x; break;
        case 2: *(uint16_t *)p = (uint16_t)v.x; break;
        case 4: *(uint32_t *)p = v.x; break;
        case 8: *(uint2 *)p = make_uint2(v.x, v.y); break;
        default: *(uint4 *)p = v; break;
    }
}
// element of generic instance j at list position k (k is wave-uniform: the table lookups are scalar loads): kernels.hip export_generic_element
__device__ __forceinline__ ExportNarrow narrow_generic_element(const NarrowExportArgs &a, uint32_t k, uint64_t j) {
    const uint32_t w = a.sel ? a.sel[k] : k;
    uint32_t row, ui;
    export_generic_source(w, a.n_witnesses, a.row_of, a.producer, a.u_index, row, ui);
    if (row == 0xFFFFFFFFu) return export_encode_narrow(fr_zero(), fr_zero(), a.size, false);
    return export_encode_narrow(fr_load_nt(a.W, row, a.Bp, j), ui != 0xFFFFFFFFu ? fr_const(a.u_factor, ui) : export_plain_factor(EXPORT_ENC_LE32), a.size, true);
}
// direct: lane = instance, blockIdx.y = list position. Witness-major, a wave reads 1 KiB per half row and writes 64 x size contiguous bytes.
// Also the instance-major kernel of a list shorter than the tiled kernel's four waves.
__global__ void __launch_bounds__(256) export_narrow_direct_kernel(const NarrowExportArgs a, uint32_t layout, uint32_t k0) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t k = k0 + blockIdx.y;
    if (i >= a.n) return;
    const ExportNarrow e = narrow_generic_element(a, k, a.first + i);
    const uint64_t at = export_element_index(layout, a.stride, i, k);
    narrow_write(a.out + at * a.size, e.lo, a.size);
    if (a.mask) a.mask[at] = (uint8_t)e.mask;
}
// instance-major: block (bx, by) owns instances [64 bx, 64 bx + 64) x list positions [T by, T by + T). Phase 1: wave v computes positions
// v, v + 4, ... with lane = instance (coalesced row loads) and writes the element into the LDS image of the instance's run -- pitch T x size
// + pad bytes, pad = max(size, 4): consecutive lanes fall on different banks. Phase 2: the tile leaves as 64 runs of T consecutive elements,
// consecutive lanes on consecutive elements of a run: no one-byte stores scattered at a stride. The mask bytes take the same way.
__global__ void __launch_bounds__(256) export_narrow_im_kernel(const NarrowExportArgs a, uint32_t T, uint32_t k0) {
    extern __shared__ uint4 narrow_tile[];  // 64 x pitch bytes of elements, then 64 x (T + 4) mask bytes
    uint8_t *tile = (uint8_t *)narrow_tile;
    const uint32_t size = a.size, pitch = T * size + (size > 4u ? size : 4u), mpitch = T + 4u;
    uint8_t *tile_mask = tile + 64u * pitch;
    const uint32_t t = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * 64u;
    const uint32_t kb = k0 + blockIdx.y * T;
    {
        const uint32_t ji = t & 63u;
        const uint64_t i = i0 + ji;
#pragma unroll 1
        for (uint32_t kk = t >> 6; kk < T; kk += 4u) {
            const uint32_t k = kb + kk;
            if (k >= a.n_sel || i >= a.n) continue;
            const ExportNarrow e = narrow_generic_element(a, k, a.first + i);
            narrow_write(tile + ji * pitch + kk * size, e.lo, size);
            tile_mask[ji * mpitch + kk] = (uint8_t)e.mask;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t g = t; g < 64u * T; g += 256u) {
        const uint32_t ji = g / T, kk = g % T;
        const uint64_t i = i0 + ji;
        const uint32_t k = kb + kk;
        if (i >= a.n || k >= a.n_sel) continue;
        const uint64_t at = export_element_index(EXPORT_INSTANCE_MAJOR, a.stride, i, k);
        narrow_write(a.out + at * size, import_narrow_read(tile + ji * pitch + kk * size, size), size);
        if (a.mask) a.mask[at] = tile_mask[ji * mpitch + kk];
    }
}
// The instances of the exact path among [first, first + n) (kernels.hip export_device_lanes_kernel): one thread per element
__global__ void __launch_bounds__(256) export_narrow_lanes_kernel(const NarrowExportArgs a, const uint32_t *__restrict__ lanes, uint32_t n_lanes, bool side,
                                                                  const uint32_t *__restrict__ assigned_bits, uint32_t n_slow, uint32_t layout, uint32_t k0) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t k = k0 + blockIdx.y;
    if (x >= n_lanes) return;
    const uint32_t t = lanes[2 * x], i = lanes[2 * x + 1];
    const uint32_t w = a.sel ? a.sel[k] : k;
    const bool assigned = export_lane_assigned(assigned_bits, n_slow, t, w, a.n_witnesses);
    ExportNarrow e;
    if (assigned) e = export_encode_narrow(fr_load(a.W, w, a.Bp, side ? (uint64_t)t : (uint64_t)a.first + i), export_plain_factor(EXPORT_ENC_LE32), a.size, true);
    else e = export_encode_narrow(fr_zero(), fr_zero(), a.size, false);
    const uint64_t at = export_element_index(layout, a.stride, i, k);
    narrow_write(a.out + at * a.size, e.lo, a.size);
    if (a.mask) a.mask[at] = (uint8_t)e.mask;
}
// acvm_batch_export_device_list in the narrow encodings (kernels.hip export_list_*_kernel): the instance of output row i comes from the list,
// and the lane decides how it is read -- no instance, an instance of the exact path, a generic one
__device__ __forceinline__ ExportNarrow narrow_list_element(const NarrowExportArgs &a, const ExportListSource &L, uint32_t k, uint32_t j, int32_t lane) {
    if (j >= L.B) return export_encode_narrow(fr_zero(), fr_zero(), a.size, false);
    if (lane < 0) return narrow_generic_element(a, k, j);
    const uint32_t w = a.sel ? a.sel[k] : k;
    const bool assigned = export_lane_assigned(L.assigned_bits, L.n_slow, (uint32_t)lane, w, a.n_witnesses);
    if (!assigned) return export_encode_narrow(fr_zero(), fr_zero(), a.size, false);
    return export_encode_narrow(fr_load(L.Wx, w, L.Bpx, L.side ? (uint64_t)(uint32_t)lane : (uint64_t)j), export_plain_factor(EXPORT_ENC_LE32), a.size, true);
}
__global__ void __launch_bounds__(256) export_narrow_list_direct_kernel(const NarrowExportArgs a, const ExportListSource L, uint32_t layout, uint32_t k0) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t k = k0 + blockIdx.y;
    if (i >= a.n) return;
    const uint32_t j = L.list[i];
    const ExportNarrow e = narrow_list_element(a, L, k, j, j < L.B ? L.lane_of[j] : -1);
    const uint64_t at = export_element_index(layout, a.stride, i, k);
    narrow_write(a.out + at * a.size, e.lo, a.size);
    if (a.mask) a.mask[at] = (uint8_t)e.mask;
}
// (export_narrow_im_kernel with the source column of each tile lane taken from the list)
__global__ void __launch_bounds__(256) export_narrow_list_im_kernel(const NarrowExportArgs a, const ExportListSource L, uint32_t T, uint32_t k0) {
    extern __shared__ uint4 narrow_list_tile[];  // 64 x pitch bytes of elements, then 64 x (T + 4) mask bytes
    uint8_t *tile = (uint8_t *)narrow_list_tile;
    const uint32_t size = a.size, pitch = T * size + (size > 4u ? size : 4u), mpitch = T + 4u;
    uint8_t *tile_mask = tile + 64u * pitch;
    const uint32_t t = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * 64u;
    const uint32_t kb = k0 + blockIdx.y * T;
    {
        const uint32_t ji = t & 63u;
        const uint64_t i = i0 + ji;
        const uint32_t j = i < a.n ? L.list[i] : 0xFFFFFFFFu;
        const int32_t lane = j < L.B ? L.lane_of[j] : -1;
#pragma unroll 1
        for (uint32_t kk = t >> 6; kk < T; kk += 4u) {
            const uint32_t k = kb + kk;
            if (k >= a.n_sel || i >= a.n) continue;
            const ExportNarrow e = narrow_list_element(a, L, k, j, lane);
            narrow_write(tile + ji * pitch + kk * size, e.lo, size);
            tile_mask[ji * mpitch + kk] = (uint8_t)e.mask;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t g = t; g < 64u * T; g += 256u) {
        const uint32_t ji = g / T, kk = g % T;
        const uint64_t i = i0 + ji;
        const uint32_t k = kb + kk;
        if (i >= a.n || k >= a.n_sel) continue;
        const uint64_t at = export_element_index(EXPORT_INSTANCE_MAJOR, a.stride, i, k);
        narrow_write(a.out + at * size, import_narrow_read(tile + ji * pitch + kk * size, size), size);
        if (a.mask) a.mask[at] = tile_mask[ji * mpitch + kk];
    }
}

// positions per tile of the instance-major kernel: runs of 64 elements up to 4 bytes wide (64 .. 256 bytes), of 16 for the wider ones (128 / 256 bytes)
static uint32_t narrow_tile_positions(uint32_t size) { return size <= 4u ? 64u : 16u; }
// LDS of one tile of either instance-major kernel (range or list): 64 runs of T elements at the padded pitch, then 64 x (T + 4) mask bytes
static uint32_t narrow_tile_lds_bytes(uint32_t T, uint32_t size) { return 64u * (T * size + (size > 4u ? size : 4u)) + 64u * (T + 4u); }

void launch_export_narrow(hipStream_t s, const ExportDevice &x, const uint4 *W, uint64_t Bp, const uint32_t *row_of, const uint32_t *producer, const Unscale &u) {
    if (!x.n || !x.n_sel) return;
    const uint32_t size = export_element_size(x.encoding);
    const NarrowExportArgs a{W, Bp, x.first, x.n, x.sel, x.n_sel, x.n_witnesses, row_of, producer, u.index, u.consts_plain, size, x.stride, (uint8_t *)x.out, x.mask};
    if (x.layout == EXPORT_WITNESS_MAJOR || x.n_sel < 4u) {
        for_grid_y_chunks(x.n_sel, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(export_narrow_direct_kernel, dim3((x.n + 255u) / 256u, m), dim3(256), 0, s, a, x.layout, done); });
        return;
    }
    const uint32_t T = narrow_tile_positions(size), tiles = (x.n_sel + T - 1u) / T;
    const uint32_t lds = narrow_tile_lds_bytes(T, size);  // 8.5 KiB (U8) .. 20.5 KiB (U32)
    for_grid_y_chunks(tiles, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(export_narrow_im_kernel, dim3((x.n + 63u) / 64u, m), dim3(256), lds, s, a, T, done * T); });
}
void launch_export_narrow_list(hipStream_t s, const ExportDevice &x, const uint4 *W, uint64_t Bp, const uint32_t *row_of, const uint32_t *producer, const Unscale &u,
                               const ExportListSource &src) {
    if (!x.n || !x.n_sel) return;
    const uint32_t size = export_element_size(x.encoding);
    const NarrowExportArgs a{W, Bp, 0u, x.n, x.sel, x.n_sel, x.n_witnesses, row_of, producer, u.index, u.consts_plain, size, x.stride, (uint8_t *)x.out, x.mask};
    if (x.layout == EXPORT_WITNESS_MAJOR || x.n_sel < 4u) {
        for_grid_y_chunks(x.n_sel, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(export_narrow_list_direct_kernel, dim3((x.n + 255u) / 256u, m), dim3(256), 0, s, a, src, x.layout, done); });
        return;
    }
    const uint32_t T = narrow_tile_positions(size), tiles = (x.n_sel + T - 1u) / T;
    const uint32_t lds = narrow_tile_lds_bytes(T, size);
    for_grid_y_chunks(tiles, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(export_narrow_list_im_kernel, dim3((x.n + 63u) / 64u, m), dim3(256), lds, s, a, src, T, done * T); });
}
void launch_export_narrow_lanes(hipStream_t s, const ExportDevice &x, const uint4 *W, uint64_t Bp, bool side, const uint32_t *lanes, uint32_t n_lanes,
                                const uint32_t *assigned_bits, uint32_t n_slow) {
    if (!n_lanes || !x.n_sel) return;
    const NarrowExportArgs a{W, Bp, x.first, x.n, x.sel, x.n_sel, x.n_witnesses, nullptr, nullptr, nullptr, nullptr, export_element_size(x.encoding), x.stride, (uint8_t *)x.out, x.mask};
    for_grid_y_chunks(x.n_sel, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(export_narrow_lanes_kernel, dim3((n_lanes + 255u) / 256u, m), dim3(256), 0, s, a, lanes, n_lanes, side, assigned_bits, n_slow, x.layout, done);
    });
}

}  // namespace acvm
