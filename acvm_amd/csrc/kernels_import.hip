// kernels_import.hip -- the device-resident witness import (include/acvm_amd.h acvm_batch_import_device): ACVM::new's initial WitnessMap
// (pwg/mod.rs:146-156) read from a caller's device buffer in any encoding, layout, stride and column list of the device export.
//
//  import_device_wm_kernel   witness-major source: streaming, lane = instance, no LDS
//  import_device_im_kernel   instance-major source: 64 instances x 4 inputs transposed through LDS, like kernels.hip import_witness_kernel
//
// A translation unit of its own: kernels.hip -- import_witness_kernel, which the plain descriptor and the two older entry points keep, and the
// level kernels of the headline -- compiles to the code object it compiled to before these kernels existed.
#include "ops_common.hpp"
#include "kernels.hpp"
#include "import_decode.hpp"

namespace acvm {

// ------------------------------------------------------------------------------------------ import from a caller's device buffer
// acvm_batch_import_device (include/acvm_amd.h): the mirror image of the device export (kernels.hip export_device_*_kernel) -- big-endian, little-endian limbs or Montgomery-256,
// instance-major or witness-major, a stride, a column per input (import_decode.hpp; element (i, c) lies at export_element_index). Both kernels
// leave what import_witness_kernel leaves: the Montgomery rows, the byte-plane words, the event words "nobody flagged"; gate as there.
struct ImportArgs {
    uint4 *W;
    uint64_t Bp;
    uint32_t B, n_in;
    const uint4 *in;          // 16-byte aligned
    const uint32_t *ids;      // rows of the inputs
    const uint32_t *columns;  // per input the column of `in` that holds it; null: input k is column k
    uint32_t encoding;
    uint64_t stride;          // in elements, >= the layout's dense stride
    const uint32_t *gate, *plane_of_input;
    uint32_t *plane, *event_reset;
};
__device__ __forceinline__ uint4 import_load_nt(const uint4 *p) {
    const fr_u32x4 x = __builtin_nontemporal_load((const fr_u32x4 *)p);  // read once
    return make_uint4(x[0], x[1], x[2], x[3]);
}
// One element: the row, and the plane word where the input has a plane (want_plane). A Montgomery-256 element without a plane needs no canonical
// value: one product from the limbs as read. Every lane of the wave that is still active must call this (the ballot): when all of them hold
// bytes -- message bytes, digits, flags -- the row comes from the closed form of ops_common.hpp fr_mont_of_byte instead of a product.
__device__ __forceinline__ Fr import_element(const uint4 &lo, const uint4 &hi, uint32_t encoding, bool want_plane, uint32_t &plane_word) {
    const Fr m = import_limbs(lo, hi, encoding);
    const bool have_canonical = encoding != EXPORT_ENC_MONT256_LE || want_plane;
    Fr x = m;
    if (have_canonical) x = import_canonical(m, encoding);
    const bool is_byte = have_canonical && import_is_byte(x);
    plane_word = (x.v[0] & 0x1fffffffu) | (is_byte ? 0x80000000u : 0u);  // (meaningless without a canonical value: nobody stores it then)
    if (__builtin_amdgcn_ballot_w64(!is_byte) == 0) return fr_mont_of_byte(x.v[0]);
    return import_row(m, x, encoding);
}
// ACVM::new: nobody has left the generic path yet (import_witness_kernel: the import leaves the event words ready for its solve)
__device__ __forceinline__ void import_event_reset(uint32_t *event_reset, uint64_t j) {
    event_reset[j] = 0xFFFFFFFFu;
    if (j == 0) { event_reset[-4] = 0u; event_reset[-3] = 0u; }
}
// witness-major source: lane = instance, blockIdx.y = input. The table is witness-major too, so this is a pure streaming kernel: two 16-byte
// nontemporal loads per lane (a wave reads 2 KiB contiguous), two 16-byte nontemporal stores (1 KiB per half row), no LDS. The column, the row,
// the plane and the encoding are wave-uniform.
__global__ void __launch_bounds__(256) import_device_wm_kernel(const ImportArgs a, uint32_t k0) {
    if (a.gate && *a.gate != 0u) return;  // (block-uniform)
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t k = k0 + blockIdx.y;
    if (j >= a.B) return;
    const uint32_t c = a.columns ? a.columns[k] : k;
    const uint32_t pl = a.plane_of_input ? a.plane_of_input[k] : 0xFFFFFFFFu;
    const uint64_t at = export_element_index(EXPORT_WITNESS_MAJOR, a.stride, j, c);
    const uint4 lo = import_load_nt(a.in + 2 * at), hi = import_load_nt(a.in + 2 * at + 1);
    uint32_t word;
    const Fr m = import_element(lo, hi, a.encoding, pl != 0xFFFFFFFFu, word);
    fr_store_nt(a.W, a.ids[k], a.Bp, j, m);
    if (pl != 0xFFFFFFFFu) a.plane[(uint64_t)pl * a.Bp + j] = word;
    if (a.event_reset && k == 0) import_event_reset(a.event_reset, j);
}
// instance-major source: transposed through LDS like import_witness_kernel -- a block converts 64 instances x 4 inputs, rows of 65 units; phase 1
// has four lanes on the four inputs of an instance, phase 2 one wave per input with lane = instance (1 KiB contiguous per half row).
// The four inputs of a group need not be adjacent columns. Adjacent, they are 128 contiguous bytes per instance: a wave's 16 instances touch 16
// lines of 128 bytes, each used whole. Under a column list that scatters them, every lane fetches its own 32 bytes from a line of its own: up to
// 64 lines per wave for the same 2 KiB, a quarter of each used -- the other inputs of the instance that share those lines are fetched again by the
// blocks of their groups (from the L2 at best). A caller who controls the producer lists adjacent columns or hands over witness-major.
__global__ void __launch_bounds__(256) import_device_im_kernel(const ImportArgs a, uint32_t g0) {
    __shared__ uint4 tile[4][2][65];
    __shared__ uint32_t tile_low[4][64];
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
            const uint32_t pl = a.plane_of_input ? a.plane_of_input[k] : 0xFFFFFFFFu;
            const uint64_t at = export_element_index(EXPORT_INSTANCE_MAJOR, a.stride, j, c);
            const uint4 lo = import_load_nt(a.in + 2 * at), hi = import_load_nt(a.in + 2 * at + 1);
            uint32_t word;
            const Fr m = import_element(lo, hi, a.encoding, pl != 0xFFFFFFFFu, word);
            tile_low[kk][ji] = word;
            tile[kk][0][ji] = make_uint4(m.v[0], m.v[1], m.v[2], m.v[3]);
            tile[kk][1][ji] = make_uint4(m.v[4], m.v[5], m.v[6], m.v[7]);
        }
    }
    __syncthreads();
    {
        const uint32_t kk = t >> 6, ji = t & 63u;
        const uint64_t j = j0 + ji;
        const uint32_t k = k0 + kk;
        if (j < a.B && k < a.n_in) {
            const uint4 lo = tile[kk][0][ji], hi = tile[kk][1][ji];
            const Fr m = {{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
            fr_store_nt(a.W, a.ids[k], a.Bp, j, m);
            if (a.plane_of_input) {  // (block-uniform per kk: a scalar load)
                const uint32_t pl = a.plane_of_input[k];
                if (pl != 0xFFFFFFFFu) a.plane[(uint64_t)pl * a.Bp + j] = tile_low[kk][ji];
            }
            if (a.event_reset && k == 0) import_event_reset(a.event_reset, j);
        }
    }
}

bool launch_import_device(hipStream_t s, const ImportDevice &x, uint4 *W, uint64_t Bp, uint32_t B, const uint32_t *ids, uint32_t n_in, const uint32_t *gate,
                          const uint32_t *plane_of_input, uint32_t *plane, uint32_t *event_reset) {
    if (!B || !n_in) return false;
    const ImportArgs a{W, Bp, B, n_in, (const uint4 *)x.in, ids, x.columns, x.encoding, x.stride, gate, plane_of_input, plane, event_reset};
    if (x.layout == EXPORT_WITNESS_MAJOR)
        for_grid_y_chunks(n_in, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(import_device_wm_kernel, dim3((B + 255u) / 256u, m), dim3(256), 0, s, a, done); });
    else
        for_grid_y_chunks((n_in + 3u) / 4u, [&](uint32_t done, uint32_t m) { hipLaunchKernelGGL(import_device_im_kernel, dim3((B + 63u) / 64u, m), dim3(256), 0, s, a, done); });
    return event_reset != nullptr;
}

}  // namespace acvm
