// kernels_wire_pack.hip -- packed wire buffers (include/acvm_amd.h acvm_batch_witness_maps_wire_packed_device,
// acvm_batch_import_device_wire_packed): the rows of the batch-wide WitnessMap wire format between the pitched slots the wire kernels write
// and read and a packed buffer with an offsets column. The arithmetic is wire_repitch.hpp's, whose header states what is stored and loaded.
//
//  wire_scan_kernel      ONE block per chunk of rows: the 64-bit exclusive scan of the chunk's lengths into its offsets, continued from the
//                        base the chunk before left in a device word (launches of one stream follow each other: no block waits on another,
//                        no host round trip), and the count of rows that end at or in front of the capacity. A chunk is bounded by the staging
//                        arena, so one block is enough.
//  wire_repitch_kernel   one lane per destination unit of 16 bytes, lanes of a wave on consecutive units of a row: the grid is rows x units
//                        of the longest row there can be, both host-known; a unit beyond its row's length exits. Packs (pitched -> packed)
//                        and unpacks (packed -> pitched) at any byte alignment of either side.
//  wire_offsets_kernel   one lane per row of an untrusted offsets column: its finding, its length, the count of findings and the smallest
//                        (instance, class) -- in words of the call's own, as kernels_wire_in.hip keeps them.
//
// A translation unit of its own: the other code objects compile to what they compiled to before.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "kernels.hpp"
#include "wire_repitch.hpp"

namespace acvm {

struct RepitchMem {
    const uint8_t *src;
    uint8_t *dst;
    __device__ __forceinline__ Unit16 load16(uint64_t off) const {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 v = __builtin_nontemporal_load((const u32x4 *)(src + off));  // read once
        return Unit16{{v.x, v.y, v.z, v.w}};
    }
    __device__ __forceinline__ uint32_t load8(uint64_t off) const { return src[off]; }
    __device__ __forceinline__ void store16(uint64_t off, const Unit16 &u) const { *(uint4 *)(dst + off) = make_uint4(u.w[0], u.w[1], u.w[2], u.w[3]); }
    __device__ __forceinline__ void store8(uint64_t off, uint32_t b) const { dst[off] = (uint8_t)b; }
};

constexpr uint32_t REPITCH_THREADS = 256;

// row0: the first row of this launch (the launcher cuts a call whose grid would not fit one launch)
__global__ void __launch_bounds__(REPITCH_THREADS) wire_repitch_kernel(const WireRepitch a, uint32_t row0, uint32_t rows) {
    const uint64_t g = (uint64_t)blockIdx.x * REPITCH_THREADS + threadIdx.x;
    const uint64_t i = g / a.units_per_row, u = g % a.units_per_row;
    if (i >= rows) return;
    const RepitchRow r = wire_repitch_row(a, row0 + i);
    wire_repitch_unit(RepitchMem{a.src, a.dst}, a, r, u);
}

__global__ void __launch_bounds__(REPITCH_SCAN_THREADS) wire_scan_kernel(const uint64_t *lengths, uint32_t m, uint64_t *offsets, uint64_t capacity, uint64_t *state) {
    __shared__ uint64_t sums[2][REPITCH_SCAN_THREADS];
    __shared__ uint64_t carry;
    __shared__ uint32_t fit;
    const uint32_t t = threadIdx.x;
    if (t == 0u) {
        carry = state[REPITCH_STATE_BASE];
        fit = 0u;
        offsets[0] = carry;  // (what the chunk before wrote there; 0 for the first)
    }
    __syncthreads();
    for (uint64_t tile0 = 0; tile0 < m; tile0 += REPITCH_SCAN_TILE) {
        const uint64_t mine = wire_scan_thread_sum(lengths, m, tile0, t);
        sums[0][t] = mine;
        __syncthreads();
        uint32_t cur = 0u;
        for (uint32_t d = 1u; d < REPITCH_SCAN_THREADS; d <<= 1, cur ^= 1u) {
            sums[cur ^ 1u][t] = wire_scan_step(sums[cur], t, d);
            __syncthreads();
        }
        const uint64_t inclusive = sums[cur][t];
        const uint32_t n_fit = wire_scan_thread_emit(lengths, m, tile0, t, carry + inclusive - mine, capacity, offsets);
        if (n_fit) atomicAdd(&fit, n_fit);  // (LDS)
        __syncthreads();
        if (t == REPITCH_SCAN_THREADS - 1u) carry += inclusive;
        __syncthreads();
    }
    if (t == 0u) {
        state[REPITCH_STATE_BASE] = carry;
        state[REPITCH_STATE_FIT] += fit;
    }
}

__global__ void __launch_bounds__(256) wire_offsets_kernel(const uint64_t *offsets, uint32_t n, uint64_t n_bytes, uint64_t longest, uint64_t *lengths, uint32_t *findings, uint64_t *result) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint64_t lo = offsets[j], hi = offsets[j + 1u];
    const uint32_t cls = wire_offsets_class(lo, hi, n_bytes, longest);
    if (lengths) lengths[j] = cls ? 0u : hi - lo;
    if (findings) findings[j] = cls;
    if (cls) {  // (findings are the exception: a lane that has one speaks for itself)
        atomicAdd((unsigned long long *)result, 1ull);
        atomicMax((unsigned long long *)result + 1, (unsigned long long)wire_offsets_key(j, cls));
    }
}

void launch_wire_scan(hipStream_t s, const uint64_t *lengths, uint32_t m, uint64_t *offsets, uint64_t capacity, uint64_t *state) {
    hipLaunchKernelGGL(wire_scan_kernel, dim3(1), dim3(REPITCH_SCAN_THREADS), 0, s, lengths, m, offsets, capacity, state);
}

void launch_wire_repitch(hipStream_t s, const WireRepitch &x) {
    if (!x.n) return;
    // at most 2^30 blocks a launch
    const uint64_t rows_per_launch = std::max<uint64_t>(1u, (((uint64_t)1 << 30) * REPITCH_THREADS) / x.units_per_row);
    for (uint64_t row0 = 0; row0 < x.n; row0 += rows_per_launch) {
        const uint64_t rows = std::min<uint64_t>(rows_per_launch, x.n - row0);
        const uint64_t blocks = (rows * x.units_per_row + REPITCH_THREADS - 1u) / REPITCH_THREADS;
        hipLaunchKernelGGL(wire_repitch_kernel, dim3((uint32_t)blocks), dim3(REPITCH_THREADS), 0, s, x, (uint32_t)row0, (uint32_t)rows);
    }
}

void launch_wire_offsets(hipStream_t s, const uint64_t *offsets, uint32_t n, uint64_t n_bytes, uint64_t longest, uint64_t *lengths, uint32_t *findings, uint64_t *result) {
    if (!n) return;
    hipLaunchKernelGGL(wire_offsets_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, offsets, n, n_bytes, longest, lengths, findings, result);
}

}  // namespace acvm
