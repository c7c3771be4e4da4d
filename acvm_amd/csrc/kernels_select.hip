// kernels_select.hip -- per-instance outcomes on the device (include/acvm_amd.h acvm_batch_outcomes_device): the status / err / opcode-index
// columns, the instance -> exact-lane map of the list export, and the ordered selection of the instances with a given status (select_scan.hpp:
// ballot + mbcnt per wave, block totals scanned by a launch of their own, no block waits for another).
#include "kernels.hpp"
#include "select_scan.hpp"

namespace acvm {

// ---- the columns: every instance of the range as a generic one (Solved, no error, opcode index 0) ...
__global__ void __launch_bounds__(256) outcomes_fill_kernel(uint32_t n, uint8_t *__restrict__ status, uint8_t *__restrict__ err, uint32_t *__restrict__ opcode_index) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (status) status[i] = 0u;  // ACVM_STATUS_SOLVED
    if (err) err[i] = 0u;        // ACVM_ERR_NONE
    if (opcode_index) opcode_index[i] = 0u;
}
// ... then the exact lanes of the range from the host's records: {status, err, opcode index, index in the range}
__global__ void __launch_bounds__(256) outcomes_lanes_kernel(const uint4 *__restrict__ records, uint32_t n_lanes, uint32_t n, uint8_t *__restrict__ status,
                                                             uint8_t *__restrict__ err, uint32_t *__restrict__ opcode_index) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_lanes) return;
    const uint4 r = records[x];
    if (r.w >= n) return;
    if (status) status[r.w] = (uint8_t)r.x;
    if (err) err[r.w] = (uint8_t)r.y;
    if (opcode_index) opcode_index[r.w] = r.z;
}
// lane_of[ids[t]] = t over a map filled with -1 (launch_fill_u32)
__global__ void __launch_bounds__(256) lane_map_scatter_kernel(int32_t *__restrict__ lane_of, uint32_t n_instances, const uint32_t *__restrict__ ids, uint32_t n_slow) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_slow) return;
    const uint32_t j = ids[t];
    if (j < n_instances) lane_of[j] = (int32_t)t;
}
// out[i] = rows[t] for the pairs (t, i) of the exact lanes: one thread per 4-byte word of a 32-byte row, stored as bytes (the column is the
// caller's and has no alignment of its own); few lanes by construction
__global__ void __launch_bounds__(256) scatter_rows32_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ lanes, uint32_t n_lanes, uint32_t n,
                                                             uint8_t *__restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t x = g >> 3, w = g & 7u;
    if (x >= n_lanes) return;
    const uint32_t t = lanes[2 * x], i = lanes[2 * x + 1];
    if (i >= n) return;
    const uint32_t v = rows[(uint64_t)t * 8 + w];
    for (uint32_t k = 0; k < 4; k++) out[(uint64_t)i * 32 + 4 * w + k] = (uint8_t)(v >> (8 * k));
}

// ---- the selection
// the ballots of a block: p[r] / rank[r] of this thread in round r, counts[] (LDS) the population of every slot
__device__ __forceinline__ void select_ballots(const uint8_t *__restrict__ status, uint32_t n, uint32_t select_mask, uint32_t *counts, bool p[SELECT_ROUNDS],
                                               uint32_t rank[SELECT_ROUNDS]) {
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (uint32_t r = 0; r < SELECT_ROUNDS; r++) {
        const uint64_t e = select_element(blockIdx.x, r, t);
        p[r] = e < n && select_predicate(status[e], select_mask);
        const uint64_t ballot = __ballot(p[r]);
        rank[r] = select_rank(ballot, t % SELECT_WAVE);
        if (t % SELECT_WAVE == 0u) counts[select_slot(r, t)] = select_count(ballot);
    }
    __syncthreads();
}
__global__ void __launch_bounds__(SELECT_THREADS) select_count_kernel(const uint8_t *__restrict__ status, uint32_t n, uint32_t select_mask, uint32_t *__restrict__ totals) {
    __shared__ uint32_t counts[SELECT_SLOTS];
    bool p[SELECT_ROUNDS];
    uint32_t rank[SELECT_ROUNDS];
    select_ballots(status, n, select_mask, counts, p, rank);
    if (threadIdx.x == 0u) totals[blockIdx.x] = select_block_total(counts);
}
// one block: totals[0 .. blocks) become their exclusive prefix sums, *count their sum. SELECT_THREADS totals per step behind a running carry.
__global__ void __launch_bounds__(SELECT_THREADS) select_scan_kernel(uint32_t *__restrict__ totals, uint32_t blocks, uint32_t *__restrict__ count) {
    __shared__ uint32_t sums[SELECT_THREADS];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t step = 0; step < select_scan_steps(blocks); step++) {  // (block-uniform)
        const uint32_t at = step * SELECT_THREADS + t;
        const uint32_t v = at < blocks ? totals[at] : 0u;
        sums[t] = v;
        __syncthreads();
        for (uint32_t d = 1; d < SELECT_THREADS; d <<= 1) {
            const uint32_t add = t >= d ? sums[t - d] : 0u;
            __syncthreads();
            sums[t] += add;
            __syncthreads();
        }
        if (at < blocks) totals[at] = carry + sums[t] - v;
        carry += sums[SELECT_THREADS - 1u];
        __syncthreads();
    }
    if (t == 0u) *count = carry;
}
__global__ void __launch_bounds__(SELECT_THREADS) select_scatter_kernel(const uint8_t *__restrict__ status, uint32_t first, uint32_t n, uint32_t select_mask,
                                                                        const uint32_t *__restrict__ offsets, uint32_t *__restrict__ out) {
    __shared__ uint32_t counts[SELECT_SLOTS];
    bool p[SELECT_ROUNDS];
    uint32_t rank[SELECT_ROUNDS];
    select_ballots(status, n, select_mask, counts, p, rank);
    const uint32_t base = offsets[blockIdx.x];
#pragma unroll
    for (uint32_t r = 0; r < SELECT_ROUNDS; r++)
        if (p[r]) out[base + select_slot_offset(counts, select_slot(r, threadIdx.x)) + rank[r]] = first + (uint32_t)select_element(blockIdx.x, r, threadIdx.x);
}

void launch_outcomes_fill(hipStream_t s, uint32_t n, uint8_t *status, uint8_t *err, uint32_t *opcode_index) {
    if (!n || (!status && !err && !opcode_index)) return;
    hipLaunchKernelGGL(outcomes_fill_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, n, status, err, opcode_index);
}
void launch_outcomes_lanes(hipStream_t s, const uint32_t *records, uint32_t n_lanes, uint32_t n, uint8_t *status, uint8_t *err, uint32_t *opcode_index) {
    if (!n_lanes || (!status && !err && !opcode_index)) return;
    hipLaunchKernelGGL(outcomes_lanes_kernel, dim3((n_lanes + 255u) / 256u), dim3(256), 0, s, (const uint4 *)records, n_lanes, n, status, err, opcode_index);
}
void launch_lane_map_scatter(hipStream_t s, int32_t *lane_of, uint32_t n_instances, const uint32_t *ids, uint32_t n_slow) {
    if (!n_slow) return;
    hipLaunchKernelGGL(lane_map_scatter_kernel, dim3((n_slow + 255u) / 256u), dim3(256), 0, s, lane_of, n_instances, ids, n_slow);
}
void launch_scatter_rows32(hipStream_t s, const uint32_t *rows, const uint32_t *lanes, uint32_t n_lanes, uint32_t n, uint8_t *out) {
    if (!n_lanes) return;
    hipLaunchKernelGGL(scatter_rows32_kernel, dim3((unsigned)(((uint64_t)n_lanes * 8 + 255u) / 256u)), dim3(256), 0, s, rows, lanes, n_lanes, n, out);
}
size_t select_scratch_words(uint32_t n) { return (size_t)select_blocks(n) + 1u; }
void launch_select(hipStream_t s, const uint8_t *status, uint32_t first, uint32_t n, uint32_t select_mask, uint32_t *scratch, uint32_t *out, uint32_t *count) {
    const uint32_t blocks = select_blocks(n);
    if (blocks) hipLaunchKernelGGL(select_count_kernel, dim3(blocks), dim3(SELECT_THREADS), 0, s, status, n, select_mask, scratch);
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SELECT_THREADS), 0, s, scratch, blocks, count);
    if (blocks && out) hipLaunchKernelGGL(select_scatter_kernel, dim3(blocks), dim3(SELECT_THREADS), 0, s, status, first, n, select_mask, scratch, out);
}

}  // namespace acvm
