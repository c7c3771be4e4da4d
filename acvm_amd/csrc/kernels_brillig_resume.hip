// kernels_brillig_resume.hip -- brillig_resume: between two retry passes the compact VM scratch may change its stride, a lane's column, the
// memory capacity and the call depth (brillig_retry_plan.hpp). One launch copies every CONTINUING lane's state from the old scratch into
// the new one: its registers, its live memory cells, its call-stack words (brillig_resume.hpp br_reloc_item: the index functions BrVm's
// set-up uses). Nothing outside a lane's live prefix is read, nothing of a lane that restarts or is final is copied.
//
// The rows are [slot][half][lane]: consecutive items of ONE lane lie a whole row apart, consecutive lanes of one item are adjacent. So the
// grid runs over (item block, lane group), and a block is shaped by how many lanes continue:
//   LANES = 64: a wave takes 64 adjacent lanes of one item -- their 16-byte halves are one contiguous 1 KiB run per row -- and the block's
//               four waves take four items;
//   LANES = 1:  a handful of lanes: every thread takes an item of its own, so one lane with 2^22 live cells is spread over the whole grid
//               instead of being walked by one thread of each wave.
// Either way a thread moves both halves of its cell, and the item blocks of a lane stride over the grid's x dimension.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "brillig_resume.hpp"
#include "kernels.hpp"

namespace acvm {

template <uint32_t LANES>
__global__ void __launch_bounds__(256) brillig_relocate_kernel(const BrRelocLane *__restrict__ lanes, uint32_t n_lanes, BrLayout from, const uint32_t *__restrict__ old_scratch,
                                                               BrLayout to, uint32_t *__restrict__ new_scratch) {
    constexpr uint32_t ITEMS = 256u / LANES;  // items a block takes per round
    for (uint64_t q = (uint64_t)blockIdx.y * LANES + threadIdx.x % LANES; q < n_lanes; q += (uint64_t)gridDim.y * LANES) {
        const BrRelocLane r = lanes[q];
        const uint64_t n_items = br_reloc_items(r);
        for (uint64_t item = (uint64_t)blockIdx.x * ITEMS + threadIdx.x / LANES; item < n_items; item += (uint64_t)gridDim.x * ITEMS)
            br_reloc_item<uint4>(r, item, from, old_scratch, to, new_scratch);
    }
}

void launch_brillig_relocate(hipStream_t s, const BrRelocLane *d_lanes, uint32_t n_lanes, uint64_t max_items, const BrLayout &from, const uint32_t *old_scratch,
                             const BrLayout &to, uint32_t *new_scratch) {
    if (!n_lanes || !max_items) return;
    const bool wide = n_lanes > 16u;
    const uint64_t per_block = wide ? 4u : 256u;
    const uint32_t gx = (uint32_t)std::min<uint64_t>((max_items + per_block - 1) / per_block, 8192u);  // (the rest: the stride loop)
    if (wide) hipLaunchKernelGGL(brillig_relocate_kernel<64>, dim3(gx, std::min<uint32_t>((n_lanes + 63u) / 64u, 65535u)), dim3(256), 0, s, d_lanes, n_lanes, from, old_scratch, to, new_scratch);
    else hipLaunchKernelGGL(brillig_relocate_kernel<1>, dim3(gx, n_lanes), dim3(256), 0, s, d_lanes, n_lanes, from, old_scratch, to, new_scratch);
}

}  // namespace acvm
