// select_scan.hpp -- the predicate, the per-block span and the offset arithmetic of the ordered selection (kernels_select.hip select_*_kernel,
// include/acvm_amd.h acvm_batch_outcomes_device). Everything here is __host__ __device__ so that the host can run what the kernels run
// (tools/select_host_test.hip, tests/test_select_on_host.py).
//
// A block owns SELECT_SPAN consecutive elements and walks them in SELECT_ROUNDS rounds of SELECT_THREADS: thread t of round r looks at element
// r * SELECT_THREADS + t of the span, so that (round, wave, lane) in that order IS the ascending order of the elements. A wave ballots the
// predicate; the lanes below a lane that are set give its rank, the ballot's population the count of slot (round, wave). Three launches, no
// block ever waits for another: count (one total per block), scan (the totals become exclusive offsets, their sum the count that goes
// back to the host), scatter (every block ballots again and writes at offset of its block + offset of its slot + rank).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SELECT_HD __host__ __device__
#else
#define SELECT_HD
#endif

namespace acvm {

constexpr uint32_t SELECT_THREADS = 256, SELECT_WAVE = 64, SELECT_WAVES = SELECT_THREADS / SELECT_WAVE, SELECT_ROUNDS = 4;
constexpr uint32_t SELECT_SPAN = SELECT_THREADS * SELECT_ROUNDS;   // elements per block
constexpr uint32_t SELECT_SLOTS = SELECT_ROUNDS * SELECT_WAVES;    // ballots per block

// bit s of the mask selects status s; a status byte of 32 or more is selected by nothing
SELECT_HD inline bool select_predicate(uint32_t status, uint32_t select_mask) { return status < 32u && ((select_mask >> status) & 1u) != 0u; }
SELECT_HD inline uint32_t select_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + SELECT_SPAN - 1u) / SELECT_SPAN); }
// the element of thread t in round r of a block (64-bit: the last block's span may reach beyond 2^32)
SELECT_HD inline uint64_t select_element(uint32_t block, uint32_t round, uint32_t t) { return (uint64_t)block * SELECT_SPAN + (uint64_t)round * SELECT_THREADS + t; }
SELECT_HD inline uint32_t select_slot(uint32_t round, uint32_t t) { return round * SELECT_WAVES + t / SELECT_WAVE; }
// selected elements of the wave in front of `lane`: what v_mbcnt gives on the device
SELECT_HD inline uint32_t select_rank(uint64_t ballot, uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
#else
    return (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
#endif
}
SELECT_HD inline uint32_t select_count(uint64_t ballot) { return (uint32_t)__builtin_popcountll(ballot); }
// selected elements of the block in front of slot `slot`: counts[] holds the population of every ballot of the block
SELECT_HD inline uint32_t select_slot_offset(const uint32_t *counts, uint32_t slot) {
    uint32_t sum = 0;
    for (uint32_t k = 0; k < SELECT_SLOTS; k++) sum += k < slot ? counts[k] : 0u;
    return sum;
}
SELECT_HD inline uint32_t select_block_total(const uint32_t *counts) { return select_slot_offset(counts, SELECT_SLOTS); }
// the scan of the block totals runs in one block, SELECT_THREADS totals per step behind a running carry: steps for `blocks` totals
SELECT_HD inline uint32_t select_scan_steps(uint32_t blocks) { return (blocks + SELECT_THREADS - 1u) / SELECT_THREADS; }

}  // namespace acvm
