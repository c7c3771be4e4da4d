// wire_rows.hpp -- which instance an output row of the batch-wide wire export names, how many entries its map has and where a list position
// ranks in it: shared by the export's kernels (kernels_wire.hip, kernels_wire_deflate.hip). Device code.
#pragma once
#include "kernels.hpp"

namespace acvm {

// the instance of output row i (i < n), and its lane of the exact path or -1
struct WireRow {
    uint32_t j;
    int32_t lane;
};
__device__ __forceinline__ WireRow wire_row(const WireExport &a, uint64_t i) {
    WireRow r{a.src.list ? a.src.list[i] : a.first + (uint32_t)i, -1};
    if (r.j < a.src.B) r.lane = a.src.lane_of[r.j];
    return r;
}
// the entries of a row: a generic instance's from the plan's table, a lane's from its prefix, none for a row that names no instance
__device__ __forceinline__ uint32_t wire_row_entries(const WireExport &a, const WireRow &r) {
    if (r.j >= a.src.B) return 0u;
    return r.lane < 0 ? a.rank[a.n_positions] : a.lane_prefix[(uint64_t)((a.n_witnesses + 31u) / 32u) * a.src.n_slow + (uint32_t)r.lane];
}
// the rank of list position k (<= n_positions) in the map of lane `lane`: its assigned list positions below k. The list ascends, so behind the
// first witness beyond the circuit there is nothing.
__device__ __forceinline__ uint32_t wire_lane_rank(const WireExport &a, uint32_t lane, uint32_t k) {
    const uint32_t n_words = (a.n_witnesses + 31u) / 32u, n_slow = a.src.n_slow;
    const uint32_t w = k < a.n_positions ? (a.sel ? a.sel[k] : k) : 0xFFFFFFFFu;
    if (w >= a.n_witnesses) return a.lane_prefix[(uint64_t)n_words * n_slow + lane];
    const uint32_t bits = a.src.assigned_bits[(uint64_t)(w >> 5) * n_slow + lane] & a.list_mask[w >> 5];
    return a.lane_prefix[(uint64_t)(w >> 5) * n_slow + lane] + __builtin_popcount(bits & ((1u << (w & 31u)) - 1u));
}

}  // namespace acvm
