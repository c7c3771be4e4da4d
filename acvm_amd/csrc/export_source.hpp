// export_source.hpp -- where an element of a device export comes from, in one place for every kernel that writes the map into a caller's
// buffer (kernels.hip export_device_* / export_list_*, kernels_typed_io.hip export_narrow_*, kernels_records_out.hip export_records_kernel):
// a GENERIC instance takes the planner's assigned set, its row through row_of under slot reuse and, where the row is scaled, a factor row; an
// instance of the EXACT path takes its bit of the assigned bitmap and its column as it is. Device code only; what is done with the row -- the
// encoding -- is export_encode.hpp's.
#pragma once
#include "export_encode.hpp"

namespace acvm {

// witness w of a generic instance: its row of the table, or 0xFFFFFFFF = unassigned (beyond the circuit, or no opcode produces it), and the row
// of the factor tables that unscales it, or 0xFFFFFFFF = stored as is. w is wave-uniform where the caller is: the lookups are scalar loads.
__device__ __forceinline__ void export_generic_source(uint32_t w, uint32_t n_witnesses, const uint32_t *row_of, const uint32_t *producer, const uint32_t *u_index, uint32_t &row, uint32_t &ui) {
    row = 0xFFFFFFFFu;
    ui = 0xFFFFFFFFu;
    if (w < n_witnesses && producer[w] != 0xFFFFFFFFu) {
        row = row_of ? row_of[w] : w;
        if (u_index) ui = u_index[w];
    }
}
// witness w of lane `lane` of the exact path: bit w of the lane at assigned_bits[(w >> 5) * n_slow + lane]
__device__ __forceinline__ bool export_lane_assigned(const uint32_t *assigned_bits, uint32_t n_slow, uint32_t lane, uint32_t w, uint32_t n_witnesses) {
    return w < n_witnesses && ((assigned_bits[(uint64_t)(w >> 5) * n_slow + lane] >> (w & 31u)) & 1u) != 0u;
}

}  // namespace acvm
