// wire_pack_plan.hpp -- the packed forms of the batch-wide wire format (include/acvm_amd.h acvm_batch_witness_maps_wire_packed_device), decided
// before anything touches a device: the checks of the caller's arguments that the pitched export does not make, the rule that cuts the rows
// into chunks, where a chunk's pieces lie in the staging arena, and what n_fit and total mean at a capacity. Pure host code like wire_plan.cpp,
// which it calls for everything the two exports share: no HIP call, no handle (tools/wire_pack_plan_host_test.cpp,
// tests/test_wire_pack_plan_on_host.py, `make asan`).
#pragma once
#include "wire_plan.hpp"

namespace acvm {

// The rows of one pass: whole blocks of 64 rows, at most WIRE_HOST_CHUNK_BYTES of pitched slots, never fewer than 64 (or all n). The host form
// of the pitched export has the same rule.
constexpr uint64_t WIRE_HOST_CHUNK_BYTES = (uint64_t)64 << 20;
uint32_t wire_chunk_rows(uint32_t n, uint64_t pitch);

// 0 and *out, or ACVM_E_INVALID and the text in *err. Refused here: a descriptor with a pitch of its own (the packed export makes its slots at
// the bound), a null offsets column, a null buffer with a capacity, a misaligned device buffer; everything else is wire_plan's, with its texts.
// bytes may be null with capacity 0: the sizing call.
int wire_pack_plan(const uint32_t *live, const uint32_t *producer, uint32_t n_witnesses, const acvm_wire_desc_t *d, bool list, const void *bytes, uint64_t capacity,
                   const void *offsets, bool device, WirePlan *out, std::string *err);

// A chunk's pieces behind `front` bytes of tables, each aligned to 256: the scan's two state words, the chunk's lengths, its pitched slots,
// the host form's packed region (as large as the slots: a chunk's rows packed) and offsets [chunk + 1]. end: the arena's size.
struct WirePackArena {
    uint64_t at_state = 0, at_lengths = 0, at_slots = 0, at_packed = 0, at_offsets = 0, end = 0;
};
WirePackArena wire_pack_arena(uint64_t front, uint32_t chunk, uint64_t pitch, bool host);

// What the call answers at a capacity, from offsets [n + 1]: *total = offsets[n], *n_fit = the leading rows with offsets[i + 1] <= capacity.
// Rows below n_fit are written complete and no byte at or behind offsets[n_fit] is written.
void wire_pack_fit(const uint64_t *offsets, uint32_t n, uint64_t capacity, uint32_t *n_fit, uint64_t *total);

}  // namespace acvm
