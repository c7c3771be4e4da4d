// wire_plan.hpp -- the batch-wide WitnessMap wire format (include/acvm_amd.h acvm_batch_witness_maps_wire_device), checked and laid out before
// anything touches a device: the checks of the caller's descriptor, the generic instance's entry list and rank table, the bound, and the CRC
// power table. Pure host code like record_out_plan.cpp: no HIP call, no handle (tools/wire_plan_host_test.cpp,
// tests/test_wire_plan_on_host.py, `make asan`). The lengths and the framing offsets are wire_encode.hpp's, which this file's functions restate
// without a HIP include.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/acvm_amd.h"

namespace acvm {

// (wire_encode.hpp's constants; kernels_wire.hip asserts that the two agree)
enum : uint32_t { WIRE_PLAN_ENTRY_BYTES = 76, WIRE_PLAN_BLOCK_BYTES = 65532, WIRE_PLAN_WINDOW = 8 };

// A LIST POSITION k is entry k of the caller's witness list, or witness k for the whole map. The GENERIC instance -- one the level kernels
// solved -- assigns exactly the planner's assigned set (assigned_view.hpp), so its map is the same in every such instance:
//   entries     the witnesses of its map, ascending
//   rank        [n_positions + 1]: rank[k] = its entries among positions < k; position k is an entry iff rank[k + 1] != rank[k]
// An instance of the exact path has ranks of its own, which the device makes from its assigned bitmap and
//   list_mask   [(n_witnesses + 31) / 32]: bit w & 31 of word w >> 5 is set when witness w (< n_witnesses) is a list position
//   crc_pow     [n_positions + 1]: x^(8 * 76 * k) mod P, reflected, P = 0xEDB88320 (GZIP_STORED only, else empty)
// A window is WIRE_PLAN_WINDOW consecutive list positions.
struct WirePlan {
    uint32_t container = 0, first = 0, n = 0;
    uint64_t pitch = 0, bound = 0;
    bool whole = true;
    uint32_t n_positions = 0, n_windows = 0;
    std::vector<uint32_t> witnesses;  // the caller's list (empty for the whole map): what the handle's state is judged by
    std::vector<uint32_t> entries, rank, list_mask, crc_pow;
    uint32_t crc_x64 = 0;  // x^64 mod P
};

// the bytes of a map of n_entries entries, and where its body byte k lies (the model of tests/wire_ref.py)
uint64_t wire_plan_length(uint32_t container, uint64_t n_entries);
uint64_t wire_plan_body_offset(uint32_t container, uint64_t k);
// the length of the longest map `n_positions` list positions can give, rounded up to 16
uint64_t wire_plan_bound(uint32_t container, uint64_t n_positions);
// the CRC power table: [n_positions + 1], entry k = x^(8 * 76 * k) mod P; *x64 = x^64 mod P (the reader's too: wire_in_plan.cpp)
std::vector<uint32_t> wire_plan_crc_powers(uint32_t n_positions, uint32_t *x64);

// 0 and *out, or ACVM_E_INVALID and the text in *err (*out is then untouched). live: null is the null batch, else the live instance count the
// range is judged by. producer / n_witnesses: the plan's assigned set. list: the call has an instance list (first must be 0; the entries are the
// device's to judge). bytes: the caller's buffer, judged for null and -- device: the device form -- for its alignment.
int wire_plan(const uint32_t *live, const uint32_t *producer, uint32_t n_witnesses, const acvm_wire_desc_t *d, bool list, const void *bytes, bool device,
              WirePlan *out, std::string *err);

}  // namespace acvm
