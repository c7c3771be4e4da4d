// wire_in_plan.hpp -- the batch-wide WitnessMap wire format read as initial witnesses (include/acvm_amd.h acvm_batch_import_device_wire),
// checked and laid out before anything touches a device: the checks of the caller's descriptor, the table the kernel looks keys up in, the
// CRC power table, and the host form's judgement of a row. Pure host code like wire_plan.cpp: no HIP call, no handle
// (tools/wire_in_plan_host_test.cpp, tests/test_wire_in_plan_on_host.py, `make asan`).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/acvm_amd.h"
#include "wire_plan.hpp"

namespace acvm {

//   keys / positions   the handle's initial ids ascending, each with its position in the order the handle was created with
//   crc_pow, crc_x64   wire_plan_crc_powers(n_initial) (GZIP_STORED only, else empty)
//   rank_bits          the width of the rank field of a finding key (wire_decode.hpp wire_in_key): instance, class and rank fit 63 bits
//   n_windows          windows of WIRE_PLAN_WINDOW entry ranks that cover n_initial: the kernel's grid, never sized by the bytes
struct WireInPlan {
    uint32_t container = 0, n_initial = 0, n_windows = 0, rank_bits = 0;
    uint64_t pitch = 0;
    std::vector<uint32_t> keys, positions, crc_pow;
    uint32_t crc_x64 = 0;
};

// 0 and *out, or ACVM_E_INVALID and the text in *err (*out is then untouched). live: null is the null batch, else the live instance count.
// device: the device form, whose buffer is judged for its alignment and whose pitch must be a multiple of 16.
int wire_in_plan(const uint32_t *live, const uint32_t *initial_ids, uint32_t n_initial, const acvm_wire_in_desc_t *d, const void *bytes, bool device, WireInPlan *out,
                 std::string *err);

// ---- the host form's rows. A body -- a row as it came, or inflated -- is CANONICAL when the device form reads it as it is: its length is that
// of its count word, which names at most n_initial entries; every length word is 64; every character is a hex digit; the keys are initial ids
// and ascend strictly. Anything else goes through the reader and comes back here as a map.
bool wire_in_body_canonical(const WireInPlan &plan, const uint8_t *body, size_t len);
// The map the reader made of a row (ids in the order read, canonical 32-byte big-endian values) as a canonical body: last one wins, ascending.
// ACVM_E_INVALID and the text for a key that is not an initial witness.
int wire_in_body_of_map(const WireInPlan &plan, const uint32_t *ids, const uint8_t *values_be32, size_t n, std::vector<uint8_t> *body, std::string *err);
// the pitch of the staged slots: the longest BINCODE body of the handle, rounded up to 16
uint64_t wire_in_stage_pitch(uint32_t n_initial);

}  // namespace acvm
