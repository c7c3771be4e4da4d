// wire_inflate_plan.hpp -- the gzip import of the batch-wide WitnessMap wire format (include/acvm_amd.h acvm_batch_import_device_wire_gzip),
// checked and laid out before anything touches a device: the checks of the caller's descriptor, the fixed code's tables, the arena of the two
// stages and the WireInPlan of the second. Pure host code like wire_in_plan.cpp: no HIP call, no handle
// (tools/wire_inflate_plan_host_test.cpp, tests/test_wire_inflate_plan_on_host.py, `make asan`).
#pragma once
#include "wire_in_plan.hpp"

namespace acvm {

// (wire_inflate.hpp's layout of a code table, which this file restates without a HIP include; kernels_wire_inflate.hip asserts that they agree)
enum : uint32_t { INFLATE_PLAN_LCNT = 0, INFLATE_PLAN_DCNT = 16, INFLATE_PLAN_LSYM = 48, INFLATE_PLAN_DSYM = 336, INFLATE_PLAN_TAB_HALFWORDS = 368 };
// a row's code tables in the arena, in dwords: the halfwords, 320 four-bit code lengths, one dword of padding
enum : uint32_t { INFLATE_PLAN_ROW_WORDS = 225 };

// The staging arena of one call, every part at a multiple of 256:
//   [scratch]   B slots of out_pitch = wire_in_stage_pitch(n_initial) bytes: what stage 1 inflates into and stage 2 reads as BINCODE slots
//   [lengths]   B u64: the inflater's output lengths, stage 2's d_lengths
//   [findings]  B x {class, block}
//   [tables]    B x INFLATE_PLAN_ROW_WORDS dwords: the rows' code tables
//   [fixed]     the fixed code's tables
//   [result]    2 u64: the findings' count and the smallest inflate_key
//   [rows]      the host form's compressed rows at rows_pitch, [row_lengths] their B u64 lengths
//   [body]      from `front` on: what the body import lays out for itself (batch_import.cpp)
struct WireInflatePlan {
    uint64_t pitch = 0;             // of the compressed rows the kernel reads (the host form: rows_pitch)
    uint64_t out_pitch = 0, out_cap = 0;  // out_cap = 8 + 76 * n_initial: the handle's longest body
    size_t at_scratch = 0, at_lengths = 0, at_findings = 0, at_tables = 0, at_fixed = 0, at_result = 0, at_rows = 0, at_row_lengths = 0, front = 0;
    std::vector<uint16_t> fixed;
    WireInPlan body;  // stage 2: ACVM_WIRE_BINCODE over the scratch
};

// the fixed code (RFC 1951 3.2.6) as the reader's table: literal/length lengths 8 x 144, 9 x 112, 7 x 24, 8 x 8 (286 and 287 have codes, which
// the reader refuses as symbols), 32 distance codes of 5 bits (30 and 31 likewise)
std::vector<uint16_t> wire_inflate_fixed_tables();

// 0 and *out, or ACVM_E_INVALID and the text in *err (*out is then untouched). live: null is the null batch. device: d->pitch and bytes are the
// caller's device buffer's (a multiple of 16, aligned). Else the host form: d->pitch is any, and host_row_bytes -- the longest readable row --
// gives the staged pitch.
int wire_inflate_plan(const uint32_t *live, const uint32_t *initial_ids, uint32_t n_initial, const acvm_wire_in_desc_t *d, const void *bytes, bool device,
                      uint64_t host_row_bytes, WireInflatePlan *out, std::string *err);

}  // namespace acvm
