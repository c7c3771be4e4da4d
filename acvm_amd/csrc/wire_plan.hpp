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
//   crc_pow     [n_positions + 1]: x^(8 * 76 * k) mod P, reflected, P = 0xEDB88320 (the gzip containers only, else empty)
// A window is WIRE_PLAN_WINDOW consecutive list positions.
struct WirePlan {
    uint32_t container = 0, first = 0, n = 0;
    uint64_t pitch = 0, bound = 0;
    bool whole = true;
    uint32_t n_positions = 0, n_windows = 0;
    std::vector<uint32_t> witnesses;  // the caller's list (empty for the whole map): what the handle's state is judged by
    std::vector<uint32_t> entries, rank, list_mask, crc_pow;
    uint32_t crc_x64 = 0;  // x^64 mod P
    std::vector<uint32_t> deflate;  // GZIP_DEFLATE only: the device's table (wire_deflate_device_table)
    uint32_t deflate_prefix_bits = 0;
};

// ---- ACVM_WIRE_GZIP_DEFLATE: the code of the format's one dynamic-Huffman block, a constant (include/acvm_amd.h; tests/wire_deflate_ref.py
// restates it). Code bits are stored REVERSED: the stream is LSB first, a Huffman code goes most significant bit first.
//   lit      [257]: literal 0 .. 255 and end-of-block (256): reversed code | length << 16
//   match    [77]: match length 3 .. 76 (below 3: zero): reversed length code | extra bits << 7, | their bit count (7 + extra) << 16
//   header   the block's constant header -- BFINAL, BTYPE, HLIT, HDIST, HCLEN, the code-length code, the run-length coded lengths -- as words,
//            LSB first, header_bits of them valid
//   lengths  [278]: the literal/length code's lengths
// The distance code needs no table: distance 1 is the bit 0, distance 76 the bit 1 and the five extra bits of 11.
enum : uint32_t { WIRE_PLAN_DEFLATE_LIT = 0, WIRE_PLAN_DEFLATE_MATCH = 257, WIRE_PLAN_DEFLATE_PREFIX = 334, WIRE_PLAN_DEFLATE_PREFIX_WORDS = 12, WIRE_PLAN_DEFLATE_WORDS = 346 };
struct WireDeflateCode {
    std::vector<uint32_t> lit, match, header;
    uint32_t header_bits = 0;
    std::vector<uint8_t> lengths;
};
// throws std::logic_error where the literal/length code or the code-length code is not complete (zlib rejects such a block)
WireDeflateCode wire_deflate_code();
// the bits a match of `length` (3 .. 76) at `distance` (1 or 76) costs, and those of the literals it replaces at their cheapest (5 each)
uint32_t wire_deflate_match_bits(const WireDeflateCode &c, uint32_t length, uint32_t distance);
// the device's table: [WIRE_PLAN_DEFLATE_LIT] lit, [_MATCH] match, [_PREFIX] the 11 bytes of the gzip head and the header behind them as one bit
// string of *prefix_bits bits
std::vector<uint32_t> wire_deflate_device_table(const WireDeflateCode &c, uint32_t *prefix_bits);

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
