// wire_deflate_plan_host_test.cpp -- the deflating container's part of the wire plan (acvm_amd/csrc/wire_plan.cpp): the code tables, the
// constant block header, the bound, the device's table, and wire_plan()'s word on every container, as a plain C++ program: no HIP, no handle.
// tests/test_wire_deflate_plan_on_host.py compiles it -- once plainly, once with the sanitizers, as `make asan` does
// (tools/asan/wire_deflate_plan_host_test) -- and judges its answers by tests/wire_deflate_ref.py.
//
//   g++ -std=c++17 -O1 tools/wire_deflate_plan_host_test.cpp acvm_amd/csrc/wire_plan.cpp -o wire_deflate_plan_host_test
//
// Commands on stdin, one per line.
//   lit                    -> 257 x "REVERSED_CODE LENGTH": literals 0 .. 255 and end-of-block
//   match                  -> 74 x "REVERSED_LENGTH_CODE|EXTRA<<7 BITS": match lengths 3 .. 76
//   lengths                -> the 278 lengths of the literal/length code
//   kraft                  -> the literal/length code's Kraft sum times 2^15 (complete: 32768)
//   header                 -> HEADER_BITS, then the header's words
//   inequality             -> per length 3 .. 76 and distance 1, 76: "LENGTH DISTANCE MATCH_BITS CHEAPEST_LITERAL_BITS"; exit status 4 and a
//                             line on stderr where a match costs more than the literals it replaces at 5 bits each
//   bound CONTAINER N      -> wire_plan_bound
//   table                  -> PREFIX_BITS, then the device table's words
//   plan CONTAINER N_WITNESSES N_LISTED|- PITCH
//                          -> wire_plan() for `live` 64 instances, every witness assigned, a 16-aligned device buffer:
//                             "ok CONTAINER PITCH BOUND N_POSITIONS N_WINDOWS N_POW N_DEFLATE PREFIX_BITS" or "err CODE TEXT"
#include "../acvm_amd/csrc/wire_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

int main() {
    const WireDeflateCode code = wire_deflate_code();  // (throws where a code is not complete)
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "lit") {
            for (uint32_t e : code.lit) printf("%u %u ", e & 0xffffu, e >> 16);
            printf("\n");
        } else if (cmd == "match") {
            for (uint32_t n = 3; n <= WIRE_PLAN_ENTRY_BYTES; n++) printf("%u %u ", code.match.at(n) & 0xffffu, code.match.at(n) >> 16);
            printf("\n");
        } else if (cmd == "lengths") {
            for (uint8_t n : code.lengths) printf("%u ", n);
            printf("\n");
        } else if (cmd == "kraft") {
            uint64_t kraft = 0;
            for (uint8_t n : code.lengths)
                if (n) kraft += 1u << (15 - n);
            printf("%" PRIu64 "\n", kraft);
        } else if (cmd == "header") {
            printf("%u", code.header_bits);
            for (uint32_t w : code.header) printf(" %u", w);
            printf("\n");
        } else if (cmd == "inequality") {
            for (uint32_t n = 3; n <= WIRE_PLAN_ENTRY_BYTES; n++)
                for (uint32_t distance : {1u, 76u}) {
                    const uint32_t bits = wire_deflate_match_bits(code, n, distance);
                    if (bits > 5u * n) { fprintf(stderr, "a match of %u at %u costs %u bits\n", n, distance, bits); return 4; }
                    printf("%u %u %u %u ", n, distance, bits, 5u * n);
                }
            printf("\n");
        } else if (cmd == "bound") {
            uint32_t container = 0;
            uint64_t n = 0;
            in >> container >> n;
            printf("%" PRIu64 "\n", wire_plan_bound(container, n));
        } else if (cmd == "table") {
            uint32_t prefix_bits = 0;
            const std::vector<uint32_t> t = wire_deflate_device_table(code, &prefix_bits);
            if (t.size() != WIRE_PLAN_DEFLATE_WORDS) { fprintf(stderr, "table size\n"); return 3; }
            printf("%u", prefix_bits);
            for (uint32_t w : t) printf(" %u", w);
            printf("\n");
        } else if (cmd == "plan") {
            acvm_wire_desc_t d{};
            uint32_t n_witnesses = 0;
            std::string listed;
            in >> d.container >> n_witnesses >> listed >> d.pitch;
            d.n = 64;
            std::unique_ptr<uint32_t[]> producer(new uint32_t[n_witnesses]), list;
            for (uint32_t w = 0; w < n_witnesses; w++) producer[w] = w;
            if (listed != "-") {
                d.n_witnesses = (uint32_t)std::stoull(listed);
                list.reset(new uint32_t[d.n_witnesses]);
                for (uint32_t k = 0; k < d.n_witnesses; k++) list[k] = k;
                d.witnesses = list.get();
            }
            const uint32_t live = 64;
            WirePlan plan;
            std::string err;
            const int rc = wire_plan(&live, producer.get(), n_witnesses, &d, false, (const void *)(uintptr_t)4096, true, &plan, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            printf("ok %u %" PRIu64 " %" PRIu64 " %u %u %zu %zu %u\n", plan.container, plan.pitch, plan.bound, plan.n_positions, plan.n_windows, plan.crc_pow.size(), plan.deflate.size(),
                   plan.deflate_prefix_bits);
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
