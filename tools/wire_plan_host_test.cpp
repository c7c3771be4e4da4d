// wire_plan_host_test.cpp -- the checks, the generic instance's entries and ranks, the bound and the CRC power table of the batch-wide wire
// format (acvm_amd/csrc/wire_plan.cpp) as a plain C++ program: no HIP, no handle. tests/test_wire_plan_on_host.py compiles it -- once plainly,
// once with the sanitizers, as `make asan` does (tools/asan/wire_plan_host_test) -- and judges its answers by tests/wire_ref.py.
//
//   g++ -std=c++17 -O1 tools/wire_plan_host_test.cpp acvm_amd/csrc/wire_plan.cpp -o wire_plan_host_test
//
// Commands on stdin, one per line.
//   live B                           the live instance count the following calls see
//   nolive                           the null batch
//   circuit N_WITNESSES N_UNPRODUCED { WITNESS } x N_UNPRODUCED
//                                    the plan's assigned set: every witness below N_WITNESSES but the listed ones
//   wire CONTAINER FIRST N PITCH PTR LIST DEVICE N_LISTED { WITNESS } x N_LISTED
//                                    LIST 0 | 1: the call has an instance list; DEVICE 0 | 1: the device form; N_LISTED `-`: the whole map
//                                    (wire null: a null descriptor)
//   length CONTAINER N / offset CONTAINER K / bound CONTAINER N
//   window                           the window in list positions
// Answers: `err CODE TEXT`, a number, or
//   ok CONTAINER FIRST N PITCH BOUND WHOLE N_POSITIONS N_WINDOWS X64 N_ENTRIES { ENTRY } { RANK } x (N_POSITIONS + 1) N_MASK { MASK } N_POW { POW }
#include "../acvm_amd/csrc/wire_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

int main() {
    uint32_t live = 0, n_witnesses = 0;
    bool have_live = false;
    std::unique_ptr<uint32_t[]> producer(new uint32_t[0]);  // exactly n_witnesses entries on the heap: a read past the end is one the sanitizer sees
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "live") { in >> live; have_live = true; }
        else if (cmd == "nolive") have_live = false;
        else if (cmd == "window") printf("%u\n", WIRE_PLAN_WINDOW);
        else if (cmd == "circuit") {
            uint32_t n_un = 0;
            in >> n_witnesses >> n_un;
            producer.reset(new uint32_t[n_witnesses]);
            for (uint32_t w = 0; w < n_witnesses; w++) producer[w] = w;
            for (uint32_t k = 0; k < n_un; k++) {
                uint32_t w = 0;
                in >> w;
                if (w < n_witnesses) producer[w] = 0xFFFFFFFFu;
            }
        } else if (cmd == "length" || cmd == "offset" || cmd == "bound") {
            uint32_t container = 0;
            uint64_t v = 0;
            in >> container >> v;
            printf("%" PRIu64 "\n", cmd == "length" ? wire_plan_length(container, v) : cmd == "offset" ? wire_plan_body_offset(container, v) : wire_plan_bound(container, v));
        } else if (cmd == "wire") {
            std::string first, count;
            in >> first;
            acvm_wire_desc_t d{};
            uint64_t ptr = 0;
            int list = 0, device = 1;
            std::unique_ptr<uint32_t[]> listed;
            if (first != "null") {
                d.container = (uint32_t)std::stoull(first);
                in >> d.first >> d.n >> d.pitch >> ptr >> list >> device >> count;
                if (count != "-") {
                    d.n_witnesses = (uint32_t)std::stoull(count);
                    listed.reset(new uint32_t[d.n_witnesses]);
                    for (uint32_t k = 0; k < d.n_witnesses; k++) in >> listed[k];
                    d.witnesses = listed.get();
                }
            }
            WirePlan plan;
            std::string err;
            const int rc = wire_plan(have_live ? &live : nullptr, producer.get(), n_witnesses, first == "null" ? nullptr : &d, list != 0, (const void *)(uintptr_t)ptr, device != 0, &plan, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            if (plan.rank.size() != (size_t)plan.n_positions + 1) { fprintf(stderr, "rank size\n"); return 3; }
            printf("ok %u %u %u %" PRIu64 " %" PRIu64 " %d %u %u %u %zu", plan.container, plan.first, plan.n, plan.pitch, plan.bound, (int)plan.whole, plan.n_positions, plan.n_windows,
                   plan.crc_x64, plan.entries.size());
            for (uint32_t w : plan.entries) printf(" %u", w);
            for (uint32_t r : plan.rank) printf(" %u", r);
            printf(" %zu", plan.list_mask.size());
            for (uint32_t m : plan.list_mask) printf(" %u", m);
            printf(" %zu", plan.crc_pow.size());
            for (uint32_t t : plan.crc_pow) printf(" %u", t);
            printf("\n");
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
