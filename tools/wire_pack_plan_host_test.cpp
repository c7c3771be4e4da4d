// wire_pack_plan_host_test.cpp -- the host-only decisions of the packed wire export (acvm_amd/csrc/wire_pack_plan.cpp) as a plain C++ program: no
// HIP, no handle. tests/test_wire_pack_plan_on_host.py compiles it -- once plainly, once with the sanitizers, as `make asan` does
// (tools/asan/wire_pack_plan_host_test) -- and judges its answers.
//
//   g++ -std=c++17 -O1 tools/wire_pack_plan_host_test.cpp acvm_amd/csrc/wire_pack_plan.cpp acvm_amd/csrc/wire_plan.cpp -o wire_pack_plan_host_test
//
// Commands on stdin, one per line.
//   live B / nolive                  the live instance count the following calls see, or the null batch
//   circuit N_WITNESSES              the plan's assigned set: every witness below N_WITNESSES
//   pack CONTAINER FIRST N PITCH PTR CAPACITY OFFSETS_PTR LIST DEVICE N_LISTED { WITNESS } x N_LISTED
//                                    N_LISTED `-`: the whole map (pack null: a null descriptor) -> `err CODE TEXT` or `ok N PITCH BOUND`
//   chunk N PITCH                    -> the rows of one pass
//   arena FRONT CHUNK PITCH HOST     -> AT_STATE AT_LENGTHS AT_SLOTS AT_PACKED AT_OFFSETS END
//   fit CAPACITY N { OFFSET } x (N + 1)   -> N_FIT TOTAL
#include "../acvm_amd/csrc/wire_pack_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

int main() {
    uint32_t live = 0, n_witnesses = 0;
    bool have_live = false;
    std::unique_ptr<uint32_t[]> producer(new uint32_t[0]);
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "live") { in >> live; have_live = true; }
        else if (cmd == "nolive") have_live = false;
        else if (cmd == "circuit") {
            in >> n_witnesses;
            producer.reset(new uint32_t[n_witnesses]);
            for (uint32_t w = 0; w < n_witnesses; w++) producer[w] = w;
        } else if (cmd == "pack") {
            std::string first, count;
            in >> first;
            acvm_wire_desc_t d{};
            uint64_t ptr = 0, capacity = 0, offsets_ptr = 0;
            int list = 0, device = 1;
            std::unique_ptr<uint32_t[]> listed;
            if (first != "null") {
                d.container = (uint32_t)std::stoull(first);
                in >> d.first >> d.n >> d.pitch >> ptr >> capacity >> offsets_ptr >> list >> device >> count;
                if (count != "-") {
                    d.n_witnesses = (uint32_t)std::stoull(count);
                    listed.reset(new uint32_t[d.n_witnesses]);
                    for (uint32_t k = 0; k < d.n_witnesses; k++) in >> listed[k];
                    d.witnesses = listed.get();
                }
            }
            WirePlan plan;
            std::string err;
            const int rc = wire_pack_plan(have_live ? &live : nullptr, producer.get(), n_witnesses, first == "null" ? nullptr : &d, list != 0, (const void *)(uintptr_t)ptr, capacity,
                                          (const void *)(uintptr_t)offsets_ptr, device != 0, &plan, &err);
            if (rc) printf("err %d %s\n", rc, err.c_str());
            else printf("ok %u %" PRIu64 " %" PRIu64 "\n", plan.n, plan.pitch, plan.bound);
        } else if (cmd == "chunk") {
            uint32_t n = 0;
            uint64_t pitch = 0;
            in >> n >> pitch;
            printf("%u\n", wire_chunk_rows(n, pitch));
        } else if (cmd == "arena") {
            uint64_t front = 0, pitch = 0;
            uint32_t chunk = 0;
            int host = 0;
            in >> front >> chunk >> pitch >> host;
            const WirePackArena a = wire_pack_arena(front, chunk, pitch, host != 0);
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", a.at_state, a.at_lengths, a.at_slots, a.at_packed, a.at_offsets, a.end);
        } else if (cmd == "fit") {
            uint64_t capacity = 0, total = 0;
            uint32_t n = 0, n_fit = 0;
            in >> capacity >> n;
            std::unique_ptr<uint64_t[]> offsets(new uint64_t[(uint64_t)n + 1]);  // exactly n + 1 words on the heap
            for (uint32_t i = 0; i <= n; i++) in >> offsets[i];
            wire_pack_fit(offsets.get(), n, capacity, &n_fit, &total);
            printf("%u %" PRIu64 "\n", n_fit, total);
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
