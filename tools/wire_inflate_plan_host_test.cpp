// wire_inflate_plan_host_test.cpp -- the checks, the arena layout and the fixed-code tables of the gzip import
// (acvm_amd/csrc/wire_inflate_plan.cpp) as a plain C++ program: no HIP, no handle. tests/test_wire_inflate_plan_on_host.py compiles it -- once
// plainly, once with the sanitizers, as `make asan` does (tools/asan/wire_inflate_plan_host_test) -- and judges its answers.
//
//   g++ -std=c++17 -O1 tools/wire_inflate_plan_host_test.cpp acvm_amd/csrc/wire_inflate_plan.cpp acvm_amd/csrc/wire_in_plan.cpp acvm_amd/csrc/wire_plan.cpp
//
// Commands on stdin, one per line.
//   live B / nolive                               the live instance count the following calls see / the null batch
//   ids N { ID } x N                              the handle's initial ids
//   plan CONTAINER PITCH PTR DEVICE HOST_ROW      DEVICE 0 | 1; HOST_ROW: the host form's longest readable row (plan null: a null descriptor)
//   fixed                                         the fixed code's tables
// Answers: `err CODE TEXT`, or
//   ok PITCH OUT_PITCH OUT_CAP AT_SCRATCH AT_LENGTHS AT_FINDINGS AT_TABLES AT_FIXED AT_RESULT AT_ROWS AT_ROW_LENGTHS FRONT BODY_CONTAINER BODY_PITCH BODY_N_INITIAL N_KEYS
//   the 368 halfwords
#include "../acvm_amd/csrc/wire_inflate_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

int main() {
    uint32_t live = 0, n_ids = 0;
    bool have_live = false;
    std::unique_ptr<uint32_t[]> ids(new uint32_t[0]);
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "live") { in >> live; have_live = true; }
        else if (cmd == "nolive") have_live = false;
        else if (cmd == "ids") {
            in >> n_ids;
            ids.reset(new uint32_t[n_ids]);  // exactly n_ids words on the heap
            for (uint32_t k = 0; k < n_ids; k++) in >> ids[k];
        } else if (cmd == "fixed") {
            const std::vector<uint16_t> t = wire_inflate_fixed_tables();
            for (size_t k = 0; k < t.size(); k++) printf("%u%s", t[k], k + 1 == t.size() ? "\n" : " ");
        } else if (cmd == "plan") {
            std::string first;
            in >> first;
            acvm_wire_in_desc_t d{};
            uint64_t ptr = 0, host_row = 0;
            int device = 1;
            if (first != "null") {
                d.container = (uint32_t)std::stoull(first);
                in >> d.pitch >> ptr >> device >> host_row;
            }
            WireInflatePlan p;
            std::string err;
            const int rc = wire_inflate_plan(have_live ? &live : nullptr, ids.get(), n_ids, first == "null" ? nullptr : &d, (const void *)(uintptr_t)ptr, device != 0, host_row, &p, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            if (p.fixed != wire_inflate_fixed_tables()) { fprintf(stderr, "fixed tables\n"); return 3; }
            printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 " %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %" PRIu64 " %u %zu\n", p.pitch, p.out_pitch, p.out_cap, p.at_scratch, p.at_lengths,
                   p.at_findings, p.at_tables, p.at_fixed, p.at_result, p.at_rows, p.at_row_lengths, p.front, p.body.container, p.body.pitch, p.body.n_initial, p.body.keys.size());
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
