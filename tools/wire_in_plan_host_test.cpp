// wire_in_plan_host_test.cpp -- the checks, the key table, the CRC power table and the host form's judgement of a row of the batch-wide wire
// import (acvm_amd/csrc/wire_in_plan.cpp) as a plain C++ program: no HIP, no handle. tests/test_wire_in_plan_on_host.py compiles it -- once
// plainly, once with the sanitizers, as `make asan` does (tools/asan/wire_in_plan_host_test) -- and judges its answers by tests/wire_ref.py.
//
//   g++ -std=c++17 -O1 tools/wire_in_plan_host_test.cpp acvm_amd/csrc/wire_in_plan.cpp acvm_amd/csrc/wire_plan.cpp -o wire_in_plan_host_test
//
// Commands on stdin, one per line.
//   live B / nolive                  the live instance count the following calls see / the null batch
//   ids N { ID } x N                 the handle's initial ids, in the order it was created with
//   plan CONTAINER PITCH PTR DEVICE  DEVICE 0 | 1: the device form (plan null: a null descriptor)
//   canonical BODY                   BODY as hex (`-`: no bytes): is it a row the device form reads as it is, for the ids above
//   ofmap N { ID VALUE } x N         the map the reader made of a row (VALUE: 32 bytes as hex) as a canonical body
//   stagepitch N_INITIAL
// Answers: `err CODE TEXT`, a number, `ok BODY`, or
//   ok CONTAINER PITCH N_INITIAL N_WINDOWS RANK_BITS X64 { KEY } x N_INITIAL { POSITION } x N_INITIAL N_POW { POW }
#include "../acvm_amd/csrc/wire_in_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

static bool parse_hex(const std::string &hex, std::unique_ptr<uint8_t[]> &out, size_t &n) {
    n = hex == "-" ? 0 : hex.size() / 2;
    out.reset(new uint8_t[n]);  // exactly n bytes on the heap: a read past the end is one the sanitizer sees
    for (size_t i = 0; i < n; i++) {
        unsigned v = 0;
        if (sscanf(hex.c_str() + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}

int main() {
    uint32_t live = 0, n_ids = 0;
    bool have_live = false;
    std::unique_ptr<uint32_t[]> ids(new uint32_t[0]);
    auto table = [&](WireInPlan &plan) {  // the plan the row judgements use: the host form's
        const acvm_wire_in_desc_t d{ACVM_WIRE_BINCODE, 1};
        const uint32_t one = 1;
        std::string err;
        return wire_in_plan(&one, ids.get(), n_ids, &d, &d, false, &plan, &err) == 0;
    };
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "live") { in >> live; have_live = true; }
        else if (cmd == "nolive") have_live = false;
        else if (cmd == "ids") {
            in >> n_ids;
            ids.reset(new uint32_t[n_ids]);
            for (uint32_t k = 0; k < n_ids; k++) in >> ids[k];
        } else if (cmd == "stagepitch") {
            uint32_t n = 0;
            in >> n;
            printf("%" PRIu64 "\n", wire_in_stage_pitch(n));
        } else if (cmd == "plan") {
            std::string first;
            in >> first;
            acvm_wire_in_desc_t d{};
            uint64_t ptr = 0;
            int device = 1;
            if (first != "null") {
                d.container = (uint32_t)std::stoull(first);
                in >> d.pitch >> ptr >> device;
            }
            WireInPlan plan;
            std::string err;
            const int rc = wire_in_plan(have_live ? &live : nullptr, ids.get(), n_ids, first == "null" ? nullptr : &d, (const void *)(uintptr_t)ptr, device != 0, &plan, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            if (plan.keys.size() != n_ids || plan.positions.size() != n_ids) { fprintf(stderr, "table size\n"); return 3; }
            printf("ok %u %" PRIu64 " %u %u %u %u", plan.container, plan.pitch, plan.n_initial, plan.n_windows, plan.rank_bits, plan.crc_x64);
            for (uint32_t k : plan.keys) printf(" %u", k);
            for (uint32_t k : plan.positions) printf(" %u", k);
            printf(" %zu", plan.crc_pow.size());
            for (uint32_t t : plan.crc_pow) printf(" %u", t);
            printf("\n");
        } else if (cmd == "canonical") {
            std::string hex;
            in >> hex;
            std::unique_ptr<uint8_t[]> body;
            size_t n = 0;
            WireInPlan plan;
            if (!parse_hex(hex, body, n) || !table(plan)) return 2;
            printf("%d\n", (int)wire_in_body_canonical(plan, body.get(), n));
        } else if (cmd == "ofmap") {
            size_t n = 0;
            in >> n;
            std::unique_ptr<uint32_t[]> keys(new uint32_t[n]);
            std::unique_ptr<uint8_t[]> values(new uint8_t[32 * n]);
            for (size_t i = 0; i < n; i++) {
                std::string hex;
                in >> keys[i] >> hex;
                std::unique_ptr<uint8_t[]> v;
                size_t m = 0;
                if (!parse_hex(hex, v, m) || m != 32) return 2;
                std::copy(v.get(), v.get() + 32, values.get() + 32 * i);
            }
            WireInPlan plan;
            if (!table(plan)) return 2;
            std::vector<uint8_t> body;
            std::string err;
            const int rc = wire_in_body_of_map(plan, keys.get(), values.get(), n, &body, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            if (!wire_in_body_canonical(plan, body.data(), body.size())) { fprintf(stderr, "the writer's body is not canonical\n"); return 3; }
            printf("ok ");
            for (uint8_t b : body) printf("%02x", b);
            printf("\n");
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
