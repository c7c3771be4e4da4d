// record_out_plan_host_test.cpp -- the checks, the window cut, the cover bitmaps and the field table of the record export
// (acvm_amd/csrc/record_out_plan.cpp) as a plain C++ program: no HIP, no handle. tests/test_record_out_plan_on_host.py compiles it -- once
// plainly, once with the sanitizers, as `make asan` does (tools/asan/record_out_plan_host_test) -- and judges its answers by a Python restatement.
//
//   g++ -std=c++17 -O1 tools/record_out_plan_host_test.cpp acvm_amd/csrc/record_out_plan.cpp acvm_amd/csrc/import_plan.cpp -o record_out_plan_host_test
//
// Commands on stdin, one per line.
//   live B                           the live instance count the following calls see
//   nolive                           the null batch
//   out PITCH PTR FIRST N LIST N_FIELDS { WITNESS ENCODING OFFSET MASK_OFFSET } x N_FIELDS
//                                    LIST 0 | 1: the call has an instance list; MASK_OFFSET `-`: ACVM_RECORD_NO_MASK
//                                    (out null: a null descriptor; N_FIELDS `nullN`: null fields, n_fields N)
//   cap                              the window cap in bytes
// Answers: `err CODE TEXT`, `cap N`, or
//   ok PITCH FIRST N N_WINDOWS N_ENTRIES MONT256 PLAIN N_DISTINCT { WITNESS } x N_DISTINCT
//      { OFFSET LENGTH FIRST_ENTRY N_ENTRIES BITMAP x 8 } x N_WINDOWS { WITNESS ENCODING BYTE KIND } x N_ENTRIES
#include "../acvm_amd/csrc/record_out_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

int main() {
    uint32_t live = 0;
    bool have_live = false;
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "live") { in >> live; have_live = true; }
        else if (cmd == "nolive") have_live = false;
        else if (cmd == "cap") printf("cap %u\n", RECORD_PLAN_WINDOW_CAP);
        else if (cmd == "out") {
            std::string first, count;
            in >> first;
            acvm_record_out_desc_t d{};
            uint64_t ptr = 0;
            int list = 0;
            std::unique_ptr<acvm_record_out_field_t[]> fields;  // exactly n_fields entries on the heap: a read past the end is one the sanitizer sees
            if (first != "null") {
                d.pitch = std::stoull(first);
                in >> ptr >> d.first >> d.n >> list >> count;
                if (count.rfind("null", 0) == 0) d.n_fields = (uint32_t)std::stoull(count.substr(4));
                else {
                    d.n_fields = (uint32_t)std::stoull(count);
                    fields.reset(new acvm_record_out_field_t[d.n_fields]);
                    for (uint32_t f = 0; f < d.n_fields; f++) {
                        std::string mask;
                        in >> fields[f].witness >> fields[f].encoding >> fields[f].offset >> mask;
                        fields[f].mask_offset = mask == "-" ? ACVM_RECORD_NO_MASK : std::stoull(mask);
                    }
                    d.fields = fields.get();
                }
            }
            RecordOutPlan plan;
            std::string err;
            const int rc = record_out_plan(have_live ? &live : nullptr, first == "null" ? nullptr : &d, list != 0, (const void *)(uintptr_t)ptr, &plan, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            printf("ok %" PRIu64 " %u %u %u %u %d %d %zu", plan.pitch, plan.first, plan.n, plan.n_windows, plan.n_entries, (int)plan.mont256, (int)plan.plain, plan.witnesses.size());
            for (uint32_t w : plan.witnesses) printf(" %u", w);
            const size_t head = (size_t)plan.n_windows * RECORD_OUT_WINDOW_WORDS;
            if (plan.tables.size() != head + (size_t)plan.n_entries * RECORD_OUT_FIELD_WORDS) { fprintf(stderr, "table size\n"); return 3; }
            for (size_t w = 0; w < head; w += RECORD_OUT_WINDOW_WORDS) {
                printf(" %" PRIu64 " %u %u %u", ((uint64_t)plan.tables[w + RECORD_WINDOW_OFFSET_HI] << 32) | plan.tables[w + RECORD_WINDOW_OFFSET_LO], plan.tables[w + RECORD_WINDOW_LENGTH],
                       plan.tables[w + RECORD_WINDOW_FIRST_FIELD], plan.tables[w + RECORD_WINDOW_N_FIELDS]);
                for (uint32_t k = 0; k < RECORD_OUT_BITMAP_WORDS; k++) printf(" %u", plan.tables[w + RECORD_OUT_WINDOW_BITMAP + k]);
            }
            for (size_t f = head; f < plan.tables.size(); f++) printf(" %u", plan.tables[f]);
            printf("\n");
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
