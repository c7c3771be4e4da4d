// record_mask_plan_host_test.cpp -- the checks, the unit placement and the tables of the masked record import (acvm_amd/csrc/record_plan.cpp
// import_plan_records_masked) as a plain C++ program: no HIP, no handle. tests/test_record_mask_plan_on_host.py compiles it -- once plainly, once
// with the sanitizers, as `make asan` does (tools/asan/record_mask_plan_host_test) -- and judges its answers by a Python restatement.
//
//   g++ -std=c++17 -O1 tools/record_mask_plan_host_test.cpp acvm_amd/csrc/record_plan.cpp acvm_amd/csrc/import_plan.cpp -o record_mask_plan_host_test
//
// Commands on stdin, one per line. A list is comma separated, `e` an empty array, `null` a null pointer.
//   view B n_in IDS ROWS PLANES      the handle the following calls see (PLANES null: a circuit without byte planes)
//   noview                           the null batch
//   records PITCH PTR N_FIELDS { POSITION ENCODING OFFSET } x N_FIELDS           the unmasked plan (import_plan_records)
//   masked PITCH PTR N_FIELDS { POSITION ENCODING OFFSET MASK } x N_FIELDS       MASK: a byte offset, or `n` = ACVM_RECORD_NO_MASK
//                                    (masked null: a null descriptor; N_FIELDS `nullN`: null fields, n_fields N)
//   eq                               whether the last two plans compare equal
//   strides                          the words per window and per field of the masked tables, and the two special mask words
// Answers: `err CODE TEXT`, `eq 0|1`, `strides WINDOW FIELD NONE FAR`, or
//   ok RECORDS MASKS PITCH N_WINDOWS N_PARTS then every word of the plan's lists
#include "../acvm_amd/csrc/record_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

// a caller's host array of exactly the listed size on the heap, so that a read past its end is one the sanitizer sees
struct List {
    std::unique_ptr<uint32_t[]> p;
    bool null = true;
    const uint32_t *data() const { return null ? nullptr : p.get(); }
};
static List read_list(std::istream &in) {
    std::string tok;
    in >> tok;
    List l;
    if (tok == "null") return l;
    l.null = false;
    std::vector<uint32_t> v;
    if (tok != "e") {
        std::stringstream ss(tok);
        for (std::string item; std::getline(ss, item, ',');) v.push_back((uint32_t)std::stoull(item));
    }
    l.p.reset(new uint32_t[v.size()]);
    for (size_t i = 0; i < v.size(); i++) l.p[i] = v[i];
    return l;
}
static void print_plan(const ImportPlan &p) {
    printf("ok %d %d %" PRIu64 " %u %zu", (int)p.records, (int)p.record_masks, p.record_pitch, p.record_windows, p.parts.size());
    for (uint32_t w : p.lists) printf(" %u", w);
    printf("\n");
}

int main() {
    ImportView view;
    List ids, rows, planes;
    bool have_view = false;
    ImportPlan last, before;
    auto answer = [&](int rc, const std::string &err, ImportPlan &plan) {
        if (rc) { printf("err %d %s\n", rc, err.c_str()); return; }
        print_plan(plan);
        before = std::move(last);
        last = std::move(plan);
    };
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "view") {
            in >> view.B >> view.n_in;
            ids = read_list(in);
            rows = read_list(in);
            planes = read_list(in);
            view.ids = ids.data();
            view.rows = rows.data();
            view.planes = planes.data();
            have_view = true;
        } else if (cmd == "noview") have_view = false;
        else if (cmd == "strides") printf("strides %u %u %u %u\n", RECORD_MWINDOW_WORDS, RECORD_MFIELD_WORDS, RECORD_MASK_NONE, RECORD_MASK_FAR);
        else if (cmd == "records" || cmd == "masked") {
            const bool masked = cmd == "masked";
            std::string first, count;
            in >> first;
            uint64_t pitch = 0, ptr = 0;
            uint32_t n_fields = 0;
            bool null_fields = true;
            std::unique_ptr<acvm_record_field_t[]> plain;  // exactly n_fields entries on the heap
            std::unique_ptr<acvm_record_masked_field_t[]> with_masks;
            if (first != "null") {
                pitch = std::stoull(first);
                in >> ptr >> count;
                if (count.rfind("null", 0) == 0) n_fields = (uint32_t)std::stoull(count.substr(4));
                else {
                    n_fields = (uint32_t)std::stoull(count);
                    null_fields = false;
                    plain.reset(new acvm_record_field_t[n_fields]);
                    with_masks.reset(new acvm_record_masked_field_t[n_fields]);
                    for (uint32_t f = 0; f < n_fields; f++) {
                        in >> plain[f].position >> plain[f].encoding >> plain[f].offset;
                        with_masks[f] = acvm_record_masked_field_t{plain[f].position, plain[f].encoding, plain[f].offset, ACVM_RECORD_NO_MASK};
                        if (masked) {
                            std::string m;
                            in >> m;
                            if (m != "n") with_masks[f].mask_offset = std::stoull(m);
                        }
                    }
                }
            }
            ImportPlan plan;
            std::string err;
            int rc;
            if (masked) {
                const acvm_record_masked_desc_t d{pitch, null_fields ? nullptr : with_masks.get(), n_fields};
                rc = import_plan_records_masked(have_view ? &view : nullptr, first == "null" ? nullptr : &d, (const void *)(uintptr_t)ptr, &plan, &err);
            } else {
                const acvm_record_desc_t d{pitch, null_fields ? nullptr : plain.get(), n_fields};
                rc = import_plan_records(have_view ? &view : nullptr, first == "null" ? nullptr : &d, (const void *)(uintptr_t)ptr, &plan, &err);
            }
            answer(rc, err, plan);
        } else if (cmd == "eq") printf("eq %d\n", (int)(last == before));
        else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
