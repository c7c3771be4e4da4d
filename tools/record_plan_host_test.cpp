// record_plan_host_test.cpp -- the checks, the field table and the window cut of the record import (acvm_amd/csrc/record_plan.cpp) as a plain
// C++ program: no HIP, no handle. tests/test_record_plan_on_host.py compiles it -- once plainly, once with the sanitizers, as `make asan` does
// (tools/asan/record_plan_host_test) -- and judges its answers by a Python restatement.
//
//   g++ -std=c++17 -O1 tools/record_plan_host_test.cpp acvm_amd/csrc/record_plan.cpp acvm_amd/csrc/import_plan.cpp -o record_plan_host_test
//
// Commands on stdin, one per line. A list is comma separated, `e` an empty array, `null` a null pointer.
//   view B n_in IDS ROWS PLANES      the handle the following calls see (PLANES null: a circuit without byte planes)
//   noview                           the null batch
//   records PITCH PTR N_FIELDS { POSITION ENCODING OFFSET } x N_FIELDS     (records null: a null descriptor; N_FIELDS `nullN`: null fields, n_fields N)
//   plain PTR                        the plain plan of the view (another plan kind, for eq)
//   eq                               whether the last two plans compare equal
//   cap                              the window cap in bytes
// Answers: `err CODE TEXT`, `eq 0|1`, `cap N`, or
//   ok RECORDS PITCH N_WINDOWS N_PARTS { OFFSET LENGTH FIRST_FIELD N_FIELDS } x N_WINDOWS { ROW PLANE ENCODING BYTE } x fields
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
    printf("ok %d %" PRIu64 " %u %zu", (int)p.records, p.record_pitch, p.record_windows, p.parts.size());
    const size_t head = p.records ? (size_t)p.record_windows * RECORD_WINDOW_WORDS : 0;
    for (size_t w = 0; w < head; w += RECORD_WINDOW_WORDS)
        printf(" %" PRIu64 " %u %u %u", ((uint64_t)p.lists[w + RECORD_WINDOW_OFFSET_HI] << 32) | p.lists[w + RECORD_WINDOW_OFFSET_LO], p.lists[w + RECORD_WINDOW_LENGTH],
               p.lists[w + RECORD_WINDOW_FIRST_FIELD], p.lists[w + RECORD_WINDOW_N_FIELDS]);
    for (size_t f = head; p.records && f < p.lists.size(); f++) printf(" %u", p.lists[f]);
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
        else if (cmd == "cap") printf("cap %u\n", RECORD_PLAN_WINDOW_CAP);
        else if (cmd == "plain") {
            uint64_t ptr;
            in >> ptr;
            ImportPlan plan = import_plan_plain(view.n_in, (const void *)(uintptr_t)ptr);
            answer(0, "", plan);
        } else if (cmd == "records") {
            std::string first, count;
            in >> first;
            acvm_record_desc_t d{};
            uint64_t ptr = 0;
            std::unique_ptr<acvm_record_field_t[]> fields;  // exactly n_fields entries on the heap
            if (first != "null") {
                d.pitch = std::stoull(first);
                in >> ptr >> count;
                if (count.rfind("null", 0) == 0) d.n_fields = (uint32_t)std::stoull(count.substr(4));
                else {
                    d.n_fields = (uint32_t)std::stoull(count);
                    fields.reset(new acvm_record_field_t[d.n_fields]);
                    for (uint32_t f = 0; f < d.n_fields; f++) in >> fields[f].position >> fields[f].encoding >> fields[f].offset;
                    d.fields = fields.get();
                }
            }
            ImportPlan plan;
            std::string err;
            const int rc = import_plan_records(have_view ? &view : nullptr, first == "null" ? nullptr : &d, (const void *)(uintptr_t)ptr, &plan, &err);
            answer(rc, err, plan);
        } else if (cmd == "eq") printf("eq %d\n", (int)(last == before));
        else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
