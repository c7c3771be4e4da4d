// import_plan_host_test.cpp -- the checks and the list layout of the device imports (acvm_amd/csrc/import_plan.cpp) as a plain C++ program:
// no HIP, no handle. tests/test_import_plan_on_host.py compiles it and judges its answers by a Python restatement; `make asan` builds it a
// second time with the sanitizers (tools/asan/import_plan_host_test), for the same command stream.
//
//   g++ -std=c++17 -O1 tools/import_plan_host_test.cpp acvm_amd/csrc/import_plan.cpp -o import_plan_host_test
//
// Commands on stdin, one per line. A list is comma separated, `e` an empty array, `null` a null pointer.
//   view B n_in IDS ROWS PLANES      the handle the following calls see (PLANES null: a circuit without byte planes)
//   noview                           the null batch
//   plain PTR
//   desc ENCODING LAYOUT N_COLUMNS STRIDE PTR COLUMNS          (desc null: a null descriptor)
//   parts N_PARTS { PTR ENCODING LAYOUT N N_COLUMNS STRIDE POSITIONS COLUMNS } x N_PARTS       (parts null N: a null array)
//   eq                               whether the last two plans compare equal
// Answers: `err CODE TEXT`, `eq 0|1`, or
//   ok PLAIN N_PARTS { ENCODING LAYOUT ELEM_SIZE STRIDE N PTR RESIDENT ROWS_AT PLANES_AT COLUMNS_AT } x N_PARTS LISTS      (-1: no such list)
#include "../acvm_amd/csrc/import_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

// a caller's host array of exactly the listed size on the heap, so that a read past its end is one the sanitizer sees
struct List {
    std::unique_ptr<uint32_t[]> p;
    size_t n = 0;
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
    l.n = v.size();
    l.p.reset(new uint32_t[v.size()]);
    for (size_t i = 0; i < v.size(); i++) l.p[i] = v[i];
    return l;
}
static long long at(size_t x) { return x == IMPORT_NO_LIST ? -1 : (long long)x; }
static void print_plan(const ImportPlan &p) {
    printf("ok %d %zu", (int)p.plain, p.parts.size());
    for (const ImportPlanPart &q : p.parts)
        printf(" %u %u %u %" PRIu64 " %u %" PRIu64 " %d %lld %lld %lld", q.encoding, q.layout, q.elem_size, q.stride, q.n, (uint64_t)(uintptr_t)q.d_values, (int)q.resident, at(q.rows_at),
               at(q.planes_at), at(q.columns_at));
    printf(" ");
    if (p.lists.empty()) printf("e");
    for (size_t i = 0; i < p.lists.size(); i++) printf(i ? ",%u" : "%u", p.lists[i]);
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
        else if (cmd == "plain") {
            uint64_t ptr;
            in >> ptr;
            ImportPlan plan = import_plan_plain(view.n_in, (const void *)(uintptr_t)ptr);
            answer(0, "", plan);
        } else if (cmd == "desc") {
            std::string first;
            in >> first;
            acvm_import_desc_t d{};
            uint64_t ptr = 0;
            List columns;
            if (first != "null") {
                d.encoding = (uint32_t)std::stoull(first);
                in >> d.layout >> d.n_columns >> d.stride >> ptr;
                columns = read_list(in);
                d.columns = columns.data();
            }
            ImportPlan plan;
            std::string err;
            const int rc = import_plan_desc(have_view ? &view : nullptr, first == "null" ? nullptr : &d, (const void *)(uintptr_t)ptr, &plan, &err);
            answer(rc, err, plan);
        } else if (cmd == "parts") {
            std::string first;
            in >> first;
            uint32_t n_parts;
            const bool null_array = first == "null";
            if (null_array) in >> n_parts;
            else n_parts = (uint32_t)std::stoull(first);
            std::vector<acvm_import_part_t> parts(null_array ? 0 : n_parts);
            std::vector<List> lists;
            for (acvm_import_part_t &pt : parts) {
                uint64_t ptr;
                in >> ptr >> pt.encoding >> pt.layout >> pt.n >> pt.n_columns >> pt.stride;
                pt.d_values = (const void *)(uintptr_t)ptr;
                lists.push_back(read_list(in));
                pt.positions = lists.back().data();
                lists.push_back(read_list(in));
                pt.columns = lists.back().data();
            }
            ImportPlan plan;
            std::string err;
            const int rc = import_plan_parts(have_view ? &view : nullptr, null_array ? nullptr : parts.data(), n_parts, &plan, &err);
            answer(rc, err, plan);
        } else if (cmd == "eq") printf("eq %d\n", (int)(last == before));
        else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
