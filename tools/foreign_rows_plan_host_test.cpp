// foreign_rows_plan_host_test.cpp -- the host-only part of acvm_batch_resolve_foreign_calls_device_rows (acvm_amd/csrc/foreign_plan.cpp): the refusals
// in their order, the lanes a mask resumes, the width check behind the sizing launch and the capacity bounds from a per-row maximum, as a plain C++
// program: no HIP, no handle. tests/test_foreign_rows_on_host.py compiles it plain and with the sanitizers and judges its answers by a Python
// restatement; `make asan` builds tools/asan/foreign_rows_plan_host_test.
//
//   g++ -std=c++17 -O1 tools/foreign_rows_plan_host_test.cpp acvm_amd/csrc/foreign_plan.cpp acvm_amd/csrc/import_plan.cpp -o foreign_rows_plan_host_test
//
// Commands on stdin, one per line. A list is comma separated, `e` an empty array, `null` a null pointer; pointers are plain numbers.
//   clear | lane INSTANCE STATUS OPCODE BRILLIG RESOLVED | view SOLVED HAS_SOLVER SITE_INTERNAL       as tools/foreign_plan_host_test.cpp
//   answers OPCODE BRILLIG FIRST N N_VALUES IS_ARRAY LENS ENCODING LAYOUT N_COLUMNS STRIDE D_VALUES D_LENS D_ANSWERED
//   resumes OPCODE BRILLIG FIRST N MASK            the mask as the call downloaded it ([N], or null)
//   width N_COLUMNS LONGEST HAS_VALUES             LONGEST: the sizing launch's answer
//   slot BOUND_WORDS BOUND_VALS HAVE_WORDS HAVE_VALS | call ADD_WORDS ADD_VALS | fold               as tools/foreign_plan_host_test.cpp
// Answers: `err CODE TEXT`, or
//   ok STRIDE TOTAL WORDS...                       (answers)
//   ok N { LANE INSTANCE } x N                     (resumes)
//   ok TOTAL                                       (width)
//   ok GROW WORDS VALS | ok BOUND_WORDS BOUND_VALS ROUND_WORDS ROUND_VALS   (call; fold)
#include "../acvm_amd/csrc/foreign_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

// a caller's host array of exactly the listed size on the heap, so that a read past its end is one the sanitizer sees
template <class T>
struct List {
    std::unique_ptr<T[]> p;
    bool null = true;
    const T *data() const { return null ? nullptr : p.get(); }
};
template <class T>
static List<T> read_list(std::istream &in) {
    std::string tok;
    in >> tok;
    List<T> l;
    if (tok == "null") return l;
    l.null = false;
    std::vector<T> v;
    if (tok != "e") {
        std::stringstream ss(tok);
        for (std::string item; std::getline(ss, item, ',');) v.push_back((T)std::stoull(item));
    }
    l.p.reset(new T[v.size()]);
    for (size_t i = 0; i < v.size(); i++) l.p[i] = v[i];
    return l;
}
template <class T>
static void read_ptr(std::istream &in, T **p) {
    uint64_t v = 0;
    in >> v;
    *p = (T *)(uintptr_t)v;
}

int main() {
    std::vector<FcLaneRecord> lanes;
    FcHandleView view;
    FcBounds slot_bounds;
    FcCapacity slot_have;
    view.solved = true;
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "clear") lanes.clear();
        else if (cmd == "lane") {
            FcLaneRecord l;
            int resolved = 0;
            in >> l.instance >> l.status >> l.opcode_index >> l.brillig_index >> resolved;
            l.resolved_new = resolved != 0;
            lanes.push_back(l);
        } else if (cmd == "view") {
            int a = 0, b = 0, c = 0;
            in >> a >> b >> c;
            view.solved = a != 0; view.has_solver = b != 0; view.site_internal = c != 0;
        } else if (cmd == "answers") {
            acvm_foreign_call_answers_rows_desc_t d{};
            in >> d.opcode_index >> d.brillig_index >> d.first_row >> d.n_rows >> d.n_values;
            const List<uint8_t> is_array = read_list<uint8_t>(in);
            const List<uint32_t> lens = read_list<uint32_t>(in);
            d.is_array = is_array.data();
            d.lens = lens.data();
            in >> d.encoding >> d.layout >> d.n_columns >> d.stride;
            read_ptr(in, &d.d_values);
            read_ptr(in, &d.d_lens);
            read_ptr(in, &d.d_answered);
            const auto list = foreign_waiting_list(lanes.data(), lanes.size(), d.opcode_index, d.brillig_index);
            uint64_t stride = 0;
            uint32_t total = 0;
            std::vector<uint32_t> words;
            std::string err;
            const int rc = foreign_check_answers_rows(&view, &d, list, &stride, &words, &total, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            printf("ok %" PRIu64 " %u", stride, total);
            for (uint32_t x : words) printf(" %u", x);
            printf("\n");
        } else if (cmd == "resumes") {
            uint32_t op = 0, bi = 0, first = 0, n = 0;
            in >> op >> bi >> first >> n;
            const List<uint8_t> mask = read_list<uint8_t>(in);
            const auto list = foreign_waiting_list(lanes.data(), lanes.size(), op, bi);
            std::vector<uint32_t> pairs;
            std::string err;
            const int rc = foreign_mask_resumes(list, first, n, mask.data(), &pairs, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            printf("ok %zu", pairs.size() / 2);
            for (uint32_t x : pairs) printf(" %u", x);
            printf("\n");
        } else if (cmd == "width") {
            uint32_t n_columns = 0, longest = 0, total = 0;
            int has_values = 0;
            in >> n_columns >> longest >> has_values;
            std::string err;
            const int rc = foreign_check_rows_width(n_columns, longest, has_values != 0, &total, &err);
            if (rc) printf("err %d %s\n", rc, err.c_str());
            else printf("ok %u\n", total);
        } else if (cmd == "slot") {
            in >> slot_bounds.words >> slot_bounds.vals >> slot_have.desc_words >> slot_have.vals_cap;
            slot_bounds.round_words = slot_bounds.round_vals = 0;
        } else if (cmd == "call") {  // one resolve call of the round: reserve, append, note the result
            uint32_t aw = 0, av = 0;
            in >> aw >> av;
            bool grow = false;
            FcCapacity want;
            std::string err;
            const int rc = foreign_capacity(slot_bounds, aw, av, slot_have, &grow, &want, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            slot_have = want;
            foreign_bounds_add(&slot_bounds, aw, av);
            printf("ok %d %u %u\n", grow ? 1 : 0, slot_have.desc_words, slot_have.vals_cap);
        } else if (cmd == "fold") {
            const FcBounds before = slot_bounds;
            foreign_bounds_fold(&slot_bounds);
            printf("ok %u %u %u %u\n", slot_bounds.words, slot_bounds.vals, before.round_words, before.round_vals);
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
