// foreign_plan_host_test.cpp -- the site list, the waiting lists, the refusals, the shape words and the capacity rule of the batch-wide foreign-call round
// trip (acvm_amd/csrc/foreign_plan.cpp) as a plain C++ program: no HIP, no handle. tests/test_foreign_plan_on_host.py compiles it and judges its answers
// by a Python restatement; `make asan` builds it a second time with the sanitizers (tools/asan/foreign_plan_host_test), for the same command stream.
//
//   g++ -std=c++17 -O1 tools/foreign_plan_host_test.cpp acvm_amd/csrc/foreign_plan.cpp acvm_amd/csrc/import_plan.cpp -o foreign_plan_host_test
//
// Commands on stdin, one per line. A list is comma separated, `e` an empty array, `null` a null pointer; pointers are plain numbers.
//   clear                                                the lanes and the declared sites are forgotten
//   decl OPCODE BRILLIG N_INPUTS INTERNAL NAME           a ForeignCall of the circuit (NAME `-`: empty)
//   lane INSTANCE STATUS OPCODE BRILLIG RESOLVED         the next exact lane
//   view SOLVED HAS_SOLVER SITE_INTERNAL                 the handle the following checks see
//   sites | list OPCODE BRILLIG | shape N_VALUES IS_ARRAY LENS
//   inputs OPCODE BRILLIG FIRST N ENCODING LAYOUT N_COLUMNS STRIDE D_VALUES D_MASK
//   width N_COLUMNS MAX D_VALUES D_MASK
//   answers OPCODE BRILLIG FIRST N N_VALUES IS_ARRAY LENS ENCODING LAYOUT N_COLUMNS STRIDE D_VALUES
//   capacity BOUND_WORDS BOUND_VALS ROUND_WORDS ROUND_VALS ADD_WORDS ADD_VALS HAVE_WORDS HAVE_VALS
//   slot BOUND_WORDS BOUND_VALS HAVE_WORDS HAVE_VALS     a device-owned slot at the start of a round
//   call ADD_WORDS ADD_VALS                              one resolve call of the round into it (reserve, note the result)
//   fold                                                 a solve consumes the round
// Answers: `err CODE TEXT`, or
//   ok N { OPCODE BRILLIG N_INPUTS N_WAITING N_RESOLVED NAME } x N      (sites; an empty name prints as -)
//   ok N { LANE INSTANCE RESOLVED } x N                                 (list)
//   ok TOTAL WORDS...                                                   (shape)
//   ok STRIDE | ok | ok STRIDE TOTAL WORDS... | ok GROW WORDS VALS      (inputs, width, answers, capacity and call: the capacities to hold)
//   ok BOUND_WORDS BOUND_VALS                                           (fold)
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
static void print_words(const std::vector<uint32_t> &w) {
    for (uint32_t x : w) printf(" %u", x);
    printf("\n");
}

int main() {
    std::vector<FcSiteDecl> decls;
    std::vector<FcLaneRecord> lanes;
    FcHandleView view;
    FcBounds slot_bounds;
    FcCapacity slot_have;
    view.solved = true;
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "clear") { decls.clear(); lanes.clear(); }
        else if (cmd == "decl") {
            FcSiteDecl d;
            int internal = 0;
            in >> d.opcode_index >> d.brillig_index >> d.n_inputs >> internal >> d.function;
            if (d.function == "-") d.function.clear();
            d.internal = internal != 0;
            decls.push_back(d);
        } else if (cmd == "lane") {
            FcLaneRecord l;
            int resolved = 0;
            in >> l.instance >> l.status >> l.opcode_index >> l.brillig_index >> resolved;
            l.resolved_new = resolved != 0;
            lanes.push_back(l);
        } else if (cmd == "view") {
            int a = 0, b = 0, c = 0;
            in >> a >> b >> c;
            view.solved = a != 0; view.has_solver = b != 0; view.site_internal = c != 0;
        } else if (cmd == "sites") {
            const auto sites = foreign_sites(decls, lanes.data(), lanes.size());
            printf("ok %zu", sites.size());
            for (auto &s : sites) printf(" %u %u %u %u %u %s", s.opcode_index, s.brillig_index, s.n_inputs, s.n_waiting, s.n_resolved, s.function[0] ? s.function : "-");
            printf("\n");
        } else if (cmd == "list") {
            uint32_t op = 0, bi = 0;
            in >> op >> bi;
            const auto list = foreign_waiting_list(lanes.data(), lanes.size(), op, bi);
            printf("ok %zu", list.size());
            for (auto &r : list) printf(" %u %u %d", r.lane, r.instance, r.resolved ? 1 : 0);
            printf("\n");
        } else if (cmd == "shape") {
            uint32_t n = 0, total = 0;
            in >> n;
            const List<uint8_t> is_array = read_list<uint8_t>(in);
            const List<uint32_t> lens = read_list<uint32_t>(in);
            std::vector<uint32_t> words;
            std::string err;
            const int rc = foreign_shape(n, is_array.data(), lens.data(), &words, &total, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            printf("ok %u", total);
            print_words(words);
        } else if (cmd == "inputs") {
            acvm_foreign_call_inputs_desc_t d{};
            in >> d.opcode_index >> d.brillig_index >> d.first_row >> d.n_rows >> d.encoding >> d.layout >> d.n_columns >> d.stride;
            read_ptr(in, &d.d_values);
            read_ptr(in, &d.d_mask);
            const auto list = foreign_waiting_list(lanes.data(), lanes.size(), d.opcode_index, d.brillig_index);
            uint64_t stride = 0;
            std::string err;
            const int rc = foreign_check_inputs(&view, &d, list, &stride, &err);
            if (rc) printf("err %d %s\n", rc, err.c_str());
            else printf("ok %" PRIu64 "\n", stride);
        } else if (cmd == "width") {
            acvm_foreign_call_inputs_desc_t d{};
            uint32_t longest = 0;
            in >> d.n_columns >> longest;
            read_ptr(in, &d.d_values);
            read_ptr(in, &d.d_mask);
            std::string err;
            const int rc = foreign_check_width(&d, longest, &err);
            if (rc) printf("err %d %s\n", rc, err.c_str());
            else printf("ok\n");
        } else if (cmd == "answers") {
            acvm_foreign_call_answers_desc_t d{};
            in >> d.opcode_index >> d.brillig_index >> d.first_row >> d.n_rows >> d.n_values;
            const List<uint8_t> is_array = read_list<uint8_t>(in);
            const List<uint32_t> lens = read_list<uint32_t>(in);
            d.is_array = is_array.data();
            d.lens = lens.data();
            in >> d.encoding >> d.layout >> d.n_columns >> d.stride;
            read_ptr(in, &d.d_values);
            const auto list = foreign_waiting_list(lanes.data(), lanes.size(), d.opcode_index, d.brillig_index);
            uint64_t stride = 0;
            uint32_t total = 0;
            std::vector<uint32_t> words;
            std::string err;
            const int rc = foreign_check_answers(&view, &d, list, &stride, &words, &total, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            printf("ok %" PRIu64 " %u", stride, total);
            print_words(words);
        } else if (cmd == "capacity") {
            uint32_t aw = 0, av = 0;
            FcBounds bounds;
            FcCapacity have, want;
            in >> bounds.words >> bounds.vals >> bounds.round_words >> bounds.round_vals >> aw >> av >> have.desc_words >> have.vals_cap;
            bool grow = false;
            std::string err;
            const int rc = foreign_capacity(bounds, aw, av, have, &grow, &want, &err);
            if (rc) printf("err %d %s\n", rc, err.c_str());
            else printf("ok %d %u %u\n", grow ? 1 : 0, want.desc_words, want.vals_cap);
        } else if (cmd == "slot") {  // a device-owned slot as batch_foreign.cpp keeps it: bounds and capacities
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
        } else if (cmd == "fold") {  // a solve consumes the round
            foreign_bounds_fold(&slot_bounds);
            printf("ok %u %u\n", slot_bounds.words, slot_bounds.vals);
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
