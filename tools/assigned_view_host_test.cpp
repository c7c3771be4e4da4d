// assigned_view_host_test.cpp -- the assigned set of a solved batch (acvm_amd/csrc/assigned_view.hpp) as a plain C++ program: no HIP, no
// handle. tests/test_assigned_view_on_host.py compiles it and judges its answers by a Python restatement; `make asan` builds it a second
// time with the sanitizers (tools/asan/assigned_view_host_test), for the same command stream.
//
//   g++ -std=c++17 -O1 tools/assigned_view_host_test.cpp -o assigned_view_host_test
//
// Commands on stdin, one per line. A list is comma separated, `e` an empty array, `null` a null pointer.
//   batch N_WITNESSES N_SLOW PRODUCER SLOW_INDEX BITMAP    what the following calls see: PRODUCER [N_WITNESSES], SLOW_INDEX per instance (-1: solved
//                                                          by the level kernels; null: instance j is lane j), BITMAP [ceil(N_WITNESSES / 32)][N_SLOW] words
//   assigned J W ...                     pairs (instance, witness), asked of ONE view
//   fill FIRST N ALL|LEVEL WHOLE SEL     WHOLE 1: the view is given the whole bitmap, 0: it copies rows; SEL null: the whole map
//   missing FIRST N LIST
// Answers, each followed by ` | ` and the rows the view copied, in order (`-`: none):
//   assigned 0|1 ...
//   fill FLAGS VALUES       per element of [N][len(SEL)]: the flag (`.`: untouched), and z = the 32 bytes are zero, k = kept, ? = anything else
//   missing J W  |  missing none
#include "../acvm_amd/csrc/assigned_view.hpp"
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

using namespace acvm;

// an array of exactly the listed size on the heap, so that a read past its end is one the sanitizer sees
template <class T>
struct List {
    std::unique_ptr<T[]> p;
    size_t n = 0;
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
        for (std::string item; std::getline(ss, item, ',');) v.push_back((T)std::stoll(item));
    }
    l.n = v.size();
    l.p.reset(new T[v.size()]);
    for (size_t i = 0; i < v.size(); i++) l.p[i] = v[i];
    return l;
}

int main() {
    uint32_t nw = 0, n_slow = 0;
    List<uint32_t> producer, bitmap;
    List<int32_t> slow_index;
    std::vector<uint32_t> copied;
    auto view = [&](bool whole) {
        copied.clear();
        if (whole) return AssignedView(producer.data(), nw, slow_index.data(), n_slow, bitmap.data());
        return AssignedView(producer.data(), nw, slow_index.data(), n_slow, [&](uint32_t word, uint32_t *row) {
            copied.push_back(word);
            memcpy(row, bitmap.data() + (size_t)word * n_slow, (size_t)n_slow * 4);
            return true;
        });
    };
    auto end_line = [&] {
        printf(" | ");
        if (copied.empty()) printf("-");
        for (size_t i = 0; i < copied.size(); i++) printf(i ? ",%u" : "%u", copied[i]);
        printf("\n");
    };
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "batch") {
            in >> nw >> n_slow;
            producer = read_list<uint32_t>(in);
            slow_index = read_list<int32_t>(in);
            bitmap = read_list<uint32_t>(in);
            if (producer.n != nw || bitmap.n != (size_t)((nw + 31) / 32) * n_slow) { fprintf(stderr, "batch: sizes disagree\n"); return 2; }
        } else if (cmd == "assigned") {
            AssignedView av = view(false);
            printf("assigned");
            for (uint32_t j, w; in >> j >> w;) printf(" %d", (int)av.assigned(j, w));
            end_line();
        } else if (cmd == "fill") {
            uint32_t first, n;
            std::string lanes;
            int whole;
            in >> first >> n >> lanes >> whole;
            const List<uint32_t> sel = read_list<uint32_t>(in);
            const uint32_t n_sel = sel.null ? nw : (uint32_t)sel.n;
            const size_t cells = (size_t)n * n_sel;
            std::unique_ptr<uint8_t[]> flags(new uint8_t[cells]), values(new uint8_t[cells * 32]);
            memset(flags.get(), 7, cells);
            memset(values.get(), 0xAB, cells * 32);
            AssignedView av = view(whole != 0);
            av.fill(first, n, sel.data(), n_sel, flags.get(), values.get(), lanes == "LEVEL" ? AssignedView::LEVEL_ONLY : AssignedView::ALL);
            std::string f, v;
            for (size_t c = 0; c < cells; c++) {
                f += flags[c] == 7 ? '.' : flags[c] == 0 ? '0' : flags[c] == 1 ? '1' : '?';
                size_t zeros = 0, kept = 0;
                for (int k = 0; k < 32; k++) { zeros += values[c * 32 + k] == 0; kept += values[c * 32 + k] == 0xAB; }
                v += zeros == 32 ? 'z' : kept == 32 ? 'k' : '?';
            }
            printf("fill %s %s", cells ? f.c_str() : "e", cells ? v.c_str() : "e");
            end_line();
            // the same call with either array null touches the other alike (and nothing else: the sanitizer's part)
            std::unique_ptr<uint8_t[]> flags2(new uint8_t[cells]), values2(new uint8_t[cells * 32]);
            memset(flags2.get(), 7, cells);
            memset(values2.get(), 0xAB, cells * 32);
            AssignedView a2 = view(whole != 0), a3 = view(whole != 0);
            a2.fill(first, n, sel.data(), n_sel, flags2.get(), nullptr, lanes == "LEVEL" ? AssignedView::LEVEL_ONLY : AssignedView::ALL);
            a3.fill(first, n, sel.data(), n_sel, nullptr, values2.get(), lanes == "LEVEL" ? AssignedView::LEVEL_ONLY : AssignedView::ALL);
            if (memcmp(flags.get(), flags2.get(), cells) || memcmp(values.get(), values2.get(), cells * 32)) { fprintf(stderr, "fill: a null array changed the other\n"); return 3; }
        } else if (cmd == "missing") {
            uint32_t first, n, j = 0, w = 0;
            in >> first >> n;
            const List<uint32_t> list = read_list<uint32_t>(in);
            AssignedView av = view(false);
            if (av.first_missing(first, n, list.data(), (uint32_t)list.n, &j, &w)) printf("missing %u %u", j, w);
            else printf("missing none");
            end_line();
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
