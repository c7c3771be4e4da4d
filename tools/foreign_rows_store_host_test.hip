// Host-side execution of the per-row append of the foreign-call result store (acvm_amd/csrc/foreign_store.hpp is __host__ __device__): what a lane of
// kernels_foreign.hip fc_append_rows_kernel and fc_answers_max_kernel runs -- the mask, the row's own lengths summed in 64 bits, the bound checks against
// the caller's columns and the slot's capacity, the shape words from the row's lengths, the decoded values, the count last -- on tables, length and mask
// columns and a value buffer of exactly the stated size on the heap. The tool judges nothing: tests/test_foreign_rows_on_host.py compares its answers
// with a Python restatement.
//   new BP DESC_WORDS VALS_CAP                                  zeroed tables of that capacity at instance stride BP
//   rows ENCODING N_COLUMNS IS_ARRAY SHAPE_LENS JS LENS MASK VALUES
//        one call for len(JS) rows, row i into instance column JS[i]. IS_ARRAY, SHAPE_LENS: the host shape (`e`: no outputs). LENS: the device column
//        [n_rows][n_values] flat, or `null`. MASK: [n_rows], or `null`. VALUES: n_rows x N_COLUMNS elements, instance-major and dense, hex digits of
//        the bytes as they lie in memory, comma separated (`e`: none)
//        -> "max M" (what the sizing launch reduces), then per row "appended|left_out|refused WORD VALUE N_RESULTS" (the walk before the append)
//   walk J | column J | values J N                              as tools/foreign_store_host_test.hip
#include "../acvm_amd/csrc/foreign_store.hpp"
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
using namespace acvm;

static bool read_list(std::istream &in, std::vector<uint32_t> *v) {  // false: `null`
    std::string tok;
    in >> tok;
    v->clear();
    if (tok == "null") return false;
    if (tok == "e") return true;
    std::stringstream ss(tok);
    for (std::string item; std::getline(ss, item, ',');) v->push_back((uint32_t)std::stoull(item));
    return true;
}

int main() {
    uint64_t Bp = 0;
    uint32_t desc_words = 0, vals_cap = 0;
    std::unique_ptr<uint32_t[]> desc;
    std::unique_ptr<uint4[]> vals;
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "new") {
            in >> Bp >> desc_words >> vals_cap;
            desc.reset(new uint32_t[(size_t)desc_words * Bp]());
            vals.reset(new uint4[(size_t)vals_cap * 2 * Bp]());
        } else if (cmd == "rows") {
            uint32_t encoding = 0, n_columns = 0;
            in >> encoding >> n_columns;
            std::vector<uint32_t> is_array, shape_lens, js, lens, mask;
            read_list(in, &is_array);
            read_list(in, &shape_lens);
            read_list(in, &js);
            const bool have_lens = read_list(in, &lens), have_mask = read_list(in, &mask);
            const size_t n = js.size();
            std::vector<uint32_t> shape = {(uint32_t)is_array.size()};
            for (size_t k = 0; k < is_array.size(); k++) { shape.push_back(is_array[k] ? 1u : 0u); shape.push_back(is_array[k] ? (have_lens ? 0u : shape_lens[k]) : 1u); }
            // the caller's columns: heap arrays of exactly their size
            std::unique_ptr<uint32_t[]> d_lens(new uint32_t[lens.size()]);
            for (size_t i = 0; i < lens.size(); i++) d_lens[i] = lens[i];
            std::unique_ptr<uint8_t[]> d_mask(new uint8_t[mask.size()]);
            for (size_t i = 0; i < mask.size(); i++) d_mask[i] = (uint8_t)mask[i];
            const uint32_t size = export_element_size(encoding);
            const size_t bytes = n * n_columns * size;
            std::unique_ptr<uint4[]> buf(new uint4[(bytes + 15) / 16]());
            uint8_t *p = (uint8_t *)buf.get();
            std::string tok;
            in >> tok;
            if (tok != "e") {
                std::stringstream ss(tok);
                size_t c = 0;
                for (std::string item; std::getline(ss, item, ','); c++)
                    for (uint32_t q = 0; q < size; q++) p[c * size + q] = (uint8_t)std::stoul(item.substr(2 * q, 2), nullptr, 16);
            }
            const FcRowAnswers sizing{have_lens ? d_lens.get() : nullptr, have_mask ? d_mask.get() : nullptr, 0u};
            uint32_t longest = 0;
            for (size_t r = 0; r < n; r++) {
                const uint32_t t = fc_row_total_saturated(shape.data(), sizing, r);
                longest = t > longest ? t : longest;
            }
            printf("max %u\n", longest);
            const FcRowAnswers ra{sizing.lens, sizing.answered, n_columns};
            const FcAnswers a{p, encoding, EXPORT_INSTANCE_MAJOR, n_columns ? n_columns : 1u};
            for (size_t r = 0; r < n; r++) {
                const FcAppendPos before = fc_store_walk(desc.get(), Bp, js[r], desc_words);
                const FcRowAppend how = fc_store_append_row(desc.get(), vals.get(), Bp, js[r], desc_words, vals_cap, shape.data(), ra, a, r);
                printf("%s %u %u %u\n", how == FC_ROW_APPENDED ? "appended" : how == FC_ROW_LEFT_OUT ? "left_out" : "refused", before.word, before.value, before.n_results);
            }
        } else if (cmd == "walk") {
            uint64_t j = 0;
            in >> j;
            const FcAppendPos q = fc_store_walk(desc.get(), Bp, j, desc_words);
            printf("%u %u %u\n", q.word, q.value, q.n_results);
        } else if (cmd == "column") {
            uint64_t j = 0;
            in >> j;
            for (uint32_t w = 0; w < desc_words; w++) printf("%s%u", w ? " " : "", desc[(size_t)w * Bp + j]);
            printf("\n");
        } else if (cmd == "values") {
            uint64_t j = 0;
            uint32_t n = 0;
            in >> j >> n;
            for (uint32_t v = 0; v < n; v++) {
                const Fr x = fr_load(vals.get(), v, Bp, j);
                printf("%s", v ? " " : "");
                for (int i = 7; i >= 0; i--) printf("%08x", x.v[i]);
            }
            printf("\n");
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
