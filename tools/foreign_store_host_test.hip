// Host-side execution of the appending side of the foreign-call result store (acvm_amd/csrc/foreign_store.hpp is __host__ __device__): what a lane of
// kernels_foreign.hip fc_append_kernel runs -- the walk over an instance's descriptor column, the bound check, the shape words, the decoded values, the
// count last -- on tables of exactly the stated size on the heap. The tool judges nothing: it answers the commands on its standard input and
// tests/test_foreign_store_on_host.py compares the answers with the layout batch_exact.cpp upload_fc_tables writes, restated in Python.
//   new BP DESC_WORDS VALS_CAP                      zeroed tables of that capacity at instance stride BP
//   append J ENCODING IS_ARRAY LENS VALUES          one result for instance J: lists as in foreign_plan_host_test (`e`: empty); VALUES: 64 hex digits per
//                                                   element as the bytes lie in memory, comma separated (`e`: none), an instance-major row of ENCODING
//                                                   -> "ok WORD VALUE N_RESULTS" (the walk's answer before the append) | "refused WORD VALUE N_RESULTS"
//   walk J                                          -> "WORD VALUE N_RESULTS"
//   column J                                        -> the descriptor words of the column, all DESC_WORDS of them
//   values J N                                      -> the first N values of the column as stored (rows x * 2^261 mod p), 64 hex digits each, most significant first
#include "../acvm_amd/csrc/foreign_store.hpp"
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
using namespace acvm;

static std::vector<uint32_t> read_list(std::istream &in) {
    std::string tok;
    in >> tok;
    std::vector<uint32_t> v;
    if (tok == "e") return v;
    std::stringstream ss(tok);
    for (std::string item; std::getline(ss, item, ',');) v.push_back((uint32_t)std::stoull(item));
    return v;
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
        } else if (cmd == "append") {
            uint64_t j = 0;
            uint32_t encoding = 0;
            in >> j >> encoding;
            const std::vector<uint32_t> is_array = read_list(in), lens = read_list(in);
            std::vector<uint32_t> shape = {(uint32_t)is_array.size()};
            for (size_t k = 0; k < is_array.size(); k++) { shape.push_back(is_array[k] ? 1u : 0u); shape.push_back(is_array[k] ? lens[k] : 1u); }
            const uint32_t total = fc_shape_total(shape.data());
            std::string tok;
            in >> tok;
            // the caller's buffer: exactly `total` elements, 16-byte aligned
            const uint32_t size = export_element_size(encoding);
            std::unique_ptr<uint4[]> buf(new uint4[((size_t)total * size + 15) / 16 + 1]());
            uint8_t *bytes = (uint8_t *)buf.get();
            if (tok != "e") {
                std::stringstream ss(tok);
                size_t c = 0;
                for (std::string item; std::getline(ss, item, ','); c++)
                    for (uint32_t q = 0; q < size; q++) bytes[c * size + q] = (uint8_t)std::stoul(item.substr(2 * q, 2), nullptr, 16);
            }
            const FcAppendPos before = fc_store_walk(desc.get(), Bp, j, desc_words);
            const FcAnswers a{bytes, encoding, EXPORT_INSTANCE_MAJOR, total ? total : 1u};
            const bool ok = fc_store_append(desc.get(), vals.get(), Bp, j, desc_words, vals_cap, shape.data(), total, a, 0);
            printf("%s %u %u %u\n", ok ? "ok" : "refused", before.word, before.value, before.n_results);
        } else if (cmd == "walk") {
            uint64_t j = 0;
            in >> j;
            const FcAppendPos p = fc_store_walk(desc.get(), Bp, j, desc_words);
            printf("%u %u %u\n", p.word, p.value, p.n_results);
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
