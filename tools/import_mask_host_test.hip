// Host-side execution of what the masked device import decides without a device: the index arithmetic of acvm_amd/csrc/import_mask.hpp (which is
// __host__ __device__: the kernels of kernels_import_mask.hip run the same functions) and the masked plan of acvm_amd/csrc/import_plan.cpp.
// The tool judges nothing: it answers the commands on its standard input and tests/test_import_mask_on_host.py compares the answers with Python
// index arithmetic. `make asan` builds it a second time with the host side sanitized (tools/asan/import_mask_host_test).
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/import_mask_host_test.hip acvm_amd/csrc/import_plan.cpp -o import_mask_host_test
//
//   byte L STRIDE I C     import_mask_byte: where the mask byte of element (instance I, column C) lies, in bytes from d_assigned
//   word K BP J           -> "WORDS INDEX BIT": import_missing_words(K + 1), and the word (index into the missing set) and bit (a mask) of position K
//                         of instance J at instance stride BP
//   key I K               -> "WORD I K": the result word of a bad byte at (instance I, position K) as 16 hex digits, and what the host reads out of it
//   pieces ADDRESS N      -> "HEAD UNITS TAIL": how an instance-major mask row of N bytes at ADDRESS is read
//   view B N_IN           the handle the following calls see: ids 1 .. N_IN, row = id, no byte planes
//   desc ENCODING LAYOUT N_COLUMNS STRIDE PTR MASK COLUMNS      import_plan_desc_masked (MASK 0: a null d_assigned; COLUMNS: comma separated or `null`)
//                         -> "ok PLAIN MASKED ENCODING LAYOUT ELEM_SIZE STRIDE N COLUMNS_AT N_LISTS" or "err CODE TEXT"
//   eq                    whether the last two plans compare equal
#include "../acvm_amd/csrc/import_mask.hpp"
#include "../acvm_amd/csrc/import_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
using namespace acvm;

int main() {
    ImportView view;
    std::unique_ptr<uint32_t[]> ids;
    ImportPlan last, before;
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "byte") {
            uint32_t layout;
            uint64_t stride, i, c;
            in >> layout >> stride >> i >> c;
            printf("%" PRIu64 "\n", import_mask_byte(layout, stride, i, c));
        } else if (cmd == "word") {
            uint32_t k;
            uint64_t Bp, j;
            in >> k >> Bp >> j;
            printf("%u %" PRIu64 " %u\n", import_missing_words(k + 1u), import_missing_word(k, Bp, j), import_missing_bit(k));
        } else if (cmd == "key") {
            uint64_t i;
            uint32_t k;
            in >> i >> k;
            const uint64_t w = import_mask_key(i, k);
            printf("%016" PRIx64 " %u %u\n", w, import_mask_key_instance(w), import_mask_key_position(w));
        } else if (cmd == "pieces") {
            uint64_t address;
            uint32_t n;
            in >> address >> n;
            const ImportMaskPieces p = import_mask_pieces(address, n);
            printf("%u %u %u\n", p.head, p.units, p.tail);
        } else if (cmd == "view") {
            in >> view.B >> view.n_in;
            ids.reset(new uint32_t[view.n_in]);  // (exactly n_in entries on the heap: a read past the end is one the sanitizer sees)
            for (uint32_t k = 0; k < view.n_in; k++) ids[k] = k + 1u;
            view.ids = view.rows = ids.get();
            view.planes = nullptr;
        } else if (cmd == "desc") {
            acvm_import_desc_t d{};
            uint64_t ptr = 0, mask = 0;
            std::string cols;
            in >> d.encoding >> d.layout >> d.n_columns >> d.stride >> ptr >> mask >> cols;
            std::unique_ptr<uint32_t[]> columns;
            if (cols != "null") {
                std::vector<uint32_t> v;
                std::stringstream ss(cols);
                for (std::string item; std::getline(ss, item, ',');) v.push_back((uint32_t)std::stoull(item));
                columns.reset(new uint32_t[v.size()]);
                for (size_t q = 0; q < v.size(); q++) columns[q] = v[q];
                d.columns = columns.get();
            }
            ImportPlan plan;
            std::string err;
            const int rc = import_plan_desc_masked(&view, &d, (const void *)(uintptr_t)ptr, (const uint8_t *)(uintptr_t)mask, &plan, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            const ImportPlanPart &q = plan.parts[0];
            printf("ok %d %d %u %u %u %" PRIu64 " %u %lld %zu\n", (int)plan.plain, (int)plan.masked(), q.encoding, q.layout, q.elem_size, q.stride, q.n,
                   q.columns_at == IMPORT_NO_LIST ? -1ll : (long long)q.columns_at, plan.lists.size());
            before = std::move(last);
            last = std::move(plan);
        } else if (cmd == "eq") printf("eq %d\n", (int)(last == before));
        else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
