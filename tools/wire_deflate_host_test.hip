// Host-side execution of what the deflating wire-format kernel runs per entry (acvm_amd/csrc/wire_deflate.hpp is __host__ __device__), over the
// code table the plan makes (acvm_amd/csrc/wire_plan.cpp). The tool judges nothing: it answers the commands on its standard input, one line
// each, and tests/test_wire_deflate_on_host.py compares the answers with tests/wire_deflate_ref.py.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/wire_deflate_host_test.hip acvm_amd/csrc/wire_plan.cpp -o wire_deflate_host_test
//
//   const              -> WIRE_GZIP_DEFLATE WIRE_DEFLATE_ENTRY_MAX_BITS WIRE_DEFLATE_MIN_MATCH WIRE_WINDOW
//   parse CUR PREV     CUR: the 76 bytes of an entry as hex; PREV: those of the entry in front of it, or `-` at rank 0
//                      -> COST N_TOKENS { LENGTH DISTANCE } x N_TOKENS   (LENGTH 0 DISTANCE byte: a literal)
//   emit OFFSET CUR PREV
//                      -> END_BIT, then the bytes of a zeroed buffer after the entry's tokens were emitted at bit OFFSET, as hex
//   bound HEADER_BITS N -> wire_deflate_bound
#include "../acvm_amd/csrc/wire_deflate.hpp"
#include "../acvm_amd/csrc/wire_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
using namespace acvm;

static_assert(WIRE_DEFLATE_WORDS == WIRE_PLAN_DEFLATE_WORDS && WIRE_DEFLATE_MATCH == WIRE_PLAN_DEFLATE_MATCH && WIRE_DEFLATE_PREFIX == WIRE_PLAN_DEFLATE_PREFIX, "one table layout");

static bool read_entry(std::unique_ptr<uint32_t[]> &out) {
    static char buf[256];
    if (scanf("%255s", buf) != 1) return false;
    if (!strcmp(buf, "-")) { out.reset(); return true; }
    if (strlen(buf) != 2 * WIRE_ENTRY_BYTES) return false;
    out.reset(new uint32_t[WIRE_ENTRY_WORDS]);  // exactly 19 words on the heap: a read past the end is one the sanitizer sees
    for (uint32_t i = 0; i < WIRE_ENTRY_BYTES; i++) {
        unsigned v = 0;
        if (sscanf(buf + 2 * i, "%2x", &v) != 1) return false;
        if (i % 4 == 0) out[i / 4] = 0u;
        out[i / 4] |= v << (8 * (i % 4));
    }
    return true;
}

struct HostSink {
    uint32_t *buf;
    size_t n;
    void shared(uint32_t word, uint32_t bits) const { if (word >= n) abort(); buf[word] |= bits; }
    void own(uint32_t word, uint32_t bits) const { if (word >= n || buf[word]) abort(); buf[word] = bits; }  // a word of its own was nobody's before
};

int main() {
    uint32_t prefix_bits = 0;
    const std::vector<uint32_t> plan_table = wire_deflate_device_table(wire_deflate_code(), &prefix_bits);
    std::unique_ptr<uint32_t[]> table(new uint32_t[WIRE_DEFLATE_WORDS]);
    memcpy(table.get(), plan_table.data(), WIRE_DEFLATE_WORDS * 4);
    const uint32_t *tab = table.get();
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "const")) printf("%u %u %u %u\n", WIRE_GZIP_DEFLATE, WIRE_DEFLATE_ENTRY_MAX_BITS, WIRE_DEFLATE_MIN_MATCH, WIRE_WINDOW);
        else if (!strcmp(cmd, "parse") || !strcmp(cmd, "emit")) {
            uint64_t offset = 0;
            if (cmd[0] == 'e' && scanf("%" SCNu64, &offset) != 1) return 2;
            std::unique_ptr<uint32_t[]> cur, prev;
            if (!read_entry(cur) || !cur || !read_entry(prev)) return 2;
            const uint32_t *c = cur.get(), *p = prev.get();
            if (cmd[0] == 'p') {
                std::unique_ptr<WireToken[]> tokens(new WireToken[WIRE_ENTRY_BYTES]);
                const uint32_t n = wire_deflate_parse(c, p, p != nullptr, tokens.get());
                const WireDeflateMasks m = wire_deflate_masks(c, p, p != nullptr);
                printf("%u %u", wire_deflate_cost(c, m, tab), n);
                uint32_t at = 0;
                for (uint32_t k = 0; k < n; k++) {
                    printf(" %u %u", tokens[k].length, tokens[k].length ? tokens[k].distance : wire_entry_byte(c, at));
                    at += tokens[k].length ? tokens[k].length : 1u;
                }
                printf("\n");
            } else {
                const size_t n_words = (size_t)((offset + WIRE_DEFLATE_ENTRY_MAX_BITS + 31) / 32);
                std::unique_ptr<uint32_t[]> buf(new uint32_t[n_words]());
                const WireDeflateMasks m = wire_deflate_masks(c, p, p != nullptr);
                const uint64_t end = wire_deflate_emit(c, m, tab, HostSink{buf.get(), n_words}, offset);
                printf("%" PRIu64 " ", end);
                for (uint64_t k = 0; k < (end + 7) / 8; k++) printf("%02x", (buf[k / 4] >> (8 * (k % 4))) & 0xffu);
                printf("\n");
            }
        } else if (!strcmp(cmd, "bound")) {
            uint32_t header_bits = 0;
            uint64_t n = 0;
            if (scanf("%u %" SCNu64, &header_bits, &n) != 2) return 2;
            printf("%" PRIu64 "\n", wire_deflate_bound(header_bits, n));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd);
            return 2;
        }
    }
    return 0;
}
