// Host-side execution of the per-row reader of the gzip import (acvm_amd/csrc/wire_inflate.hpp is __host__ __device__): what a lane of
// kernels_wire_inflate.hip runs for its row. The tool judges nothing: it answers the commands on its standard input, one line each, and
// tests/test_wire_inflate_on_host.py compares the answers with tests/wire_inflate_ref.py. Built with the host side sanitized (`make asan`,
// and by the test itself) every access past a bound is reported: a row's input lies in a heap block of exactly its readable bytes, its output
// in one of exactly OUT_CAP bytes, its tables in blocks of exactly their sizes.
//   inflate OUT_CAP ROW       ROW: the readable bytes as hex, or - for none -> CLASS BLOCK LENGTH CRC OUTPUT (hex, or - for none)
//   codes                     -> the base and extra bits of the 29 length and 30 distance symbols and the 19 places of the code-length order
//   key INSTANCE CLASS BLOCK  -> the finding key as decimal and the three fields read back from it
#include "../acvm_amd/csrc/wire_inflate.hpp"
#include "../acvm_amd/csrc/wire_inflate_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
using namespace acvm;

struct HostIn {
    const uint8_t *row;
    uint32_t operator()(uint64_t k) const { return row[k]; }
};
struct HostOut {
    uint8_t *slot;
    void store(uint64_t k, uint32_t b) { slot[k] = (uint8_t)b; }
    uint32_t load(uint64_t k, uint64_t) const { return slot[k]; }
    void finish(uint64_t) {}
};
struct HostTab {
    uint16_t *half;
    uint8_t *nibbles;
    uint32_t get(uint32_t i) const { return half[i]; }
    void set(uint32_t i, uint32_t v) const { half[i] = (uint16_t)v; }
    uint32_t len(uint32_t i) const { return (nibbles[i >> 1] >> (4u * (i & 1u))) & 15u; }
    void set_len(uint32_t i, uint32_t v) const {
        const uint32_t shift = 4u * (i & 1u);
        nibbles[i >> 1] = (uint8_t)((nibbles[i >> 1] & ~(15u << shift)) | (v << shift));
    }
};

static bool read_hex(std::vector<uint8_t> &out) {
    static char buf[1 << 21];
    if (scanf("%2097151s", buf) != 1) return false;
    out.clear();
    if (!strcmp(buf, "-")) return true;
    const size_t n = strlen(buf);
    if (n % 2) return false;
    out.resize(n / 2);
    for (size_t i = 0; i < out.size(); i++) {
        auto nibble = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; };
        const int hi = nibble(buf[2 * i]), lo = nibble(buf[2 * i + 1]);
        if (hi < 0 || lo < 0) return false;
        out[i] = (uint8_t)(hi << 4 | lo);
    }
    return true;
}

int main() {
    std::unique_ptr<uint32_t[]> crc_table(new uint32_t[256]);
    for (uint32_t k = 0; k < 256; k++) crc_table[k] = wire_crc_table_entry(k);
    const std::vector<uint16_t> fixed_made = wire_inflate_fixed_tables();
    if (fixed_made.size() != INFLATE_TAB_HALFWORDS) return 3;
    std::unique_ptr<uint16_t[]> fixed(new uint16_t[INFLATE_TAB_HALFWORDS]);
    memcpy(fixed.get(), fixed_made.data(), INFLATE_TAB_HALFWORDS * 2);
    char cmd[16];
    std::vector<uint8_t> row;
    std::string line;
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "inflate")) {
            uint64_t out_cap = 0;
            if (scanf("%" SCNu64, &out_cap) != 1 || !read_hex(row)) return 2;
            std::unique_ptr<uint8_t[]> in(new uint8_t[row.size()]), out(new uint8_t[out_cap]);
            if (!row.empty()) memcpy(in.get(), row.data(), row.size());
            std::unique_ptr<uint16_t[]> half(new uint16_t[INFLATE_TAB_HALFWORDS]);
            std::unique_ptr<uint8_t[]> nibbles(new uint8_t[INFLATE_LEN_NIBBLES / 2]);
            memset(half.get(), 0xee, INFLATE_TAB_HALFWORDS * 2);  // (a kernel's LDS holds whatever the block before left there)
            memset(nibbles.get(), 0xee, INFLATE_LEN_NIBBLES / 2);
            const HostIn hin{in.get()};
            HostOut hout{out.get()};
            const HostTab tab{half.get(), nibbles.get()};
            const uint16_t *fixed_table = fixed.get();
            const uint32_t *crc = crc_table.get();
            const InflateRow r = wire_inflate_row(hin, (uint64_t)row.size(), hout, out_cap, tab, fixed_table, crc);
            line.clear();
            static const char *digits = "0123456789abcdef";
            for (uint64_t k = 0; k < r.length; k++) { line.push_back(digits[out[k] >> 4]); line.push_back(digits[out[k] & 15]); }
            printf("%u %u %" PRIu64 " %u %s\n", r.cls, r.block, r.length, r.crc, r.length ? line.c_str() : "-");
        } else if (!strcmp(cmd, "codes")) {
            for (uint32_t i = 0; i < 29; i++) { uint32_t base, extra; inflate_length_code(i, base, extra); printf("%u %u ", base, extra); }
            for (uint32_t d = 0; d < 30; d++) { uint32_t base, extra; inflate_distance_code(d, base, extra); printf("%u %u ", base, extra); }
            for (uint32_t k = 0; k < 19; k++) printf("%u%s", inflate_clc_order(k), k == 18 ? "\n" : " ");
        } else if (!strcmp(cmd, "key")) {
            uint64_t instance = 0;
            uint32_t cls = 0, block = 0;
            if (scanf("%" SCNu64 " %u %u", &instance, &cls, &block) != 3) return 2;
            const uint64_t key = inflate_key(instance, cls, block);
            printf("%" PRIu64 " %u %u %u\n", key, inflate_key_instance(key), inflate_key_class(key), inflate_key_block(key));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd);
            return 2;
        }
    }
    return 0;
}
