// Host-side execution of what the wire-format kernels run per entry and per row (acvm_amd/csrc/wire_encode.hpp is __host__ __device__).
// The tool judges nothing: it answers the commands on its standard input, one line each, and tests/test_wire_encode_on_host.py compares the
// answers with binascii.hexlify, zlib.crc32 and tests/wire_ref.py.
//   const                     WIRE_ENTRY_BYTES WIRE_BLOCK_BYTES WIRE_WINDOW WIRE_LDS_PITCH WIRE_ROWS
//   hex ELEMENT               ELEMENT: 32 bytes as hex, memory order (an export_encode BE32 element) -> its 64 characters (the 16 dwords in memory order)
//   entry WITNESS ELEMENT     -> the 76 bytes of the entry as hex
//   raw BYTES                 BYTES: a multiple of 4 bytes as hex -> the raw CRC (zero register, no final xor) as decimal
//   raw4 BYTES                the same through the table sliced by 4, what the kernel runs
//   mul A B                   -> A * B mod P
//   xpow BYTES                -> x^(8 BYTES) mod P
//   crc N { WITNESS ELEMENT } x N   the CRC-32 of the body of these entries by the combination rule, each entry's raw CRC shifted on its own
//   length CONTAINER N        -> wire_length
//   offset CONTAINER K        -> wire_body_offset
//   head L                    -> the 16 bytes at a member's start for a body of L bytes, as hex
//   joint L BLOCK             -> the 20 bytes in front of stored block BLOCK of a body of L bytes, as hex
#include "../acvm_amd/csrc/wire_encode.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
using namespace acvm;

static bool parse_hex(const std::string &hex, std::vector<uint8_t> &out) {
    if (hex.size() % 2) return false;
    out.resize(hex.size() / 2);
    for (size_t i = 0; i < out.size(); i++) {
        unsigned v = 0;
        if (sscanf(hex.c_str() + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
static bool read_hex(std::vector<uint8_t> &out) {
    static char buf[1 << 16];
    if (scanf("%65535s", buf) != 1) return false;
    return parse_hex(buf, out);
}
static bool read_element(ExportElement &e) {
    std::vector<uint8_t> raw;
    if (!read_hex(raw) || raw.size() != 32) return false;
    memcpy(&e.lo, raw.data(), 16);
    memcpy(&e.hi, raw.data() + 16, 16);
    return true;
}
static void print_words(const uint32_t *words, size_t n) {
    for (size_t k = 0; k < n; k++)
        for (int b = 0; b < 4; b++) printf("%02x", (words[k] >> (8 * b)) & 0xffu);
    printf("\n");
}

int main() {
    std::unique_ptr<uint32_t[]> table(new uint32_t[256]);  // exactly 256 entries on the heap: a lookup past the end is one the sanitizer sees
    for (uint32_t k = 0; k < 256; k++) table[k] = wire_crc_table_entry(k);
    std::unique_ptr<uint32_t[]> sliced(new uint32_t[WIRE_CRC_SLICED_WORDS]);
    for (uint32_t k = 0; k < WIRE_CRC_SLICED_WORDS; k++) sliced[k] = wire_crc_sliced_entry(k);
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "const")) printf("%u %u %u %u %u\n", WIRE_ENTRY_BYTES, WIRE_BLOCK_BYTES, WIRE_WINDOW, WIRE_LDS_PITCH, WIRE_ROWS);
        else if (!strcmp(cmd, "hex")) {
            ExportElement e;
            if (!read_element(e)) return 2;
            uint32_t out[16];
            wire_hex(e, out);
            print_words(out, 16);
        } else if (!strcmp(cmd, "entry")) {
            uint32_t w = 0;
            ExportElement e;
            if (scanf("%u", &w) != 1 || !read_element(e)) return 2;
            uint32_t out[WIRE_ENTRY_WORDS];
            wire_entry(w, e, out);
            print_words(out, WIRE_ENTRY_WORDS);
        } else if (!strcmp(cmd, "raw") || !strcmp(cmd, "raw4")) {
            std::vector<uint8_t> raw;
            if (!read_hex(raw) || raw.size() % 4) return 2;
            std::vector<uint32_t> words(raw.size() / 4);
            memcpy(words.data(), raw.data(), raw.size());
            printf("%u\n", cmd[3] ? wire_crc_raw_sliced(words.data(), (uint32_t)words.size(), sliced.get()) : wire_crc_raw(words.data(), (uint32_t)words.size(), table.get()));
        } else if (!strcmp(cmd, "mul")) {
            uint32_t a = 0, b = 0;
            if (scanf("%u %u", &a, &b) != 2) return 2;
            printf("%u\n", wire_crc_mul(a, b));
        } else if (!strcmp(cmd, "xpow")) {
            uint64_t bytes = 0;
            if (scanf("%" SCNu64, &bytes) != 1) return 2;
            printf("%u\n", wire_crc_xpow_bytes(bytes));
        } else if (!strcmp(cmd, "crc")) {
            uint32_t n = 0;
            if (scanf("%u", &n) != 1) return 2;
            const uint32_t step = wire_crc_xpow_bytes(WIRE_ENTRY_BYTES);
            std::vector<uint32_t> pow((size_t)n + 1);  // the plan's power table
            pow[0] = 0x80000000u;
            for (uint32_t k = 1; k <= n; k++) pow[k] = wire_crc_mul(pow[k - 1], step);
            uint32_t entries = 0;
            for (uint32_t r = 0; r < n; r++) {
                uint32_t w = 0;
                ExportElement e;
                if (scanf("%u", &w) != 1 || !read_element(e)) return 2;
                uint32_t words[WIRE_ENTRY_WORDS];
                wire_entry(w, e, words);
                entries ^= wire_crc_mul(pow[n - 1 - r], wire_crc_raw_sliced(words, WIRE_ENTRY_WORDS, sliced.get()));
            }
            const uint32_t count[2] = {n, 0u};
            printf("%u\n", wire_crc_combine(pow[n], wire_crc_xpow_bytes(8), wire_crc_raw(count, 2, table.get()), entries));
        } else if (!strcmp(cmd, "length") || !strcmp(cmd, "offset")) {
            uint32_t container = 0;
            uint64_t v = 0;
            if (scanf("%u %" SCNu64, &container, &v) != 2) return 2;
            printf("%" PRIu64 "\n", cmd[0] == 'l' ? wire_length(container, v) : wire_body_offset(container, v));
        } else if (!strcmp(cmd, "head")) {
            uint64_t L = 0;
            if (scanf("%" SCNu64, &L) != 1) return 2;
            uint32_t out[4];
            wire_head(L, out);
            print_words(out, 4);
        } else if (!strcmp(cmd, "joint")) {
            uint64_t L = 0, block = 0;
            if (scanf("%" SCNu64 " %" SCNu64, &L, &block) != 2) return 2;
            uint32_t out[5];
            wire_joint(L, block, out);
            print_words(out, 5);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd);
            return 2;
        }
    }
    return 0;
}
