// Host-side execution of what the record export runs per element behind the encoding (acvm_amd/csrc/record_encode.hpp is __host__ __device__).
// The tool judges nothing: it answers the commands on its standard input and tests/test_record_encode_on_host.py compares the answers with a
// byte-wise restatement.
//   put N_WORDS { BYTE SIZE ELEMENT } ...   record_scatter of each element (hex, SIZE bytes, memory order) at byte BYTE of a ZEROED image of exactly
//                         N_WORDS words on the heap, in the order given -> "IMAGE OPS": the image as hex in memory order, and per scatter call the
//                         words it touched as s<word> (plain store) / o<word> (OR), comma separated, calls separated by ';'
//   round BYTE SIZE ELEMENT   record_scatter into a zeroed image of exactly the element's dwords, then record_assemble from it -> the 32 bytes lo | hi
//   nib PHASE LENGTH K BITMAP   record_cover_nibble: BITMAP as 8 decimal words -> the nibble
//   lds PITCH BASE OFFSET BYTE   record_lds_word(i, phase_i, BYTE) for the 64 rows of a block (as tools/record_decode_host_test.hip)
//   const                 RECORD_WINDOW_CAP RECORD_IMAGE_WORDS RECORD_LDS_PITCH RECORD_LDS_WORDS
#include "../acvm_amd/csrc/record_encode.hpp"
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
using namespace acvm;

static bool parse_hex(const char *hex, size_t n_bytes, uint8_t *out) {
    if (strlen(hex) != 2 * n_bytes) return false;
    for (size_t i = 0; i < n_bytes; i++) {
        unsigned v = 0;
        if (sscanf(hex + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
static bool read_element(unsigned size, uint4 &lo, uint4 &hi) {
    static char hex[80];
    uint8_t raw[32] = {0};
    if (size < 1 || size > 32 || scanf("%79s", hex) != 1 || !parse_hex(hex, size, raw)) return false;
    memcpy(&lo, raw, 16);
    memcpy(&hi, raw + 16, 16);
    return true;
}
int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "put")) {
            unsigned n_words = 0;
            if (scanf("%u", &n_words) != 1) { printf("bad command\n"); return 1; }
            std::unique_ptr<uint32_t[]> image(new uint32_t[n_words]());  // exactly n_words: a word beyond is one the sanitizer sees
            std::string ops;
            unsigned byte = 0, size = 0;
            int c;
            while ((c = getchar()) == ' ') {
                uint4 lo, hi;
                if (scanf("%u %u", &byte, &size) != 2 || !read_element(size, lo, hi)) { printf("bad command\n"); return 1; }
                if (!ops.empty()) ops += ";";
                bool first = true;
                auto note = [&](char kind, uint32_t word) { ops += (first ? "" : ",") + std::string(1, kind) + std::to_string(word); first = false; };
                record_scatter(byte, size, lo, hi, [&](uint32_t word, uint32_t v) { note('s', word); image[word] = v; }, [&](uint32_t word, uint32_t v) { note('o', word); image[word] |= v; });
            }
            for (unsigned w = 0; w < n_words; w++) {
                uint8_t b[4];
                memcpy(b, &image[w], 4);
                printf("%02x%02x%02x%02x", b[0], b[1], b[2], b[3]);
            }
            printf(" %s\n", ops.empty() ? "-" : ops.c_str());
        } else if (!strcmp(cmd, "round")) {
            unsigned byte = 0, size = 0;
            uint4 lo, hi;
            if (scanf("%u %u", &byte, &size) != 2 || !read_element(size, lo, hi)) { printf("bad command\n"); return 1; }
            const unsigned n_words = (byte + size + 3u) / 4u;
            std::unique_ptr<uint32_t[]> image(new uint32_t[n_words]());
            record_scatter(byte, size, lo, hi, [&](uint32_t word, uint32_t v) { image[word] = v; }, [&](uint32_t word, uint32_t v) { image[word] |= v; });
            uint4 alo, ahi;
            record_assemble(image.get(), byte, size, alo, ahi);
            uint8_t out[32];
            memcpy(out, &alo, 16);
            memcpy(out + 16, &ahi, 16);
            for (int i = 0; i < 32; i++) printf("%02x", out[i]);
            printf("\n");
        } else if (!strcmp(cmd, "nib")) {
            unsigned phase = 0, length = 0, k = 0;
            std::unique_ptr<uint32_t[]> bitmap(new uint32_t[RECORD_WINDOW_CAP / 32u]);
            if (scanf("%u %u %u", &phase, &length, &k) != 3) { printf("bad command\n"); return 1; }
            for (uint32_t w = 0; w < RECORD_WINDOW_CAP / 32u; w++)
                if (scanf("%u", &bitmap[w]) != 1) { printf("bad command\n"); return 1; }
            printf("%u\n", record_cover_nibble(bitmap.get(), length, phase, k));
        } else if (!strcmp(cmd, "lds")) {
            unsigned long long pitch = 0, base = 0, offset = 0;
            unsigned byte = 0;
            if (scanf("%llu %llu %llu %u", &pitch, &base, &offset, &byte) != 4) { printf("bad command\n"); return 1; }
            for (uint32_t i = 0; i < RECORD_BLOCK_INSTANCES; i++) printf(i ? " %u" : "%u", record_lds_word(i, record_phase(base + i * pitch + offset), byte));
            printf("\n");
        } else if (!strcmp(cmd, "const")) printf("%u %u %u %u\n", RECORD_WINDOW_CAP, RECORD_IMAGE_WORDS, RECORD_LDS_PITCH, RECORD_LDS_WORDS);
        else { printf("bad command\n"); return 1; }
    }
    return 0;
}
