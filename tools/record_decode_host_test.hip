// Host-side execution of what the record import runs per element in front of the decoding (acvm_amd/csrc/record_decode.hpp is
// __host__ __device__). The tool judges nothing: it answers the commands on its standard input and tests/test_record_decode_on_host.py compares
// the answers with Python integers.
//   asm BYTE SIZE IMAGE   record_assemble of the SIZE bytes at byte BYTE of the word image IMAGE (hex, memory order, whole dwords: exactly the
//                         aligned dwords that hold a byte of the element, on the heap) -> the 32 bytes lo | hi as 64 hex digits, memory order
//   dec BYTE E IMAGE      record_decode of the element of encoding E there -> "CANONICAL ROW PLANE" as tools/import_device_host_test.hip prints them
//   lds PITCH BASE OFFSET BYTE   for the 64 instances of a block whose records lie PITCH bytes apart from byte address BASE, the window at OFFSET
//                         of the record: record_lds_word(i, phase_i, BYTE) for i = 0 .. 63
//   const                 RECORD_WINDOW_CAP RECORD_IMAGE_WORDS RECORD_LDS_PITCH RECORD_LDS_WORDS
#include "../acvm_amd/csrc/record_decode.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace acvm;

static bool parse_image(const char *hex, std::vector<uint32_t> &words) {
    const size_t n = strlen(hex);
    if (n % 8) return false;
    std::vector<uint8_t> b(n / 2);
    for (size_t i = 0; i < b.size(); i++) {
        unsigned v = 0;
        if (sscanf(hex + 2 * i, "%2x", &v) != 1) return false;
        b[i] = (uint8_t)v;
    }
    words.assign(b.size() / 4, 0u);
    if (!b.empty()) memcpy(words.data(), b.data(), b.size());
    return true;
}
static void print_fr(const Fr &x) {
    for (int i = 7; i >= 0; i--) printf("%08x", x.v[i]);
}
int main() {
    char cmd[16];
    static char image[4096];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "asm") || !strcmp(cmd, "dec")) {
            unsigned byte = 0, arg = 0;
            std::vector<uint32_t> words;
            if (scanf("%u %u %4095s", &byte, &arg, image) != 3 || !parse_image(image, words)) { printf("bad command\n"); return 1; }
            const uint32_t size = cmd[0] == 'a' ? arg : export_element_size(arg);
            if ((byte + size + 3u) / 4u != words.size()) { printf("bad image\n"); return 1; }  // exactly the element's dwords
            if (cmd[0] == 'a') {
                uint4 lo, hi;
                record_assemble(words.data(), byte, size, lo, hi);
                uint8_t out[32];
                memcpy(out, &lo, 16);
                memcpy(out + 16, &hi, 16);
                for (int i = 0; i < 32; i++) printf("%02x", out[i]);
                printf("\n");
            } else {
                const ImportDecoded d = record_decode(words.data(), byte, arg);
                print_fr(d.canonical);
                printf(" ");
                print_fr(d.row);
                printf(" %08x\n", d.plane);
            }
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
