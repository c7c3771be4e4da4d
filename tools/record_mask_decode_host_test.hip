// Host-side execution of the masked record import's addressing (acvm_amd/csrc/record_decode.hpp and import_mask.hpp are __host__ __device__): the
// presence byte in a record's word image, the word and bit of the missing set, and the block's OR of those bits in its LDS words. The tool
// judges nothing: it answers the commands on its standard input and tests/test_record_mask_decode_on_host.py compares the answers with Python.
//   presence BYTE IMAGE        record_presence_byte at byte BYTE of the word image IMAGE (hex, memory order, exactly the aligned dwords up to
//                              the one that holds the byte, on the heap) -> the byte
//   bit POSITION BP J          import_missing_word(POSITION, BP, J) import_missing_bit(POSITION)
//   slot POSITION BASE         record_miss_slot(POSITION, BASE) (4294967295: no slot)
//   or BASE N { INSTANCE POSITION } x N   what a block does with N absent (instance in block, position) pairs: each ORs its bit into
//                              record_miss_lds_word(slot, instance) of a zeroed LDS array, or -- no slot -- is listed as direct; -> the nonzero
//                              LDS words as `WORD:INSTANCE:BITS` in ascending LDS order (WORD = BASE + slot), then `direct` and the pairs without a slot
//   const                      RECORD_MISS_SLOTS RECORD_MISS_LDS_WORDS RECORD_LDS_WORDS
#include "../acvm_amd/csrc/record_decode.hpp"
#include "../acvm_amd/csrc/import_mask.hpp"
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
using namespace acvm;

int main() {
    char cmd[16];
    static char image[4096];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "presence")) {
            unsigned byte = 0;
            if (scanf("%u %4095s", &byte, image) != 2 || strlen(image) % 8) { printf("bad command\n"); return 1; }
            const size_t n_words = strlen(image) / 8;
            if (byte / 4u + 1u != n_words) { printf("bad image\n"); return 1; }  // the byte's dword is the last one: a read behind it is seen
            std::unique_ptr<uint32_t[]> words(new uint32_t[n_words]);
            for (size_t i = 0; i < n_words; i++) {
                uint8_t b[4];
                for (int q = 0; q < 4; q++) {
                    unsigned v = 0;
                    sscanf(image + 8 * i + 2 * q, "%2x", &v);
                    b[q] = (uint8_t)v;
                }
                memcpy(&words[i], b, 4);
            }
            printf("%u\n", record_presence_byte(words.get(), byte));
        } else if (!strcmp(cmd, "bit")) {
            unsigned position = 0;
            unsigned long long bp = 0, j = 0;
            if (scanf("%u %llu %llu", &position, &bp, &j) != 3) { printf("bad command\n"); return 1; }
            printf("%llu %u\n", (unsigned long long)import_missing_word(position, bp, j), import_missing_bit(position));
        } else if (!strcmp(cmd, "slot")) {
            unsigned position = 0, base = 0;
            if (scanf("%u %u", &position, &base) != 2) { printf("bad command\n"); return 1; }
            printf("%u\n", record_miss_slot(position, base));
        } else if (!strcmp(cmd, "or")) {
            unsigned base = 0, n = 0;
            if (scanf("%u %u", &base, &n) != 2) { printf("bad command\n"); return 1; }
            std::unique_ptr<uint32_t[]> miss(new uint32_t[RECORD_MISS_LDS_WORDS]());
            std::string direct;
            for (unsigned q = 0; q < n; q++) {
                unsigned inst = 0, position = 0;
                if (scanf("%u %u", &inst, &position) != 2 || inst >= RECORD_BLOCK_INSTANCES) { printf("bad command\n"); return 1; }
                const uint32_t slot = record_miss_slot(position, base);
                if (slot == RECORD_MISS_NO_SLOT) direct += " " + std::to_string(inst) + ":" + std::to_string(position);
                else miss[record_miss_lds_word(slot, inst)] |= import_missing_bit(position);
            }
            bool any = false;
            for (uint32_t q = 0; q < RECORD_MISS_LDS_WORDS; q++)
                if (miss[q]) {
                    printf(any ? " %u:%u:%u" : "%u:%u:%u", base + q / RECORD_BLOCK_INSTANCES, q % RECORD_BLOCK_INSTANCES, miss[q]);
                    any = true;
                }
            printf("%sdirect%s\n", any ? " " : "", direct.c_str());
        } else if (!strcmp(cmd, "const")) printf("%u %u %u\n", RECORD_MISS_SLOTS, RECORD_MISS_LDS_WORDS, RECORD_LDS_WORDS);
        else { printf("bad command\n"); return 1; }
    }
    return 0;
}
