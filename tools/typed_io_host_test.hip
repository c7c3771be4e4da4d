// Host-side execution of what the narrow encodings of the device I/O run per element (acvm_amd/csrc/import_decode.hpp and export_encode.hpp are
// __host__ __device__). The tool judges nothing: it answers the commands on its standard input and tests/test_typed_io_on_host.py compares the
// answers with Python integers.
//   dec E BYTES      import_decode_narrow of the element's bytes (2 x size hex digits, in memory order) in the narrow encoding E, read from an
//                    address aligned to the size and no further (import_narrow_read)
//                    -> "CANONICAL ROW PLANE": the canonical value and the row as 64 hex digits, most significant first, the plane word as 8
//   enc E A ROW FACTOR   export_encode_narrow in the narrow encoding E, assigned A (0 / 1), of the row and the factor (64 hex digits each, most
//                    significant first) -> "BYTES MASK": the element's bytes in memory order, the mask byte
//   size E           "VALID NARROW SIZE" of encoding E
//   at L STRIDE I C SIZE   export_element_offset(layout L, STRIDE, instance I, column C, SIZE): where element (I, C) lies, in bytes
//   part             sizeof(acvm_import_part_t) and the offsets of its members, in the order of the declaration
#include "../acvm_amd/csrc/import_decode.hpp"
#include "../include/acvm_amd.h"
#include <cstddef>
#include <cstdio>
#include <cstring>
using namespace acvm;

static bool parse_fr(const char *hex, Fr &x) {
    if (strlen(hex) != 64) return false;
    for (int i = 0; i < 8; i++)
        if (sscanf(hex + 8 * (7 - i), "%8x", &x.v[i]) != 1) return false;
    return true;
}
static void print_fr(const Fr &x) {
    for (int i = 7; i >= 0; i--) printf("%08x", x.v[i]);
}
int main() {
    static_assert(ACVM_ENC_U8 == EXPORT_ENC_U8 && ACVM_ENC_U128 == EXPORT_ENC_U128 && ACVM_LAYOUT_BROADCAST == EXPORT_LAYOUT_BROADCAST, "the header's values");
    char cmd[16], a[80], f[80];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "dec")) {
            unsigned enc = 0;
            if (scanf("%u %79s", &enc, a) != 2 || !export_enc_is_narrow(enc)) { printf("bad command\n"); return 1; }
            const uint32_t size = export_element_size(enc);
            if (strlen(a) != 2 * size) { printf("bad command\n"); return 1; }
            alignas(32) uint8_t mem[64];
            memset(mem, 0xA5, sizeof mem);
            uint8_t *at = mem + 32 - (size < 16 ? size : 0);  // aligned to size; for the narrower ones not to 2 x size
            for (uint32_t i = 0; i < size; i++) {
                unsigned v = 0;
                if (sscanf(a + 2 * i, "%2x", &v) != 1) { printf("bad command\n"); return 1; }
                at[i] = (uint8_t)v;
            }
            const ImportDecoded d = import_decode_narrow(import_narrow_read(at, size));
            print_fr(d.canonical);
            printf(" ");
            print_fr(d.row);
            printf(" %08x\n", d.plane);
        } else if (!strcmp(cmd, "enc")) {
            unsigned enc = 0, assigned = 0;
            Fr row, factor;
            if (scanf("%u %u %79s %79s", &enc, &assigned, a, f) != 4 || !export_enc_is_narrow(enc) || !parse_fr(a, row) || !parse_fr(f, factor)) { printf("bad command\n"); return 1; }
            const uint32_t size = export_element_size(enc);
            const ExportNarrow e = export_encode_narrow(row, factor, size, assigned != 0);
            uint8_t b[16];
            memcpy(b, &e.lo, 16);
            for (uint32_t i = size; i < 16; i++)
                if (b[i]) { printf("bad: byte %u beyond the element is not zero\n", i); return 1; }
            for (uint32_t i = 0; i < size; i++) printf("%02x", b[i]);
            printf(" %u\n", e.mask);
        } else if (!strcmp(cmd, "size")) {
            unsigned enc = 0;
            if (scanf("%u", &enc) != 1) { printf("bad command\n"); return 1; }
            printf("%d %d %u\n", (int)export_enc_is_valid(enc), (int)export_enc_is_narrow(enc), export_element_size(enc));
        } else if (!strcmp(cmd, "at")) {
            unsigned layout = 0, size = 0;
            unsigned long long stride = 0, i = 0, c = 0;
            if (scanf("%u %llu %llu %llu %u", &layout, &stride, &i, &c, &size) != 5) { printf("bad command\n"); return 1; }
            printf("%llu\n", (unsigned long long)export_element_offset(layout, stride, i, c, size));
        } else if (!strcmp(cmd, "part")) {
            printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(acvm_import_part_t), offsetof(acvm_import_part_t, d_values), offsetof(acvm_import_part_t, encoding),
                   offsetof(acvm_import_part_t, layout), offsetof(acvm_import_part_t, positions), offsetof(acvm_import_part_t, columns), offsetof(acvm_import_part_t, n),
                   offsetof(acvm_import_part_t, n_columns), offsetof(acvm_import_part_t, stride));
        } else { printf("bad command\n"); return 1; }
    }
    return 0;
}
