// Host-side execution of what the device-resident witness import runs per element (acvm_amd/csrc/import_decode.hpp is __host__ __device__).
// The tool judges nothing: it answers the commands on its standard input and tests/test_import_device_on_host.py compares the answers with
// Python integers.
//   dec E BYTES   import_decode of the element's 32 bytes (64 hex digits, in memory order) in encoding E
//                 -> "CANONICAL ROW PLANE": the canonical value and the row as 64 hex digits, most significant first, the plane word as 8
//   pieces E BYTES  the same through the pieces the kernels call one by one (import_limbs, import_canonical, import_row, import_plane_word)
//   const         2^266 mod p, 2^522 mod p and 2^5 as 64 hex digits each, most significant first
//   at L STRIDE I C   export_element_index(layout L, STRIDE, instance I, column C): where element (I, C) of a caller's buffer lies, in elements
#include "../acvm_amd/csrc/import_decode.hpp"
#include <cstdio>
#include <cstring>
using namespace acvm;

static bool parse_bytes(const char *hex, uint4 &lo, uint4 &hi) {
    if (strlen(hex) != 64) return false;
    uint8_t b[32];
    for (int i = 0; i < 32; i++) {
        unsigned v = 0;
        if (sscanf(hex + 2 * i, "%2x", &v) != 1) return false;
        b[i] = (uint8_t)v;
    }
    memcpy(&lo, b, 16);
    memcpy(&hi, b + 16, 16);
    return true;
}
static void print_fr(const Fr &x) {
    for (int i = 7; i >= 0; i--) printf("%08x", x.v[i]);
}
int main() {
    char cmd[16], a[80];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "dec") || !strcmp(cmd, "pieces")) {
            unsigned enc = 0;
            uint4 lo, hi;
            if (scanf("%u %79s", &enc, a) != 2 || enc >= EXPORT_N_ENC || !parse_bytes(a, lo, hi)) { printf("bad command\n"); return 1; }
            ImportDecoded d;
            if (cmd[0] == 'd') d = import_decode(lo, hi, enc);
            else {
                const Fr m = import_limbs(lo, hi, enc);
                d.canonical = import_canonical(m, enc);
                d.row = import_row(m, d.canonical, enc);
                d.plane = import_plane_word(d.canonical);
            }
            print_fr(d.canonical);
            printf(" ");
            print_fr(d.row);
            printf(" %08x\n", d.plane);
        } else if (!strcmp(cmd, "const")) {
            print_fr(import_r266());
            printf(" ");
            print_fr(import_r522());
            printf(" ");
            print_fr(import_two5());
            printf("\n");
        } else if (!strcmp(cmd, "at")) {
            unsigned layout = 0;
            unsigned long long stride = 0, i = 0, c = 0;
            if (scanf("%u %llu %llu %llu", &layout, &stride, &i, &c) != 4 || layout >= EXPORT_N_LAYOUT) { printf("bad command\n"); return 1; }
            printf("%llu\n", (unsigned long long)export_element_index(layout, stride, i, c));
        } else { printf("bad command\n"); return 1; }
    }
    return 0;
}
