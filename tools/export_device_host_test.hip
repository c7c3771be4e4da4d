// Host-side execution of what the device-resident witness export runs per element and per tile (acvm_amd/csrc/export_encode.hpp is
// __host__ __device__). The tool judges nothing: it answers the commands on its standard input and tests/test_export_device_on_host.py
// compares the answers with Python integers.
//   enc E A ROW FACTOR      export_encode(row, factor, encoding E, assigned A); ROW / FACTOR: 64 hex digits, most significant first
//                           -> the element's 32 bytes in memory order, as hex
//   factor E                export_plain_factor(E) as 64 hex digits, most significant first
//   tile L N NSEL T STRIDE  every 16-byte unit the grid of layout L writes for n = N instances x NSEL list positions, stride STRIDE, by the
//                           tiled kernel with tiles of T positions (instance-major) or, T = 0, by the direct kernel (either layout):
//                           one line "u OFFSET" per store (OFFSET in 16-byte units), "m INDEX" per mask byte, then "end";
//                           "bad ..." if phase 2 of the tiled kernel would read a tile slot that phase 1 did not fill
#include "../acvm_amd/csrc/export_encode.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace acvm;

static bool parse_fr(const char *hex, Fr &out) {
    if (strlen(hex) != 64) return false;
    for (int i = 0; i < 8; i++) {
        unsigned v = 0;
        if (sscanf(hex + 8 * (7 - i), "%8x", &v) != 1) return false;
        out.v[i] = v;
    }
    return true;
}
static void print_bytes(const ExportElement &e) {
    uint8_t b[32];
    memcpy(b, &e.lo, 16);
    memcpy(b + 16, &e.hi, 16);
    for (int i = 0; i < 32; i++) printf("%02x", b[i]);
    printf("\n");
}
static void tile(uint32_t layout, uint32_t n, uint32_t n_sel, uint32_t T, uint64_t stride) {
    if (T == 0) {  // export_device_direct_kernel: lane = instance, blockIdx.y = list position
        for (uint32_t k = 0; k < n_sel; k++)
            for (uint32_t bx = 0; bx < (n + 255u) / 256u; bx++)
                for (uint32_t t = 0; t < 256u; t++) {
                    const uint64_t i = (uint64_t)bx * 256u + t;
                    if (i >= n) continue;
                    const uint64_t at = export_element_index(layout, stride, i, k);
                    printf("u %llu\nu %llu\nm %llu\n", (unsigned long long)(2 * at), (unsigned long long)(2 * at + 1), (unsigned long long)at);
                }
        printf("end\n");
        return;
    }
    // export_device_im_kernel<T>
    for (uint32_t bx = 0; bx < (n + EXPORT_TILE_I - 1u) / EXPORT_TILE_I; bx++)
        for (uint32_t by = 0; by < (n_sel + T - 1u) / T; by++) {
            const uint64_t i0 = (uint64_t)bx * EXPORT_TILE_I;
            const uint32_t kb = by * T;
            std::vector<uint8_t> filled((size_t)T * 64u, 0);
            for (uint32_t t = 0; t < EXPORT_THREADS; t++) {
                const uint32_t ji = export_tile_lane(t);
                for (uint32_t kk = export_tile_first_position(t); kk < T; kk += EXPORT_WAVES) {
                    if (kb + kk >= n_sel || i0 + ji >= n) continue;
                    if (filled[(size_t)kk * 64u + ji]++) printf("bad: tile slot filled twice\n");
                }
            }
            for (uint32_t step = 0; step < export_tile_steps(T); step++)
                for (uint32_t t = 0; t < EXPORT_THREADS; t++) {
                    const ExportTileUnit q = export_tile_unit(T, t, step);
                    const uint64_t i = i0 + q.ji;
                    const uint32_t k = kb + q.kk;
                    if (i >= n || k >= n_sel) continue;
                    if (q.ji >= 64u || q.kk >= T || !filled[(size_t)q.kk * 64u + q.ji]) printf("bad: phase 2 reads an empty tile slot\n");
                    const uint64_t at = export_element_index(layout, stride, i, k);
                    printf("u %llu\n", (unsigned long long)(2 * at + q.half));
                    if (q.half == 0) printf("m %llu\n", (unsigned long long)at);
                }
        }
    printf("end\n");
}
int main() {
    char cmd[16], a[80], b[80];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "enc")) {
            unsigned enc = 0, assigned = 0;
            Fr row, factor;
            if (scanf("%u %u %79s %79s", &enc, &assigned, a, b) != 4 || !parse_fr(a, row) || !parse_fr(b, factor)) { printf("bad command\n"); return 1; }
            print_bytes(export_encode(row, factor, enc, assigned != 0));
        } else if (!strcmp(cmd, "factor")) {
            unsigned enc = 0;
            if (scanf("%u", &enc) != 1) { printf("bad command\n"); return 1; }
            const Fr f = export_plain_factor(enc);
            for (int i = 7; i >= 0; i--) printf("%08x", f.v[i]);
            printf("\n");
        } else if (!strcmp(cmd, "tile")) {
            unsigned layout = 0, n = 0, n_sel = 0, T = 0;
            unsigned long long stride = 0;
            if (scanf("%u %u %u %u %llu", &layout, &n, &n_sel, &T, &stride) != 5 || T % EXPORT_WAVES || (T == 0) != (layout == EXPORT_WITNESS_MAJOR || n_sel < EXPORT_WAVES)) { printf("bad command\n"); return 1; }
            tile(layout, n, n_sel, T, stride);
        } else { printf("bad command\n"); return 1; }
    }
    return 0;
}
