// Host-side execution of the precomputed coefficient x row reduction: the planner's table builder (lin_table.hpp lin_table_of, fed the way
// plan.cpp feeds it: the inline device-form words push_coef writes) and fr29_lin_add<1 / 2> (fr_device.hpp, __host__ __device__) over a
// case list, raw limbs out. tests/test_lin_table_on_host.py writes the cases and compares every table word and every result with Python
// integers. Beside each result the tool runs the same column scan with a 128-bit accumulator: the largest column sum it ever holds is
// reported (the 64-bit one of the real routine must never wrap), and its limbs must be the real routine's.
//   lin_table_host_test <in> <out>
//   in:  u32 n_items, then with n_groups = ceil(n_items / 64) -- 64 items share their coefficients, as the lanes of a wave do on the device
//        (acvm_debug_lin_add takes the same arrays) --
//        n_groups x u32 n_terms (1 | 2), n_groups x 2 x 8 u32 coefficient (canonical, little-endian words),
//        n_items x 2 x 8 u32 rows (any 256-bit pattern), n_items x 9 u32 h (any limbs)
//   out: n_groups x 2 x 81 u32 tables, n_items x 9 u32 result limbs, 2 x u64 largest column accumulator (N = 1, N = 2), u32 items whose
//        128-bit scan disagrees with the routine
#include "../acvm_amd/csrc/fr_device.hpp"
#include "../acvm_amd/csrc/lin_table.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
using namespace acvm;

typedef unsigned __int128 u128w;
static u128w g_max_acc[2];
// fr29_lin_add, column for column, in 128 bits
template <int N>
static Fr29 lin_add_wide(const uint32_t *tab, const Fr29 (&x)[N], const Fr29 &h) {
    constexpr uint32_t M = 0x1fffffffu;
    u128w acc = 0;
    uint32_t m[2] = {0, 0};
    Fr29 r;
    auto seen = [&]() { if (acc > g_max_acc[N - 1]) g_max_acc[N - 1] = acc; };
    for (int k = 0; k < 9; k++) {
        for (int t = 0; t < N; t++)
            for (int i = 0; i < 9; i++) acc += (u128w)x[t].v[i] * tab[81 * t + 9 * k + i];
        if (k >= 1) acc += (u128w)m[0] * fr_p29(k);
        if (k >= 2) acc += (u128w)m[1] * fr_p29(k - 1);
        if (k < 2) {
            const uint32_t lo = (uint32_t)acc;
            m[k] = (((lo & 1u) << 28) - lo) & M;
            acc += ((u128w)m[k] << 28) + m[k];
            seen();
            if ((uint32_t)acc & M) { fprintf(stderr, "column %d of the scan does not end in 29 zero bits\n", k); exit(1); }
        } else {
            acc += h.v[k - 2];
            seen();
            r.v[k - 2] = (uint32_t)acc & M;
        }
        acc >>= 29;
    }
    acc += (u128w)m[1] * fr_p29(8) + h.v[7];
    seen();
    r.v[7] = (uint32_t)acc & M;
    acc >>= 29;
    r.v[8] = (uint32_t)acc + h.v[8];
    return r;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<uint8_t> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() < 4) { fprintf(stderr, "short input\n"); return 1; }
    uint32_t n_items;
    memcpy(&n_items, raw.data(), 4);
    const size_t n_groups = ((size_t)n_items + 63) / 64;
    const size_t want = 4 + 4 * (n_groups + n_groups * 16 + (size_t)n_items * 16 + (size_t)n_items * 9);
    if (raw.size() != want) { fprintf(stderr, "input holds %zu bytes, %zu expected\n", raw.size(), want); return 1; }
    std::vector<uint32_t> w((raw.size() - 4) / 4);
    memcpy(w.data(), raw.data() + 4, w.size() * 4);
    const uint32_t *n_terms = w.data(), *coef = n_terms + n_groups, *rows = coef + n_groups * 16, *hs = rows + (size_t)n_items * 16;
    std::vector<uint32_t> tables(n_groups * 2 * GATE_LIN_TABLE_WORDS, 0), out((size_t)n_items * 9);
    for (size_t g = 0; g < n_groups; g++) {
        if (n_terms[g] != 1 && n_terms[g] != 2) { fprintf(stderr, "group %zu: %u terms\n", g, n_terms[g]); return 1; }
        for (uint32_t t = 0; t < n_terms[g]; t++) {
            // the planner's road: the coefficient as a field element -> the record's inline words (plan.cpp push_coef) -> the table
            uint64_t c[4];
            for (int i = 0; i < 4; i++) c[i] = coef[g * 16 + t * 8 + 2 * i] | (uint64_t)coef[g * 16 + t * 8 + 2 * i + 1] << 32;
            const FrH d = frh::to_device_form(frh::from_canonical(c));
            uint32_t inline_words[8];
            for (int i = 0; i < 4; i++) { inline_words[2 * i] = (uint32_t)d.l[i]; inline_words[2 * i + 1] = (uint32_t)(d.l[i] >> 32); }
            lin_table_of(inline_words, &tables[(g * 2 + t) * GATE_LIN_TABLE_WORDS]);
        }
    }
    uint32_t disagree = 0;
    for (uint32_t j = 0; j < n_items; j++) {
        const size_t g = j / 64;
        const uint32_t *tab = &tables[g * 2 * GATE_LIN_TABLE_WORDS];
        Fr a, b;
        Fr29 h;
        memcpy(a.v, rows + (size_t)j * 16, 32);
        memcpy(b.v, rows + (size_t)j * 16 + 8, 32);
        memcpy(h.v, hs + (size_t)j * 9, 36);
        Fr29 r, rw;
        if (n_terms[g] == 1) {
            const Fr29 x[1] = {fr29_from(a)};
            r = fr29_lin_add<1>(tab, x, h);
            rw = lin_add_wide<1>(tab, x, h);
        } else {
            const Fr29 x[2] = {fr29_from(a), fr29_from(b)};
            r = fr29_lin_add<2>(tab, x, h);
            rw = lin_add_wide<2>(tab, x, h);
        }
        disagree += memcmp(r.v, rw.v, 36) != 0;
        memcpy(&out[(size_t)j * 9], r.v, 36);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    fwrite(tables.data(), 4, tables.size(), o);
    fwrite(out.data(), 4, out.size(), o);
    for (int n = 0; n < 2; n++) {
        if (g_max_acc[n] >> 64) { fprintf(stderr, "the column accumulator of N = %d passed 64 bits\n", n + 1); fclose(o); return 1; }
        const uint64_t m = (uint64_t)g_max_acc[n];
        fwrite(&m, 8, 1, o);
    }
    fwrite(&disagree, 4, 1, o);
    fclose(o);
    printf("%u items, %zu groups, largest column accumulator %.4f x 2^58 (N = 1), %.4f x 2^58 (N = 2), %u disagreements\nOK\n", n_items, n_groups,
           (double)(uint64_t)g_max_acc[0] / 288230376151711744.0, (double)(uint64_t)g_max_acc[1] / 288230376151711744.0, disagree);
    return 0;
}
