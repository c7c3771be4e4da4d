// Host-side execution of the per-lane body of the repitch kernel, of the scan's block arithmetic and of the offsets judgement
// (acvm_amd/csrc/wire_repitch.hpp is __host__ __device__): what kernels_wire_pack.hip runs. The tool judges nothing: it answers the commands on
// its standard input, one line each, and tests/test_wire_pack_on_host.py compares the answers with plain Python slices. Built with the host
// side sanitized (`make asan`, and by the test itself) every access past a bound is reported: the source lies in a heap block of exactly its
// stated bytes, the destination in one of exactly its bytes, the columns in blocks of exactly their sizes. An aligned 16-byte access is a
// memcpy of 16 bytes here -- the alignments are the command's, not the heap's.
//   copy SRC_ALIGN DST_ALIGN SRC_BYTES DST_BYTES N  then per row SRC_OFF DST_OFF LEN
//        the source is byte k = (k * 131 + 7) mod 251, the destination starts as 0xA5; every unit of every row is run as the kernel's lanes run
//        it (units_per_row from the longest row) -> the destination as hex (- for none)
//   unpack SRC_ALIGN DST_ALIGN N_BYTES PITCH N  then N + 1 offsets
//        the packed source as above into N slots at PITCH, 0xA5 before -> N classes, then the destination as hex
//   pack SRC_ALIGN DST_ALIGN PITCH CAPACITY DST_BYTES N  then N lengths
//        pitched rows (the source pattern over N * PITCH bytes), offsets by the scan -> the destination as hex
//   scan BASE CAPACITY CHUNK M  then M lengths -> the M + 1 offsets, the base left behind and the fit count, chunk by chunk as the launcher runs it
//   key INSTANCE CLASS -> the finding key as decimal and the two fields read back from it
#include "../acvm_amd/csrc/wire_repitch.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
using namespace acvm;

struct HostMem {
    const uint8_t *src;
    uint8_t *dst;
    Unit16 load16(uint64_t off) const {
        Unit16 u;
        memcpy(u.w, src + off, 16);
        return u;
    }
    uint32_t load8(uint64_t off) const { return src[off]; }
    void store16(uint64_t off, const Unit16 &u) const { memcpy(dst + off, u.w, 16); }
    void store8(uint64_t off, uint32_t b) const { dst[off] = (uint8_t)b; }
};

static std::unique_ptr<uint8_t[]> pattern(uint64_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    for (uint64_t k = 0; k < n; k++) p[k] = (uint8_t)((k * 131u + 7u) % 251u);
    return p;
}
static void print_hex(const uint8_t *p, uint64_t n) {
    static const char *digits = "0123456789abcdef";
    std::string line;
    for (uint64_t k = 0; k < n; k++) { line.push_back(digits[p[k] >> 4]); line.push_back(digits[p[k] & 15]); }
    printf("%s\n", n ? line.c_str() : "-");
}
// every lane of the grid, as launch_wire_repitch sizes it
static void run(const WireRepitch &a) {
    const HostMem m{a.src, a.dst};
    for (uint64_t i = 0; i < a.n; i++) {
        const RepitchRow r = wire_repitch_row(a, i);
        for (uint64_t u = 0; u < a.units_per_row; u++) wire_repitch_unit(m, a, r, u);
    }
}
// the scan of one chunk as wire_scan_kernel runs it: the threads of a block in lockstep, phase by phase
static void scan_chunk(const uint64_t *lengths, uint32_t m, uint64_t *offsets, uint64_t capacity, uint64_t *state) {
    std::unique_ptr<uint64_t[]> sums0(new uint64_t[REPITCH_SCAN_THREADS]), sums1(new uint64_t[REPITCH_SCAN_THREADS]), mine(new uint64_t[REPITCH_SCAN_THREADS]);
    uint64_t *sums[2] = {sums0.get(), sums1.get()};
    uint64_t carry = state[REPITCH_STATE_BASE];
    uint32_t fit = 0;
    offsets[0] = carry;
    for (uint64_t tile0 = 0; tile0 < m; tile0 += REPITCH_SCAN_TILE) {
        for (uint32_t t = 0; t < REPITCH_SCAN_THREADS; t++) sums[0][t] = mine[t] = wire_scan_thread_sum(lengths, m, tile0, t);
        uint32_t cur = 0;
        for (uint32_t d = 1; d < REPITCH_SCAN_THREADS; d <<= 1, cur ^= 1u)
            for (uint32_t t = 0; t < REPITCH_SCAN_THREADS; t++) sums[cur ^ 1u][t] = wire_scan_step(sums[cur], t, d);
        for (uint32_t t = 0; t < REPITCH_SCAN_THREADS; t++) fit += wire_scan_thread_emit(lengths, m, tile0, t, carry + sums[cur][t] - mine[t], capacity, offsets);
        carry += sums[cur][REPITCH_SCAN_THREADS - 1u];
    }
    state[REPITCH_STATE_BASE] = carry;
    state[REPITCH_STATE_FIT] += fit;
}

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "copy")) {
            uint32_t src_align = 0, dst_align = 0, n = 0;
            uint64_t src_bytes = 0, dst_bytes = 0;
            if (scanf("%u %u %" SCNu64 " %" SCNu64 " %u", &src_align, &dst_align, &src_bytes, &dst_bytes, &n) != 5) return 2;
            // (general rows: both sides packed, the source's offsets column made of pairs so that any row may lie anywhere)
            std::unique_ptr<uint8_t[]> src = pattern(src_bytes), dst(new uint8_t[dst_bytes]);
            memset(dst.get(), 0xA5, dst_bytes);
            uint64_t longest = 0;
            std::vector<uint64_t> so(n), doff(n), len(n);
            for (uint32_t i = 0; i < n; i++) {
                if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &so[i], &doff[i], &len[i]) != 3) return 2;
                longest = len[i] > longest ? len[i] : longest;
            }
            for (uint32_t i = 0; i < n; i++) {  // one call per row: a two-entry source column, a one-entry destination column
                std::unique_ptr<uint64_t[]> s2(new uint64_t[2]), d1(new uint64_t[1]);
                s2[0] = so[i], s2[1] = so[i] + len[i], d1[0] = doff[i];
                run(WireRepitch{1u, src.get(), 0u, s2.get(), src_bytes, src_align, nullptr, dst.get(), 0u, d1.get(), 0u, dst_bytes, dst_align, wire_repitch_units(longest)});
            }
            print_hex(dst.get(), dst_bytes);
        } else if (!strcmp(cmd, "unpack")) {
            uint32_t src_align = 0, dst_align = 0, n = 0;
            uint64_t n_bytes = 0, pitch = 0;
            if (scanf("%u %u %" SCNu64 " %" SCNu64 " %u", &src_align, &dst_align, &n_bytes, &pitch, &n) != 5) return 2;
            std::unique_ptr<uint8_t[]> src = pattern(n_bytes), dst(new uint8_t[(uint64_t)n * pitch]);
            memset(dst.get(), 0xA5, (uint64_t)n * pitch);
            std::unique_ptr<uint64_t[]> offsets(new uint64_t[(uint64_t)n + 1]);
            for (uint32_t i = 0; i <= n; i++)
                if (scanf("%" SCNu64, &offsets[i]) != 1) return 2;
            const WireRepitch a{n, src.get(), 0u, offsets.get(), n_bytes, src_align, nullptr, dst.get(), pitch, nullptr, 0u, 0u, dst_align, wire_repitch_units(pitch)};
            for (uint32_t i = 0; i < n; i++) printf("%u ", wire_offsets_class(offsets[i], offsets[i + 1], n_bytes, pitch));
            run(a);
            print_hex(dst.get(), (uint64_t)n * pitch);
        } else if (!strcmp(cmd, "pack")) {
            uint32_t src_align = 0, dst_align = 0, n = 0;
            uint64_t pitch = 0, capacity = 0, dst_bytes = 0;
            if (scanf("%u %u %" SCNu64 " %" SCNu64 " %" SCNu64 " %u", &src_align, &dst_align, &pitch, &capacity, &dst_bytes, &n) != 6) return 2;
            std::unique_ptr<uint8_t[]> src = pattern((uint64_t)n * pitch), dst(new uint8_t[dst_bytes]);
            memset(dst.get(), 0xA5, dst_bytes);
            std::unique_ptr<uint64_t[]> lengths(new uint64_t[n]), offsets(new uint64_t[(uint64_t)n + 1]);
            for (uint32_t i = 0; i < n; i++)
                if (scanf("%" SCNu64, &lengths[i]) != 1) return 2;
            uint64_t state[REPITCH_STATE_WORDS] = {0u, 0u};
            scan_chunk(lengths.get(), n, offsets.get(), capacity, state);
            run(WireRepitch{n, src.get(), pitch, nullptr, (uint64_t)n * pitch, src_align, lengths.get(), dst.get(), 0u, offsets.get(), 0u, capacity, dst_align, wire_repitch_units(pitch)});
            print_hex(dst.get(), dst_bytes);
        } else if (!strcmp(cmd, "scan")) {
            uint64_t base = 0, capacity = 0;
            uint32_t chunk = 0, m = 0;
            if (scanf("%" SCNu64 " %" SCNu64 " %u %u", &base, &capacity, &chunk, &m) != 4 || !chunk) return 2;
            std::unique_ptr<uint64_t[]> lengths(new uint64_t[m]), offsets(new uint64_t[(uint64_t)m + 1]);
            for (uint32_t i = 0; i < m; i++)
                if (scanf("%" SCNu64, &lengths[i]) != 1) return 2;
            uint64_t state[REPITCH_STATE_WORDS] = {base, 0u};
            offsets[0] = base;
            for (uint32_t done = 0; done < m; done += chunk) scan_chunk(lengths.get() + done, m - done < chunk ? m - done : chunk, offsets.get() + done, capacity, state);
            for (uint32_t i = 0; i <= m; i++) printf("%" PRIu64 " ", offsets[i]);
            printf("%" PRIu64 " %" PRIu64 "\n", state[REPITCH_STATE_BASE], state[REPITCH_STATE_FIT]);
        } else if (!strcmp(cmd, "key")) {
            uint64_t instance = 0;
            uint32_t cls = 0;
            if (scanf("%" SCNu64 " %u", &instance, &cls) != 2) return 2;
            const uint64_t key = wire_offsets_key(instance, cls);
            printf("%" PRIu64 " %" PRIu64 " %u\n", key, wire_offsets_key_instance(key), wire_offsets_key_class(key));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd);
            return 2;
        }
    }
    return 0;
}
