// Host-side execution of the ordered selection's arithmetic (acvm_amd/csrc/select_scan.hpp is __host__ __device__): the three launches of
// kernels_select.hip -- count, scan, scatter -- walked block by block, round by round, wave by wave with the header's own functions. The tool
// judges nothing but the bounds of its own stores: it answers the commands on its standard input and tests/test_select_on_host.py compares
// the answers with a plain loop.
//   span                    -> SELECT_SPAN SELECT_THREADS SELECT_ROUNDS
//   sel FIRST MASK HEX      the status bytes HEX (two digits each; "-" for none) selected by MASK, numbered from FIRST
//                           -> "COUNT: i0 i1 ..." (the list's first COUNT entries); "bad ..." instead if a store left [0, n) or hit an entry twice
#include "../acvm_amd/csrc/select_scan.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace acvm;

// the ballot of wave `wave` of round r of block b: what __ballot gives the kernels
static uint64_t ballot_of(const std::vector<uint8_t> &status, uint32_t mask, uint32_t b, uint32_t r, uint32_t wave) {
    uint64_t ballot = 0;
    for (uint32_t lane = 0; lane < SELECT_WAVE; lane++) {
        const uint64_t e = select_element(b, r, wave * SELECT_WAVE + lane);
        if (e < status.size() && select_predicate(status[e], mask)) ballot |= 1ull << lane;
    }
    return ballot;
}
static void fill_counts(const std::vector<uint8_t> &status, uint32_t mask, uint32_t b, uint32_t *counts) {
    for (uint32_t r = 0; r < SELECT_ROUNDS; r++)
        for (uint32_t wave = 0; wave < SELECT_WAVES; wave++) counts[select_slot(r, wave * SELECT_WAVE)] = select_count(ballot_of(status, mask, b, r, wave));
}
static void run(uint32_t first, uint32_t mask, const std::vector<uint8_t> &status) {
    const uint32_t n = (uint32_t)status.size(), blocks = select_blocks(n);
    std::vector<uint32_t> totals(blocks + 1, 0);
    uint32_t counts[SELECT_SLOTS];
    for (uint32_t b = 0; b < blocks; b++) {  // select_count_kernel
        fill_counts(status, mask, b, counts);
        totals[b] = select_block_total(counts);
    }
    uint32_t carry = 0;  // select_scan_kernel
    for (uint32_t step = 0; step < select_scan_steps(blocks); step++) {
        uint32_t sums[SELECT_THREADS], v[SELECT_THREADS];
        for (uint32_t t = 0; t < SELECT_THREADS; t++) {
            const uint32_t at = step * SELECT_THREADS + t;
            v[t] = at < blocks ? totals[at] : 0u;
            sums[t] = v[t] + (t ? sums[t - 1] : 0u);
        }
        for (uint32_t t = 0; t < SELECT_THREADS; t++) {
            const uint32_t at = step * SELECT_THREADS + t;
            if (at < blocks) totals[at] = carry + sums[t] - v[t];
        }
        carry += sums[SELECT_THREADS - 1];
    }
    const uint32_t count = carry;
    std::vector<uint32_t> out(n, 0);
    std::vector<uint8_t> written(n, 0);
    for (uint32_t b = 0; b < blocks; b++) {  // select_scatter_kernel
        fill_counts(status, mask, b, counts);
        for (uint32_t r = 0; r < SELECT_ROUNDS; r++)
            for (uint32_t t = 0; t < SELECT_THREADS; t++) {
                const uint64_t ballot = ballot_of(status, mask, b, r, t / SELECT_WAVE);
                if (!((ballot >> (t % SELECT_WAVE)) & 1u)) continue;
                const uint64_t at = (uint64_t)totals[b] + select_slot_offset(counts, select_slot(r, t)) + select_rank(ballot, t % SELECT_WAVE);
                if (at >= count || at >= n || written[at]) {
                    printf("bad store at %llu (count %u, n %u)\n", (unsigned long long)at, count, n);
                    return;
                }
                written[at] = 1;
                out[at] = first + (uint32_t)select_element(b, r, t);
            }
    }
    printf("%u:", count);
    for (uint32_t i = 0; i < count; i++) printf(" %u", out[i]);
    printf("\n");
}

int main() {
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        unsigned first = 0, mask = 0;
        static char hex[1 << 16];
        if (!strncmp(line, "span", 4)) printf("%u %u %u\n", SELECT_SPAN, SELECT_THREADS, SELECT_ROUNDS);
        else if (sscanf(line, "sel %u %u %65000s", &first, &mask, hex) == 3) {
            std::vector<uint8_t> status;
            if (strcmp(hex, "-") != 0)
                for (size_t i = 0; i + 1 < strlen(hex); i += 2) {
                    unsigned v = 0;
                    sscanf(hex + i, "%2x", &v);
                    status.push_back((uint8_t)v);
                }
            run(first, mask, status);
        } else {
            printf("bad command\n");
            return 1;
        }
    }
    return 0;
}
