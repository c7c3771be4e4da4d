// Host-side execution of inverse_batch_kernel_shared<G>'s body (acvm_amd/csrc/inverse_batch.hpp is __host__ __device__): a workgroup of G waves as
// three loops over its waves -- every wave's prefix pass, the share step (one field inversion per lane for the G waves, through the word-major table
// the kernel keeps in LDS), every wave's back-substitution -- over tables in host memory laid out like the device's, block and chunk as the
// kernel's grid makes them, lanes and waves past B predicated off as in the kernel. Run by tests/test_inverse_share_on_host.py with the cases and
// the assertions of the GPU test, and compared byte for byte with tools/inverse_batch_host_test.hip's table. Built with --cuda-host-only; nothing is launched.
//   inverse_share_host_test <in> <out> <G>
//   in:  u32 n_jobs, B, chunk (jobs per wave after the launcher's spreading), n_jobs x u32 inverse slot, n_jobs x B x 8 u32 denominators
//   out: n_jobs x B x 8 u32 rows of the inverse table, B event words, u32 count of flagged instances
#include "../acvm_amd/csrc/inverse_batch.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace acvm;

// the accesses of the body on the host; flag: ops_common.hpp flag_instance without the wave (the first flag of an instance counts it, event[-4])
struct InverseHostPolicy {
    static Fr load_den(const uint4 *W, uint32_t row, uint64_t Bp, uint64_t j) { return fr_load(W, row, Bp, j); }
    static Fr load_den_last(const uint4 *W, uint32_t row, uint64_t Bp, uint64_t j) { return fr_load(W, row, Bp, j); }
    static void park(uint4 *Inv, uint32_t slot, uint64_t Bp, uint64_t j, const Fr &a) { fr_store(Inv, slot, Bp, j, a); }
    static Fr parked(const uint4 *Inv, uint32_t slot, uint64_t Bp, uint64_t j) { return fr_load(Inv, slot, Bp, j); }
    static void store_inverse(uint4 *Inv, uint32_t slot, uint64_t Bp, uint64_t j, const Fr &a) { fr_store(Inv, slot, Bp, j, a); }
    static void flag(uint32_t *event, uint64_t j, uint32_t opcode) {
        if (event[j] == 0xFFFFFFFFu) event[-4] += 1;
        if (opcode < event[j]) event[j] = opcode;
    }
};

// one workgroup of inverse_batch_kernel_shared<G>: block x, jobs [first, first + n)
template <int G>
static void run_block(const uint4 *W, uint4 *Inv, uint64_t Bp, uint32_t B, const uint32_t *stream, const uint32_t *offset, uint32_t first, uint32_t n,
                      uint32_t *event, uint64_t x) {
    std::vector<uint32_t> rows((size_t)(G + 1) * INVERSE_SHARE_ROW_WORDS, 0xDEADBEEFu);
    for (uint32_t w = 0; w < (uint32_t)G; w++)  // forward
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t j = (x * G + w) * 64 + lane;
            Fr29 total = fr29_from(fr_one());
            if (j < B) total = inverse_batch_forward<InverseHostPolicy>(W, Inv, Bp, j, stream, offset, first, n, event);
            inverse_share_row_store(rows.data(), w, lane, total);
        }
    for (uint32_t lane = 0; lane < 64; lane++) {  // share: wave 0
        const InverseShareRows totals{rows.data(), lane};
        inverse_share_row_store(rows.data(), G, lane, inverse_share_total_inverse<G>(totals));
    }
    for (uint32_t w = 0; w < (uint32_t)G; w++)  // every wave's own 1 / total, and its way back
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t j = (x * G + w) * 64 + lane;
            if (j >= B) continue;
            const InverseShareRows totals{rows.data(), lane};
            inverse_batch_backward<InverseHostPolicy>(W, Inv, Bp, j, stream, offset, first, n,
                                                      inverse_share_own<G>(totals, inverse_share_row_load(rows.data(), G, lane), w));
        }
}

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: inverse_share_host_test <in> <out> <G>\n"); return 1; }
    const uint32_t G = (uint32_t)atoi(argv[3]);
    if (G != 2 && G != 4 && G != 8) { fprintf(stderr, "G is 2, 4 or 8\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3) { fprintf(stderr, "truncated header\n"); return 1; }
    const uint32_t n_jobs = hdr[0], B = hdr[1], chunk = hdr[2];
    if (!n_jobs || !B || !chunk) { fprintf(stderr, "bad header\n"); return 1; }
    std::vector<uint32_t> slot(n_jobs), den((size_t)n_jobs * B * 8);
    if (fread(slot.data(), 4, n_jobs, f) != n_jobs || fread(den.data(), 4, den.size(), f) != den.size()) { fprintf(stderr, "truncated input\n"); return 1; }
    fclose(f);
    for (uint32_t k = 0; k < n_jobs; k++)
        if (slot[k] >= n_jobs) { fprintf(stderr, "bad slot\n"); return 1; }
    const uint64_t Bp = ((uint64_t)B + 63) / 64 * 64;
    std::vector<uint4> W((size_t)n_jobs * 2 * Bp, make_uint4(0, 0, 0, 0)), Inv(W.size(), make_uint4(0, 0, 0, 0));
    std::vector<uint32_t> stream((size_t)n_jobs * 3), offset(n_jobs), event_base((size_t)B + 4, 0xFFFFFFFFu);
    uint32_t *event = event_base.data() + 4;
    event[-4] = 0;
    for (uint32_t k = 0; k < n_jobs; k++) {
        for (uint32_t j = 0; j < B; j++) {
            Fr d;
            for (int i = 0; i < 8; i++) d.v[i] = den[((size_t)k * B + j) * 8 + i];
            fr_store(W.data(), k, Bp, j, d);
        }
        stream[3 * (size_t)k] = k;
        stream[3 * (size_t)k + 1] = k;
        stream[3 * (size_t)k + 2] = slot[k];
        offset[k] = 3 * k;
    }
    const uint64_t waves = ((uint64_t)B + 63) / 64, blocks = (waves + G - 1) / G;  // grid.x
    for (uint32_t first = 0; first < n_jobs; first += chunk) {                     // grid.y; the launcher's second launch is the same loop on the host
        const uint32_t n = n_jobs - first < chunk ? n_jobs - first : chunk;
        for (uint64_t x = 0; x < blocks; x++) {
            if (G == 2) run_block<2>(W.data(), Inv.data(), Bp, B, stream.data(), offset.data(), first, n, event, x);
            else if (G == 4) run_block<4>(W.data(), Inv.data(), Bp, B, stream.data(), offset.data(), first, n, event, x);
            else run_block<8>(W.data(), Inv.data(), Bp, B, stream.data(), offset.data(), first, n, event, x);
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    std::vector<uint32_t> out((size_t)n_jobs * B * 8);
    for (uint32_t k = 0; k < n_jobs; k++)
        for (uint32_t j = 0; j < B; j++) {
            const Fr v = fr_load(Inv.data(), k, Bp, j);
            for (int i = 0; i < 8; i++) out[((size_t)k * B + j) * 8 + i] = v.v[i];
        }
    fwrite(out.data(), 4, out.size(), f);
    fwrite(event, 4, B, f);
    fwrite(event - 4, 4, 1, f);
    fclose(f);
    printf("OK\n");
    return 0;
}
