// Host-side execution of inverse_batch_kernel's body (acvm_amd/csrc/inverse_batch.hpp is __host__ __device__): the prefix-product pass, the
// prefixes parked in the jobs' own inverse slots and the back-substitution over tables in host memory laid out like the device's, one call per
// lane and chunk as the kernel's grid makes them. Run by tests/test_inverse_batch_on_host.py with the cases and the assertions of the GPU test.
// Built with --cuda-host-only; nothing is launched.
//   inverse_batch_host_test <in> <out>
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

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: inverse_batch_host_test <in> <out>\n"); return 1; }
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
    for (uint32_t first = 0; first < n_jobs; first += chunk) {  // grid.y; the launcher's second launch is the same loop on the host
        const uint32_t n = n_jobs - first < chunk ? n_jobs - first : chunk;
        for (uint64_t j = 0; j < B; j++) inverse_batch_body<InverseHostPolicy>(W.data(), Inv.data(), Bp, j, stream.data(), offset.data(), first, n, event);
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
