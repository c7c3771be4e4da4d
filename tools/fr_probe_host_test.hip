// Host-side execution of the acvm_debug_fr probe's per-item switch (acvm_amd/csrc/fr_probe.hpp is __host__ __device__): the cases of
// tests/fr_ref.py through the C forms of the field library, no GPU. Run by tests/test_fr_probe_on_host.py, which compares every word of
// the output with Python integers. Built with --cuda-host-only; nothing is launched.
//   fr_probe_host_test <in> <out>
//   fr_probe_host_test --words      prints "what words-in words-out" of every routine (the header's table, for the tests to compare with theirs)
//   in:  sections of u32 words: what, n_items, 18 words of the two uniform factors, then n_items x words-in(what) words
//   out: per section n_items x words-out(what) u32 words, in the order of the input
// Exit status 2: a section names a routine the host pass cannot run (the byte tables are in the device's constant memory).
#include "../acvm_amd/csrc/fr_probe.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
using namespace acvm;

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "--words") {
        for (uint32_t w = 0; fr_probe_words_in(w); w++) printf("%u %u %u\n", w, fr_probe_words_in(w), fr_probe_words_out(w));
        return 0;
    }
    if (argc < 3) { fprintf(stderr, "usage: fr_probe_host_test <in> <out>\n"); return 1; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<uint32_t> in;
    uint32_t buf[4096];
    for (size_t n; (n = fread(buf, 4, 4096, f)) > 0;) in.insert(in.end(), buf, buf + n);
    fclose(f);
    std::vector<uint32_t> out;
    size_t pos = 0, items = 0;
    while (pos < in.size()) {
        if (in.size() - pos < 20) { fprintf(stderr, "truncated section header\n"); return 1; }
        const uint32_t what = in[pos], n = in[pos + 1];
        FrProbeUniform un;
        for (int k = 0; k < 18; k++) un.u[k / 9].v[k % 9] = in[pos + 2 + k];
        pos += 20;
        if (!fr_probe_supported(what)) { fprintf(stderr, "routine %u does not run on the host\n", what); return 2; }
        const uint32_t wi = fr_probe_words_in(what), wo = fr_probe_words_out(what);
        if ((in.size() - pos) / wi < n) { fprintf(stderr, "truncated section of routine %u\n", what); return 1; }
        const size_t base = out.size();
        out.resize(base + (size_t)n * wo, 0u);
        for (uint32_t i = 0; i < n; i++) fr_probe_item(what, in.data() + pos + (size_t)i * wi, un, out.data() + base + (size_t)i * wo);
        pos += (size_t)n * wi;
        items += n;
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    if (!out.empty() && fwrite(out.data(), 4, out.size(), f) != out.size()) { perror("write"); return 1; }
    fclose(f);
    printf("%zu items OK\n", items);
    return 0;
}
