// probes.cpp -- measurement and self-test entry points of the C ABI (include/acvm_amd.h): the device self test of the field library, the
// back-to-back product probes behind the ALU rooflines, the streaming ceiling behind the HBM roofline, the component probes of the Grumpkin kernels.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>
#include "batch_internal.hpp"
#include "lin_table.hpp"

int acvm_selftest(uint32_t n, uint64_t seed) {
    uint32_t *d = nullptr, h = 0;
    HIPCHK(hipMalloc((void **)&d, 4));
    HIPCHK(hipMemset(d, 0, 4));
    launch_fr_selftest(nullptr, seed, n, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(&h, d, 4, hipMemcpyDeviceToHost));
    hipFree(d);
    return (int)h;
}

// Peak of the ALU roofline: back-to-back Montgomery products on every SIMD, `waves_per_simd` chains interleaved.
// field: 0 = BN254-Fr in the 29-bit working form (fr29_mul), 1 / 2 = the base field of secp256k1 / secp256r1 (sp_mul, sp_sqr in turn)
static int product_rate(uint32_t field, uint32_t iters, uint32_t waves_per_simd, double *per_s, uint64_t *n_products) {
    if (!per_s || !iters || !waves_per_simd || field > 2) return set_err(ACVM_E_INVALID, "bad argument");
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, dev));
    const uint32_t blocks = (uint32_t)prop.multiProcessorCount * waves_per_simd;  // 256 threads = one wave per SIMD of a CU
    uint32_t *d = nullptr;
    HIPCHK(hipMalloc((void **)&d, (size_t)blocks * 256 * 4));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    float best = 1e30f;
    for (int r = 0; r < 4; r++) {  // the first run warms the clocks up
        hipEventRecord(e0, nullptr);
        if (field == 0) launch_modmul_rate(nullptr, d, blocks, iters);
        else launch_secp_rate(nullptr, field - 1, d, blocks, iters);
        hipEventRecord(e1, nullptr);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        if (r && ms < best) best = ms;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(d);
    HIPCHK(hipGetLastError());
    const double n = (double)blocks * 256.0 * iters * 2.0;
    *per_s = n / (best * 1e-3);
    if (n_products) *n_products = (uint64_t)n;
    return 0;
}
int acvm_debug_modmul_rate(uint32_t iters, uint32_t waves_per_simd, double *modmul_per_s, uint64_t *n_modmul) try {
    return product_rate(0, iters, waves_per_simd, modmul_per_s, n_modmul);
} catch (...) { return set_err(ACVM_E_DEVICE, "probe failed"); }
int acvm_debug_secp_rate(uint32_t curve, uint32_t iters, uint32_t waves_per_simd, double *products_per_s, uint64_t *n_products) try {
    if (curve > 1) return set_err(ACVM_E_INVALID, "curve: 0 = secp256k1, 1 = secp256r1");
    return product_rate(1 + curve, iters, waves_per_simd, products_per_s, n_products);
} catch (...) { return set_err(ACVM_E_DEVICE, "probe failed"); }

// The measured streaming ceiling beside the spec peak of the HBM roofline: two rows of `bytes` read and one written by a kernel with the
// gate kernel's access shape (kernels.hip stream_rate_kernel), best of four; bytes moved = 3 x bytes.
int acvm_debug_stream_rate(size_t bytes, double *gb_per_s) {
    if (!gb_per_s || bytes < (1u << 20)) return set_err(ACVM_E_INVALID, "bad argument");
    const uint64_t n = bytes / 16 / 256 * 256;
    uint4 *buf[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < 3; k++)
        if (hipMalloc((void **)&buf[k], n * 16) != hipSuccess) {
            for (int q = 0; q < k; q++) hipFree(buf[q]);
            return set_err(ACVM_E_DEVICE, "hipMalloc failed");
        }
    for (int k = 0; k < 3; k++) HIPCHK(hipMemset(buf[k], k + 1, n * 16));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    float best = 1e30f;
    for (int r = 0; r < 5; r++) {
        hipEventRecord(e0, nullptr);
        launch_stream_rate(nullptr, buf[0], buf[1], buf[2], n);
        hipEventRecord(e1, nullptr);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        if (r && ms < best) best = ms;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    for (int k = 0; k < 3; k++) hipFree(buf[k]);
    HIPCHK(hipGetLastError());
    *gb_per_s = 3.0 * (double)(n * 16) / (best * 1e-3) / 1e9;
    return 0;
}

// Component probes of the Grumpkin kernels for the parity tests: what = 0 host table point (param = table << 24 | index),
// 1 device hash_single(in[0], parity = param), 2 device hash-ladder compress(in[0..n_in)), 3 device fixed_base_mul(table
// base param, integer in[0]), 4 device table point. in: n_in x 32 bytes big-endian; out: 64 bytes (x || y) big-endian.
int acvm_debug_secp(uint32_t curve, uint32_t what, const uint8_t *in_be32, uint32_t n_items, uint8_t *out_be32) try {
    static const uint32_t WIN[17] = {2, 1, 2, 2, 1, 1, 3, 5, 1, 2, 2, 1, 2, 1, 1, 4, 6}, WOUT[17] = {1, 1, 1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 1, 1, 4, 3, 2};
    if (curve > 1u || what > 16u || !in_be32 || !out_be32) return set_err(ACVM_E_INVALID, "bad argument");
    if (what == 14u && curve != 0u) return set_err(ACVM_E_INVALID, "the endomorphism split (what = 14) is secp256k1's: curve 0 only");
    if (!n_items) return 0;
    const uint32_t wi = WIN[what], wo = WOUT[what];
    // what = 15, 16 read the device's own generator tables (the set dp.ecdsa_g points into): held while the probe runs, from BEFORE it asks for their
    // address, like acvm_debug_grumpkin holds its tables
    struct Hold {
        int d = -1;
        void take(int dev_) { d = dev_; device_tables_retain(d); }
        ~Hold() { if (d >= 0) device_tables_unref(d); }
    } hold;
    const uint32_t *gtabs = nullptr;
    if (what >= 15u) {
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        hold.take(dev);
        gtabs = ecdsa_generator_tables();
        if (!gtabs) {
            (void)hipGetLastError();
            return set_err(ACVM_E_DEVICE, "could not build the ECDSA generator tables on the device");
        }
    }
    std::vector<uint32_t> in((size_t)n_items * wi * 8, 0), out((size_t)n_items * wo * 8, 0);
    for (size_t i = 0; i < (size_t)n_items * wi; i++)
        for (int k = 0; k < 32; k++) in[8 * i + k / 4] |= (uint32_t)in_be32[32 * i + 31 - k] << (8 * (k % 4));
    uint32_t *d_in = nullptr, *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_in, in.size() * 4));
    HIPCHK(hipMalloc((void **)&d_out, out.size() * 4));
    HIPCHK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_out, 0, out.size() * 4));
    launch_secp_probe(nullptr, curve, what, d_in, n_items, wi, wo, d_out, gtabs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    hipFree(d_in);
    hipFree(d_out);
    for (size_t i = 0; i < (size_t)n_items * wo; i++)
        for (int k = 0; k < 32; k++) out_be32[32 * i + 31 - k] = (uint8_t)(out[8 * i + k / 4] >> (8 * (k % 4)));
    return 0;
} ABI_CATCH

int acvm_debug_grumpkin(uint32_t what, uint32_t param, const uint8_t *in_be32, uint32_t n_in, uint8_t *out_be64) try {
    if (!out_be64) return set_err(ACVM_E_INVALID, "null argument");
    if (what == 0) return grumpkin_host_point(param >> 24, param & 0xffffffu, out_be64) ? 0 : set_err(ACVM_E_INVALID, "bad table index");
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    // the probe holds the device's tables while it runs, from BEFORE it asks for their addresses: with tables_keep = 0 another handle's
    // destruction between the two would free what was just handed out (acvm_device_release_tables refuses meanwhile)
    struct Hold {
        int d;
        explicit Hold(int dev_) : d(dev_) { device_tables_retain(d); }
        ~Hold() { device_tables_unref(d); }
    } hold(dev);
    GrumpkinTables tabs;
    if (!grumpkin_tables(&tabs)) return set_err(ACVM_E_DEVICE, "could not build the Grumpkin tables on the device");
    const GrumpkinTables *t = &tabs;
    std::vector<uint32_t> in(8 * (n_in ? n_in : 1), 0), out(16, 0);
    for (uint32_t i = 0; i < n_in; i++)
        for (int k = 0; k < 32; k++) in[8 * i + k / 4] |= (uint32_t)in_be32[32 * i + 31 - k] << (8 * (k % 4));
    uint32_t *d_in = nullptr, *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_in, in.size() * 4));
    HIPCHK(hipMalloc((void **)&d_out, 64));
    HIPCHK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_out, 0, 64));
    launch_grumpkin_probe(nullptr, *t, what, param, d_in, n_in, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out.data(), d_out, 64, hipMemcpyDeviceToHost));
    hipFree(d_in);
    hipFree(d_out);
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < 32; k++) out_be64[32 * c + 31 - k] = (uint8_t)(out[8 * c + k / 4] >> (8 * (k % 4)));
    return 0;
} ABI_CATCH

// One routine of ops_grumpkin.hpp per call, one device lane per item, raw u32 words in and out (kernels_grumpkin.hip grumpkin_items_kernel). The probe holds
// the device's tables like acvm_debug_grumpkin, and owns the per-lane window tables of what = 6.
int acvm_debug_grumpkin_items(uint32_t what, uint32_t param, const uint32_t *in_words, uint32_t n_items, uint32_t *out_words) try {
    const uint32_t wi = grumpkin_items_words(what, false), wo = grumpkin_items_words(what, true);
    if (!wi || !wo) return set_err(ACVM_E_INVALID, "no such routine");
    if (what == 5u && param > 2u) return set_err(ACVM_E_INVALID, "ladder_term: param is the position 0..2");
    if (!n_items) return 0;
    if (!in_words || !out_words) return set_err(ACVM_E_INVALID, "null argument");
    if (n_items > (1u << 20)) return set_err(ACVM_E_INVALID, "at most 2^20 items a call");
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    struct Hold {
        int d;
        explicit Hold(int dev_) : d(dev_) { device_tables_retain(d); }
        ~Hold() { device_tables_unref(d); }
    } hold(dev);
    GrumpkinTables tabs;
    if (!grumpkin_tables(&tabs)) return set_err(ACVM_E_DEVICE, "could not build the Grumpkin tables on the device");
    struct Mem {
        uint32_t *in = nullptr, *out = nullptr, *scratch = nullptr;
        ~Mem() {
            for (void *p : {(void *)in, (void *)out, (void *)scratch})
                if (p) hipFree(p);
        }
    } m;
    const uint64_t Bp = ((uint64_t)n_items + 63) / 64 * 64;
    int rc = 0;
    auto step = [&](hipError_t e, const char *what_) { if (!rc && e != hipSuccess) rc = set_err(ACVM_E_DEVICE, std::string(what_) + ": " + hipGetErrorString(e)); };
    step(hipMalloc((void **)&m.in, (size_t)n_items * wi * 4), "hipMalloc");
    step(hipMalloc((void **)&m.out, (size_t)n_items * wo * 4), "hipMalloc");
    if (what == 6u) step(hipMalloc((void **)&m.scratch, (size_t)Bp * GRUMPKIN_VARBASE_SCRATCH_WORDS * 4), "hipMalloc");
    if (!rc) step(hipMemcpy(m.in, in_words, (size_t)n_items * wi * 4, hipMemcpyHostToDevice), "hipMemcpy");
    if (!rc) step(hipMemset(m.out, 0, (size_t)n_items * wo * 4), "hipMemset");
    if (!rc) launch_grumpkin_items(nullptr, tabs, what, param, m.in, n_items, m.out, m.scratch, Bp);
    step(hipGetLastError(), "grumpkin_items_kernel");
    step(hipDeviceSynchronize(), "hipDeviceSynchronize");
    if (!rc) step(hipMemcpy(out_words, m.out, (size_t)n_items * wo * 4, hipMemcpyDeviceToHost), "hipMemcpy");
    return rc;
} ABI_CATCH

// Read-back of the lookup tables (grumpkin_host.hpp: TABLE_*), entry by entry and in the form they are stored in. The table is built by the function the
// product builds it with; the probe holds the device's set like acvm_debug_grumpkin.
int acvm_debug_table_info(uint32_t table, uint64_t *n_entries, int *built) try {
    const uint64_t n = device_table_entries(table);
    if (!n || !n_entries || !built) return set_err(ACVM_E_INVALID, "no such table, or a null argument");
    *n_entries = n;
    *built = device_table_built(table) ? 1 : 0;
    (void)hipGetLastError();  // (asked without a device: not an error of this call)
    return 0;
} ABI_CATCH

int acvm_debug_table_read(uint32_t table, const uint64_t *entries, uint32_t n, uint32_t *out_words16) try {
    static const char *const NAME[N_DEVICE_TABLES] = {"ped", "win", "small", "skew", "ped2", "win16", "pedw", "ECDSA secp256k1", "ECDSA secp256r1"};
    const uint64_t n_entries = device_table_entries(table);
    if (!n_entries) return set_err(ACVM_E_INVALID, "no such table");
    if (n && (!entries || !out_words16)) return set_err(ACVM_E_INVALID, "null argument");
    for (uint32_t i = 0; i < n; i++)
        if (entries[i] >= n_entries)
            return set_err(ACVM_E_INVALID, "entries[" + std::to_string(i) + "] = " + std::to_string(entries[i]) + " is outside the " + NAME[table] + " table (" +
                                               std::to_string(n_entries) + " entries)");
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    struct Hold {
        int d;
        explicit Hold(int dev_) : d(dev_) { device_tables_retain(d); }
        ~Hold() { device_tables_unref(d); }
    } hold(dev);
    GrumpkinTables tabs{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const uint4 *src = nullptr;
    const char *why = "";
    if (table == TABLE_ECDSA_K1 || table == TABLE_ECDSA_R1) {
        const uint32_t *g = ecdsa_generator_tables();
        if (g) src = (const uint4 *)(g + (table == TABLE_ECDSA_R1 ? n_entries * 16 : 0));
    } else if (table == TABLE_PED2) {
        if (grumpkin_pair_table(&tabs)) src = tabs.ped2;
    } else if (table == TABLE_PEDW) {
        if (grumpkin_window_table(&tabs)) src = tabs.pedw;
        why = ": it needs its own bytes plus a quarter of the device's memory free";
    } else if (grumpkin_tables(&tabs)) {
        src = table == TABLE_PED ? tabs.ped : table == TABLE_WIN ? tabs.win : table == TABLE_SMALL ? tabs.small : table == TABLE_SKEW ? tabs.skew : tabs.win16;
        why = ": it is built with the device's host tables, when tuning win16 is set and its 268 MB are free";
    }
    if (!src) {
        (void)hipGetLastError();
        return set_err(ACVM_E_DEVICE, std::string("could not build the ") + NAME[table] + " table on the device" + why);
    }
    if (!n) return 0;
    uint64_t *d_idx = nullptr;
    uint4 *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_idx, (size_t)n * 8));
    if (hipMalloc((void **)&d_out, (size_t)n * 64) != hipSuccess) {
        hipFree(d_idx);
        return set_err(ACVM_E_DEVICE, "hipMalloc failed");
    }
    int rc = 0;
    auto step = [&](hipError_t e, const char *what_) { if (!rc && e != hipSuccess) rc = set_err(ACVM_E_DEVICE, std::string(what_) + ": " + hipGetErrorString(e)); };
    step(hipMemcpy(d_idx, entries, (size_t)n * 8, hipMemcpyHostToDevice), "hipMemcpy");
    if (!rc) launch_table_gather(nullptr, src, d_idx, n, d_out);
    step(hipGetLastError(), "table_gather_kernel");
    step(hipDeviceSynchronize(), "hipDeviceSynchronize");
    step(hipMemcpy(out_words16, d_out, (size_t)n * 64, hipMemcpyDeviceToHost), "hipMemcpy");
    hipFree(d_idx);
    hipFree(d_out);
    return rc;
} ABI_CATCH

// Which of the device-built tables the handle's device program reads (ACVM_TABLE_BIT_*): its kernels pick by these pointers alone (pedersen_walk takes
// pedw when it is there and ped2 otherwise, fixed_base_mul takes win16 when it is there).
int acvm_debug_batch_tables(const acvm_batch_t *b, uint32_t *mask) {
    if (!b || !mask) return set_err(ACVM_E_INVALID, "null argument");
    const GrumpkinTables &t = b->dp.grumpkin;
    *mask = (t.ped2 && !t.pedw ? 1u : 0u) | (t.win16 ? 2u : 0u) | (t.pedw ? 4u : 0u) | (b->dp.ecdsa_g ? 8u : 0u);
    return 0;
}

// One routine of the BN254-Fr device library per call, one device lane per item, raw limbs in and out (fr_probe.hpp).
int acvm_debug_fr(uint32_t what, const uint32_t *in, uint32_t n_items, const uint32_t *uniform18, uint32_t *out) try {
    const uint32_t wi = fr_probe_words(what, false), wo = fr_probe_words(what, true);
    if (!wi || !wo) return set_err(ACVM_E_INVALID, "no such routine");
    if (!n_items) return 0;
    if (!in || !out) return set_err(ACVM_E_INVALID, "null argument");
    uint32_t *d_in = nullptr, *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_in, (size_t)n_items * wi * 4));
    if (hipMalloc((void **)&d_out, (size_t)n_items * wo * 4) != hipSuccess) {
        hipFree(d_in);
        return set_err(ACVM_E_DEVICE, "hipMalloc failed");
    }
    int rc = 0;
    auto step = [&](hipError_t e, const char *what_) { if (!rc && e != hipSuccess) rc = set_err(ACVM_E_DEVICE, std::string(what_) + ": " + hipGetErrorString(e)); };
    step(hipMemcpy(d_in, in, (size_t)n_items * wi * 4, hipMemcpyHostToDevice), "hipMemcpy");
    step(hipMemset(d_out, 0, (size_t)n_items * wo * 4), "hipMemset");
    if (!rc) launch_fr_probe(nullptr, what, d_in, n_items, uniform18, d_out);
    step(hipGetLastError(), "fr_probe_kernel");
    step(hipDeviceSynchronize(), "hipDeviceSynchronize");
    step(hipMemcpy(out, d_out, (size_t)n_items * wo * 4, hipMemcpyDeviceToHost), "hipMemcpy");
    hipFree(d_in);
    hipFree(d_out);
    return rc;
} ABI_CATCH

// fr29_lin_add<1 / 2> on the device over tables the planner's builder makes for the call (include/acvm_amd.h). The coefficient takes the planner's
// road: field element -> the record's inline words (plan.cpp push_coef) -> lin_table_of.
int acvm_debug_lin_add(const uint32_t *n_terms, const uint32_t *coef, const uint32_t *rows, const uint32_t *h, uint32_t n_items, uint32_t *tables_out, uint32_t *out) try {
    if (!n_items) return 0;
    if (!n_terms || !coef || !rows || !h || !out) return set_err(ACVM_E_INVALID, "null argument");
    const size_t n_groups = ((size_t)n_items + 63) / 64;
    std::vector<uint32_t> tables(n_groups * 2 * GATE_LIN_TABLE_WORDS, 0);
    for (size_t g = 0; g < n_groups; g++) {
        if (n_terms[g] != 1 && n_terms[g] != 2) return set_err(ACVM_E_INVALID, "a group has one or two terms");
        for (uint32_t t = 0; t < n_terms[g]; t++) {
            uint64_t c[4];
            for (int i = 0; i < 4; i++) c[i] = coef[g * 16 + t * 8 + 2 * i] | (uint64_t)coef[g * 16 + t * 8 + 2 * i + 1] << 32;
            if (frh::geq_p(c)) return set_err(ACVM_E_INVALID, "a coefficient is not canonical");
            const FrH d = frh::to_device_form(frh::from_canonical(c));
            uint32_t inline_words[8];
            for (int i = 0; i < 4; i++) { inline_words[2 * i] = (uint32_t)d.l[i]; inline_words[2 * i + 1] = (uint32_t)(d.l[i] >> 32); }
            lin_table_of(inline_words, &tables[(g * 2 + t) * GATE_LIN_TABLE_WORDS]);
        }
    }
    if (tables_out) memcpy(tables_out, tables.data(), tables.size() * 4);
    const size_t bytes[5] = {n_groups * 4, tables.size() * 4, (size_t)n_items * 16 * 4, (size_t)n_items * 9 * 4, (size_t)n_items * 9 * 4};
    const void *src[4] = {n_terms, tables.data(), rows, h};
    uint32_t *d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    auto step = [&](hipError_t e, const char *what_) { if (!rc && e != hipSuccess) rc = set_err(ACVM_E_DEVICE, std::string(what_) + ": " + hipGetErrorString(e)); };
    for (int k = 0; k < 5; k++) step(hipMalloc((void **)&d[k], bytes[k]), "hipMalloc");
    for (int k = 0; k < 4 && !rc; k++) step(hipMemcpy(d[k], src[k], bytes[k], hipMemcpyHostToDevice), "hipMemcpy");
    if (!rc) step(hipMemset(d[4], 0, bytes[4]), "hipMemset");
    if (!rc) launch_lin_add_probe(nullptr, d[0], d[1], d[2], d[3], n_items, d[4]);
    step(hipGetLastError(), "lin_add_probe_kernel");
    step(hipDeviceSynchronize(), "hipDeviceSynchronize");
    if (!rc) step(hipMemcpy(out, d[4], bytes[4], hipMemcpyDeviceToHost), "hipMemcpy");
    for (int k = 0; k < 5; k++)
        if (d[k]) hipFree(d[k]);
    return rc;
} ABI_CATCH

// The shipped inverse_batch_kernel through its launcher on a table made for the call: row k of W = the denominators of job k, job k = {row k, opcode
// k, inverse slot slot_of[k] (k when null)}, the batch's row stride, event words behind the header a batch gives them (event_words_new).
// (inv_share: the waves to a field inversion, as the launcher takes them)
static int debug_inverse_batch(const uint32_t *den, uint32_t n_jobs, uint32_t B, uint32_t inv_chunk, uint32_t inv_share, const uint32_t *slot_of, uint32_t *inv_out,
                               uint32_t *event_out, uint32_t *device_count, uint32_t *host_count) {
    if (!den || !n_jobs || !B || !inv_out || !event_out || !device_count || !host_count) return set_err(ACVM_E_INVALID, "bad argument");
    if (slot_of) {  // a permutation of [0, n_jobs): every job owns one row of the inverse table
        std::vector<uint8_t> seen(n_jobs, 0);
        for (uint32_t k = 0; k < n_jobs; k++) {
            if (slot_of[k] >= n_jobs || seen[slot_of[k]]) return set_err(ACVM_E_INVALID, "slot_of is not a permutation");
            seen[slot_of[k]] = 1;
        }
    }
    const uint64_t Bp = ((uint64_t)B + 63) / 64 * 64;
    const size_t row = (size_t)2 * Bp, table_bytes = (size_t)n_jobs * row * sizeof(uint4);
    std::vector<uint4> hW((size_t)n_jobs * row, make_uint4(0, 0, 0, 0));
    std::vector<uint32_t> stream((size_t)n_jobs * 3), offset(n_jobs);
    for (uint32_t k = 0; k < n_jobs; k++) {
        for (uint32_t j = 0; j < B; j++) {
            const uint32_t *v = den + ((size_t)k * B + j) * 8;
            hW[(size_t)k * row + j] = make_uint4(v[0], v[1], v[2], v[3]);
            hW[(size_t)k * row + Bp + j] = make_uint4(v[4], v[5], v[6], v[7]);
        }
        stream[3 * (size_t)k] = k;
        stream[3 * (size_t)k + 1] = k;
        stream[3 * (size_t)k + 2] = slot_of ? slot_of[k] : k;
        offset[k] = 3 * k;
    }
    struct Mem {
        uint4 *W = nullptr, *inv = nullptr;
        uint32_t *stream = nullptr, *offset = nullptr, *event_base = nullptr, *event = nullptr, *h_count = nullptr;
        ~Mem() {
            for (void *p : {(void *)W, (void *)inv, (void *)stream, (void *)offset, (void *)event_base})
                if (p) hipFree(p);
            if (h_count) hipHostFree(h_count);
        }
    } m;
    HIPCHK(hipMalloc((void **)&m.W, table_bytes));
    HIPCHK(hipMalloc((void **)&m.inv, table_bytes));
    HIPCHK(hipMemcpy(m.W, hW.data(), table_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(m.inv, 0, table_bytes));
    if (int rc = upload(&m.stream, stream)) return rc;
    if (int rc = upload(&m.offset, offset)) return rc;
    if (int rc = event_words_new(B, &m.event_base, &m.event, &m.h_count)) return rc;
    *m.h_count = 0;
    launch_event_reset(nullptr, m.event, B);
    launch_inverse_batch(nullptr, m.W, m.inv, Bp, B, m.stream, m.offset, n_jobs, m.event, inv_chunk, inv_share);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(hW.data(), m.inv, table_bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(event_out, m.event, (size_t)B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(device_count, m.event - 4, 4, hipMemcpyDeviceToHost));
    *host_count = *(volatile uint32_t *)m.h_count;
    for (uint32_t k = 0; k < n_jobs; k++)
        for (uint32_t j = 0; j < B; j++) {
            const uint4 lo = hW[(size_t)k * row + j], hi = hW[(size_t)k * row + Bp + j];
            uint32_t *v = inv_out + ((size_t)k * B + j) * 8;
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        }
    return 0;
}
// ... with the process-wide inv_share (what a handle created now would snapshot): the shipped default unless the caller set another
int acvm_debug_inverse_batch(const uint32_t *den, uint32_t n_jobs, uint32_t B, uint32_t inv_chunk, const uint32_t *slot_of, uint32_t *inv_out,
                             uint32_t *event_out, uint32_t *device_count, uint32_t *host_count) try {
    return debug_inverse_batch(den, n_jobs, B, inv_chunk, inverse_share_clamp(tuning().inv_share), slot_of, inv_out, event_out, device_count, host_count);
} ABI_CATCH
// ... with inv_share of the caller's (1, 2, 4, 8; anything else: the next lower of those)
int acvm_debug_inverse_batch_shared(const uint32_t *den, uint32_t n_jobs, uint32_t B, uint32_t inv_chunk, uint32_t inv_share, const uint32_t *slot_of,
                                    uint32_t *inv_out, uint32_t *event_out, uint32_t *device_count, uint32_t *host_count) try {
    return debug_inverse_batch(den, n_jobs, B, inv_chunk, inverse_share_clamp(inv_share), slot_of, inv_out, event_out, device_count, host_count);
} ABI_CATCH

// Host-only: the gate stream of the plan a handle of these options would use, copied word for word beside acvm_debug_plan_fingerprint's hashes of it
// (tests/test_arith_cases.py reads the record shapes -- kinds, counts, flags -- that its case lists reach). out: [n_programs, n_stream_words,
// gate_offset[n_programs], lin_offset[n_programs] (GATE_LIN_NONE where the plan has none), gate_stream[n_stream_words]]; returns the number of words
// that is, of which the first min(that, cap) are written (out may be null with cap = 0: ask for the size first).
int acvm_debug_gate_records(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids, uint32_t n_keep,
                            uint32_t *out, uint32_t cap) try {
    if (!c || (n_initial && !initial_ids) || (n_keep && !keep_ids) || (cap && !out)) return set_err(ACVM_E_INVALID, "null argument");
    PlanOpts opts;
    opts.fold_digest = (flags & (ACVM_BATCH_FOLD_DIGEST | ACVM_BATCH_REUSE_SLOTS)) != 0;
    opts.reuse_slots = (flags & ACVM_BATCH_REUSE_SLOTS) != 0;
    opts.host_blackbox = (flags & 0x100u) != 0;
    opts.keep.assign(keep_ids, keep_ids + n_keep);
    const std::shared_ptr<const Plan> sp = plan_for(c, initial_ids, n_initial, opts);
    const Plan &p = *sp;
    if (!p.unsupported.empty()) return set_err(ACVM_E_UNSUPPORTED, p.unsupported);
    const uint64_t n_prog = p.gate_offset.size(), n_words = p.gate_stream.size(), total = 2 + 2 * n_prog + n_words;
    if (total > 0x7FFFFFFFull) return set_err(ACVM_E_INVALID, "the gate stream is too large for this probe");
    std::vector<uint32_t> all;
    all.reserve((size_t)total);
    all.push_back((uint32_t)n_prog);
    all.push_back((uint32_t)n_words);
    all.insert(all.end(), p.gate_offset.begin(), p.gate_offset.end());
    for (size_t q = 0; q < n_prog; q++) all.push_back(q < p.lin_offset.size() ? p.lin_offset[q] : GATE_LIN_NONE);
    all.insert(all.end(), p.gate_stream.begin(), p.gate_stream.end());
    if (cap) memcpy(out, all.data(), (size_t)std::min<uint64_t>(total, cap) * 4);
    return (int)total;
} ABI_CATCH

// Host-only: the per-lane scratch words the plan reserves for each opcode's record (Plan::prog_scratch: hash messages, the working memory of
// Directive::PermutationSort, Schnorr's preimage and window table, the Brillig VM), one word per opcode in program order, 0 where the record takes
// none. tests/test_sort_cases.py holds the reservation of a sort against the allocation walk of ops_sort.hpp. Returns the number of opcodes and writes
// the first min(that, cap) words (out may be null with cap = 0).
int acvm_debug_record_scratch(const acvm_circuit_t *c, const uint32_t *initial_ids, uint32_t n_initial, uint32_t flags, const uint32_t *keep_ids, uint32_t n_keep,
                              uint32_t *out, uint32_t cap) try {
    if (!c || (n_initial && !initial_ids) || (n_keep && !keep_ids) || (cap && !out)) return set_err(ACVM_E_INVALID, "null argument");
    PlanOpts opts;
    opts.fold_digest = (flags & (ACVM_BATCH_FOLD_DIGEST | ACVM_BATCH_REUSE_SLOTS)) != 0;
    opts.reuse_slots = (flags & ACVM_BATCH_REUSE_SLOTS) != 0;
    opts.host_blackbox = (flags & 0x100u) != 0;
    opts.keep.assign(keep_ids, keep_ids + n_keep);
    const std::shared_ptr<const Plan> sp = plan_for(c, initial_ids, n_initial, opts);
    const Plan &p = *sp;
    if (!p.unsupported.empty()) return set_err(ACVM_E_UNSUPPORTED, p.unsupported);
    if (p.prog_scratch.size() > 0x7FFFFFFFull) return set_err(ACVM_E_INVALID, "too many opcodes for this probe");
    if (cap) memcpy(out, p.prog_scratch.data(), std::min<size_t>(p.prog_scratch.size(), cap) * 4);
    return (int)p.prog_scratch.size();
} ABI_CATCH

// The shipped selection kernels through their launcher on a status array of the caller's (kernels_select.hip launch_select). The device's list starts as the
// caller's out_list, so that what the kernels leave alone comes back as it went in.
int acvm_debug_select(const uint8_t *status, uint32_t n, uint32_t select_mask, uint32_t *out_list, uint32_t *n_selected) try {
    if (!n_selected || (n && !status)) return set_err(ACVM_E_INVALID, "null argument");
    struct Mem {
        uint8_t *status = nullptr;
        uint32_t *list = nullptr, *scratch = nullptr;
        ~Mem() {
            for (void *p : {(void *)status, (void *)list, (void *)scratch})
                if (p) hipFree(p);
        }
    } m;
    const size_t words = select_scratch_words(n);
    HIPCHK(hipMalloc((void **)&m.status, n ? n : 1));
    HIPCHK(hipMalloc((void **)&m.scratch, (words + 1) * 4));
    if (n) HIPCHK(hipMemcpy(m.status, status, n, hipMemcpyHostToDevice));
    if (out_list && n) {
        HIPCHK(hipMalloc((void **)&m.list, (size_t)n * 4));
        HIPCHK(hipMemcpy(m.list, out_list, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    launch_select(nullptr, m.status, 0, n, select_mask, m.scratch, m.list, m.scratch + words);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(n_selected, m.scratch + words, 4, hipMemcpyDeviceToHost));
    if (m.list) HIPCHK(hipMemcpy(out_list, m.list, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
} ABI_CATCH
