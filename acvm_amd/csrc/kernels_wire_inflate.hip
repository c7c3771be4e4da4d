// kernels_wire_inflate.hip -- the gzip import of the batch-wide WitnessMap wire format, stage 1 (include/acvm_amd.h
// acvm_batch_import_device_wire_gzip): every row's gzip member -- any RFC 1951 stream, other programs' output -- inflated into the row's scratch
// slot, which stage 2 (kernels_wire_in.hip) reads as an ACVM_WIRE_BINCODE slot. The bytes are untrusted; the reader is wire_inflate.hpp's, whose
// header states what keeps every index inside its bound and every row finite.
//
//  wire_inflate_kernel  one lane per row, a wave (= a block of 64 threads) per 64 consecutive rows. A row is a sequential bit stream: nothing of
//                       it is parallel, so the batch is. Per block in LDS: the CRC-32 byte table and the fixed code's tables, once. Per row
//                       its code tables -- counts and symbols of 288 + 32 codes and the 320 four-bit code lengths a dynamic block's
//                       description is held in while its tables are built, 900 bytes -- in the call's arena in global memory, where the
//                       caches hold them: in LDS (57 KiB a wave) a CU holds two such waves, and the kernel waits on latency, not on
//                       bandwidth -- measured, the arena is 1.1 to 1.2 times as fast (NOTEBOOK, "Batch-wide wire format: inflate"). No array
//                       is a lane's own: nothing lands in private scratch memory. History for back-references is the row's scratch slot in
//                       global memory (32 KiB a row do not fit on chip). Input is fetched byte by byte (eight bytes a load measured 4 %
//                       slower). Stores are gathered: four output bytes leave as one dword (the slot is 16-aligned and the reader stores
//                       ascending), a back-reference into the dword still being gathered reads the register; the last 0 .. 3 bytes leave
//                       one by one, so that nothing at or behind the row's length is written.
//
// Per row: its length, its finding {class, block} and its CRC-32; per batch the count of findings and the smallest (instance, class, block).
// A translation unit of its own: the other code objects compile to what they compiled to before.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "wire_inflate.hpp"
#include "wire_inflate_plan.hpp"

namespace acvm {

static_assert(INFLATE_LCNT == INFLATE_PLAN_LCNT && INFLATE_DCNT == INFLATE_PLAN_DCNT && INFLATE_LSYM == INFLATE_PLAN_LSYM && INFLATE_DSYM == INFLATE_PLAN_DSYM &&
                  INFLATE_TAB_HALFWORDS == INFLATE_PLAN_TAB_HALFWORDS,
              "the reader (wire_inflate.hpp) and the plan (wire_inflate_plan.hpp) agree on a code table's layout");

constexpr uint32_t INFLATE_ROWS = 64;
// a row's tables in the arena: the halfwords, the nibbles behind them, one dword of padding that makes the pitch odd
constexpr uint32_t INFLATE_ROW_WORDS = (INFLATE_TAB_HALFWORDS / 2u + INFLATE_LEN_NIBBLES / 8u) | 1u;
static_assert(INFLATE_TAB_HALFWORDS % 2u == 0 && INFLATE_LEN_NIBBLES % 8u == 0 && INFLATE_ROW_WORDS == INFLATE_PLAN_ROW_WORDS, "184 + 40 dwords and one of padding");

struct InflateIn {
    const uint8_t *row;
    __device__ __forceinline__ uint32_t operator()(uint64_t k) const { return row[k]; }
};
struct InflateTab {
    uint16_t *half;
    uint8_t *nibbles;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return half[i]; }
    __device__ __forceinline__ void set(uint32_t i, uint32_t v) const { half[i] = (uint16_t)v; }
    __device__ __forceinline__ uint32_t len(uint32_t i) const { return (nibbles[i >> 1] >> (4u * (i & 1u))) & 15u; }
    __device__ __forceinline__ void set_len(uint32_t i, uint32_t v) const {
        const uint32_t shift = 4u * (i & 1u);
        nibbles[i >> 1] = (uint8_t)((nibbles[i >> 1] & ~(15u << shift)) | (v << shift));
    }
};
// the row's scratch slot: four bytes gathered into a dword before they leave (the reader stores byte k = the bytes stored so far)
struct InflateOut {
    uint8_t *slot;
    uint32_t pending = 0u;  // bytes [4 * (k >> 2), k) of the dword byte k falls into
    __device__ __forceinline__ void store(uint64_t k, uint32_t b) {
        pending |= b << (8u * ((uint32_t)k & 3u));
        if (((uint32_t)k & 3u) == 3u) {
            *(uint32_t *)(slot + (k & ~(uint64_t)3)) = pending;
            pending = 0u;
        }
    }
    // (k < stored: the caller's rule. The dword being gathered is the one `stored` falls into; the reader loads before it stores)
    __device__ __forceinline__ uint32_t load(uint64_t k, uint64_t stored) const {
        if ((k >> 2) == (stored >> 2)) return (pending >> (8u * ((uint32_t)k & 3u))) & 0xffu;
        return slot[k];
    }
    __device__ __forceinline__ void finish(uint64_t n) {
        for (uint64_t k = n & ~(uint64_t)3; k < n; k++) slot[k] = (uint8_t)(pending >> (8u * ((uint32_t)k & 3u)));
    }
};

__global__ void __launch_bounds__(INFLATE_ROWS) wire_inflate_kernel(const WireInflate a) {
    __shared__ uint32_t crc_table[256];
    __shared__ uint16_t fixed[INFLATE_TAB_HALFWORDS];
    const uint32_t t = threadIdx.x;
    for (uint32_t x = t; x < 256u; x += INFLATE_ROWS) crc_table[x] = wire_crc_table_entry(x);
    for (uint32_t x = t; x < INFLATE_TAB_HALFWORDS; x += INFLATE_ROWS) fixed[x] = a.fixed[x];
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * INFLATE_ROWS + t;
    if (j >= a.n) return;
    uint64_t n_in = a.pitch;
    if (a.lengths) {
        const uint64_t length = a.lengths[j];
        n_in = length < n_in ? length : n_in;
    }
    uint32_t *mine = a.tables + j * INFLATE_ROW_WORDS;
    const InflateTab tab{(uint16_t *)mine, (uint8_t *)(mine + INFLATE_TAB_HALFWORDS / 2u)};
    const InflateIn in{a.in + j * a.pitch};
    InflateOut out{a.out + j * a.out_pitch};
    const uint16_t *fixed_table = fixed;
    const uint32_t *crc = crc_table;
    const InflateRow r = wire_inflate_row(in, n_in, out, a.out_cap, tab, fixed_table, crc);
    a.out_lengths[j] = r.length;
    a.findings[2u * j] = r.cls;
    a.findings[2u * j + 1u] = r.block;
    if (a.crcs) a.crcs[j] = r.crc;
    if (r.cls && a.result) {  // (findings are the exception: a lane that has one speaks for itself)
        atomicAdd((unsigned long long *)a.result, 1ull);
        atomicMax((unsigned long long *)a.result + 1, (unsigned long long)inflate_key(j, r.cls, r.block));
    }
}

void launch_wire_inflate(hipStream_t s, const WireInflate &x) {
    if (!x.n) return;
    hipLaunchKernelGGL(wire_inflate_kernel, dim3((x.n + INFLATE_ROWS - 1u) / INFLATE_ROWS), dim3(INFLATE_ROWS), 0, s, x);
}

}  // namespace acvm
