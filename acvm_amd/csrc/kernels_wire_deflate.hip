// kernels_wire_deflate.hip -- the deflating container of the batch-wide WitnessMap wire format (include/acvm_amd.h ACVM_WIRE_GZIP_DEFLATE): every
// output row's map as one gzip member of one dynamic-Huffman block whose code is a constant of the format (wire_plan.cpp) and whose tokens are
// a function of the body alone (wire_deflate.hpp).
//
//  wire_deflate_kernel  a block of 256 threads owns 64 consecutive output rows and walks the windows of WIRE_WINDOW list positions in list
//                       order: a row's bit position depends on everything in front of it, so the stored container's grid of (rows x windows)
//                       does not carry over. Per row in LDS: the window's entries, the last entry of the window before, a bit buffer and its
//                       cursor. Once per row: the gzip head, the constant block header and the 8 count literals. Per window: (a) one wave per
//                       list position, lane = row, encodes as wire_entries_kernel does and folds the entry's raw CRC into the row's; (b) one
//                       thread per (row, entry) makes the entry's equality masks and its cost in bits, a prefix over the row's at most
//                       WIRE_WINDOW costs gives its bit offset; (c) the same thread emits its tokens there -- neighbours meet in one dword,
//                       which both OR in with an LDS atomic; (d) each row's COMPLETE dwords leave as consecutive dwords on consecutive lanes,
//                       nontemporal, and the partial dword moves to the buffer's front. Once per row at the end: end-of-block, the CRC-32 and
//                       ISIZE at the next byte, the remaining dwords and the last 0 .. 3 bytes one by one, the length.
//
// No byte of the caller's buffer is loaded, and none at or behind a row's length is written: a complete dword of the stream always has
// end-of-block and the trailer behind it. A row's position is a 64-bit dword index plus a cursor below 32 bits.
//
// The loop bound is the block's: it ends at the first window from which on none of its rows has an entry left (rows that name no instance, short
// maps of the exact path), and rows that are done idle while their neighbours go on.
//
// LDS: 64 rows x (153 + 111 + 19) dwords, the tables and the per-row words: 78 KiB, two blocks of four waves on a CU of 160 KiB. A window of 8
// is the stored kernel's and the plan's; a window of 16 would leave one block per CU, a window of 4 twice the barriers per entry.
#include "ops_common.hpp"
#include "kernels.hpp"
#include "export_source.hpp"
#include "wire_deflate.hpp"
#include "wire_plan.hpp"
#include "wire_rows.hpp"

namespace acvm {

static_assert(WIRE_GZIP_DEFLATE == ACVM_WIRE_GZIP_DEFLATE, "the container of include/acvm_amd.h");
static_assert(WIRE_DEFLATE_LIT == WIRE_PLAN_DEFLATE_LIT && WIRE_DEFLATE_MATCH == WIRE_PLAN_DEFLATE_MATCH && WIRE_DEFLATE_PREFIX == WIRE_PLAN_DEFLATE_PREFIX &&
                  WIRE_DEFLATE_PREFIX_WORDS == WIRE_PLAN_DEFLATE_PREFIX_WORDS && WIRE_DEFLATE_WORDS == WIRE_PLAN_DEFLATE_WORDS && WIRE_WINDOW == WIRE_PLAN_WINDOW,
              "the kernel (wire_deflate.hpp) and the plan (wire_plan.hpp) agree on the table and the window");

// A row's bit buffer: the partial dword in front (< 32 bits) and a window's entries at their dearest; the prologue (the prefix and 8 literals of
// at most 10 bits) and the epilogue (end-of-block, 7 bits of padding, the trailer) are far shorter. An odd pitch: lane = row.
constexpr uint32_t DEFLATE_BUF_WORDS = (31u + WIRE_WINDOW * WIRE_DEFLATE_ENTRY_MAX_BITS + 31u) / 32u, DEFLATE_BUF_PITCH = DEFLATE_BUF_WORDS | 1u;
static_assert(DEFLATE_BUF_WORDS == 111u && DEFLATE_BUF_PITCH == 111u && 31u + WIRE_WINDOW * WIRE_DEFLATE_ENTRY_MAX_BITS <= DEFLATE_BUF_WORDS * 32u,
              "the worst case -- 31 carried bits and 8 entries of 440 -- is 3 551 of the buffer's 3 552 bits: the dword the cursor stands in is always inside");
static_assert(WIRE_DEFLATE_PREFIX_WORDS * 32u + 8u * 10u <= DEFLATE_BUF_WORDS * 32u, "the prologue fits the bit buffer");
constexpr uint32_t DEFLATE_PER_THREAD = WIRE_ROWS * WIRE_WINDOW / 256u;  // (row, entry) pairs of a window per thread
static_assert(DEFLATE_PER_THREAD * 256u == WIRE_ROWS * WIRE_WINDOW, "a whole number of pairs per thread");

struct DeflateLdsSink {
    uint32_t *buf;
    __device__ __forceinline__ void shared(uint32_t word, uint32_t bits) const { atomicOr(buf + word, bits); }
    __device__ __forceinline__ void own(uint32_t word, uint32_t bits) const { buf[word] = bits; }
};

__global__ void __launch_bounds__(256) wire_deflate_kernel(const WireExport a, uint32_t n_windows) {
    __shared__ uint32_t image[WIRE_ROWS * WIRE_LDS_PITCH];
    __shared__ uint32_t bitbuf[WIRE_ROWS * DEFLATE_BUF_PITCH];
    __shared__ uint32_t last[WIRE_ROWS * WIRE_ENTRY_WORDS];  // (19 dwords: an odd pitch)
    __shared__ uint32_t cost[WIRE_WINDOW * WIRE_ROWS];
    __shared__ uint32_t crc_table[256], table[WIRE_DEFLATE_WORDS];
    __shared__ uint32_t row_j[WIRE_ROWS], row_base[WIRE_ROWS], row_count[WIRE_ROWS], row_entries[WIRE_ROWS], row_crc[WIRE_ROWS];
    __shared__ uint32_t row_cursor[WIRE_ROWS], row_next[WIRE_ROWS];  // the bits in the row's buffer: before and behind what is being emitted
    __shared__ uint64_t row_word[WIRE_ROWS];                         // the dword of the slot the buffer's front is
    __shared__ int32_t row_lane[WIRE_ROWS];
    __shared__ uint32_t block_more;  // whether a row of the block has an entry at or behind the window's first position
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint64_t i0 = (uint64_t)blockIdx.x * WIRE_ROWS;
    const uint32_t nb = a.n - i0 < WIRE_ROWS ? (uint32_t)(a.n - i0) : WIRE_ROWS;  // (the grid has no block at or behind n)

    // (d) the complete dwords of every row leave; the partial one moves to the front. row_next: the bits in the buffer. Two barriers, the
    // second of which ends the phase.
    auto flush = [&]() {
        uint32_t carry = 0u, full_t = 0u;
        if (t < WIRE_ROWS) {
            full_t = row_next[t] >> 5;
            carry = bitbuf[t * DEFLATE_BUF_PITCH + full_t];
        }
        for (uint32_t i = wave; i < nb; i += 4u) {
            const uint32_t full = row_next[i] >> 5;
            uint32_t *dst = (uint32_t *)(a.out + (i0 + i) * a.pitch) + row_word[i];
            for (uint32_t x = lane; x < full; x += 64u) __builtin_nontemporal_store(bitbuf[i * DEFLATE_BUF_PITCH + x], dst + x);
        }
        __syncthreads();
        for (uint32_t i = wave; i < WIRE_ROWS; i += 4u) {
            const uint32_t full = row_next[i] >> 5;
            for (uint32_t x = 1u + lane; x <= full; x += 64u) bitbuf[i * DEFLATE_BUF_PITCH + x] = 0u;
        }
        if (t < WIRE_ROWS) {
            if (full_t) bitbuf[t * DEFLATE_BUF_PITCH] = carry;
            row_word[t] += full_t;
            row_cursor[t] = row_next[t] & 31u;
        }
        __syncthreads();
    };

    // ---- the tables, the rows, an empty buffer
    for (uint32_t x = t; x < 256u; x += 256u) crc_table[x] = wire_crc_table_entry(x);
    for (uint32_t x = t; x < WIRE_DEFLATE_WORDS; x += 256u) table[x] = a.deflate[x];
    for (uint32_t x = t; x < WIRE_ROWS * DEFLATE_BUF_PITCH; x += 256u) bitbuf[x] = 0u;
    if (t < WIRE_ROWS) {
        WireRow r{0xFFFFFFFFu, -1};
        uint32_t entries = 0u;
        if (t < nb) {
            r = wire_row(a, i0 + t);
            entries = wire_row_entries(a, r);
        }
        row_j[t] = r.j;
        row_lane[t] = r.lane;
        row_entries[t] = entries;
        row_crc[t] = 0u;
        row_word[t] = 0u;
        row_cursor[t] = 0u;
        row_next[t] = 0u;
    }
    __syncthreads();
    // ---- once per row: the gzip head and the constant header, then the count's 8 bytes as literals
    if (t < nb) {
        uint32_t *buf = bitbuf + t * DEFLATE_BUF_PITCH;
        for (uint32_t x = 0; x < WIRE_DEFLATE_PREFIX_WORDS; x++) buf[x] = table[WIRE_DEFLATE_PREFIX + x];
        WireBitWriter<DeflateLdsSink> w(DeflateLdsSink{buf}, a.deflate_prefix_bits);
        const uint32_t entries = row_entries[t];
        for (uint32_t k = 0; k < 8u; k++) {
            const uint32_t e = table[WIRE_DEFLATE_LIT + (k < 4u ? (entries >> (8u * k)) & 0xffu : 0u)];
            w.put(e & 0xffffu, e >> 16);
        }
        row_next[t] = (uint32_t)w.finish();
    }
    __syncthreads();
    flush();

    for (uint32_t window = 0; window < n_windows; window++) {
        const uint32_t k0 = window * WIRE_WINDOW, k1 = a.n_positions - k0 < WIRE_WINDOW ? a.n_positions : k0 + WIRE_WINDOW;  // (k0 < n_positions)
        // ---- where each row's run of this window starts and how long it is
        if (t < WIRE_ROWS) {
            uint32_t base = 0u, count = 0u;
            const uint32_t j = row_j[t];
            const int32_t ln = row_lane[t];
            if (j < a.src.B) {
                base = ln < 0 ? a.rank[k0] : wire_lane_rank(a, (uint32_t)ln, k0);
                count = (ln < 0 ? a.rank[k1] : wire_lane_rank(a, (uint32_t)ln, k1)) - base;
            }
            row_base[t] = base;
            row_count[t] = count;
            row_next[t] = row_cursor[t];
            const unsigned long long more = __ballot(base < row_entries[t]);  // (t < WIRE_ROWS is wave 0, whole)
            if (t == 0) block_more = more != 0ull;
        }
        __syncthreads();
        if (!block_more) break;  // (block-uniform; written again only behind the barrier that ends flush())
        // ---- (a) one wave per list position, lane = row, as kernels_wire.hip wire_entries_kernel phase 1
        {
            const uint32_t i = lane;
            const uint32_t j = row_j[i], base = row_base[i], entries = row_entries[i];
            const int32_t ln = row_lane[i];
            const ExportListSource &L = a.src;
            uint32_t *img = image + i * WIRE_LDS_PITCH;
            uint32_t crc = 0u;
            for (uint32_t k = k0 + wave; k < k1; k += 4u) {
                const uint32_t w = a.sel ? a.sel[k] : k;
                if (j >= L.B) continue;
                uint32_t rank;
                Fr row, factor;
                if (ln < 0) {
                    uint32_t at, ui;
                    export_generic_source(w, a.n_witnesses, a.row_of, a.producer, a.u_index, at, ui);
                    if (at == 0xFFFFFFFFu) continue;
                    rank = a.rank[k];
                    row = fr_load_nt(a.W, at, a.Bp, j);
                    factor = ui != 0xFFFFFFFFu ? fr_const(a.u_plain, ui) : export_plain_factor(EXPORT_ENC_BE32);
                } else {
                    if (!export_lane_assigned(L.assigned_bits, L.n_slow, (uint32_t)ln, w, a.n_witnesses)) continue;
                    rank = wire_lane_rank(a, (uint32_t)ln, k);
                    row = fr_load(L.Wx, w, L.Bpx, L.side ? (uint64_t)(uint32_t)ln : (uint64_t)j);
                    factor = export_plain_factor(EXPORT_ENC_BE32);
                }
                uint32_t entry[WIRE_ENTRY_WORDS];
                wire_entry(w, export_encode(row, factor, EXPORT_ENC_BE32, true), entry);
                uint32_t *at = img + (rank - base) * WIRE_ENTRY_WORDS;  // (rank - base < row_count <= WIRE_WINDOW)
#pragma unroll
                for (uint32_t x = 0; x < WIRE_ENTRY_WORDS; x++) at[x] = entry[x];
                crc ^= wire_crc_mul(a.crc_pow[entries - 1u - rank], wire_crc_raw(entry, WIRE_ENTRY_WORDS, crc_table));
            }
            if (crc) atomicXor(&row_crc[i], crc);
        }
        __syncthreads();
        // ---- (b) the cost of entry e of row `lane`, e = wave, wave + 4: against the entry in front of it, which for e = 0 is `last`
        WireDeflateMasks masks[DEFLATE_PER_THREAD];
        const uint32_t count = row_count[lane];
#pragma unroll
        for (uint32_t r = 0; r < DEFLATE_PER_THREAD; r++) {
            const uint32_t e = wave + 4u * r;
            if (e >= count) continue;
            const uint32_t *cur = image + lane * WIRE_LDS_PITCH + e * WIRE_ENTRY_WORDS;
            const uint32_t *prev = e ? cur - WIRE_ENTRY_WORDS : last + lane * WIRE_ENTRY_WORDS;
            masks[r] = wire_deflate_masks(cur, prev, row_base[lane] + e != 0u);
            cost[e * WIRE_ROWS + lane] = wire_deflate_cost(cur, masks[r], table);
        }
        __syncthreads();
        // ---- (c) its tokens at the row's cursor plus the costs in front of it; the row's last entry says where the row stands afterwards
#pragma unroll
        for (uint32_t r = 0; r < DEFLATE_PER_THREAD; r++) {
            const uint32_t e = wave + 4u * r;
            if (e >= count) continue;
            uint32_t at = row_cursor[lane];
            for (uint32_t f = 0; f < e; f++) at += cost[f * WIRE_ROWS + lane];
            const uint32_t *cur = image + lane * WIRE_LDS_PITCH + e * WIRE_ENTRY_WORDS;
            const uint32_t end = (uint32_t)wire_deflate_emit(cur, masks[r], table, DeflateLdsSink{bitbuf + lane * DEFLATE_BUF_PITCH}, at);
            if (e + 1u == count) row_next[lane] = end;
        }
        __syncthreads();
        // the window's last entry is the next window's predecessor
        if (count)
            for (uint32_t x = wave; x < WIRE_ENTRY_WORDS; x += 4u) last[lane * WIRE_ENTRY_WORDS + x] = image[lane * WIRE_LDS_PITCH + (count - 1u) * WIRE_ENTRY_WORDS + x];
        // ---- (d)
        flush();
    }

    // ---- once per row: end-of-block, the trailer at the next byte, what is left of the buffer, the length
    if (t < nb) {
        uint32_t *buf = bitbuf + t * DEFLATE_BUF_PITCH;
        const uint32_t entries = row_entries[t];
        WireBitWriter<DeflateLdsSink> w(DeflateLdsSink{buf}, row_cursor[t]);
        const uint32_t eob = table[WIRE_DEFLATE_LIT + WIRE_DEFLATE_EOB];
        w.put(eob & 0xffffu, eob >> 16);
        const uint32_t block_bytes = ((uint32_t)w.finish() + 7u) / 8u;
        uint32_t raw_count = entries;  // raw(u64le N): eight table-free byte steps are 64 shift steps
        for (int k = 0; k < 64; k++) raw_count = (raw_count >> 1) ^ (WIRE_CRC_POLY & (0u - (raw_count & 1u)));
        WireBitWriter<DeflateLdsSink> trailer(DeflateLdsSink{buf}, 8u * block_bytes);
        trailer.put(wire_crc_combine(a.crc_pow[entries], a.crc_x64, raw_count, row_crc[t]), 32u);
        trailer.put((uint32_t)wire_body_bytes(entries), 32u);
        trailer.finish();
        const uint32_t bytes = block_bytes + WIRE_TRAILER_BYTES;  // (< 4 * DEFLATE_BUF_WORDS)
        uint8_t *slot = a.out + (i0 + t) * a.pitch + 4u * row_word[t];
        for (uint32_t x = 0; x < bytes / 4u; x++) __builtin_nontemporal_store(buf[x], (uint32_t *)slot + x);
        for (uint32_t y = bytes & ~3u; y < bytes; y++) slot[y] = (uint8_t)(buf[y >> 2] >> (8u * (y & 3u)));
        if (a.lengths) a.lengths[i0 + t] = 4u * row_word[t] + bytes;
    }
}

void launch_wire_deflate(hipStream_t s, const WireExport &x, uint32_t n_windows) {
    if (!x.n) return;
    hipLaunchKernelGGL(wire_deflate_kernel, dim3((x.n + WIRE_ROWS - 1u) / WIRE_ROWS), dim3(256), 0, s, x, n_windows);
}

}  // namespace acvm
