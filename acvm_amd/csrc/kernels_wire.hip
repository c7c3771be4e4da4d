// kernels_wire.hip -- the batch-wide WitnessMap wire format (include/acvm_amd.h acvm_batch_witness_maps_wire_device): every output row's map
// as the reference's own bytes -- the bincode body, alone or inside a stored-block gzip member (wire_encode.hpp) -- at a pitch.
//
//  wire_lane_prefix_kernel  one thread per lane of the exact path: the prefix of its assigned list positions per 32-witness word, the ranks of
//                           a lane's entries (a generic instance's ranks are the plan's table, wire_plan.hpp)
//  wire_entries_kernel      a block of 256 threads owns 64 consecutive output rows and one window of WIRE_WINDOW list positions. A row's
//                           entries of a window are contiguous in its body, at 8 + 76 * rank(window start). Phase 0: the rows' runs. Phase 1:
//                           one wave per list position, lane = row -- the element from where the other exports take it (export_source.hpp),
//                           encoded, hex-expanded (wire_encode.hpp) and placed in the row's LDS image at its rank inside the window; its raw
//                           CRC (table sliced by 4, in LDS) times x^(8 * 76 * (N - 1 - rank)) joins the row's XOR. Phase 2: each row's run
//                           leaves as consecutive aligned dwords on consecutive lanes, nontemporal; where a run crosses a stored-block
//                           boundary the 20 bytes of the joint are written by the thread that owns the boundary's dword. One XOR per
//                           (row, window) into the row's CRC word.
//  wire_finish_kernel       behind them in stream order, one thread per row: the count word, the gzip head, the trailer, the length.
//
// No byte of the caller's buffer is loaded, and none at or behind a row's length is written. A translation unit of its own: the other code
// objects compile to what they compiled to before.
#include "ops_common.hpp"
#include "kernels.hpp"
#include "export_source.hpp"
#include "wire_encode.hpp"
#include "wire_plan.hpp"
#include "wire_rows.hpp"

namespace acvm {

static_assert(WIRE_ENTRY_BYTES == WIRE_PLAN_ENTRY_BYTES && WIRE_BLOCK_BYTES == WIRE_PLAN_BLOCK_BYTES && WIRE_WINDOW == WIRE_PLAN_WINDOW,
              "the kernel (wire_encode.hpp) and the plan (wire_plan.hpp) agree on the format and the window");
static_assert(WIRE_BINCODE == ACVM_WIRE_BINCODE && WIRE_GZIP_STORED == ACVM_WIRE_GZIP_STORED, "the containers of include/acvm_amd.h");

__global__ void __launch_bounds__(256) wire_lane_prefix_kernel(const uint32_t *assigned_bits, uint32_t n_slow, uint32_t n_words, const uint32_t *list_mask, uint32_t *lane_prefix) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_slow) return;
    uint32_t acc = 0u;
    for (uint32_t word = 0; word < n_words; word++) {
        lane_prefix[(uint64_t)word * n_slow + t] = acc;
        acc += __builtin_popcount(assigned_bits[(uint64_t)word * n_slow + t] & list_mask[word]);
    }
    lane_prefix[(uint64_t)n_words * n_slow + t] = acc;
}

// blockIdx.x: the 64 output rows, blockIdx.y (+ w0): the window
__global__ void __launch_bounds__(256) wire_entries_kernel(const WireExport a, uint32_t w0) {
    __shared__ uint32_t image[WIRE_ROWS * WIRE_LDS_PITCH];
    __shared__ uint32_t crc_sliced[WIRE_CRC_SLICED_WORDS];
    __shared__ uint32_t row_j[WIRE_ROWS], row_base[WIRE_ROWS], row_count[WIRE_ROWS], row_entries[WIRE_ROWS], row_crc[WIRE_ROWS];
    __shared__ int32_t row_lane[WIRE_ROWS];
    const uint32_t t = threadIdx.x;
    const bool gzip = a.container == WIRE_GZIP_STORED;
    const uint64_t i0 = (uint64_t)blockIdx.x * WIRE_ROWS;
    const uint32_t nb = a.n - i0 < WIRE_ROWS ? (uint32_t)(a.n - i0) : WIRE_ROWS;  // (the grid has no block at or behind n)
    const uint32_t k0 = (w0 + blockIdx.y) * WIRE_WINDOW, k1 = a.n_positions - k0 < WIRE_WINDOW ? a.n_positions : k0 + WIRE_WINDOW;  // (k0 < n_positions)
    // ---- phase 0: the CRC table, and per row its instance, where its run of this window starts and how long it is
    if (gzip)
        for (uint32_t x = t; x < WIRE_CRC_SLICED_WORDS; x += 256u) crc_sliced[x] = wire_crc_sliced_entry(x);
    if (t < WIRE_ROWS) {
        WireRow r{0xFFFFFFFFu, -1};
        uint32_t base = 0u, count = 0u, entries = 0u;
        if (t < nb) {
            r = wire_row(a, i0 + t);
            entries = wire_row_entries(a, r);
            if (r.j < a.src.B) {
                base = r.lane < 0 ? a.rank[k0] : wire_lane_rank(a, (uint32_t)r.lane, k0);
                count = (r.lane < 0 ? a.rank[k1] : wire_lane_rank(a, (uint32_t)r.lane, k1)) - base;
            }
        }
        row_j[t] = r.j;
        row_lane[t] = r.lane;
        row_base[t] = base;
        row_count[t] = count;
        row_entries[t] = entries;
        row_crc[t] = 0u;
    }
    __syncthreads();
    // ---- phase 1: one wave per list position, lane = row. w is wave-uniform: the table lookups are scalar loads.
    {
        const uint32_t wave = t >> 6, i = t & 63u;
        const uint32_t j = row_j[i], base = row_base[i], entries = row_entries[i];
        const int32_t lane = row_lane[i];
        const ExportListSource &L = a.src;
        uint32_t *img = image + i * WIRE_LDS_PITCH;
        uint32_t crc = 0u;
        for (uint32_t k = k0 + wave; k < k1; k += 4u) {
            const uint32_t w = a.sel ? a.sel[k] : k;
            if (j >= L.B) continue;
            uint32_t rank;
            Fr row, factor;
            if (lane < 0) {  // as kernels.hip export_generic_element
                uint32_t at, ui;
                export_generic_source(w, a.n_witnesses, a.row_of, a.producer, a.u_index, at, ui);
                if (at == 0xFFFFFFFFu) continue;
                rank = a.rank[k];
                row = fr_load_nt(a.W, at, a.Bp, j);
                factor = ui != 0xFFFFFFFFu ? fr_const(a.u_plain, ui) : export_plain_factor(EXPORT_ENC_BE32);
            } else {  // as export_list_element: its column of the side table or its own column, nothing scaled
                if (!export_lane_assigned(L.assigned_bits, L.n_slow, (uint32_t)lane, w, a.n_witnesses)) continue;
                rank = wire_lane_rank(a, (uint32_t)lane, k);
                row = fr_load(L.Wx, w, L.Bpx, L.side ? (uint64_t)(uint32_t)lane : (uint64_t)j);
                factor = export_plain_factor(EXPORT_ENC_BE32);
            }
            uint32_t entry[WIRE_ENTRY_WORDS];
            wire_entry(w, export_encode(row, factor, EXPORT_ENC_BE32, true), entry);
            uint32_t *at = img + (rank - base) * WIRE_ENTRY_WORDS;  // (rank - base < row_count <= WIRE_WINDOW)
#pragma unroll
            for (uint32_t x = 0; x < WIRE_ENTRY_WORDS; x++) at[x] = entry[x];
            if (gzip) crc ^= wire_crc_mul(a.crc_pow[entries - 1u - rank], wire_crc_raw_sliced(entry, WIRE_ENTRY_WORDS, crc_sliced));
        }
        if (crc) atomicXor(&row_crc[i], crc);
    }
    __syncthreads();
    // ---- phase 2: row i's run is 19 * count dwords from body dword 2 + 19 * base, consecutive lanes on consecutive dwords of one row
    for (uint32_t g = t; g < WIRE_ROWS * WIRE_IMAGE_WORDS; g += 256u) {
        const uint32_t i = g / WIRE_IMAGE_WORDS, x = g % WIRE_IMAGE_WORDS;
        if (i >= nb || x >= row_count[i] * WIRE_ENTRY_WORDS) continue;
        const uint64_t q = 2u + (uint64_t)row_base[i] * WIRE_ENTRY_WORDS + x;  // the body dword
        uint8_t *slot = a.out + (i0 + i) * a.pitch;
        uint64_t at = 4u * q;
        if (gzip) {
            const uint64_t block = (q >> 32) ? q / WIRE_BLOCK_WORDS : (uint64_t)((uint32_t)q / WIRE_BLOCK_WORDS);  // (32-bit below 16 GiB of body)
            at += WIRE_HEAD_BYTES + WIRE_JOINT_BYTES * block;
            if (q == block * WIRE_BLOCK_WORDS) {  // the first dword of a stored block (never block 0: q >= 2): its joint is this thread's
                uint32_t joint[5];
                wire_joint(wire_body_bytes(row_entries[i]), block, joint);
#pragma unroll
                for (uint32_t y = 0; y < 5u; y++) __builtin_nontemporal_store(joint[y], (uint32_t *)(slot + at - WIRE_JOINT_BYTES) + y);
            }
        }
        __builtin_nontemporal_store(image[i * WIRE_LDS_PITCH + x], (uint32_t *)(slot + at));
    }
    if (gzip && t < nb && row_crc[t]) atomicXor(&a.crc[i0 + t], row_crc[t]);
}

__global__ void __launch_bounds__(256) wire_finish_kernel(const WireExport a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t entries = wire_row_entries(a, wire_row(a, i));
    const uint64_t L = wire_body_bytes(entries);
    uint32_t *slot = (uint32_t *)(a.out + i * a.pitch);
    uint32_t *body = slot;
    if (a.container == WIRE_GZIP_STORED) {
        uint32_t head[4];
        wire_head(L, head);
#pragma unroll
        for (uint32_t y = 0; y < 4u; y++) slot[y] = head[y];
        body = slot + WIRE_HEAD_BYTES / 4u;
        // raw(u64le N) from the arithmetic alone: eight table-free byte steps are 64 shift steps
        uint32_t raw_count = entries;
        for (int k = 0; k < 64; k++) raw_count = (raw_count >> 1) ^ (WIRE_CRC_POLY & (0u - (raw_count & 1u)));
        uint32_t *trailer = slot + (wire_length(WIRE_GZIP_STORED, entries) - WIRE_TRAILER_BYTES) / 4u;
        trailer[0] = wire_crc_combine(a.crc_pow[entries], a.crc_x64, raw_count, a.crc[i]);
        trailer[1] = (uint32_t)L;
    }
    body[0] = entries;
    body[1] = 0u;
    if (a.lengths) a.lengths[i] = wire_length(a.container, entries);
}

void launch_wire_lane_prefix(hipStream_t s, const uint32_t *assigned_bits, uint32_t n_slow, uint32_t n_words, const uint32_t *list_mask, uint32_t *lane_prefix) {
    if (!n_slow) return;
    hipLaunchKernelGGL(wire_lane_prefix_kernel, dim3((n_slow + 255u) / 256u), dim3(256), 0, s, assigned_bits, n_slow, n_words, list_mask, lane_prefix);
}

void launch_wire_export(hipStream_t s, const WireExport &x, uint32_t n_windows) {
    if (!x.n) return;
    if (x.container == ACVM_WIRE_GZIP_DEFLATE) return launch_wire_deflate(s, x, n_windows);  // (kernels_wire_deflate.hip)
    for_grid_y_chunks(n_windows, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(wire_entries_kernel, dim3((x.n + WIRE_ROWS - 1u) / WIRE_ROWS, m), dim3(256), 0, s, x, done);
    });
    hipLaunchKernelGGL(wire_finish_kernel, dim3((x.n + 255u) / 256u), dim3(256), 0, s, x);
}

}  // namespace acvm
