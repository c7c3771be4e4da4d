// kernels_wire_in.hip -- the batch-wide WitnessMap wire format read as initial witnesses (include/acvm_amd.h acvm_batch_import_device_wire):
// every instance's possibly partial map from the reference's own bytes -- the bincode body, alone or inside a stored-block gzip member
// (wire_encode.hpp, wire_decode.hpp) -- in a slot at a pitch. The bytes are untrusted: a row's count word is judged before any of its entries
// is read, every load lies in front of min(derived length, pitch) of its slot, and what a row claims never sizes a grid or an index.
//
//  wire_in_clear_kernel    one thread per instance: its missing-set words to all ones (masked to n_initial), its CRC word to zero
//  wire_in_entries_kernel  a block of 256 threads owns 64 consecutive instances and one window of WIRE_WINDOW entry ranks; a row's entries of a
//                          window are contiguous in its body. Phase 0: the rows' counts, judged, the key in front of the window, and the sorted id
//                          table into LDS where it fits. Phase 1: each row's run as consecutive aligned dwords on consecutive lanes into the
//                          row's LDS image (odd pitch), several loads in flight per lane. Phase 2: one wave per entry, lane = row -- the
//                          checks, the key looked up by binary search in the sorted id table, the value
//                          decoded (wire_decode.hpp, import_decode.hpp) and stored as the two halves of its row, the plane word, its bit of the
//                          missing set cleared, its raw CRC times its power of x XORed into the row's word.
//  wire_in_finish_kernel   behind them in stream order, one thread per instance: the count finding, the framing words and the CRC of a gzip
//                          row, the event word, the zero row and plane word 0x80000000 of every input whose missing bit is still set, and the
//                          count of instances that lack an input.
//
// A finding is counted and its key kept with atomicMax (wire_decode.hpp wire_in_key); a row with a count finding reads no entries. A
// translation unit of its own: the other code objects compile to what they compiled to before.
#include "ops_common.hpp"
#include "kernels.hpp"
#include "import_mask.hpp"
#include "wire_decode.hpp"
#include "wire_in_plan.hpp"

namespace acvm {

static_assert(WIRE_ENTRY_BYTES == WIRE_PLAN_ENTRY_BYTES && WIRE_BLOCK_BYTES == WIRE_PLAN_BLOCK_BYTES && WIRE_WINDOW == WIRE_PLAN_WINDOW,
              "the kernel (wire_encode.hpp) and the plan (wire_in_plan.hpp) agree on the format and the window");
static_assert(WIRE_BINCODE == ACVM_WIRE_BINCODE && WIRE_GZIP_STORED == ACVM_WIRE_GZIP_STORED, "the containers of include/acvm_amd.h");

// phase 1 keeps WIRE_IN_BATCH loads in flight per lane; a handle of up to WIRE_IN_TABLE initial witnesses has its key table in LDS
constexpr uint32_t WIRE_IN_BATCH = 8, WIRE_IN_TABLE = 512;

__device__ __forceinline__ uint32_t wire_in_load(const uint8_t *p) { return __builtin_nontemporal_load((const uint32_t *)p); }  // read once

// where body dword q of a row lies in its slot
__device__ __forceinline__ uint64_t wire_in_dword_offset(bool gzip, uint64_t q) {
    uint64_t at = 4u * q;
    if (gzip) at += WIRE_HEAD_BYTES + WIRE_JOINT_BYTES * ((q >> 32) ? q / WIRE_BLOCK_WORDS : (uint64_t)((uint32_t)q / WIRE_BLOCK_WORDS));
    return at;
}
// The entries of instance j's map, or WIRE_IN_NO_MAP: the count word is read only where the slot holds one, and judged here -- nothing else of
// a row is loaded before (wire_decode.hpp wire_in_count_ok: N <= n_in and the map's bytes <= pitch).
__device__ __forceinline__ uint32_t wire_in_row_entries(const WireImport &a, uint64_t j) {
    if (!wire_in_count_readable(a.container, a.pitch)) return WIRE_IN_NO_MAP;
    const uint8_t *count = a.in + j * a.pitch + wire_body_offset(a.container, 0);
    const uint32_t lo = wire_in_load(count), hi = wire_in_load(count + 4);
    const uint64_t length = a.lengths ? a.lengths[j] : 0u;
    return wire_in_count_ok(a.container, a.pitch, a.n_in, ((uint64_t)hi << 32) | lo, a.lengths != nullptr, length) ? lo : WIRE_IN_NO_MAP;
}
// what a thread found: counted, and the smallest key kept
struct WireFindings {
    uint32_t n = 0;
    uint64_t key = 0;  // the largest complemented key = the smallest (instance, class, rank)
    __device__ __forceinline__ void add(const WireImport &a, uint64_t j, uint32_t cls, uint32_t rank) {
        const uint64_t k = wire_in_key(j, cls, rank, a.rank_bits);
        key = k > key ? k : key;
        n++;
    }
    // (findings are the exception: a thread that has some speaks for itself)
    __device__ __forceinline__ void report(const WireImport &a) const {
        if (!n) return;
        atomicAdd((unsigned long long *)a.result + IMPORT_MASK_BAD, (unsigned long long)n);
        atomicMax((unsigned long long *)a.result + IMPORT_MASK_BAD_KEY, (unsigned long long)key);
    }
};

__global__ void __launch_bounds__(256) wire_in_clear_kernel(const WireImport a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= a.B) return;
    const uint32_t n_words = import_missing_words(a.n_in);
    for (uint32_t word = 0; word < n_words; word++)
        a.missing[(uint64_t)word * a.Bp + j] = a.n_in - word * 32u >= 32u ? 0xFFFFFFFFu : (1u << (a.n_in & 31u)) - 1u;
    if (a.container == WIRE_GZIP_STORED) a.crc[j] = 0u;
}

// blockIdx.x: the 64 instances, blockIdx.y (+ w0): the window of entry ranks
__global__ void __launch_bounds__(256) wire_in_entries_kernel(const WireImport a, uint32_t w0) {
    __shared__ uint32_t image[WIRE_ROWS * WIRE_LDS_PITCH];
    __shared__ uint32_t crc_sliced[WIRE_CRC_SLICED_WORDS];
    __shared__ uint32_t row_entries[WIRE_ROWS], row_previous[WIRE_ROWS], row_crc[WIRE_ROWS];
    __shared__ uint32_t table_keys[WIRE_IN_TABLE], table_positions[WIRE_IN_TABLE];
    const uint32_t t = threadIdx.x;
    const bool table = a.n_in <= WIRE_IN_TABLE;  // (a longer table stays in global memory: the lookup's steps are loads from the L2 then)
    const bool gzip = a.container == WIRE_GZIP_STORED;
    const uint64_t j0 = (uint64_t)blockIdx.x * WIRE_ROWS;
    const uint32_t nb = a.B - j0 < WIRE_ROWS ? (uint32_t)(a.B - j0) : WIRE_ROWS;  // (the grid has no block at or behind B)
    const uint32_t k0 = (w0 + blockIdx.y) * WIRE_WINDOW;                          // (k0 < n_in)
    // ---- phase 0: the CRC table; per row its count -- a row that is no map of its slot has no entries here -- and the key in front of the window
    if (gzip)
        for (uint32_t x = t; x < WIRE_CRC_SLICED_WORDS; x += 256u) crc_sliced[x] = wire_crc_sliced_entry(x);
    if (table)
        for (uint32_t x = t; x < a.n_in; x += 256u) {
            table_keys[x] = a.keys[x];
            table_positions[x] = a.positions[x];
        }
    if (t < WIRE_ROWS) {
        uint32_t entries = 0u, previous = 0u;
        if (t < nb) {
            entries = wire_in_row_entries(a, j0 + t);
            if (entries == WIRE_IN_NO_MAP) entries = 0u;
            if (k0 && k0 < entries) previous = wire_in_load(a.in + (j0 + t) * a.pitch + wire_in_dword_offset(gzip, 2u + (uint64_t)(k0 - 1u) * WIRE_ENTRY_WORDS));
        }
        row_entries[t] = entries;
        row_previous[t] = previous;
        row_crc[t] = 0u;
    }
    __syncthreads();
    // ---- phase 1: row i's run is 19 dwords per entry of [k0, min(k0 + WIRE_WINDOW, N)) from body dword 2 + 19 k0 -- all in front of the row's
    // derived length, which its count word's judgement put in front of the pitch
    // (WIRE_IN_BATCH loads are in flight per lane before the first of them is waited for: one load per trip is a trip per memory latency)
    for (uint32_t g0 = t; g0 < WIRE_ROWS * WIRE_IMAGE_WORDS; g0 += 256u * WIRE_IN_BATCH) {
        uint32_t value[WIRE_IN_BATCH], where[WIRE_IN_BATCH];
#pragma unroll
        for (uint32_t u = 0; u < WIRE_IN_BATCH; u++) {
            const uint32_t g = g0 + 256u * u, i = g / WIRE_IMAGE_WORDS, x = g % WIRE_IMAGE_WORDS;
            const uint32_t entries = g < WIRE_ROWS * WIRE_IMAGE_WORDS ? row_entries[i] : 0u;
            const uint32_t count = entries > k0 ? (entries - k0 < WIRE_WINDOW ? entries - k0 : WIRE_WINDOW) : 0u;
            where[u] = x < count * WIRE_ENTRY_WORDS ? i * WIRE_LDS_PITCH + x : 0xFFFFFFFFu;
            value[u] = 0u;
            if (where[u] != 0xFFFFFFFFu) value[u] = wire_in_load(a.in + (j0 + i) * a.pitch + wire_in_dword_offset(gzip, 2u + (uint64_t)k0 * WIRE_ENTRY_WORDS + x));
        }
#pragma unroll
        for (uint32_t u = 0; u < WIRE_IN_BATCH; u++)
            if (where[u] != 0xFFFFFFFFu) image[where[u]] = value[u];
    }
    __syncthreads();
    // ---- phase 2: one wave per entry, lane = row
    {
        const uint32_t wave = t >> 6, i = t & 63u;
        const uint64_t j = j0 + i;
        const uint32_t entries = row_entries[i];
        WireFindings found;
        uint32_t crc = 0u;
        for (uint32_t e = wave; e < WIRE_WINDOW; e += 4u) {
            const uint32_t r = k0 + e;
            if (r >= entries) continue;  // (lanes at or beyond N_j or B: entries is 0 there)
            const uint32_t *at = image + i * WIRE_LDS_PITCH + e * WIRE_ENTRY_WORDS;
            uint32_t entry[WIRE_ENTRY_WORDS];
#pragma unroll
            for (uint32_t x = 0; x < WIRE_ENTRY_WORDS; x++) entry[x] = at[x];
            if (gzip) crc ^= wire_crc_entry(entry, a.crc_pow[entries - 1u - r], crc_sliced);
            const uint32_t key = entry[0], previous = e ? at[-(int)WIRE_ENTRY_WORDS] : row_previous[i];
            uint4 lo, hi;
            const bool hex = wire_unhex(entry + 3, lo, hi);
            // (the global table is tried at the entry's own rank first: where a row names every initial witness that is its key's place)
            const uint32_t position = table               ? wire_in_position(table_keys, table_positions, a.n_in, key)
                                      : a.keys[r] == key ? a.positions[r]
                                                         : wire_in_position(a.keys, a.positions, a.n_in, key);
            const uint32_t cls = entry[1] != 64u || entry[2] != 0u ? WIRE_IN_LENGTH : !hex ? WIRE_IN_HEX : position == 0xFFFFFFFFu ? WIRE_IN_KEY : r && key <= previous ? WIRE_IN_ORDER : 0u;
            if (cls) {
                found.add(a, j, cls, r);
                continue;
            }
            // the element as import_element (kernels_import.hip) decodes a BE32 one: reduced, and when every lane still here holds a byte the
            // row from the closed form instead of the product -- the same row either way, the representation is unique
            const Fr x = import_reduce(import_limbs(lo, hi, EXPORT_ENC_BE32));
            const bool is_byte = import_is_byte(x);
            const Fr row = __builtin_amdgcn_ballot_w64(!is_byte) == 0 ? fr_mont_of_byte(x.v[0]) : fr_mul(x, import_r522());
            fr_store_nt(a.W, a.rows[position], a.Bp, j, row);
            if (a.plane_of_input) {
                const uint32_t pl = a.plane_of_input[position];
                if (pl != 0xFFFFFFFFu) a.plane[(uint64_t)pl * a.Bp + j] = import_plane_word(x);
            }
            // (keys ascend strictly in a row without findings: nobody else clears this bit, and other bits of the word are other blocks' too)
            atomicAnd(&a.missing[import_missing_word(position, a.Bp, j)], ~import_missing_bit(position));
        }
        found.report(a);
        if (crc) atomicXor(&row_crc[i], crc);
    }
    __syncthreads();
    if (gzip && t < nb && row_crc[t]) atomicXor(&a.crc[j0 + t], row_crc[t]);
}

__global__ void __launch_bounds__(256) wire_in_finish_kernel(const WireImport a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    bool any_missing = false;
    if (j < a.B) {
        WireFindings found;
        const uint32_t entries = wire_in_row_entries(a, j);
        if (entries == WIRE_IN_NO_MAP) found.add(a, j, WIRE_IN_COUNT, 0u);
        else if (a.container == WIRE_GZIP_STORED) {
            // (head, joints and trailer lie in front of wire_length(N) <= pitch)
            const uint8_t *slot = a.in + j * a.pitch;
            const uint64_t L = wire_body_bytes(entries);
            uint32_t want[5], differ = 0u;
            wire_head(L, want);
#pragma unroll
            for (uint32_t y = 0; y < 4u; y++) differ |= wire_in_load(slot + 4u * y) ^ want[y];
            for (uint64_t block = 1; block < wire_blocks(L); block++) {
                wire_joint(L, block, want);
#pragma unroll
                for (uint32_t y = 0; y < 5u; y++) differ |= wire_in_load(slot + wire_in_joint_offset(block) + 4u * y) ^ want[y];
            }
            const uint8_t *trailer = slot + wire_in_trailer_offset(entries);
            differ |= wire_in_load(trailer + 4) ^ wire_in_isize(entries);
            if (differ) found.add(a, j, WIRE_IN_FRAMING, 0u);
            else if (wire_in_load(trailer) != wire_in_crc(entries, a.crc_pow[entries], a.crc_x64, a.crc[j])) found.add(a, j, WIRE_IN_CRC, 0u);
        }
        found.report(a);
        // ACVM::new: nobody has left the generic path yet (kernels_import.hip import_event_reset)
        a.event_reset[j] = 0xFFFFFFFFu;
        if (j == 0) { a.event_reset[-4] = 0u; a.event_reset[-3] = 0u; }
        // what no entry supplied is absent: the zero row, the plane word of zero (kernels_import_mask.hip mask_word)
        const uint32_t n_words = import_missing_words(a.n_in);
        for (uint32_t word = 0; word < n_words; word++) {
            uint32_t bits = a.missing[(uint64_t)word * a.Bp + j];
            any_missing = any_missing || bits != 0u;
            while (bits) {
                const uint32_t k = word * 32u + (uint32_t)__builtin_ctz(bits);
                bits &= bits - 1u;
                fr_store(a.W, a.rows[k], a.Bp, j, fr_zero());
                if (a.plane_of_input) {
                    const uint32_t pl = a.plane_of_input[k];
                    if (pl != 0xFFFFFFFFu) a.plane[(uint64_t)pl * a.Bp + j] = 0x80000000u;
                }
            }
        }
    }
    // the instances with at least one absent input: one atomic per wave that has one (ballot, the lowest lane speaks)
    const uint64_t lacking = __builtin_amdgcn_ballot_w64(any_missing);
    if (lacking && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(lacking))
        atomicAdd((unsigned long long *)a.result + IMPORT_MASK_MISSING, (unsigned long long)__builtin_popcountll(lacking));
}

bool launch_wire_import(hipStream_t s, const WireImport &x, uint32_t n_windows) {
    if (!x.B) return false;
    const dim3 per_instance((x.B + 255u) / 256u);
    hipLaunchKernelGGL(wire_in_clear_kernel, per_instance, dim3(256), 0, s, x);
    for_grid_y_chunks(n_windows, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(wire_in_entries_kernel, dim3((x.B + WIRE_ROWS - 1u) / WIRE_ROWS, m), dim3(256), 0, s, x, done);
    });
    hipLaunchKernelGGL(wire_in_finish_kernel, per_instance, dim3(256), 0, s, x);
    return true;
}

}  // namespace acvm
