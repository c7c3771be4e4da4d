// kernels_import_mask.hip -- the masked device import (include/acvm_amd.h acvm_batch_import_device_masked): ACVM::new takes a WitnessMap in which
// absence means unassigned (pwg/mod.rs:146-156), and an instance of the batch may lack some of the handle's initial ids.
//
//  import_mask_wm_kernel / import_mask_im_kernel   the mask pass, behind the value import: mask bytes -> the handle's missing set (import_mask.hpp),
//                                                  the rows of absent elements zeroed, three small results
//  import_missing_flag_kernel                      the flag pass, behind the level schedule of a solve: every instance that lacks an input leaves
//                                                  the generic path at opcode 0
//  import_missing_clear_kernel                     the clear pass, behind init_assigned_kernel: the absent inputs leave the exact lanes' assigned set
//
// A translation unit of its own: kernels.hip and kernels_import.hip compile to the code objects they compiled to before these kernels existed, and
// a handle whose missing set is empty launches none of them.
#include "ops_common.hpp"
#include "kernels.hpp"
#include "import_mask.hpp"

namespace acvm {

struct ImportMaskArgs {
    const uint8_t *mask;      // one byte per element, any alignment
    uint64_t stride;          // in elements, as launched
    const uint32_t *columns;  // per input the column that holds it; null: input k is column k
    uint32_t B, n_in;
    uint4 *W;
    uint64_t Bp;
    const uint32_t *rows;     // per input its row of W
    const uint32_t *plane_of_input;
    uint32_t *plane;
    uint32_t *missing;        // [import_missing_words(n_in)][Bp]
    unsigned long long *result;  // IMPORT_MASK_RESULT_WORDS words
};

// what a lane gathers over its instance's inputs
struct MaskLane {
    uint32_t n_bad = 0, first_bad = 0;
    bool any_missing = false;
};
// One mask byte of input k. Anything but 1 leaves the element absent (a refused import leaves the handle without initial witnesses anyway).
__device__ __forceinline__ void mask_byte(MaskLane &l, uint32_t &bits, uint32_t k, uint32_t byte) {
    if (byte != 1u) bits |= import_missing_bit(k);
    if (byte > 1u) {
        if (!l.n_bad) l.first_bad = k;
        l.n_bad++;
    }
}
// a finished word of the lane's missing set: stored, and the rows of its absent inputs zeroed (the plane word of zero: a byte, low bits 0)
__device__ __forceinline__ void mask_word(const ImportMaskArgs &a, MaskLane &l, uint32_t word, uint64_t j, uint32_t bits) {
    a.missing[(uint64_t)word * a.Bp + j] = bits;
    l.any_missing = l.any_missing || bits != 0u;
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
// The three results, one atomic each per wave that has something to say (ops_common.hpp flag_instance: ballot, the lowest lane speaks). Every lane
// of the wave arrives here, live or not. Lanes hold ascending instances, so the lowest lane with a bad byte holds the wave's smallest key.
__device__ __forceinline__ void mask_results(const ImportMaskArgs &a, const MaskLane &l, uint64_t j) {
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint64_t bad = __builtin_amdgcn_ballot_w64(l.n_bad != 0u);
    if (bad) {  // (wave-uniform)
        uint32_t n = l.n_bad;
        for (int off = 32; off; off >>= 1) n += __shfl_down(n, off, 64);
        if (lane == 0) atomicAdd(a.result + IMPORT_MASK_BAD, (unsigned long long)n);
        if (lane == (uint32_t)__builtin_ctzll(bad)) atomicMax(a.result + IMPORT_MASK_BAD_KEY, (unsigned long long)import_mask_key(j, l.first_bad));
    }
    const uint64_t missing = __builtin_amdgcn_ballot_w64(l.any_missing);
    if (l.any_missing && lane == (uint32_t)__builtin_ctzll(missing)) atomicAdd(a.result + IMPORT_MASK_MISSING, (unsigned long long)__builtin_popcountll(missing));
}

// witness-major source: lane = instance, so a wave reads 64 consecutive bytes per input; the 32 loads of a word are independent of each other.
__global__ void __launch_bounds__(256) import_mask_wm_kernel(const ImportMaskArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    MaskLane l;
    if (j < a.B) {
        const uint32_t n_words = import_missing_words(a.n_in);
        for (uint32_t word = 0; word < n_words; word++) {
            const uint32_t k0 = word * 32u, n = min(32u, a.n_in - k0);
            uint32_t bytes[32];
#pragma unroll
            for (uint32_t q = 0; q < 32u; q++) {
                const uint32_t k = k0 + (q < n ? q : 0u);  // (a ragged last word reads its first input again: no branch around the load)
                const uint32_t c = a.columns ? a.columns[k] : k;
                bytes[q] = a.mask[import_mask_byte(IMPORT_MASK_WITNESS_MAJOR, a.stride, j, c)];
            }
            uint32_t bits = 0;
#pragma unroll
            for (uint32_t q = 0; q < 32u; q++)
                if (q < n) mask_byte(l, bits, k0 + q, bytes[q]);
            mask_word(a, l, word, j, bits);
        }
    }
    mask_results(a, l, j);
}

// instance-major source: lane = instance, which owns the mask row [i * stride, i * stride + n_in) and walks it once. Without a column list
// position k is byte k of the row: bytes up to the first 16-byte boundary, 16-byte units, bytes again (import_mask.hpp import_mask_pieces).
// Under a column list the bytes of a row are visited in the list's order, which no unit follows: one byte per input, from the lines the lane
// has to itself.
__global__ void __launch_bounds__(256) import_mask_im_kernel(const ImportMaskArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    MaskLane l;
    if (j < a.B) {
        const uint8_t *row = a.mask + import_mask_byte(IMPORT_MASK_INSTANCE_MAJOR, a.stride, j, 0);
        uint32_t bits = 0, k = 0;
        // (a word is finished when its last input has been seen: k counts the inputs seen so far)
        auto take = [&](uint32_t byte) {
            mask_byte(l, bits, k, byte);
            k++;
            if (!(k & 31u) || k == a.n_in) {
                mask_word(a, l, (k - 1u) >> 5, j, bits);
                bits = 0;
            }
        };
        if (a.columns) {
            for (uint32_t q = 0; q < a.n_in; q++) take(row[a.columns[q]]);
        } else {
            const ImportMaskPieces p = import_mask_pieces((uint64_t)(uintptr_t)row, a.n_in);
            for (uint32_t q = 0; q < p.head; q++) take(row[q]);
            const uint4 *units = (const uint4 *)(row + p.head);
            for (uint32_t u = 0; u < p.units; u++) {
                const uint4 x = units[u];
                const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (uint32_t q = 0; q < 16u; q++) take((w[q >> 2] >> (8u * (q & 3u))) & 0xffu);
            }
            const uint8_t *tail = row + p.head + 16u * (size_t)p.units;
            for (uint32_t q = 0; q < p.tail; q++) take(tail[q]);
        }
    }
    mask_results(a, l, j);
}

void launch_import_mask(hipStream_t s, const ImportMaskSource &x, uint4 *W, uint64_t Bp, uint32_t B, const uint32_t *rows, uint32_t n_in, const uint32_t *plane_of_input,
                        uint32_t *plane, uint32_t *missing, uint64_t *result) {
    if (!B || !n_in) return;
    const ImportMaskArgs a{x.mask, x.stride, x.columns, B, n_in, W, Bp, rows, plane_of_input, plane, missing, (unsigned long long *)result};
    if (x.layout == IMPORT_MASK_WITNESS_MAJOR) hipLaunchKernelGGL(import_mask_wm_kernel, dim3((B + 255u) / 256u), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(import_mask_im_kernel, dim3((B + 255u) / 256u), dim3(256), 0, s, a);
}

// ---- the flag pass: an instance that lacks an input is none of the generic plan's. Behind the last step of the level schedule on the main
// stream, so behind the reset of the event words whether the schedule's reset step ran or the import had left them ready; atomicMin makes the
// order against the level kernels' own flags irrelevant.
__global__ void __launch_bounds__(256) import_missing_flag_kernel(const uint32_t *__restrict__ missing, uint32_t n_words, uint64_t Bp, uint32_t B, uint32_t *__restrict__ event) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= B) return;
    uint32_t any = 0;
    for (uint32_t word = 0; word < n_words; word++) any |= missing[(uint64_t)word * Bp + j];
    if (any) flag_instance(event, j, 0u);
}
void launch_import_missing_flag(hipStream_t s, const uint32_t *missing, uint32_t n_in, uint64_t Bp, uint32_t B, uint32_t *event) {
    if (!B || !n_in) return;
    hipLaunchKernelGGL(import_missing_flag_kernel, dim3((B + 255u) / 256u), dim3(256), 0, s, missing, import_missing_words(n_in), Bp, B, event);
}

// ---- the clear pass: init_assigned_kernel marks every initial witness; exact lane t (instance slow_ids[t]) takes back the ones its instance
// lacks. The lane owns column t of the bitmap: no atomics.
__global__ void __launch_bounds__(256) import_missing_clear_kernel(const uint32_t *__restrict__ missing, uint32_t n_in, uint64_t Bp, const uint32_t *__restrict__ init_ids,
                                                                   const uint32_t *__restrict__ slow_ids, uint32_t n_slow, uint32_t *__restrict__ assigned) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_slow) return;
    const uint64_t j = slow_ids[t];
    const uint32_t n_words = import_missing_words(n_in);
    for (uint32_t word = 0; word < n_words; word++) {
        uint32_t bits = missing[(uint64_t)word * Bp + j];
        while (bits) {
            const uint32_t k = word * 32u + (uint32_t)__builtin_ctz(bits);
            bits &= bits - 1u;
            const uint32_t w = init_ids[k];  // (the mask pass sets bits of positions below n_in only)
            assigned[(uint64_t)(w >> 5) * n_slow + t] &= ~(1u << (w & 31u));
        }
    }
}
void launch_import_missing_clear(hipStream_t s, const uint32_t *missing, uint32_t n_in, uint64_t Bp, const uint32_t *init_ids, const uint32_t *slow_ids, uint32_t n_slow,
                                 uint32_t *assigned) {
    if (!n_slow || !n_in) return;
    hipLaunchKernelGGL(import_missing_clear_kernel, dim3((n_slow + 255u) / 256u), dim3(256), 0, s, missing, n_in, Bp, init_ids, slow_ids, n_slow, assigned);
}

}  // namespace acvm
