// record_stage.hpp -- what the two record import kernels share on the device (kernels_records.hip import_records_kernel,
// kernels_records_masked.hip import_records_masked_kernel): the arguments, the staging of a block's window into LDS (phase 1), and one element
// from that image (phase 2). Device code only, every function __forceinline__: each kernel compiles it into itself, and the unmasked kernel's
// instructions are those it had when these lines stood in kernels_records.hip (NOTEBOOK.md "Masked record import": one scalar add takes its two
// sources in the other order).
#pragma once
#include "ops_common.hpp"
#include "kernels.hpp"
#include "record_decode.hpp"
#include "record_plan.hpp"

namespace acvm {

static_assert(RECORD_WINDOW_CAP == RECORD_PLAN_WINDOW_CAP, "the kernel (record_decode.hpp) and the window cut (record_plan.cpp) agree on the window size");

struct RecordImportArgs {
    uint4 *W;
    uint64_t Bp;
    uint32_t B;
    const uint8_t *in;        // any alignment
    uint64_t pitch;
    const uint32_t *windows;  // [n_windows][RECORD_WINDOW_WORDS] (the masked tables: RECORD_MWINDOW_WORDS)
    const uint32_t *fields;   // [n_fields][RECORD_FIELD_WORDS], window by window (the masked tables: RECORD_MFIELD_WORDS)
    const uint32_t *gate;
    uint32_t *plane, *event_reset;
};
// ACVM::new: nobody has left the generic path yet (kernels_import.hip import_event_reset)
__device__ __forceinline__ void record_event_reset(uint32_t *event_reset, uint64_t j) {
    event_reset[j] = 0xFFFFFFFFu;
    if (j == 0) { event_reset[-4] = 0u; event_reset[-3] = 0u; }
}

// One element from the block's image: the row and the plane word. encoding (and with it the size) is wave-uniform; every lane of the wave that
// is still active must arrive (the ballots): a wave of bytes -- message bytes, digits, flags -- takes the row from the closed form of
// ops_common.hpp fr_mont_of_byte instead of a product, and U8 always (kernels_typed_io.hip typed_narrow_row, kernels_import.hip import_element).
// MASKED (the masked kernel): a lane that is not `present` takes the element of zero bytes whatever its image holds -- the byte zero in every
// encoding: the zero row, the plane word 0x80000000, and no say in a ballot.
template <bool MASKED>
__device__ __forceinline__ Fr record_element(const uint32_t *image, uint32_t byte, uint32_t encoding, bool want_plane, bool present, uint32_t &plane_word) {
    const uint32_t size = export_element_size(encoding);
    uint4 lo, hi;
    record_assemble(image, byte, size, lo, hi);
    if (MASKED && !present) lo = hi = make_uint4(0u, 0u, 0u, 0u);
    if (size == 1u) {
        plane_word = lo.x | 0x80000000u;
        return fr_mont_of_byte(lo.x);
    }
    if (size != 32u) {
        const Fr x = import_narrow_limbs(lo);
        plane_word = import_plane_word(x);
        if (__builtin_amdgcn_ballot_w64(!import_is_byte(x)) == 0) return fr_mont_of_byte(lo.x);
        return fr_mul(x, import_r522());
    }
    const Fr m = import_limbs(lo, hi, encoding);
    const bool have_canonical = encoding != EXPORT_ENC_MONT256_LE || want_plane;
    Fr x = m;
    if (have_canonical) x = import_canonical(m, encoding);
    const bool is_byte = have_canonical && import_is_byte(x);
    plane_word = (x.v[0] & 0x1fffffffu) | (is_byte ? 0x80000000u : 0u);  // (meaningless without a canonical value: nobody stores it then)
    if (__builtin_amdgcn_ballot_w64(!is_byte) == 0) return fr_mont_of_byte(x.v[0]);
    return import_row(m, x, encoding);
}

// ---- phase 1 of a block of 256 threads (t = threadIdx.x): the window of win_length bytes of its nb records, the first of them at byte address
// S, into `image`. Record i takes the (phase_i + length + 3) / 4 aligned dwords that hold a byte of its window, consecutive lanes on consecutive
// dwords: a group of G lanes per record, G the power of two that holds the most dwords a record of this block takes (no division anywhere).
// Only dwords that hold a byte of a window of the block's records are loaded. For a pitch up to the window size the window is the record
// and the nb records are one contiguous span: neighbouring groups then meet in the dword at the joint, which both load. Four loads are in
// flight per lane before the first of them is stored: the phase is as long as one load's latency, not four. (Plain loads: the blocks of
// the other windows of these records read the same lines again.) The caller synchronises the block behind it.
__device__ __forceinline__ void record_stage(uint32_t *image, uint64_t S, uint64_t pitch, uint32_t win_length, uint32_t nb, uint32_t t) {
    // a pitch of whole dwords keeps the phase of the first record; any other takes every phase
    const uint32_t row_words = ((pitch & 3u) ? win_length + 6u : record_phase(S) + win_length + 3u) / 4u;  // 1 .. 65
    const uint32_t shift = row_words > 1u ? 32u - __builtin_clz(row_words - 1u) : 0u;                    // G = 1 << shift >= row_words, at most 128
    const uint32_t total = RECORD_BLOCK_INSTANCES << shift;
    for (uint32_t g0 = t; g0 < total; g0 += 1024u) {
        uint32_t v[4], at_lds[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint32_t g = g0 + 256u * u, i = g >> shift, k = g & ((1u << shift) - 1u);
            const uint64_t at = S + (uint64_t)i * pitch;
            const uint32_t phase = record_phase(at);
            const bool mine = g < total && i < nb && k < (phase + win_length + 3u) / 4u;
            at_lds[u] = mine ? i * RECORD_LDS_PITCH + k : 0xFFFFFFFFu;
            v[u] = mine ? *(const uint32_t *)(at - phase + 4u * (uint64_t)k) : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++)
            if (at_lds[u] != 0xFFFFFFFFu) image[at_lds[u]] = v[u];
    }
}

}  // namespace acvm
