// export_encode.hpp -- the per-element encoding and the tile index maps of the device-resident witness export (kernels.hip
// export_device_*_kernel, include/acvm_amd.h acvm_batch_export_device). Everything here is __host__ __device__ so that the host can run
// what the kernels run (tools/export_device_host_test.hip, tests/test_export_device_on_host.py).
#pragma once
#include "fr_device.hpp"

namespace acvm {

// (the values of ACVM_ENC_* / ACVM_LAYOUT_* of include/acvm_amd.h)
enum : uint32_t { EXPORT_ENC_BE32 = 0, EXPORT_ENC_LE32 = 1, EXPORT_ENC_MONT256_LE = 2, EXPORT_N_ENC = 3 };
enum : uint32_t { EXPORT_INSTANCE_MAJOR = 0, EXPORT_WITNESS_MAJOR = 1, EXPORT_N_LAYOUT = 2 };

// instances and threads per block of the tiled kernel; EXPORT_TILE_T selected witnesses per block: 2 T consecutive 16-byte units (512 B at
// T = 16) of an instance's run leave the block together, for T x 2 x 65 x 16 B (32.5 KiB) of LDS
constexpr uint32_t EXPORT_TILE_I = 64, EXPORT_THREADS = 256, EXPORT_TILE_T = 16;

// the 32 bytes of one element as they lie in memory: lo = bytes [0, 16), hi = bytes [16, 32)
struct ExportElement {
    uint4 lo, hi;
};

// 2^256 mod p as a canonical integer (fr_host.hpp frh::R1)
FR_HD __forceinline__ Fr export_r256() {
    Fr r = {{0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}};
    return r;
}
// The factor of a row that is stored as is: a row holds x * 2^261 (times its scale, plan.cpp "projective witnesses"), the Montgomery product
// divides by 2^261, so the canonical integer 1 gives x and 2^256 mod p gives x * 2^256 mod p. A scaled row takes 1 / scale resp.
// 2^256 / scale from the plan's tables instead (Unscale::consts_plain, the Montgomery-256 table of batch_export.cpp).
FR_HD __forceinline__ Fr export_plain_factor(uint32_t encoding) {
    if (encoding == EXPORT_ENC_MONT256_LE) return export_r256();
    Fr one = fr_zero();
    one.v[0] = 1;
    return one;
}
// One element: row = any representative below 2^256 of the stored residue (relaxed rows included: the product reduces), factor as above.
// The byte order is made in registers; an unassigned element is 32 zero bytes in every encoding.
FR_HD __forceinline__ ExportElement export_encode(const Fr &row, const Fr &factor, uint32_t encoding, bool assigned) {
    ExportElement e;
    if (!assigned) {
        e.lo = make_uint4(0u, 0u, 0u, 0u);
        e.hi = e.lo;
        return e;
    }
    const Fr x = fr_mul(row, factor);
    if (encoding == EXPORT_ENC_BE32) {  // byte 0 is the most significant: limb 7 first, each limb byte-swapped
        e.lo = make_uint4(__builtin_bswap32(x.v[7]), __builtin_bswap32(x.v[6]), __builtin_bswap32(x.v[5]), __builtin_bswap32(x.v[4]));
        e.hi = make_uint4(__builtin_bswap32(x.v[3]), __builtin_bswap32(x.v[2]), __builtin_bswap32(x.v[1]), __builtin_bswap32(x.v[0]));
    } else {  // 4 x u64 little-endian limbs = 8 x u32 little-endian limbs = 32 bytes little-endian
        e.lo = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
        e.hi = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
    }
    return e;
}

// ---- where things go
// element (i, k) of the output -- i: instance of the range, k: position in the witness list -- in elements (32 bytes / one mask byte each)
FR_HD __forceinline__ uint64_t export_element_index(uint32_t layout, uint64_t stride, uint64_t i, uint64_t k) {
    return layout == EXPORT_WITNESS_MAJOR ? k * stride + i : i * stride + k;
}
// the dense stride of a layout; a caller's stride must not be below it
FR_HD __forceinline__ uint64_t export_dense_stride(uint32_t layout, uint32_t n, uint32_t n_sel) { return layout == EXPORT_WITNESS_MAJOR ? n : n_sel; }

// ---- the narrow encodings (ACVM_ENC_U8 .. ACVM_ENC_U128): an element is an unsigned little-endian integer of 1, 2, 4, 8 or 16 bytes.
// EXPORT_N_ENC keeps guarding the 32-byte range [0, 3); 3 .. 15 and 21 and up stay invalid.
enum : uint32_t { EXPORT_ENC_U8 = 16, EXPORT_ENC_U16 = 17, EXPORT_ENC_U32 = 18, EXPORT_ENC_U64 = 19, EXPORT_ENC_U128 = 20 };
enum : uint32_t { EXPORT_LAYOUT_BROADCAST = 16 };  // (ACVM_LAYOUT_BROADCAST: parts of acvm_batch_import_device_parts only)
FR_HD __forceinline__ bool export_enc_is_narrow(uint32_t encoding) { return encoding >= EXPORT_ENC_U8 && encoding <= EXPORT_ENC_U128; }
FR_HD __forceinline__ bool export_enc_is_valid(uint32_t encoding) { return encoding < EXPORT_N_ENC || export_enc_is_narrow(encoding); }
// bytes per element: 32, or the width of the integer
FR_HD __forceinline__ uint32_t export_element_size(uint32_t encoding) { return export_enc_is_narrow(encoding) ? 1u << (encoding - EXPORT_ENC_U8) : 32u; }
// where element (i, k) lies, in BYTES from the buffer's start: the index rule above times the element's size; a broadcast column holds one
// element for every instance
FR_HD __forceinline__ uint64_t export_element_offset(uint32_t layout, uint64_t stride, uint64_t i, uint64_t k, uint32_t size) {
    return (layout == EXPORT_LAYOUT_BROADCAST ? k : export_element_index(layout, stride, i, k)) * size;
}
// One narrow element: the low `size` bytes of the canonical value, little-endian, in the low bytes of `lo` (the rest zero) -- the truncation
// of FieldElement::to_u128 -- and the mask byte: 0 unassigned (zero bytes), 1 the value fits, 2 the value is 2^(8 size) or more.
struct ExportNarrow {
    uint4 lo;
    uint32_t mask;
};
FR_HD __forceinline__ ExportNarrow export_encode_narrow(const Fr &row, const Fr &factor, uint32_t size, bool assigned) {
    ExportNarrow e;
    e.lo = make_uint4(0u, 0u, 0u, 0u);
    e.mask = 0u;
    if (!assigned) return e;
    const Fr x = fr_mul(row, factor);
    uint32_t above = x.v[4] | x.v[5] | x.v[6] | x.v[7];
    e.lo = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    if (size < 16u) { above |= e.lo.z | e.lo.w; e.lo.z = 0u; e.lo.w = 0u; }
    if (size < 8u) { above |= e.lo.y; e.lo.y = 0u; }
    if (size < 4u) {
        const uint32_t keep = size == 1u ? 0xffu : 0xffffu;
        above |= e.lo.x & ~keep;
        e.lo.x &= keep;
    }
    e.mask = above ? 2u : 1u;
    return e;
}

// The tiled (instance-major) kernel: block (bx, by) owns instances [64 bx, 64 bx + 64) x list positions [T by, T by + T).
// Phase 1: wave v of the block's four computes positions v, v + 4, ... of the tile, lane = instance (coalesced row loads).
// Phase 2: the tile leaves as 64 runs of 2 T consecutive 16-byte units; in step s thread t moves unit g = 256 s + t of the tile, counted
// along the runs: consecutive lanes on consecutive units of one instance's run. T / 2 steps move all 128 T units.
constexpr uint32_t EXPORT_WAVES = EXPORT_THREADS / 64u;
FR_HD __forceinline__ uint32_t export_tile_lane(uint32_t t) { return t & 63u; }            // phase 1: the thread's instance inside the tile ...
FR_HD __forceinline__ uint32_t export_tile_first_position(uint32_t t) { return t >> 6; }  // ... and its first list position; the next is EXPORT_WAVES further
struct ExportTileUnit {
    uint32_t ji, kk, half;  // instance and list position inside the tile; which 16 bytes of the element
};
FR_HD __forceinline__ uint32_t export_tile_steps(uint32_t T) { return EXPORT_TILE_I * 2u * T / EXPORT_THREADS; }
FR_HD __forceinline__ ExportTileUnit export_tile_unit(uint32_t T, uint32_t t, uint32_t step) {
    const uint32_t g = step * EXPORT_THREADS + t;
    ExportTileUnit q;
    q.ji = g / (2u * T);
    q.kk = (g % (2u * T)) >> 1;
    q.half = g & 1u;
    return q;
}

}  // namespace acvm
