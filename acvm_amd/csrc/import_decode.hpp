// import_decode.hpp -- the per-element decoding of the device-resident witness import (kernels_import.hip import_device_*_kernel, include/acvm_amd.h
// acvm_batch_import_device): the counterpart of export_encode.hpp, with the same encodings, layouts and stride rule. Everything here is
// __host__ __device__ so that the host can run what the kernels run (tools/import_device_host_test.hip, tests/test_import_device_on_host.py).
#pragma once
#include "export_encode.hpp"

namespace acvm {

// 2^266 mod p and 2^5 as canonical integers: the two factors of a Montgomery-256 element m = x * 2^256 (any representative below 2^256).
// The Montgomery product divides by 2^261, so m * 2^266 gives m * 2^5 = x * 2^261, the row, and m * 2^5 gives m * 2^-256 = x, the value.
FR_HD __forceinline__ Fr import_r266() {
    Fr r = {{0x8fffead7u, 0x97aa889eu, 0x4b110e2au, 0x4da1da68u, 0xa60934c8u, 0xe56cdd25u, 0xdce9ed32u, 0x05800320u}};
    return r;
}
FR_HD __forceinline__ Fr import_r522() {  // R^2 = 2^522 mod p (ops_common.hpp fr_r2, which is device-only)
    Fr r = {{0x45b69bd4u, 0x38c2e14bu, 0x85883377u, 0x0ffedb18u, 0xabc6e54du, 0x7840f9f0u, 0x848b0f05u, 0x0a054a3eu}};
    return r;
}
FR_HD __forceinline__ Fr import_two5() {
    Fr r = fr_zero();
    r.v[0] = 32u;
    return r;
}

// the 256-bit integer the 32 bytes spell, as little-endian limbs: lo = bytes [0, 16), hi = bytes [16, 32) as they lie in memory
FR_HD __forceinline__ Fr import_limbs(const uint4 &lo, const uint4 &hi, uint32_t encoding) {
    Fr x;
    if (encoding == EXPORT_ENC_BE32) {  // byte 0 is the most significant: limb 7 first, each limb byte-swapped
        x.v[7] = __builtin_bswap32(lo.x); x.v[6] = __builtin_bswap32(lo.y); x.v[5] = __builtin_bswap32(lo.z); x.v[4] = __builtin_bswap32(lo.w);
        x.v[3] = __builtin_bswap32(hi.x); x.v[2] = __builtin_bswap32(hi.y); x.v[1] = __builtin_bswap32(hi.z); x.v[0] = __builtin_bswap32(hi.w);
    } else {  // 4 x u64 little-endian limbs = 8 x u32 little-endian limbs
        x.v[0] = lo.x; x.v[1] = lo.y; x.v[2] = lo.z; x.v[3] = lo.w;
        x.v[4] = hi.x; x.v[5] = hi.y; x.v[6] = hi.z; x.v[7] = hi.w;
    }
    return x;
}
// from_be_bytes_reduce: x mod p for any x < 2^256 (2^256 / p < 6), by the quotient estimate of import_witness_kernel: q = how many multiples of
// p7 + 1 fit into x7 (p7 = p's top limb), floor(x / p) is q or q + 1, so x - q p and ONE conditional subtraction
FR_HD __forceinline__ Fr import_reduce(Fr x) {
    const uint32_t p7 = fr_p(7) + 1u;
    const uint32_t q = (x.v[7] >= p7) + (x.v[7] >= 2u * p7) + (x.v[7] >= 3u * p7) + (x.v[7] >= 4u * p7) + (x.v[7] >= 5u * p7);
    int64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int64_t tt = (int64_t)x.v[i] - (int64_t)((uint64_t)q * fr_p(i)) + carry;  // q p_i < 2^35
        x.v[i] = (uint32_t)tt;
        carry = tt >> 32;
    }
    return fr_cond_sub_p(x);
}
// The operand contract of fr_mul for the Montgomery-256 element: fr29_from takes any 256-bit integer (top working limb < 2^24), fr29_mul any two
// values below 8p (2^256 < 5.3p) and returns less than p + a b / 2^261. With a < 2^256 and the canonical constant b < p that is below p + p / 32,
// and with b = 2^5 below p + 1: fr_mul's conditional subtraction leaves both the row and the value in [0, p), whatever representative m is
// (m >= p included: the product reduces it).
FR_HD __forceinline__ Fr import_mont256_row(const Fr &m) { return fr_mul(m, import_r266()); }
FR_HD __forceinline__ Fr import_mont256_canonical(const Fr &m) { return fr_mul(m, import_two5()); }

FR_HD __forceinline__ bool import_is_byte(const Fr &canonical) {
    return !(canonical.v[1] | canonical.v[2] | canonical.v[3] | canonical.v[4] | canonical.v[5] | canonical.v[6] | canonical.v[7]) && canonical.v[0] < 256u;
}
// byte planes (plan.hpp): low 29 bits of the canonical value | is-byte << 31
FR_HD __forceinline__ uint32_t import_plane_word(const Fr &canonical) {
    return (canonical.v[0] & 0x1fffffffu) | (import_is_byte(canonical) ? 0x80000000u : 0u);
}
// the canonical value of an element; m: the limbs as read (import_limbs)
FR_HD __forceinline__ Fr import_canonical(const Fr &m, uint32_t encoding) {
    return encoding == EXPORT_ENC_MONT256_LE ? import_mont256_canonical(m) : import_reduce(m);
}
// the row x * 2^261 mod p, fully reduced. A Montgomery-256 element takes ONE product from the limbs as read; the canonical encodings take the
// product of the canonical value with R^2.
FR_HD __forceinline__ Fr import_row(const Fr &m, const Fr &canonical, uint32_t encoding) {
    return encoding == EXPORT_ENC_MONT256_LE ? import_mont256_row(m) : fr_mul(canonical, import_r522());
}

// One element, everything: what the kernels compute piece by piece (they skip the canonical value of a Montgomery-256 input without a byte plane,
// and a wave whose 64 values are all bytes takes the row from fr_mont_of_byte instead of the product: the same row, the representation is unique)
struct ImportDecoded {
    Fr canonical, row;
    uint32_t plane;
};
FR_HD __forceinline__ ImportDecoded import_decode(const uint4 &lo, const uint4 &hi, uint32_t encoding) {
    ImportDecoded d;
    const Fr m = import_limbs(lo, hi, encoding);
    d.canonical = import_canonical(m, encoding);
    d.row = import_row(m, d.canonical, encoding);
    d.plane = import_plane_word(d.canonical);
    return d;
}

// ---- the narrow encodings (export_encode.hpp EXPORT_ENC_U8 ..): the value IS the integer, below 2^128 < p, so nothing is reduced.
// lo: the element's bytes, zero-extended to 16
FR_HD __forceinline__ Fr import_narrow_limbs(const uint4 &lo) {
    Fr x = fr_zero();
    x.v[0] = lo.x; x.v[1] = lo.y; x.v[2] = lo.z; x.v[3] = lo.w;
    return x;
}
// the element's `size` bytes at p (aligned to size), zero-extended: one load of the natural width
FR_HD __forceinline__ uint4 import_narrow_read(const void *p, uint32_t size) {
    uint4 lo = make_uint4(0u, 0u, 0u, 0u);
    switch (size) {
        case 1: lo.x = *(const uint8_t *)p; break;
        case 2: lo.x = *(const uint16_t *)p; break;
        case 4: lo.x = *(const uint32_t *)p; break;
        case 8: { const uint2 v = *(const uint2 *)p; lo.x = v.x; lo.y = v.y; break; }
        default: lo = *(const uint4 *)p; break;
    }
    return lo;
}
// One narrow element, everything (the kernels take a wave of bytes from fr_mont_of_byte instead of the product, and U8 always: the same row)
FR_HD __forceinline__ ImportDecoded import_decode_narrow(const uint4 &lo) {
    ImportDecoded d;
    d.canonical = import_narrow_limbs(lo);
    d.row = fr_mul(d.canonical, import_r522());
    d.plane = import_plane_word(d.canonical);
    return d;
}

}  // namespace acvm
