// fr_probe.hpp -- one routine of the BN254-Fr device library (fr_device.hpp, the helpers of ops_common.hpp) applied to one item of raw limbs:
// the per-item evaluation of the acvm_debug_fr probe (kernels.hip fr_probe_kernel runs it one lane per item; tools/fr_probe_host_test.hip
// runs the same switch through the host compiler). Nothing is converted on the way: storage-form values are 8 x u32, working-form values
// 9 x u32 exactly as the routine takes and returns them, so unreduced representatives go in and the raw result comes out. The expected
// values are Python integers (tests/fr_ref.py, which also lists the contract of every routine).
#pragma once
#include "fr_device.hpp"
#if defined(__HIP_DEVICE_COMPILE__)
#include "ops_common.hpp"  // fr_low_limb / fr_is_byte / fr_from_byte and their tables
#endif

namespace acvm {

// `what` of acvm_debug_fr. Items: S = storage form (8 words), W = working form (9 words), k = one word.
enum FrProbe : uint32_t {
    FRP_MUL = 0,           // S a, S b -> S fr_mul(a, b)
    FRP_MUL_PORTABLE = 1,  // S a, S b -> S fr_mul_portable(a, b)
    FRP_SQR = 2,           // S a -> S
    FRP_ADD = 3,           // S a, S b -> S
    FRP_SUB = 4,           // S a, S b -> S
    FRP_NEG = 5,           // S a -> S
    FRP_INV = 6,           // S a -> S
    FRP_INV_EEA = 7,       // S a -> S
    FRP_TO_CANONICAL = 8,  // S a -> S
    FRP_LOW_LIMB = 9,      // S a -> k low limb, k is_byte                      (device only: the byte tables are in constant memory)
    FRP_IS_BYTE = 10,      // S a -> k is_byte, k the byte (the key table's candidate when is_byte = 0)   (device only)
    FRP_FROM_BYTE = 11,    // k d -> S                                                                     (device only)
    FRP_FROM29 = 12,       // S a -> W
    FRP_PACK29 = 13,       // W a -> S
    FRP_MUL29 = 14,        // W a, W b -> W fr29_mul
    FRP_MUL29_B = 15,      // W a, W b -> W fr29_mul_b (the asm-block scan on the device)
    FRP_SQR29 = 16,        // W a -> W
    FRP_REDC_LOW = 17,     // W a -> k
    FRP_COND_SUB_P = 18,   // W a -> W
    FRP_CSUB = 19,         // W a, k klog2 (0..4) -> W
    FRP_LT2P = 20,         // W a -> W
    FRP_WEAK = 21,         // W a -> W
    FRP_CANON = 22,        // W a -> W
    FRP_NORM = 23,         // W a -> W
    FRP_SUBL = 24,         // W a, W b, k klog2 (1..4) -> W
    FRP_ADDL = 25,         // W a, W b -> W
    FRP_DBLL = 26,         // W a -> W
    FRP_IS_ZERO_MOD_P = 27,  // W a -> k
    FRP_DOT1 = 28,         // W a0, W b0 -> W fr29_dot<1>
    FRP_DOT2 = 29,         // W a0, W b0, W a1, W b1 -> W fr29_dot<2>
    FRP_DOT3 = 30,         // W a0, W b0, W a1, W b1, W a2, W b2 -> W fr29_dot<3>
    FRP_DOT_ADD1 = 31,     // W a0, W b0, W h -> W fr29_dot_add<1>
    FRP_DOT_ADD2 = 32,     // W a0, W b0, W a1, W b1, W h -> W fr29_dot_add<2>
    FRP_DOT_ADD_B1_V = 33,   // as 31: fr29_dot_add_b<1, 0>
    FRP_DOT_ADD_B2_VV = 34,  // as 32: fr29_dot_add_b<2, 0>
    FRP_DOT_ADD_B1_U = 35,   // W a0, W h -> W fr29_dot_add_b<1, 1>(a0 * u0 + h)
    FRP_DOT_ADD_B2_VU = 36,  // W a0, W b0, W a1, W h -> W fr29_dot_add_b<2, 2>(a0 * b0 + a1 * u0 + h)
    FRP_DOT_ADD_B2_UU = 37,  // W a0, W a1, W h -> W fr29_dot_add_b<2, 3>(a0 * u0 + a1 * u1 + h)
    FRP_COUNT = 38
};
// The wave-uniform factors u0, u1 of the "U" forms: ONE value per launch (a kernel argument on the device), never a per-lane value --
// the asm blocks take them through scalar-register operands (gate_eval.hpp gate_coef29).
struct FrProbeUniform {
    Fr29 u[2];
};

FR_HD inline uint32_t fr_probe_words_in(uint32_t what) {
    constexpr uint8_t W[FRP_COUNT] = {16, 16, 8, 16, 16, 8, 8, 8, 8, 8, 8, 1, 8, 9, 18, 18, 9, 9, 9, 10, 9, 9, 9, 9, 19, 18, 9, 9,
                                      18, 36, 54, 27, 45, 27, 45, 18, 36, 27};
    return what < FRP_COUNT ? W[what] : 0u;
}
FR_HD inline uint32_t fr_probe_words_out(uint32_t what) {
    constexpr uint8_t W[FRP_COUNT] = {8, 8, 8, 8, 8, 8, 8, 8, 8, 2, 2, 8, 9, 8, 9, 9, 9, 1, 9, 9, 9, 9, 9, 9, 9, 9, 9, 1,
                                      9, 9, 9, 9, 9, 9, 9, 9, 9, 9};
    return what < FRP_COUNT ? W[what] : 0u;
}
// can this pass run `what` (the host pass has no byte tables)
FR_HD inline bool fr_probe_supported(uint32_t what) {
#if defined(__HIP_DEVICE_COMPILE__)
    return what < FRP_COUNT;
#else
    return what < FRP_COUNT && what != FRP_LOW_LIMB && what != FRP_IS_BYTE && what != FRP_FROM_BYTE;
#endif
}

// in: fr_probe_words_in(what) words, out: fr_probe_words_out(what) words
FR_HD inline void fr_probe_item(uint32_t what, const uint32_t *in, const FrProbeUniform &un, uint32_t *out) {
    auto S = [&](uint32_t off) { Fr c; for (int k = 0; k < 8; k++) c.v[k] = in[off + k]; return c; };
    auto W = [&](uint32_t off) { Fr29 c; for (int k = 0; k < 9; k++) c.v[k] = in[off + k]; return c; };
    auto stS = [&](const Fr &c) { for (int k = 0; k < 8; k++) out[k] = c.v[k]; };
    auto stW = [&](const Fr29 &c) { for (int k = 0; k < 9; k++) out[k] = c.v[k]; };
    switch (what) {
    case FRP_MUL: stS(fr_mul(S(0), S(8))); break;
    case FRP_MUL_PORTABLE: stS(fr_mul_portable(S(0), S(8))); break;
    case FRP_SQR: stS(fr_sqr(S(0))); break;
    case FRP_ADD: stS(fr_add(S(0), S(8))); break;
    case FRP_SUB: stS(fr_sub(S(0), S(8))); break;
    case FRP_NEG: stS(fr_neg(S(0))); break;
    case FRP_INV: stS(fr_inv(S(0))); break;
    case FRP_INV_EEA: stS(fr_inv_eea(S(0))); break;
    case FRP_TO_CANONICAL: stS(fr_to_canonical(S(0))); break;
#if defined(__HIP_DEVICE_COMPILE__)
    case FRP_LOW_LIMB: {
        bool isb;
        out[0] = fr_low_limb(S(0), isb);
        out[1] = isb ? 1u : 0u;
        break;
    }
    case FRP_IS_BYTE: {
        uint32_t d;
        out[0] = fr_is_byte(S(0), d) ? 1u : 0u;
        out[1] = d;
        break;
    }
    case FRP_FROM_BYTE: stS(fr_from_byte(in[0])); break;
#endif
    case FRP_FROM29: stW(fr29_from(S(0))); break;
    case FRP_PACK29: stS(fr29_pack(W(0))); break;
    case FRP_MUL29: stW(fr29_mul(W(0), W(9))); break;
    case FRP_MUL29_B: stW(fr29_mul_b(W(0), W(9))); break;
    case FRP_SQR29: stW(fr29_sqr(W(0))); break;
    case FRP_REDC_LOW: out[0] = fr29_redc_low(W(0)); break;
    case FRP_COND_SUB_P: stW(fr29_cond_sub_p(W(0))); break;
    case FRP_CSUB: stW(fr29_csub(W(0), (int)(in[9] <= 4u ? in[9] : 4u))); break;
    case FRP_LT2P: stW(fr29_lt2p(W(0))); break;
    case FRP_WEAK: stW(fr29_weak(W(0))); break;
    case FRP_CANON: stW(fr29_canon(W(0))); break;
    case FRP_NORM: stW(fr29_norm(W(0))); break;
    case FRP_SUBL: stW(fr29_subl(W(0), W(9), (int)(in[18] >= 1u && in[18] <= 4u ? in[18] : 1u))); break;
    case FRP_ADDL: stW(fr29_addl(W(0), W(9))); break;
    case FRP_DBLL: stW(fr29_dbll(W(0))); break;
    case FRP_IS_ZERO_MOD_P: out[0] = fr29_is_zero_mod_p(W(0)) ? 1u : 0u; break;
    case FRP_DOT1: {
        const Fr29 a[1] = {W(0)}, b[1] = {W(9)};
        stW(fr29_dot<1>(a, b));
        break;
    }
    case FRP_DOT2: {
        const Fr29 a[2] = {W(0), W(18)}, b[2] = {W(9), W(27)};
        stW(fr29_dot<2>(a, b));
        break;
    }
    case FRP_DOT3: {
        const Fr29 a[3] = {W(0), W(18), W(36)}, b[3] = {W(9), W(27), W(45)};
        stW(fr29_dot<3>(a, b));
        break;
    }
    case FRP_DOT_ADD1: {
        const Fr29 a[1] = {W(0)}, b[1] = {W(9)};
        stW(fr29_dot_add<1>(a, b, W(18)));
        break;
    }
    case FRP_DOT_ADD2: {
        const Fr29 a[2] = {W(0), W(18)}, b[2] = {W(9), W(27)};
        stW(fr29_dot_add<2>(a, b, W(36)));
        break;
    }
    case FRP_DOT_ADD_B1_V: {
        const Fr29 a[1] = {W(0)}, b[1] = {W(9)};
        stW(fr29_dot_add_b<1, 0u>(a, b, W(18)));
        break;
    }
    case FRP_DOT_ADD_B2_VV: {
        const Fr29 a[2] = {W(0), W(18)}, b[2] = {W(9), W(27)};
        stW(fr29_dot_add_b<2, 0u>(a, b, W(36)));
        break;
    }
    case FRP_DOT_ADD_B1_U: {
        const Fr29 a[1] = {W(0)}, b[1] = {un.u[0]};
        stW(fr29_dot_add_b<1, 1u>(a, b, W(9)));
        break;
    }
    case FRP_DOT_ADD_B2_VU: {
        const Fr29 a[2] = {W(0), W(18)}, b[2] = {W(9), un.u[0]};
        stW(fr29_dot_add_b<2, 2u>(a, b, W(27)));
        break;
    }
    case FRP_DOT_ADD_B2_UU: {
        const Fr29 a[2] = {W(0), W(9)}, b[2] = {un.u[0], un.u[1]};
        stW(fr29_dot_add_b<2, 3u>(a, b, W(18)));
        break;
    }
    default: break;
    }
}

}  // namespace acvm
