// lin_table.hpp -- the precomputed reduction of a coefficient x witness term (gate_record.hpp "linear tables"; evaluation: fr_device.hpp
// fr29_lin_add). For a coefficient c (a plain field element) the table holds the nine canonical constants
//     C_i = c * 2^(29 i + 58) mod p,   i = 0..8,
// nine 29-bit limbs each, column-major: word [9 k + i] = limb k of C_i, so that column k of S = sum_i x_i C_i reads nine consecutive words.
// Host only, shared by the planner that writes the tables (plan.cpp) and the checker that recomputes them (schedule_check.cpp).
#pragma once
#include "fr_host.hpp"
#include "gate_record.hpp"

namespace acvm {

// coef: the eight inline words of the record's term (the device's Montgomery form, c * 2^261 mod p)
inline void lin_table_of(const uint32_t *coef, uint32_t *out) {
    FrH d;
    for (int i = 0; i < 4; i++) d.l[i] = coef[2 * i] | (uint64_t)coef[2 * i + 1] << 32;
    FrH t = frh::mul(frh::from_device_form(d), frh::from_u64(1ull << 58));
    const FrH step = frh::from_u64(1ull << 29);
    for (int i = 0; i < 9; i++, t = frh::mul(t, step)) {
        uint64_t v[4];
        frh::to_canonical(t, v);
        for (int k = 0; k < 9; k++) {
            const int bit = 29 * k, w = bit >> 6, sh = bit & 63;
            uint64_t limb = v[w] >> sh;
            if (sh > 35 && w + 1 < 4) limb |= v[w + 1] << (64 - sh);
            out[9 * k + i] = (uint32_t)limb & 0x1fffffffu;
        }
    }
}

}  // namespace acvm
