// inverse_batch.hpp -- the body of the inversion kernels (kernels.hip inverse_batch_kernel, inverse_batch_kernel_shared<G>): the inversions of one
// lane's chunk of jobs by Montgomery's trick, written once, __host__ __device__ and templated on the policy for its memory accesses and its
// flagging, so that the code the kernels run is executed on the host against integers (tools/inverse_batch_host_test.hip,
// tools/inverse_share_host_test.hip, tests/test_inverse_batch_on_host.py, tests/test_inverse_share_on_host.py) -- the pattern of gate_eval.hpp.
// The tables stay parameters of the pieces (the policy is stateless: static members), so that the kernel's __restrict__ qualifiers reach the code.
//   P:  Fr load_den(W, row, Bp, j)        the denominator, first read (prefix pass)
//       Fr load_den_last(W, row, Bp, j)   the same row, second and last read (way back)
//       void park(Inv, slot, Bp, j, x) / Fr parked(Inv, slot, Bp, j)   a prefix product in the job's own inverse slot
//       void store_inverse(Inv, slot, Bp, j, x)
//       void flag(event, j, opcode)       the instance leaves the generic path at this opcode
// A job is three words of the stream: {denominator row, opcode, inverse slot}; jobs [first, first + n) are this lane's.
//
// Three pieces: inverse_batch_forward (prefix pass -> the chunk's total), the share step (inverse_share_total_inverse, inverse_share_own: ONE
// field inversion for the same lane of G waves, from their G totals), inverse_batch_backward (back-substitution from 1 / total). With G = 1 the
// share step is the plain field inversion and the three are inverse_batch_body, the one-wave kernel. With G > 1 wave w starts its way back from
// S_w = (1 / (T_0 ... T_{G-1})) * prod_{v != w} T_v, made canonical: the very value fr_inv gives for 1 / T_w, so every row either kernel writes is the same.
// Bounds: a total is a product whose last factor is canonical, below p + 1.01 p * p / 2^261 < 1.007 p (fr29_mul's contract, p / 2^261 < 0.006); a
// product of two values below 1.01 p is again below 1.007 p, so every chain of the share step stays there, far below the 2 p of fr29_cond_sub_p.
#pragma once
#include "fr_device.hpp"

namespace acvm {

// Prefix pass: prefix_i = den_0 ... den_i parked in job i's inverse slot; returns the total (the working form, not canonical). A zero denominator
// flags the instance and counts as 1.
template <class P>
FR_HD __forceinline__ Fr29 inverse_batch_forward(const uint4 *__restrict__ W, uint4 *__restrict__ Inv, uint64_t Bp, uint64_t j, const uint32_t *__restrict__ gate_stream,
                                                 const uint32_t *__restrict__ job_offset, uint32_t first, uint32_t n, uint32_t *__restrict__ event) {
    Fr29 prefix = fr29_from(fr_one());
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t *__restrict__ g = gate_stream + job_offset[first + i];
        Fr den = P::load_den(W, g[0], Bp, j);
        if (fr_is_zero(den)) {  // zero-coefficient drop (arithmetic.rs:217-221): this instance leaves the generic path at the gate
            P::flag(event, j, g[1]);
            den = fr_one();
        }
        prefix = fr29_mul(prefix, fr29_from(den));
        P::park(Inv, g[2], Bp, j, fr29_pack(prefix));
    }
    return prefix;
}

// Way back from inv = the CANONICAL 1 / (den_0 ... den_{n-1}): the parked prefixes are replaced by the inverses.
template <class P>
FR_HD __forceinline__ void inverse_batch_backward(const uint4 *__restrict__ W, uint4 *__restrict__ Inv, uint64_t Bp, uint64_t j, const uint32_t *__restrict__ gate_stream,
                                                  const uint32_t *__restrict__ job_offset, uint32_t first, uint32_t n, Fr29 inv) {
    for (uint32_t i = n; i-- > 0;) {
        const uint32_t *__restrict__ g = gate_stream + job_offset[first + i];
        Fr den = P::load_den_last(W, g[0], Bp, j);  // second and last read of the row by this launch
        if (fr_is_zero(den)) den = fr_one();
        // (the first job's "prefix before it" is 1: one product more per wave, and no second path for the compiler to merge with 126 register moves per job)
        const Fr prev = i > 0 ? P::parked(Inv, gate_stream[job_offset[first + i - 1] + 2], Bp, j) : fr_one();
        const Fr29 inv_i = fr29_mul(inv, fr29_from(prev));
        inv = fr29_mul(inv, fr29_from(den));
        P::store_inverse(Inv, g[2], Bp, j, fr29_pack(inv_i));  // read once, by a gate levels later
    }
}

// ---- the share step. `totals(v)` gives T_v, the total of wave v for this lane (v < G), as forward left it.
// 1 / (T_0 ... T_{G-1}), canonical: the one field inversion of the lane's G chunks
template <int G, class Totals>
FR_HD __forceinline__ Fr29 inverse_share_total_inverse(const Totals &totals) {
    Fr29 t = totals(0);
#pragma unroll 1
    for (uint32_t v = 1; v < (uint32_t)G; v++) t = fr29_mul(t, totals(v));
    return fr29_from(fr_inv(fr29_pack(fr29_cond_sub_p(t))));
}
// S_w = inv_all * prod_{v != w} T_v = 1 / T_w, canonical (inv_all: inverse_share_total_inverse of the same totals)
template <int G, class Totals>
FR_HD __forceinline__ Fr29 inverse_share_own(const Totals &totals, const Fr29 &inv_all, uint32_t w) {
    if constexpr (G == 1) {
        return inv_all;
    } else {
        Fr29 s = inv_all;
#pragma unroll 1
        for (uint32_t v = 0; v < (uint32_t)G; v++)
            if (v != w) s = fr29_mul(s, totals(v));
        return fr29_cond_sub_p(s);
    }
}
// The workgroup's table of totals: rows of 9 words x 64 lanes, word-major (word i of the 64 lanes side by side: 32-bit accesses without bank
// conflicts). Rows [0, G) = the waves' totals, row G = inv_all. (G + 1) * INVERSE_SHARE_ROW_WORDS words.
constexpr uint32_t INVERSE_SHARE_ROW_WORDS = 9 * 64;
FR_HD __forceinline__ void inverse_share_row_store(uint32_t *rows, uint32_t row, uint32_t lane, const Fr29 &a) {
#pragma unroll
    for (int i = 0; i < 9; i++) rows[row * INVERSE_SHARE_ROW_WORDS + i * 64 + lane] = a.v[i];
}
FR_HD __forceinline__ Fr29 inverse_share_row_load(const uint32_t *rows, uint32_t row, uint32_t lane) {
    Fr29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = rows[row * INVERSE_SHARE_ROW_WORDS + i * 64 + lane];
    return r;
}
struct InverseShareRows {  // Totals over such a table, for one lane
    const uint32_t *rows;
    uint32_t lane;
    FR_HD __forceinline__ Fr29 operator()(uint32_t v) const { return inverse_share_row_load(rows, v, lane); }
};

// One lane, one chunk, one wave to an inversion (G = 1): the body of inverse_batch_kernel.
template <class P>
FR_HD __forceinline__ void inverse_batch_body(const uint4 *__restrict__ W, uint4 *__restrict__ Inv, uint64_t Bp, uint64_t j, const uint32_t *__restrict__ gate_stream,
                                              const uint32_t *__restrict__ job_offset, uint32_t first, uint32_t n, uint32_t *__restrict__ event) {
    const Fr29 total = inverse_batch_forward<P>(W, Inv, Bp, j, gate_stream, job_offset, first, n, event);
    const auto totals = [&](uint32_t) { return total; };
    const Fr29 inv = inverse_share_total_inverse<1>(totals);  // 1 / (den_0 ... den_{n-1})
    inverse_batch_backward<P>(W, Inv, Bp, j, gate_stream, job_offset, first, n, inverse_share_own<1>(totals, inv, 0));
}

}  // namespace acvm
