// inverse_batch.hpp -- the body of inverse_batch_kernel (kernels.hip): the inversions of one lane's chunk of jobs by Montgomery's trick, written
// once, __host__ __device__ and templated on the policy for its memory accesses and its flagging, so that the code the kernel runs is
// executed on the host against integers (tools/inverse_batch_host_test.hip, tests/test_inverse_batch_on_host.py) -- the pattern of gate_eval.hpp.
// The tables stay parameters of the body (the policy is stateless: static members), so that the kernel's __restrict__ qualifiers reach the code.
//   P:  Fr load_den(W, row, Bp, j)        the denominator, first read (prefix pass)
//       Fr load_den_last(W, row, Bp, j)   the same row, second and last read (way back)
//       void park(Inv, slot, Bp, j, x) / Fr parked(Inv, slot, Bp, j)   a prefix product in the job's own inverse slot
//       void store_inverse(Inv, slot, Bp, j, x)
//       void flag(event, j, opcode)       the instance leaves the generic path at this opcode
// A job is three words of the stream: {denominator row, opcode, inverse slot}; jobs [first, first + n) are this lane's.
#pragma once
#include "fr_device.hpp"

namespace acvm {

template <class P>
FR_HD __forceinline__ void inverse_batch_body(const uint4 *__restrict__ W, uint4 *__restrict__ Inv, uint64_t Bp, uint64_t j, const uint32_t *__restrict__ gate_stream,
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
    Fr29 inv = fr29_from(fr_inv(fr29_pack(fr29_cond_sub_p(prefix))));  // 1 / (den_0 ... den_{n-1})
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

}  // namespace acvm
