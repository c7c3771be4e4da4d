// import_mask.hpp -- where the mask bytes of a masked import lie and where the handle's missing set keeps what they said (include/acvm_amd.h
// acvm_batch_import_device_masked, kernels_import_mask.hip). Everything here is __host__ __device__ index arithmetic, so that the host can run
// what the kernels run (tools/import_mask_host_test.hip, tests/test_import_mask_on_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acvm {

// (the values of ACVM_LAYOUT_* of include/acvm_amd.h; export_encode.hpp EXPORT_INSTANCE_MAJOR / EXPORT_WITNESS_MAJOR)
enum : uint32_t { IMPORT_MASK_INSTANCE_MAJOR = 0, IMPORT_MASK_WITNESS_MAJOR = 1 };

// The byte of element (instance i, column c), from d_assigned: the index rule of the values (export_encode.hpp export_element_index) with one
// byte per element. stride in elements, as launched (never 0).
__host__ __device__ __forceinline__ uint64_t import_mask_byte(uint32_t layout, uint64_t stride, uint64_t i, uint64_t c) {
    return layout == IMPORT_MASK_WITNESS_MAJOR ? c * stride + i : i * stride + c;
}

// ---- the missing set: bit (k & 31) of word missing[(k >> 5) * Bp + j] is set when instance j does NOT hold the initial witness at position k
// of initial_ids. Witness-major like every table of the handle: lane = instance, a wave reads and writes 64 consecutive words.
__host__ __device__ __forceinline__ uint32_t import_missing_words(uint32_t n_in) { return (n_in + 31u) >> 5; }
__host__ __device__ __forceinline__ uint64_t import_missing_word(uint32_t k, uint64_t Bp, uint64_t j) { return (uint64_t)(k >> 5) * Bp + j; }
__host__ __device__ __forceinline__ uint32_t import_missing_bit(uint32_t k) { return 1u << (k & 31u); }

// ---- what a mask pass reports, three 64-bit words on the device (zeroed before the pass):
//   [0] the bytes other than 0 / 1
//   [1] ~(the smallest (instance << 32 | position) among them): kept with atomicMax so that zero means "none"
//   [2] the instances with at least one absent input
enum : uint32_t { IMPORT_MASK_BAD = 0, IMPORT_MASK_BAD_KEY = 1, IMPORT_MASK_MISSING = 2, IMPORT_MASK_RESULT_WORDS = 3 };
__host__ __device__ __forceinline__ uint64_t import_mask_key(uint64_t instance, uint32_t position) { return ~(instance << 32 | position); }
__host__ __device__ __forceinline__ uint32_t import_mask_key_instance(uint64_t word) { return (uint32_t)(~word >> 32); }
__host__ __device__ __forceinline__ uint32_t import_mask_key_position(uint64_t word) { return (uint32_t)~word; }

// ---- an instance-major mask row [p, p + n) is read in pieces: bytes up to the first 16-byte boundary, 16-byte units, bytes again
// (kernels_import_mask.hip import_mask_im_kernel). head: the bytes in front of the first unit; units: whole 16-byte units behind them.
struct ImportMaskPieces {
    uint32_t head, units, tail;
};
__host__ __device__ __forceinline__ ImportMaskPieces import_mask_pieces(uint64_t address, uint32_t n) {
    ImportMaskPieces p;
    const uint32_t to_boundary = (uint32_t)((16u - (address & 15u)) & 15u);
    p.head = to_boundary < n ? to_boundary : n;
    p.units = (n - p.head) >> 4;
    p.tail = n - p.head - 16u * p.units;
    return p;
}

}  // namespace acvm
