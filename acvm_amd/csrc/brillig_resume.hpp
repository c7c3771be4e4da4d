// brillig_resume.hpp -- what a Brillig lane of the exact path needs to CONTINUE after a device limit instead of starting over
// (tuning.hpp brillig_resume): the checkpoint record of a lane, and the address arithmetic of the compact VM scratch of a retry pass
// (batch_exact.cpp retry_device_limits). The VM's state already lies in device memory: registers and memory cells are
// [slot][half][lane] rows of the compact scratch, the call stack is words behind them, the rest is five scalars -- the record. Between
// two passes the scratch may change its stride, a lane's column, the memory capacity and the call depth; the word region starts behind
// the slots, so it moves with the capacity. One set of index functions serves BrVm's set-up (ops_brillig.hpp), the relocation kernel
// (kernels_brillig_resume.hip) and the host test (tools/brillig_resume_host_test.hip). Host-runnable: no HIP call, no device-only code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BR_HD __host__ __device__
#else
#define BR_HD
#endif

namespace acvm {

// ---- the checkpoint record of exact lane t: words [t * 8, t * 8 + 8) of a buffer of its own (ExactLanes::br_ckpt), independent of the
// scratch layout. Written by op_brillig on every exit of the VM loop of a compact pass under brillig_resume; whether it is VALID for the
// next pass is decided by the host from the pass's results (brillig_retry_plan.cpp), never by the kernel from what it finds here.
constexpr uint32_t BR_CKPT_WORDS = 8;
constexpr uint32_t BR_CKPT_NONE = 0;   // state: the lane entered the opcode and has not left the VM loop (or stopped while loading inputs)
constexpr uint32_t BR_CKPT_LIMIT = 5;  // state: the VM's status at the exit of the loop (1 finished, 2 failure, 3 waiting, 4 panic, 5 device limit)
struct BrCkpt {
    uint32_t pc = 0, n_mem = 0, n_cs = 0, fc_counter = 0;
    uint64_t steps = 0;   // VM steps this run of the opcode has executed over all its passes
    uint32_t opcode = 0;  // index of the Brillig opcode in the circuit
    uint32_t state = BR_CKPT_NONE;
};
BR_HD inline void br_ckpt_encode(const BrCkpt &c, uint32_t *w) {
    w[0] = c.pc; w[1] = c.n_mem; w[2] = c.n_cs; w[3] = c.fc_counter;
    w[4] = (uint32_t)c.steps; w[5] = (uint32_t)(c.steps >> 32);
    w[6] = c.opcode; w[7] = c.state;
}
BR_HD inline BrCkpt br_ckpt_decode(const uint32_t *w) {
    BrCkpt c;
    c.pc = w[0]; c.n_mem = w[1]; c.n_cs = w[2]; c.fc_counter = w[3];
    c.steps = (uint64_t)w[5] << 32 | w[4];
    c.opcode = w[6]; c.state = w[7];
    return c;
}

// ---- the compact scratch of one pass under brillig_resume. A lane owns column `col` of every row; a record with n_regs registers sees
//   slot s (register r: s = r; memory cell c: s = n_regs + c), half h: uint4 number (2 s + h) * stride + col
//   call-stack word k:                                             u32 number (max_regs + mem_cap) * 8 * stride + k * stride + col
//   hash staging word w:                                           behind the call_depth stack words (not live between two instructions)
// The word region lies behind the slots of the record with the MOST registers of the circuit, not behind the lane's own: the lanes of one
// pass may stand at different Brillig opcodes, and a region that started behind a lane's own registers ran, four columns to a cell, through
// the topmost cells of a lane whose record has more of them. (Passes without resume keep the layout they had, behind the lane's own slots.)
struct BrLayout {
    uint64_t stride = 0;      // lanes, a multiple of 64
    uint32_t mem_cap = 0;     // memory cells of a lane
    uint32_t call_depth = 0;  // call-stack words of a lane
    uint32_t max_regs = 0;    // most registers any Brillig record of the circuit uses
};
BR_HD inline bool br_layout_equal(const BrLayout &a, const BrLayout &b) {
    return a.stride == b.stride && a.mem_cap == b.mem_cap && a.call_depth == b.call_depth && a.max_regs == b.max_regs;
}
BR_HD inline uint64_t br_slot_index(const BrLayout &l, uint64_t slot, uint32_t half, uint64_t col) { return (slot * 2u + half) * l.stride + col; }
BR_HD inline uint64_t br_words_base(const BrLayout &l) { return ((uint64_t)l.max_regs + l.mem_cap) * 8u * l.stride; }
BR_HD inline uint64_t br_stack_index(const BrLayout &l, uint64_t k, uint64_t col) { return br_words_base(l) + k * l.stride + col; }
// u32 words of the whole scratch
BR_HD inline uint64_t br_scratch_words(const BrLayout &l) {
    return (((uint64_t)l.max_regs + l.mem_cap) * 8u + l.call_depth + l.mem_cap / 4u + 16u) * l.stride;
}

// ---- relocation of one continuing lane from the old scratch into the new one: its n_regs registers, its n_mem live cells, its n_cs
// call-stack words -- nothing outside the live prefix. Items [0, n_regs + n_mem) are slots (both halves), the next n_cs are stack words.
struct BrRelocLane {
    uint32_t old_col, new_col, n_regs, n_mem, n_cs;
};
BR_HD inline uint64_t br_reloc_items(const BrRelocLane &r) { return (uint64_t)r.n_regs + r.n_mem + r.n_cs; }
// One item. T4 is the 16-byte unit the slots are made of (uint4 on the device; the host test brings its own).
template <class T4>
BR_HD inline void br_reloc_item(const BrRelocLane &r, uint64_t item, const BrLayout &from, const uint32_t *old_scratch, const BrLayout &to, uint32_t *new_scratch) {
    const uint64_t n_slots = (uint64_t)r.n_regs + r.n_mem;
    if (item < n_slots) {
        const T4 *src = (const T4 *)old_scratch;
        T4 *dst = (T4 *)new_scratch;
        dst[br_slot_index(to, item, 0, r.new_col)] = src[br_slot_index(from, item, 0, r.old_col)];
        dst[br_slot_index(to, item, 1, r.new_col)] = src[br_slot_index(from, item, 1, r.old_col)];
    } else {
        const uint64_t k = item - n_slots;
        new_scratch[br_stack_index(to, k, r.new_col)] = old_scratch[br_stack_index(from, k, r.old_col)];
    }
}

}  // namespace acvm
