// brillig_retry_plan.hpp -- the host-only decisions of one look at the Brillig lanes that stopped at a device limit (batch_exact.cpp
// retry_device_limits is the caller): which lane continues from its checkpoint, which one runs its opcode again, which one is final;
// the limits, the stride, the columns and the bytes of the next pass's compact scratch; and what the relocation kernel has to copy.
// A pure function like node_foreign_plan.hpp: no HIP call, no handle (tools/brillig_retry_plan_host_test.cpp,
// tests/test_brillig_retry_plan_on_host.py, `make asan`).
#pragma once
#include <vector>
#include "brillig_resume.hpp"

namespace acvm {

constexpr uint32_t BR_MSG_MEM_CAP = 17u, BR_MSG_STEP_LIMIT = 18u, BR_MSG_CALL_DEPTH = 28u;  // DevMsg codes of the three limits (ops_common.hpp)
constexpr uint32_t BR_NO_COLUMN = 0xFFFFFFFFu;
// the kinds of include/acvm_amd.h ACVM_LIMIT_* (static_assert'ed against the header in batch_exact.cpp)
constexpr uint32_t BR_KIND_STEPS = 1u, BR_KIND_CALL_DEPTH = 2u, BR_KIND_MEMORY = 3u, BR_KIND_DEVICE_MEMORY = 4u;

// the tuning keys, clamped (tuning.hpp)
struct BrRetryCaps {
    uint64_t max_steps = 0;    // 2^brillig_steps_max_log2 (0..31): most steps of one pass
    uint64_t max_depth = 0;    // brillig_call_depth_max (1..2^24)
    uint64_t max_cells = 0;    // 2^brillig_mem_max_log2 (0..30)
    uint64_t total_steps = 0;  // 2^brillig_steps_total_log2 (0..62): most steps of one run of an opcode over all its passes, under resume
    bool resume = false;       // brillig_resume
};
BrRetryCaps brillig_retry_caps(int64_t steps_max_log2, int64_t call_depth_max, int64_t mem_max_log2, int64_t resume, int64_t steps_total_log2);

// limits and layout of a pass (kernels.hpp BrilligLimits without the device types)
struct BrRetryLimits {
    uint32_t steps = 0, call_depth = 0;
    uint32_t mem_cap = 0;  // 0: every record's own estimate (the class scratch of the first pass)
    uint64_t stride = 0;
};

struct BrRetryLane {
    uint32_t msg = 0;            // the lane's result: one of BR_MSG_*, or 0 -- it is not at a device limit
    uint32_t x0 = 0;             // ... the cell a write wanted (BR_MSG_MEM_CAP)
    uint32_t opcode = 0;         // ... its Brillig opcode
    uint32_t record_cells = 0;   // the planner's memory estimate of that opcode's record
    uint32_t n_regs = 0;         // registers of that record
    uint32_t prev_col = BR_NO_COLUMN;  // its column in the pass that just ended, BR_NO_COLUMN: it did not run in a compact scratch
    BrCkpt ckpt;                 // its checkpoint record as the pass left it
};

enum BrAction : uint32_t { BR_SKIP = 0, BR_CONTINUE = 1, BR_RESTART = 2, BR_FINAL = 3 };
struct BrRetryDecision {
    uint32_t action = BR_SKIP;
    uint32_t col = BR_NO_COLUMN;          // BR_CONTINUE / BR_RESTART: column in the next pass's scratch
    uint32_t kind = 0;                    // BR_FINAL: ACVM_LIMIT_*, the limit's value and what the lane wanted
    uint64_t limit = 0, wanted = 0;
    uint64_t steps_done = 0;              // BR_CONTINUE: steps behind the lane
};

struct BrRetryPlan {
    std::vector<BrRetryDecision> lanes;
    uint32_t n_retried = 0, n_continued = 0, n_restarted = 0;
    BrRetryLimits next;                   // n_retried != 0: the next pass
    uint64_t scratch_bytes = 0;
    // n_continued != 0: the scratch's layout or a continuing lane's column changes -- the next pass needs a NEW buffer and the copy below.
    // false with continuing lanes: the pass runs in the buffer it has, there is nothing to launch.
    bool relocate = false;
    BrLayout from, to;
    std::vector<BrRelocLane> reloc;
    uint64_t cells_relocated = 0;         // sum of the live prefixes (n_mem) of reloc
};

// cur: the limits of the pass that just ended; compact: it ran in a compact scratch (false: the class scratch -- no lane has a checkpoint).
// With caps.resume == false no lane continues and the decisions are those of the restart loop: a lane at the step limit with
// cur.steps >= max_steps is final, and so on.
void brillig_retry_plan(const BrRetryCaps &caps, const BrRetryLimits &cur, bool compact, uint32_t max_regs, const std::vector<BrRetryLane> &lanes, BrRetryPlan *out);
// the device refused the scratch (or the second buffer a relocation needs): every lane the plan retried is final with ACVM_LIMIT_DEVICE_MEMORY
void brillig_retry_refused(BrRetryPlan *plan);

}  // namespace acvm
