// node_foreign_plan.hpp -- the host-only decisions of the node's foreign-call loop (include/acvm_amd.h acvm_node_set_foreign_call_handler; the loop
// itself: node.cpp foreign_rounds): the checks of a handler, the row_base rule of both node forms, the scratch a site needs for its inputs and
// for an uploaded answer, the round cap and what a handler's return value means. Pure host code like node_io_plan.hpp: no HIP call, no handle,
// no thread-local error text (tools/node_foreign_plan_host_test.cpp, tests/test_foreign_rows_on_host.py, `make asan`).
#pragma once
#include "import_plan.hpp"

namespace acvm {

// 0, or the refusal's code and text: ACVM_E_STATE while a node call runs, ACVM_E_UNSUPPORTED for a node with a caller's BlackBoxFunctionSolver,
// ACVM_E_INVALID for a null fn, an unknown space, encoding or layout -- in this order. h == null (no handler) passes the last two.
int node_foreign_check_handler(const acvm_node_foreign_handler_t *h, bool has_solver, bool running, std::string *err);

constexpr uint32_t NODE_FOREIGN_DEFAULT_ROUNDS = 256;
inline uint32_t node_foreign_max_rounds(uint32_t asked) { return asked ? asked : NODE_FOREIGN_DEFAULT_ROUNDS; }

// THE numbering rule: the caller's number of row i of a round is row_base + rows[i], rows[i] the instance number inside the tile.
// acvm_node_solve: the global instance number -- the lane owns [lane_first, ...) of the global batch; acvm_node_solve_device: the row number
// of the lane's own buffers (lane_first is not read).
inline uint64_t node_foreign_row_base(bool device_form, uint64_t lane_first, uint32_t tile_index, uint32_t tile) {
    return (device_form ? 0 : lane_first) + (uint64_t)tile_index * tile;
}

// what a handler's return value means
enum NodeForeignVerdict { NODE_FOREIGN_ANSWERED = 0, NODE_FOREIGN_DECLINED = 1, NODE_FOREIGN_ABORT = 2 };
// *rc: the node call's error for NODE_FOREIGN_ABORT -- the handler's negative value, ACVM_E_INVALID for any other one
NodeForeignVerdict node_foreign_verdict(int returned, int *rc);

// Scratch of one site's inputs: rows [n_rows] u32 | lens [n_rows][n_inputs] u32 | values n_rows x max_values elements | mask n_rows x max_values
// bytes, each part 256-byte aligned (the typed export's alignment rule holds for any encoding). false: the sizes do not fit 2^40 bytes.
struct NodeForeignInputs {
    uint64_t o_rows = 0, o_lens = 0, o_values = 0, o_mask = 0, bytes = 0;
    uint64_t rows_bytes = 0, lens_bytes = 0, values_bytes = 0, mask_bytes = 0;
};
bool node_foreign_inputs_scratch(uint32_t n_rows, uint32_t n_inputs, uint32_t max_values, uint32_t elem_size, NodeForeignInputs *out);

// Scratch of an answer uploaded from host memory: values | row_lens | answered, behind the inputs. values_bytes runs from the first to the last
// element of the described buffer. 0, or ACVM_E_INVALID and the text: an unknown encoding or layout, a stride below the dense one, null arrays.
struct NodeForeignAnswer {
    uint64_t o_values = 0, o_lens = 0, o_answered = 0, bytes = 0;
    uint64_t values_bytes = 0, lens_bytes = 0, answered_bytes = 0;
};
int node_foreign_answer_scratch(const acvm_node_foreign_answer_t *a, uint32_t n_rows, NodeForeignAnswer *out, std::string *err);

// grow-only with a quarter of slack: the bytes to allocate for a buffer that holds `have` and must hold `need` (0: it is large enough)
uint64_t node_foreign_grow(uint64_t have, uint64_t need);

}  // namespace acvm
