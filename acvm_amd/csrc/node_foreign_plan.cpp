// node_foreign_plan.cpp -- see node_foreign_plan.hpp
#include "node_foreign_plan.hpp"

namespace acvm {

namespace {
constexpr uint64_t LIMIT = 1ull << 40;
uint64_t align256(uint64_t x) { return (x + 255) / 256 * 256; }
}  // namespace

int node_foreign_check_handler(const acvm_node_foreign_handler_t *h, bool has_solver, bool running, std::string *err) {
    if (running) { *err = "a node call is running: the foreign-call handler cannot be changed now"; return ACVM_E_STATE; }
    if (!h) return 0;
    if (has_solver) { *err = "a node with a caller's BlackBoxFunctionSolver takes no foreign-call handler (the device resolve refuses such handles)"; return ACVM_E_UNSUPPORTED; }
    if (!h->fn) { *err = "null handler function"; return ACVM_E_INVALID; }
    if (h->space != ACVM_SPACE_DEVICE && h->space != ACVM_SPACE_HOST) { *err = "unknown space " + std::to_string(h->space); return ACVM_E_INVALID; }
    const std::string shape = buffer_check_shape(h->in_encoding, h->in_layout, false);
    if (!shape.empty()) { *err = shape; return ACVM_E_INVALID; }
    return 0;
}

NodeForeignVerdict node_foreign_verdict(int returned, int *rc) {
    *rc = 0;
    if (returned == 0) return NODE_FOREIGN_ANSWERED;
    if (returned == 1) return NODE_FOREIGN_DECLINED;
    *rc = returned < 0 ? returned : ACVM_E_INVALID;
    return NODE_FOREIGN_ABORT;
}

bool node_foreign_inputs_scratch(uint32_t n_rows, uint32_t n_inputs, uint32_t max_values, uint32_t elem_size, NodeForeignInputs *out) {
    NodeForeignInputs s;
    const uint64_t cells = (uint64_t)n_rows * max_values;  // (both below 2^32: no overflow)
    if (cells > LIMIT || (uint64_t)n_rows * n_inputs > LIMIT) return false;
    s.rows_bytes = (uint64_t)n_rows * 4;
    s.lens_bytes = (uint64_t)n_rows * n_inputs * 4;
    s.values_bytes = cells * elem_size;
    s.mask_bytes = cells;
    s.o_rows = 0;
    s.o_lens = s.o_rows + align256(s.rows_bytes);
    s.o_values = s.o_lens + align256(s.lens_bytes);
    s.o_mask = s.o_values + align256(s.values_bytes);
    s.bytes = s.o_mask + align256(s.mask_bytes);
    if (s.bytes > LIMIT) return false;
    *out = s;
    return true;
}

int node_foreign_answer_scratch(const acvm_node_foreign_answer_t *a, uint32_t n_rows, NodeForeignAnswer *out, std::string *err) {
    const std::string shape = buffer_check_shape(a->encoding, a->layout, false);
    if (!shape.empty()) { *err = shape; return ACVM_E_INVALID; }
    if (a->n_values && !a->is_array) { *err = "null is_array"; return ACVM_E_INVALID; }
    uint64_t stride = a->stride;
    const std::string st = buffer_check_stride(a->layout, n_rows, a->n_columns, &stride);
    if (!st.empty()) { *err = st; return ACVM_E_INVALID; }
    NodeForeignAnswer s;
    const uint64_t size = buffer_element_size(a->encoding);
    uint64_t elements = 0;  // from the first to the last element
    if (n_rows && a->n_columns) {
        const uint64_t outer = a->layout == ACVM_LAYOUT_WITNESS_MAJOR ? a->n_columns : n_rows, inner = a->layout == ACVM_LAYOUT_WITNESS_MAJOR ? n_rows : a->n_columns;
        if (stride > LIMIT || (outer - 1) * stride + inner > LIMIT) { *err = "the answer's buffer is too large"; return ACVM_E_INVALID; }
        elements = (outer - 1) * stride + inner;
    }
    if (elements && !a->values) { *err = "null values"; return ACVM_E_INVALID; }
    s.values_bytes = elements * size;
    s.lens_bytes = a->row_lens ? (uint64_t)n_rows * a->n_values * 4 : 0;
    s.answered_bytes = a->answered ? n_rows : 0;
    s.o_values = 0;
    s.o_lens = s.o_values + align256(s.values_bytes);
    s.o_answered = s.o_lens + align256(s.lens_bytes);
    s.bytes = s.o_answered + align256(s.answered_bytes);
    if (s.bytes > LIMIT) { *err = "the answer's buffer is too large"; return ACVM_E_INVALID; }
    *out = s;
    return 0;
}

uint64_t node_foreign_grow(uint64_t have, uint64_t need) {
    if (need <= have) return 0;
    return align256(need + need / 4 + 256);
}

}  // namespace acvm
