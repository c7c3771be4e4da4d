// node_io_plan.hpp -- the device form of the node driver (include/acvm_amd.h acvm_node_solve_device) before anything touches a device: the
// checks of every lane's buffers, and the one rule that turns (lane, tile k, tile size) into that tile's import descriptor, export view and
// column pointers. Pure host code like import_plan.hpp, whose buffer checks it reuses: no HIP call, no handle, no thread-local error text
// (tools/node_io_plan_host_test.cpp, tests/test_node_io_plan_on_host.py, `make asan`).
#pragma once
#include "import_plan.hpp"

namespace acvm {

// what the checks need of a node
struct NodeIoShape {
    uint32_t n_in = 0, n_keep = 0;  // initial witnesses, kept witnesses
    uint32_t tile = 0;              // instances per tile (acvm_node_tile_instances), never 0
};
// a lane that passed: the caller's descriptor with both strides as launched (never 0 where the buffer has elements)
struct NodeLaneIo {
    acvm_node_lane_io_t io{};
    uint32_t in_size = 32, kept_size = 32;  // bytes per element
    uint32_t n_tiles = 0;
};
// Every lane, before any lane starts: 0 and *out (one entry per lane), or ACVM_E_INVALID and the text in *err, which names the lane.
int node_io_check(const NodeIoShape &s, const acvm_node_lane_io_t *lanes, uint32_t n_lanes, uint32_t n_expected, std::vector<NodeLaneIo> *out, std::string *err);

// THE address rule. A tile is rows [k * tile, k * tile + m) of the lane. Instance-major, the tile starts k * tile * stride elements behind the
// base and keeps the stride; witness-major, k * tile elements behind it and keeps the lane-wide stride; a column of one element per row ([n]
// status / err / opcode index, [n][32] digests) is instance-major with stride 1. Bytes = elements * size, in 64-bit arithmetic: false when
// it does not fit.
bool node_io_tile_offset(uint32_t layout, uint64_t k, uint64_t tile, uint64_t stride, uint64_t size, uint64_t *bytes);

// tile k of a checked lane: what batch_import_desc_async and the tile's outcome sink are given
struct NodeTileIo {
    uint64_t first = 0;  // the tile's first row of the lane
    uint32_t m = 0;      // its live instances
    const void *d_values = nullptr;
    acvm_import_desc_t in{};
    void *d_kept = nullptr;
    uint8_t *d_kept_assigned = nullptr;
    uint64_t kept_stride = 0;
    uint8_t *d_status = nullptr, *d_err = nullptr;
    uint32_t *d_opcode_index = nullptr;
    uint8_t *d_digests32 = nullptr;
};
int node_io_tile(const NodeIoShape &s, const NodeLaneIo &lane, uint32_t k, NodeTileIo *out, std::string *err);

}  // namespace acvm
