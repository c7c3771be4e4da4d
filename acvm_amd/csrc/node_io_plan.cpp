// node_io_plan.cpp -- the checks and the tile views of acvm_node_solve_device (node_io_plan.hpp). Everything the caller controls about a lane's
// buffers is judged here, with the checks of the batch's device import and export (import_plan.cpp); nothing here knows a device.
#include "node_io_plan.hpp"

namespace acvm {

bool node_io_tile_offset(uint32_t layout, uint64_t k, uint64_t tile, uint64_t stride, uint64_t size, uint64_t *bytes) {
    uint64_t elements = 0;
    if (__builtin_mul_overflow(k, tile, &elements)) return false;
    if (layout != ACVM_LAYOUT_WITNESS_MAJOR && __builtin_mul_overflow(elements, stride, &elements)) return false;
    return !__builtin_mul_overflow(elements, size, bytes);
}

// one lane; the text without the lane's number
static std::string check_lane(const NodeIoShape &s, const acvm_node_lane_io_t &l, NodeLaneIo *out) {
    if (l.n >> 32) return "n " + std::to_string(l.n) + " is not below 2^32";
    out->io = l;
    out->n_tiles = (uint32_t)((l.n + s.tile - 1) / s.tile);
    if (!l.n) return std::string();  // the lane idles: none of its pointers is read
    const uint32_t n = (uint32_t)l.n;
    {   // the inputs: acvm_batch_import_device's checks for a handle of n live instances
        ImportView view;
        view.B = n;
        view.n_in = s.n_in;
        ImportPlan plan;
        std::string err;
        if (import_plan_desc(&view, &l.in, l.d_values, &plan, &err)) return "input: " + err;
        out->io.in.stride = plan.parts[0].stride;
        out->in_size = plan.parts[0].elem_size;
    }
    if (!s.n_keep || !l.d_kept) {
        if (s.n_keep && l.d_kept_assigned) return "kept: d_kept_assigned without d_kept";
        out->io.d_kept = nullptr;
        out->io.d_kept_assigned = nullptr;
        return std::string();
    }
    // the kept witnesses: acvm_batch_export_device's checks of the buffer for n instances x n_keep positions
    std::string err = buffer_check_shape(l.kept_encoding, l.kept_layout, false);
    if (err.empty()) err = buffer_check_pointer(l.kept_encoding, l.d_kept);
    uint64_t stride = l.kept_stride;
    if (err.empty()) err = buffer_check_stride(l.kept_layout, n, s.n_keep, &stride);
    if (err.empty()) {  // (the byte offset of the last element fits 63 bits, as for an import)
        const unsigned __int128 rows = l.kept_layout == ACVM_LAYOUT_WITNESS_MAJOR ? s.n_keep : n;
        if (rows * stride > ((unsigned __int128)1 << 57)) err = "stride " + std::to_string(stride) + " is beyond any device buffer";
    }
    if (!err.empty()) return "kept: " + err;
    out->io.kept_stride = stride;
    out->kept_size = buffer_element_size(l.kept_encoding);
    return std::string();
}

int node_io_check(const NodeIoShape &s, const acvm_node_lane_io_t *lanes, uint32_t n_lanes, uint32_t n_expected, std::vector<NodeLaneIo> *out, std::string *err) {
    if (n_lanes != n_expected) { *err = "n_lanes " + std::to_string(n_lanes) + " is not the node's number of handles, " + std::to_string(n_expected); return ACVM_E_INVALID; }
    if (n_lanes && !lanes) { *err = "null argument"; return ACVM_E_INVALID; }
    if (!s.tile) { *err = "tile of 0 instances"; return ACVM_E_INVALID; }
    std::vector<NodeLaneIo> checked(n_lanes);
    for (uint32_t l = 0; l < n_lanes; l++) {
        const std::string text = check_lane(s, lanes[l], &checked[l]);
        if (!text.empty()) { *err = "lane " + std::to_string(l) + ": " + text; return ACVM_E_INVALID; }
    }
    *out = std::move(checked);
    return 0;
}

// base + the tile's offset by the rule; null stays null
template <class T>
static bool tile_pointer(T *base, uint32_t layout, uint64_t k, uint64_t tile, uint64_t stride, uint64_t size, T **out) {
    *out = nullptr;
    if (!base) return true;
    uint64_t bytes = 0;
    uintptr_t at = 0;
    if (!node_io_tile_offset(layout, k, tile, stride, size, &bytes) || __builtin_add_overflow((uintptr_t)base, (uintptr_t)bytes, &at)) return false;
    *out = (T *)at;
    return true;
}

int node_io_tile(const NodeIoShape &s, const NodeLaneIo &lane, uint32_t k, NodeTileIo *out, std::string *err) {
    const acvm_node_lane_io_t &l = lane.io;
    if (k >= lane.n_tiles) { *err = "tile " + std::to_string(k) + " is not below the lane's " + std::to_string(lane.n_tiles) + " tiles"; return ACVM_E_INVALID; }
    NodeTileIo t;
    t.first = (uint64_t)k * s.tile;
    t.m = (uint32_t)(l.n - t.first < s.tile ? l.n - t.first : s.tile);
    t.in = l.in;
    t.kept_stride = l.kept_stride;
    const uint32_t IM = ACVM_LAYOUT_INSTANCE_MAJOR;
    const bool ok = tile_pointer((const uint8_t *)l.d_values, l.in.layout, k, s.tile, l.in.stride, lane.in_size, (const uint8_t **)&t.d_values) &&
                    tile_pointer((uint8_t *)l.d_kept, l.kept_layout, k, s.tile, l.kept_stride, lane.kept_size, (uint8_t **)&t.d_kept) &&
                    tile_pointer(l.d_kept_assigned, l.kept_layout, k, s.tile, l.kept_stride, 1, &t.d_kept_assigned) &&
                    tile_pointer(l.d_status, IM, k, s.tile, 1, 1, &t.d_status) && tile_pointer(l.d_err, IM, k, s.tile, 1, 1, &t.d_err) &&
                    tile_pointer((uint8_t *)l.d_opcode_index, IM, k, s.tile, 1, 4, (uint8_t **)&t.d_opcode_index) &&
                    tile_pointer(l.d_digests32, IM, k, s.tile, 1, 32, &t.d_digests32);
    if (!ok) { *err = "tile " + std::to_string(k) + ": a buffer's offset does not fit 64 bits"; return ACVM_E_INVALID; }
    *out = t;
    return 0;
}

}  // namespace acvm
