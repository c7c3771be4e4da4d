// node_io_plan_host_test.cpp -- the checks and the tile views of acvm_node_solve_device (acvm_amd/csrc/node_io_plan.cpp) as a plain C++ program:
// no HIP, no node. tests/test_node_io_plan_on_host.py compiles it and judges its answers by a Python restatement; `make asan` builds it a second
// time with the sanitizers (tools/asan/node_io_plan_host_test), for the same command stream.
//
//   g++ -std=c++17 -O1 tools/node_io_plan_host_test.cpp acvm_amd/csrc/node_io_plan.cpp acvm_amd/csrc/import_plan.cpp -o node_io_plan_host_test
//
// Commands on stdin, one per line. A list is comma separated, `e` an empty array, `null` a null pointer; pointers are plain numbers.
//   shape N_IN N_KEEP TILE           the node the following calls see
//   check N_EXPECTED N_LANES { N VALUES ENCODING LAYOUT N_COLUMNS STRIDE COLUMNS KEPT MASK KEPT_ENCODING KEPT_LAYOUT KEPT_STRIDE STATUS ERR OPCODE DIGESTS } x N_LANES
//   check N_EXPECTED null N_LANES    a null array
//   tile LANE K                      tile K of lane LANE of the last check that passed
//   offset LAYOUT K TILE STRIDE SIZE the address rule alone
// Answers: `err CODE TEXT`, or
//   ok N_LANES { IN_STRIDE IN_SIZE KEPT MASK KEPT_STRIDE KEPT_SIZE N_TILES } x N_LANES
//   ok FIRST M VALUES IN_STRIDE KEPT MASK KEPT_STRIDE STATUS ERR OPCODE DIGESTS
//   ok BYTES | overflow
#include "../acvm_amd/csrc/node_io_plan.hpp"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>

using namespace acvm;

// a caller's host array of exactly the listed size on the heap, so that a read past its end is one the sanitizer sees
struct List {
    std::unique_ptr<uint32_t[]> p;
    bool null = true;
    const uint32_t *data() const { return null ? nullptr : p.get(); }
};
static List read_list(std::istream &in) {
    std::string tok;
    in >> tok;
    List l;
    if (tok == "null") return l;
    l.null = false;
    std::vector<uint32_t> v;
    if (tok != "e") {
        std::stringstream ss(tok);
        for (std::string item; std::getline(ss, item, ',');) v.push_back((uint32_t)std::stoull(item));
    }
    l.p.reset(new uint32_t[v.size()]);
    for (size_t i = 0; i < v.size(); i++) l.p[i] = v[i];
    return l;
}
static uint64_t num(const void *p) { return (uint64_t)(uintptr_t)p; }
template <class T>
static void read_ptr(std::istream &in, T **p) {
    uint64_t v = 0;
    in >> v;
    *p = (T *)(uintptr_t)v;
}

int main() {
    NodeIoShape shape;
    std::vector<NodeLaneIo> checked;
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "shape") in >> shape.n_in >> shape.n_keep >> shape.tile;
        else if (cmd == "check") {
            uint32_t n_expected, n_lanes;
            std::string first;
            in >> n_expected >> first;
            const bool null_array = first == "null";
            if (null_array) in >> n_lanes;
            else n_lanes = (uint32_t)std::stoull(first);
            std::vector<acvm_node_lane_io_t> lanes(null_array ? 0 : n_lanes);
            std::vector<List> columns;
            for (acvm_node_lane_io_t &l : lanes) {
                l = acvm_node_lane_io_t{};
                in >> l.n;
                read_ptr(in, &l.d_values);
                in >> l.in.encoding >> l.in.layout >> l.in.n_columns >> l.in.stride;
                columns.push_back(read_list(in));
                l.in.columns = columns.back().data();
                read_ptr(in, &l.d_kept);
                read_ptr(in, &l.d_kept_assigned);
                in >> l.kept_encoding >> l.kept_layout >> l.kept_stride;
                read_ptr(in, &l.d_status);
                read_ptr(in, &l.d_err);
                read_ptr(in, &l.d_opcode_index);
                read_ptr(in, &l.d_digests32);
            }
            std::vector<NodeLaneIo> out;
            std::string err;
            const int rc = node_io_check(shape, null_array ? nullptr : lanes.data(), n_lanes, n_expected, &out, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            printf("ok %zu", out.size());
            for (NodeLaneIo &l : out) {
                printf(" %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u", l.io.in.stride, l.in_size, num(l.io.d_kept), num(l.io.d_kept_assigned), l.io.kept_stride, l.kept_size,
                       l.n_tiles);
                l.io.in.columns = nullptr;  // (the caller's list does not outlive the command)
            }
            printf("\n");
            checked = std::move(out);
        } else if (cmd == "tile") {
            uint32_t lane, k;
            in >> lane >> k;
            if (lane >= checked.size()) { fprintf(stderr, "no such lane\n"); return 2; }
            NodeTileIo t;
            std::string err;
            const int rc = node_io_tile(shape, checked[lane], k, &t, &err);
            if (rc) { printf("err %d %s\n", rc, err.c_str()); continue; }
            printf("ok %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", t.first, t.m, num(t.d_values),
                   t.in.stride, num(t.d_kept), num(t.d_kept_assigned), t.kept_stride, num(t.d_status), num(t.d_err), num(t.d_opcode_index), num(t.d_digests32));
        } else if (cmd == "offset") {
            uint32_t layout;
            uint64_t k, tile, stride, size, bytes = 0;
            in >> layout >> k >> tile >> stride >> size;
            if (node_io_tile_offset(layout, k, tile, stride, size, &bytes)) printf("ok %" PRIu64 "\n", bytes);
            else printf("overflow\n");
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
