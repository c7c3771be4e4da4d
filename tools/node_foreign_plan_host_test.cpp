// node_foreign_plan_host_test.cpp -- the host-only decisions of the node's foreign-call loop (acvm_amd/csrc/node_foreign_plan.cpp) as a plain program:
// one command per line on stdin, one answer line per command (tests/test_foreign_rows_on_host.py; `make asan` builds it with the sanitizers).
//   handler <null|set> <fn 0|1> <space> <encoding> <layout> <has_solver> <running>   -> "<rc> <text>"
//   row_base <device_form> <lane_first> <tile_index> <tile>                          -> "<row_base>"
//   inputs <n_rows> <n_inputs> <max_values> <elem_size>                              -> "ok <o_rows> <o_lens> <o_values> <o_mask> <bytes>" | "too-large"
//   answer <encoding> <layout> <n_columns> <stride> <n_rows> <n_values> <values 0|1> <row_lens 0|1> <answered 0|1>
//                                                                                    -> "0 <o_values> <o_lens> <o_answered> <bytes> <values_bytes>" | "<rc> <text>"
//   rounds <asked>                                                                   -> "<max_rounds>"
//   verdict <returned>                                                               -> "<answered|declined|abort> <rc>"
//   grow <have> <need>                                                               -> "<bytes to allocate, 0 = none>"
#include <cstdio>
#include <iostream>
#include <sstream>
#include "../acvm_amd/csrc/node_foreign_plan.hpp"

using namespace acvm;

static int echo_handler(void *, const acvm_node_foreign_round_t *, acvm_node_foreign_answer_t *) { return 0; }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "handler") {
            std::string kind;
            int fn = 0, has_solver = 0, running = 0;
            acvm_node_foreign_handler_t h{};
            in >> kind >> fn >> h.space >> h.in_encoding >> h.in_layout >> has_solver >> running;
            h.fn = fn ? echo_handler : nullptr;
            std::string err;
            const int rc = node_foreign_check_handler(kind == "null" ? nullptr : &h, has_solver != 0, running != 0, &err);
            std::cout << rc << " " << err << "\n";
        } else if (cmd == "row_base") {
            int device_form = 0;
            uint64_t lane_first = 0;
            uint32_t k = 0, tile = 0;
            in >> device_form >> lane_first >> k >> tile;
            std::cout << node_foreign_row_base(device_form != 0, lane_first, k, tile) << "\n";
        } else if (cmd == "inputs") {
            uint32_t n_rows = 0, n_inputs = 0, max_values = 0, size = 0;
            in >> n_rows >> n_inputs >> max_values >> size;
            NodeForeignInputs s;
            if (!node_foreign_inputs_scratch(n_rows, n_inputs, max_values, size, &s)) std::cout << "too-large\n";
            else std::cout << "ok " << s.o_rows << " " << s.o_lens << " " << s.o_values << " " << s.o_mask << " " << s.bytes << "\n";
        } else if (cmd == "answer") {
            acvm_node_foreign_answer_t a{};
            uint32_t n_rows = 0;
            int values = 0, row_lens = 0, answered = 0;
            static const uint8_t kinds[64] = {0};
            static const uint32_t some = 0;
            in >> a.encoding >> a.layout >> a.n_columns >> a.stride >> n_rows >> a.n_values >> values >> row_lens >> answered;
            a.is_array = a.n_values <= 64 ? kinds : nullptr;
            a.values = values ? &some : nullptr;  // (never read: only judged against null)
            a.row_lens = row_lens ? &some : nullptr;
            a.answered = answered ? kinds : nullptr;
            NodeForeignAnswer s;
            std::string err;
            const int rc = node_foreign_answer_scratch(&a, n_rows, &s, &err);
            if (rc) std::cout << rc << " " << err << "\n";
            else std::cout << "0 " << s.o_values << " " << s.o_lens << " " << s.o_answered << " " << s.bytes << " " << s.values_bytes << "\n";
        } else if (cmd == "rounds") {
            uint32_t asked = 0;
            in >> asked;
            std::cout << node_foreign_max_rounds(asked) << "\n";
        } else if (cmd == "verdict") {
            int returned = 0, rc = 0;
            in >> returned;
            const NodeForeignVerdict v = node_foreign_verdict(returned, &rc);
            std::cout << (v == NODE_FOREIGN_ANSWERED ? "answered" : v == NODE_FOREIGN_DECLINED ? "declined" : "abort") << " " << rc << "\n";
        } else if (cmd == "grow") {
            uint64_t have = 0, need = 0;
            in >> have >> need;
            std::cout << node_foreign_grow(have, need) << "\n";
        } else if (!cmd.empty()) {
            std::cout << "unknown command\n";
            return 2;
        }
    }
    return 0;
}
