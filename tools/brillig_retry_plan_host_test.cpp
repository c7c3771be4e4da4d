// brillig_retry_plan_host_test.cpp -- the host-only decisions of the Brillig retry loop (acvm_amd/csrc/brillig_retry_plan.cpp) as a plain program:
// one command per line on stdin, one answer line per command (tests/test_brillig_retry_plan_on_host.py; `make asan` builds it with the sanitizers).
//   plan <refuse 0|1> <resume> <steps_max_log2> <call_depth_max> <mem_max_log2> <steps_total_log2>
//        <cur steps> <cur call_depth> <cur mem_cap> <cur stride> <compact 0|1> <max_regs> <n_lanes>
//        then per lane: <msg> <x0> <opcode> <record_cells> <n_regs> <prev_col> <ckpt n_mem> <ckpt n_cs> <ckpt steps> <ckpt opcode> <ckpt state>
//     -> "<n_retried> <n_continued> <n_restarted> <next steps> <next call_depth> <next mem_cap> <next stride> <scratch_bytes> <relocate> <cells_relocated>"
//        " L" then per lane " <action> <col> <kind> <limit> <wanted> <steps_done>", " R" then per relocated lane " <old_col> <new_col> <n_regs> <n_mem> <n_cs>"
//        (refuse = 1: the answer after brillig_retry_refused -- the allocation of the scratch was refused)
//   caps <steps_max_log2> <call_depth_max> <mem_max_log2> <resume> <steps_total_log2>  -> "<max_steps> <max_depth> <max_cells> <total_steps> <resume>"
#include <cstdio>
#include <iostream>
#include <sstream>
#include "../acvm_amd/csrc/brillig_retry_plan.hpp"

using namespace acvm;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "caps") {
            int64_t a = 0, b = 0, c = 0, d = 0, e = 0;
            in >> a >> b >> c >> d >> e;
            const BrRetryCaps caps = brillig_retry_caps(a, b, c, d, e);
            std::cout << caps.max_steps << " " << caps.max_depth << " " << caps.max_cells << " " << caps.total_steps << " " << (caps.resume ? 1 : 0) << "\n";
        } else if (cmd == "plan") {
            int refuse = 0, compact = 0;
            int64_t resume = 0, steps_max = 0, depth_max = 0, mem_max = 0, total = 0;
            BrRetryLimits cur;
            uint32_t max_regs = 0, n = 0;
            in >> refuse >> resume >> steps_max >> depth_max >> mem_max >> total >> cur.steps >> cur.call_depth >> cur.mem_cap >> cur.stride >> compact >> max_regs >> n;
            std::vector<BrRetryLane> lanes(n);
            for (BrRetryLane &l : lanes)
                in >> l.msg >> l.x0 >> l.opcode >> l.record_cells >> l.n_regs >> l.prev_col >> l.ckpt.n_mem >> l.ckpt.n_cs >> l.ckpt.steps >> l.ckpt.opcode >> l.ckpt.state;
            if (!in) { std::cout << "bad command\n"; return 2; }
            BrRetryPlan plan;
            brillig_retry_plan(brillig_retry_caps(steps_max, depth_max, mem_max, resume, total), cur, compact != 0, max_regs, lanes, &plan);
            if (refuse) brillig_retry_refused(&plan);
            std::cout << plan.n_retried << " " << plan.n_continued << " " << plan.n_restarted << " " << plan.next.steps << " " << plan.next.call_depth << " " << plan.next.mem_cap << " "
                      << plan.next.stride << " " << plan.scratch_bytes << " " << (plan.relocate ? 1 : 0) << " " << plan.cells_relocated << " L";
            for (const BrRetryDecision &d : plan.lanes) std::cout << " " << d.action << " " << d.col << " " << d.kind << " " << d.limit << " " << d.wanted << " " << d.steps_done;
            std::cout << " R";
            for (const BrRelocLane &r : plan.reloc) std::cout << " " << r.old_col << " " << r.new_col << " " << r.n_regs << " " << r.n_mem << " " << r.n_cs;
            std::cout << "\n";
        } else if (!cmd.empty()) {
            std::cout << "unknown command\n";
            return 2;
        }
    }
    return 0;
}
