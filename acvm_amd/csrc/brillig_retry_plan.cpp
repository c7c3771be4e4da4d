// brillig_retry_plan.cpp -- see brillig_retry_plan.hpp.
#include "brillig_retry_plan.hpp"
#include <algorithm>

namespace acvm {

BrRetryCaps brillig_retry_caps(int64_t steps_max_log2, int64_t call_depth_max, int64_t mem_max_log2, int64_t resume, int64_t steps_total_log2) {
    BrRetryCaps c;
    c.max_steps = 1ull << (uint32_t)std::min<int64_t>(std::max<int64_t>(steps_max_log2, 0), 31);
    c.max_depth = (uint64_t)std::min<int64_t>(std::max<int64_t>(call_depth_max, 1), 1 << 24);
    c.max_cells = 1ull << (uint32_t)std::min<int64_t>(std::max<int64_t>(mem_max_log2, 0), 30);
    c.total_steps = 1ull << (uint32_t)std::min<int64_t>(std::max<int64_t>(steps_total_log2, 0), 62);
    c.resume = resume != 0;
    return c;
}

static BrRetryDecision final_lane(uint32_t kind, uint64_t limit, uint64_t wanted) {
    BrRetryDecision d;
    d.action = BR_FINAL;
    d.kind = kind;
    d.limit = limit;
    d.wanted = wanted;
    return d;
}

// The checkpoint of a lane is valid for the next pass when the pass that just ended ran it in the compact scratch, under resume, and left
// the VM loop of the SAME opcode at a device limit; its counts must fit the layout it was written in (the relocation reads no further).
static bool checkpoint_valid(const BrRetryCaps &caps, const BrRetryLimits &cur, bool compact, const BrRetryLane &l) {
    if (!caps.resume || !compact || l.prev_col == BR_NO_COLUMN || l.prev_col >= cur.stride) return false;
    const BrCkpt &c = l.ckpt;
    return c.state == BR_CKPT_LIMIT && c.opcode == l.opcode && c.n_mem <= cur.mem_cap && c.n_cs <= cur.call_depth;
}

void brillig_retry_plan(const BrRetryCaps &caps, const BrRetryLimits &cur, bool compact, uint32_t max_regs, const std::vector<BrRetryLane> &lanes, BrRetryPlan *out) {
    *out = BrRetryPlan();
    out->lanes.resize(lanes.size());
    // the memory a retried lane runs with so far (0 = the planner's estimate of its record)
    uint64_t record_cells = 0;
    auto at_limit = [](const BrRetryLane &l) { return l.msg == BR_MSG_MEM_CAP || l.msg == BR_MSG_STEP_LIMIT || l.msg == BR_MSG_CALL_DEPTH; };
    for (const BrRetryLane &l : lanes)
        if (at_limit(l)) record_cells = std::max<uint64_t>(record_cells, l.record_cells);
    const uint64_t cur_cells = cur.mem_cap ? cur.mem_cap : record_cells;
    // lanes past a stated maximum are final; the rest is retried with the limits they reached raised
    bool hit_steps = false, hit_depth = false, hit_mem = false;
    uint64_t want_cells = 0;
    std::vector<uint32_t> retried;
    for (uint32_t t = 0; t < lanes.size(); t++) {
        const BrRetryLane &l = lanes[t];
        if (!at_limit(l)) continue;
        const bool valid = checkpoint_valid(caps, cur, compact, l);
        if (l.msg == BR_MSG_STEP_LIMIT) {
            // resume: a pass is a slice, the total ends the lane (a lane without a checkpoint has lost at most one base pass and starts its count)
            if (caps.resume ? valid && l.ckpt.steps >= caps.total_steps : cur.steps >= caps.max_steps) {
                out->lanes[t] = final_lane(BR_KIND_STEPS, caps.resume ? caps.total_steps : caps.max_steps, 0);
                continue;
            }
        }
        if (l.msg == BR_MSG_CALL_DEPTH && cur.call_depth >= caps.max_depth) { out->lanes[t] = final_lane(BR_KIND_CALL_DEPTH, caps.max_depth, 0); continue; }
        // (the lane's own capacity so far: the raised one of an earlier pass, else the planner's estimate of ITS record)
        const uint64_t own_cells = cur.mem_cap ? cur.mem_cap : l.record_cells;
        if (l.msg == BR_MSG_MEM_CAP && ((uint64_t)l.x0 + 1 > caps.max_cells || own_cells >= caps.max_cells)) {
            out->lanes[t] = final_lane(BR_KIND_MEMORY, caps.max_cells, l.x0);
            continue;
        }
        BrRetryDecision &d = out->lanes[t];
        d.action = valid ? BR_CONTINUE : BR_RESTART;
        d.col = (uint32_t)retried.size();
        d.steps_done = valid ? l.ckpt.steps : 0;
        retried.push_back(t);
        (valid ? out->n_continued : out->n_restarted)++;
        hit_steps |= l.msg == BR_MSG_STEP_LIMIT;
        hit_depth |= l.msg == BR_MSG_CALL_DEPTH;
        if (l.msg == BR_MSG_MEM_CAP) {
            hit_mem = true;
            want_cells = std::max<uint64_t>(want_cells, (uint64_t)l.x0 + 1);
        }
    }
    out->n_retried = (uint32_t)retried.size();
    if (retried.empty()) return;
    BrRetryLimits next = cur;
    if (hit_steps) next.steps = (uint32_t)std::min<uint64_t>((uint64_t)cur.steps * 16, caps.max_steps);
    if (hit_depth) next.call_depth = (uint32_t)std::min<uint64_t>((uint64_t)cur.call_depth * 16, caps.max_depth);
    uint64_t cells = std::max<uint64_t>(cur_cells, 64);
    if (hit_mem) cells = std::min<uint64_t>(std::max<uint64_t>(2 * want_cells, 4 * cells), caps.max_cells);
    // (a capacity never shrinks: cells >= cur_cells, and a lane whose capacity stands at max_cells is final above, so the minimum cuts nothing live)
    next.mem_cap = (uint32_t)cells;
    next.stride = ((uint64_t)retried.size() + 63) / 64 * 64;
    out->next = next;
    out->to.stride = next.stride;
    out->to.mem_cap = next.mem_cap;
    out->to.call_depth = next.call_depth;
    out->to.max_regs = max_regs;
    out->scratch_bytes = br_scratch_words(out->to) * 4;
    if (!out->n_continued) return;
    out->from.stride = cur.stride;
    out->from.mem_cap = cur.mem_cap;
    out->from.call_depth = cur.call_depth;
    out->from.max_regs = max_regs;
    bool moved = !br_layout_equal(out->from, out->to);
    for (uint32_t t : retried)
        if (out->lanes[t].action == BR_CONTINUE) moved |= out->lanes[t].col != lanes[t].prev_col;
    out->relocate = moved;
    if (!moved) return;
    for (uint32_t t : retried) {
        if (out->lanes[t].action != BR_CONTINUE) continue;
        const BrRetryLane &l = lanes[t];
        out->reloc.push_back(BrRelocLane{l.prev_col, out->lanes[t].col, l.n_regs, l.ckpt.n_mem, l.ckpt.n_cs});
        out->cells_relocated += l.ckpt.n_mem;
    }
}

void brillig_retry_refused(BrRetryPlan *plan) {
    for (BrRetryDecision &d : plan->lanes)
        if (d.action == BR_CONTINUE || d.action == BR_RESTART) d = final_lane(BR_KIND_DEVICE_MEMORY, plan->scratch_bytes >> 20, 0);
    plan->n_retried = plan->n_continued = plan->n_restarted = 0;
    plan->relocate = false;
    plan->reloc.clear();
    plan->cells_relocated = 0;
}

}  // namespace acvm
