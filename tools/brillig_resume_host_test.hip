// brillig_resume_host_test.hip -- the checkpoint record, the compact scratch's index functions and the relocation of acvm_amd/csrc/brillig_resume.hpp
// run on the HOST over heap arrays of exactly their sizes (tests/test_brillig_resume_on_host.py; `make asan` builds it with the host side
// sanitized): one command per line on stdin, one answer line per command.
//   ckpt <pc> <n_mem> <n_cs> <fc_counter> <steps> <opcode> <state>   -> the 8 record words, then the 7 fields decoded from them
//   index <stride> <mem_cap> <call_depth> <max_regs> <what 0 slot|1 stack> <a> <half> <col>   -> the uint4 number of the slot's half / the u32 number of stack word a
//   cover <stride> <mem_cap> <call_depth> <max_regs>
//       every u32 word of every register, cell and stack word of every column -- column c holds a record of 1 + c % max_regs registers -- is
//       marked in an array of br_scratch_words bytes
//       -> "ok <words marked> <scratch words>" | "twice <word>" (two addresses on one word)
//   relocate <seed> <from stride> <from mem_cap> <from call_depth> <to stride> <to mem_cap> <to call_depth> <max_regs> <n_lanes>
//            then per lane: <old_col> <new_col> <n_regs> <n_mem> <n_cs>
//       the old scratch holds word i = i * 2654435761 + seed; every item of every lane goes through br_reloc_item into a new scratch, twice over two
//       different fills; then the new scratch is read the way BrVm reads it (ops_brillig.hpp: fr_load's rows, the word region behind the slots)
//       -> "<words of the new scratch the relocation wrote>" then per lane " <sum of (ordinal + 1) * word over its live words, mod 2^64>"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <vector>
#include "../acvm_amd/csrc/brillig_resume.hpp"

using namespace acvm;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "ckpt") {
            BrCkpt c;
            in >> c.pc >> c.n_mem >> c.n_cs >> c.fc_counter >> c.steps >> c.opcode >> c.state;
            std::vector<uint32_t> w(BR_CKPT_WORDS);
            br_ckpt_encode(c, w.data());
            const BrCkpt d = br_ckpt_decode(w.data());
            for (uint32_t x : w) std::cout << x << " ";
            std::cout << d.pc << " " << d.n_mem << " " << d.n_cs << " " << d.fc_counter << " " << d.steps << " " << d.opcode << " " << d.state << "\n";
        } else if (cmd == "index") {
            BrLayout l;
            uint32_t what = 0, half = 0;
            uint64_t a = 0, col = 0;
            in >> l.stride >> l.mem_cap >> l.call_depth >> l.max_regs >> what >> a >> half >> col;
            std::cout << (what ? br_stack_index(l, a, col) : br_slot_index(l, a, half, col)) << "\n";
        } else if (cmd == "cover") {
            BrLayout l;
            in >> l.stride >> l.mem_cap >> l.call_depth >> l.max_regs;
            if (!l.max_regs) { std::cout << "bad command\n"; return 2; }
            const uint64_t words = br_scratch_words(l);
            std::vector<uint8_t> seen(words, 0);
            uint64_t marked = 0, twice = ~0ull;
            auto mark = [&](uint64_t w) {
                if (seen[w]++) twice = w;
                marked++;
            };
            for (uint64_t col = 0; col < l.stride; col++) {
                const uint32_t n_regs = 1u + (uint32_t)(col % l.max_regs);
                for (uint64_t slot = 0; slot < (uint64_t)n_regs + l.mem_cap; slot++)
                    for (uint32_t half = 0; half < 2; half++)
                        for (uint32_t k = 0; k < 4; k++) mark(br_slot_index(l, slot, half, col) * 4 + k);
                for (uint64_t k = 0; k < l.call_depth; k++) mark(br_stack_index(l, k, col));
            }
            if (twice != ~0ull) std::cout << "twice " << twice << "\n";
            else std::cout << "ok " << marked << " " << words << "\n";
        } else if (cmd == "relocate") {
            uint32_t seed = 0, max_regs = 0, n = 0;
            BrLayout from, to;
            in >> seed >> from.stride >> from.mem_cap >> from.call_depth >> to.stride >> to.mem_cap >> to.call_depth >> max_regs >> n;
            from.max_regs = to.max_regs = max_regs;
            std::vector<BrRelocLane> lanes(n);
            for (BrRelocLane &r : lanes) in >> r.old_col >> r.new_col >> r.n_regs >> r.n_mem >> r.n_cs;
            if (!in) { std::cout << "bad command\n"; return 2; }
            const uint64_t old_words = br_scratch_words(from), new_words = br_scratch_words(to);
            // (heap blocks of exactly the scratches' sizes, 16-byte aligned like a device allocation: an access outside is a report)
            uint4 *old_block = new uint4[(old_words + 3) / 4], *a_block = new uint4[(new_words + 3) / 4], *b_block = new uint4[(new_words + 3) / 4];
            uint32_t *old_scratch = (uint32_t *)old_block, *a = (uint32_t *)a_block, *b = (uint32_t *)b_block;
            for (uint64_t i = 0; i < old_words; i++) old_scratch[i] = (uint32_t)(i * 2654435761ull + seed);
            for (uint64_t i = 0; i < new_words; i++) { a[i] = 0x5A5A5A5Au; b[i] = 0xA5A5A5A5u; }
            for (const BrRelocLane &r : lanes)
                for (uint64_t item = 0; item < br_reloc_items(r); item++) {
                    br_reloc_item<uint4>(r, item, from, old_scratch, to, a);
                    br_reloc_item<uint4>(r, item, from, old_scratch, to, b);
                }
            uint64_t written = 0;
            for (uint64_t i = 0; i < new_words; i++) written += a[i] == b[i];
            std::cout << written;
            for (const BrRelocLane &r : lanes) {
                // BrVm of the next pass: slots = scratch, Bp = to.stride, j = new_col, words = scratch + (max_regs + mem_cap) * 8 * Bp
                const uint4 *slots = (const uint4 *)a;
                const uint32_t *words = a + (uint64_t)(max_regs + to.mem_cap) * 8u * to.stride;
                uint64_t sum = 0, ordinal = 0;
                for (uint32_t slot = 0; slot < r.n_regs + r.n_mem; slot++) {
                    const uint4 lo = slots[(uint64_t)slot * 2 * to.stride + r.new_col], hi = slots[((uint64_t)slot * 2 + 1) * to.stride + r.new_col];
                    for (uint32_t v : {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}) sum += ++ordinal * v;
                }
                for (uint32_t k = 0; k < r.n_cs; k++) sum += ++ordinal * words[(uint64_t)k * to.stride + r.new_col];
                std::cout << " " << sum;
            }
            std::cout << "\n";
            delete[] old_block;
            delete[] a_block;
            delete[] b_block;
        } else if (!cmd.empty()) {
            std::cout << "unknown command\n";
            return 2;
        }
    }
    return 0;
}
