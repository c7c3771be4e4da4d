"""The resumable Brillig VM without a device: the checkpoint record, the index functions of the compact VM scratch and the relocation between two
scratches (acvm_amd/csrc/brillig_resume.hpp) compiled for the host (tools/brillig_resume_host_test.hip), once as it is and once through
`make asan` over heap arrays of exactly the scratches' sizes, and judged by Python index arithmetic: every register, cell and stack word of every
column has a word of its own inside the scratch; a relocated state lies where the VM of the next pass reads it, and nothing else was written.
Plus the pieces of the public interface that need no GPU."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "brillig_resume_host_test.hip")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("brillig_resume") / "brillig_resume_host_test")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", SOURCE, "-o", exe])
    else:  # a stand-alone program with the host side sanitized
        exe = os.path.join(ROOT, "tools", "asan", "brillig_resume_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/brillig_resume_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def scratch_words(stride, mem_cap, depth, max_regs):
    return ((max_regs + mem_cap) * 8 + depth + mem_cap // 4 + 16) * stride


def slot_word(stride, slot, half, col, k):
    """u32 number of word k of half `half` of a slot: rows of 16-byte units, [slot][half][lane]"""
    return ((slot * 2 + half) * stride + col) * 4 + k


def stack_word(stride, mem_cap, max_regs, k, col):
    """the word region lies behind the slots of the circuit's LARGEST record, whichever record the lane runs"""
    return (max_regs + mem_cap) * 8 * stride + k * stride + col


def test_checkpoint_record_round_trip(tool):
    rng = random.Random(0xB411)
    cases = [(0, 0, 0, 0, 0, 0, 0), (1, 2, 3, 4, 5, 6, 5), ((1 << 32) - 1,) * 4 + ((1 << 64) - 1, (1 << 32) - 1, 5), (7, 0, 0, 0, 1 << 32, 9, 1), (7, 0, 0, 0, (1 << 32) - 1, 9, 3)]
    cases += [tuple(rng.randrange(1 << 32) for _ in range(4)) + (rng.randrange(1 << 64), rng.randrange(1 << 32), rng.randrange(6)) for _ in range(100)]
    got = tool(["ckpt %d %d %d %d %d %d %d" % c for c in cases])
    for c, g in zip(cases, got):
        v = [int(x) for x in g.split()]
        pc, n_mem, n_cs, fc, steps, opcode, state = c
        assert v[:8] == [pc, n_mem, n_cs, fc, steps & 0xFFFFFFFF, steps >> 32, opcode, state]  # the record: 8 words, steps as two
        assert tuple(v[8:]) == c


def test_index_functions(tool):
    rng = random.Random(0xB412)
    cases = []
    for _ in range(200):
        stride = 64 * rng.randrange(1, 40)
        cases.append((stride, rng.choice([64, 100, 4096, 1 << 22]), rng.choice([4, 64, 65536]), rng.randrange(1, 300), rng.randrange(2), rng.randrange(1 << 22), rng.randrange(2),
                      rng.randrange(stride)))
    cases.append((1 << 20, 1 << 22, 65536, 200, 0, (1 << 22) + 199, 1, (1 << 20) - 1))  # beyond 2^32 units
    got = tool(["index %d %d %d %d %d %d %d %d" % c for c in cases])
    for (stride, mem_cap, depth, max_regs, what, a, half, col), g in zip(cases, got):
        want = stack_word(stride, mem_cap, max_regs, a, col) if what else slot_word(stride, a, half, col, 0) // 4
        assert int(g) == want


@pytest.mark.parametrize("layout", [(64, 64, 4, 6), (64, 64, 4, 9), (128, 100, 64, 5), (192, 1, 1, 1), (64, 602, 256, 12), (64, 0, 0, 3)])
def test_every_address_has_a_word_of_its_own_inside_the_scratch(tool, layout):
    """old and new layouts alike: the offsets are injective and in bounds (the array has exactly br_scratch_words bytes under the sanitizer) -- with
    the columns holding records of 1 .. max_regs registers side by side, as the lanes of one pass may stand at different Brillig opcodes"""
    stride, mem_cap, depth, max_regs = layout
    g = tool(["cover %d %d %d %d" % layout])[0].split()
    assert g[0] == "ok", g
    marked = sum((1 + col % max_regs + mem_cap) * 8 + depth for col in range(stride))
    assert int(g[1]) == marked and int(g[2]) == scratch_words(stride, mem_cap, depth, max_regs) >= marked


def relocate_case(rng, n_lanes, frm, to, max_regs):
    old_cols = rng.sample(range(frm[0]), n_lanes)
    new_cols = rng.sample(range(to[0]), n_lanes)
    lanes = []
    for q in range(n_lanes):
        lanes.append((old_cols[q], new_cols[q], rng.randrange(1, max_regs + 1), rng.choice([0, 1, min(frm[1], to[1]) // 2, min(frm[1], to[1])]),
                      rng.choice([0, 1, min(frm[2], to[2])])))
    return lanes


def test_a_relocated_state_lies_where_the_next_pass_reads_it(tool):
    rng = random.Random(0xB413)
    cases = []
    for frm, to, n in [((64, 64, 4), (64, 256, 4), 1), ((64, 64, 4), (64, 64, 64), 3), ((128, 64, 4), (64, 64, 4), 60), ((128, 100, 16), (192, 602, 256), 70),
                       ((64, 256, 8), (64, 256, 8), 5), ((64, 4096, 4), (64, 8192, 4), 2)]:
        max_regs = rng.randrange(3, 12)
        cases.append((rng.randrange(1 << 32), frm, to, max_regs, relocate_case(rng, n, frm, to, max_regs)))
    got = tool(["relocate %d %d %d %d %d %d %d %d %d " % ((seed,) + frm + to + (max_regs, len(lanes))) + " ".join("%d %d %d %d %d" % l for l in lanes)
                for seed, frm, to, max_regs, lanes in cases])
    for (seed, frm, to, max_regs, lanes), g in zip(cases, got):
        v = [int(x) for x in g.split()]
        old = lambda i: (i * 2654435761 + seed) & 0xFFFFFFFF
        live = 0
        for (old_col, new_col, n_regs, n_mem, n_cs), s in zip(lanes, v[1:]):
            want, ordinal = 0, 0
            for slot in range(n_regs + n_mem):
                for half in range(2):
                    for k in range(4):
                        ordinal += 1
                        want += ordinal * old(slot_word(frm[0], slot, half, old_col, k))
            for k in range(n_cs):
                ordinal += 1
                want += ordinal * old(stack_word(frm[0], frm[1], max_regs, k, old_col))
            assert s == want & ((1 << 64) - 1), (frm, to, old_col, new_col)
            live += ordinal
        assert v[0] == live  # the live prefixes and nothing else


def test_the_step_count_of_the_counting_loop():
    """counting_loop(n) of tests/test_gpu_brillig_limits.py runs 4 n + 6 steps by the Python VM, a padded one 4 n + 6 + pad: the step budgets of
    tests/test_gpu_brillig_resume.py stand on it"""
    import brillig_ref
    from brillig_steps import count_steps, loop_of, padded_loop
    from test_gpu_brillig_limits import counting_loop
    for n in (0, 1, 10, 63):
        assert count_steps(counting_loop(), {1: n}) [1] == 4 * n + 6
        for pad in (0, 1, 3):
            outcome, steps = count_steps(padded_loop(pad), {1: n})
            assert outcome.kind == brillig_ref.SOLVED and steps == 4 * n + 6 + pad
    for steps in (255, 256, 257, 1792, 4096, 4097):
        pad, n = loop_of(steps)
        assert count_steps(padded_loop(pad), {1: n})[1] == steps


def test_the_public_interface_names_the_feature():
    import acvm_amd
    assert "acvm_debug_brillig_resume_stats" in acvm_amd.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "acvm_amd.h")).read()
    assert "int acvm_debug_brillig_resume_stats(const acvm_batch_t *b, uint64_t out[6]);" in header
    tuning = open(os.path.join(ROOT, "acvm_amd", "csrc", "tuning.cpp")).read() + open(os.path.join(ROOT, "acvm_amd", "csrc", "tuning.hpp")).read()
    for key, default in (("brillig_resume", "0"), ("brillig_steps_total_log2", "32")):
        assert '{"%s", &Tuning::%s}' % (key, key) in tuning and "int64_t %s = %s;" % (key, default) in tuning
        assert "`%s`" % key in open(os.path.join(ROOT, "README.md")).read()
    assert hasattr(acvm_amd.Batch, "brillig_resume_stats")
