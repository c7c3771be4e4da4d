"""The decisions of the Brillig retry loop (acvm_amd/csrc/brillig_retry_plan.cpp) without a device and without a handle: the module is compiled as
plain C++ (tools/brillig_retry_plan_host_test.cpp), once as it is and once through `make asan`, and its answers -- who continues from a
checkpoint, who runs the opcode again, who is final with which limit, the next pass's limits, stride, columns and bytes, and what the relocation
copies -- are judged by the Python restatement below. With brillig_resume = 0 the restatement is the restart loop as it stood before the plan
existed, on the shapes tests/test_gpu_brillig_limits.py runs on the device."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tools", "brillig_retry_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "brillig_retry_plan.cpp")]
MEM, STEPS, DEPTH = 17, 18, 28
NONE = 0xFFFFFFFF
SKIP, CONTINUE, RESTART, FINAL = 0, 1, 2, 3
K_STEPS, K_DEPTH, K_MEMORY, K_DEVICE = 1, 2, 3, 4


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    """the tool compiled as it is, and the second binary of `make asan` (AddressSanitizer + UndefinedBehaviorSanitizer): a stand-alone program on
    the CPU, given the same command streams -- a report ends it with a non-zero status"""
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("brillig_retry_plan") / "brillig_retry_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + SOURCES + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "brillig_retry_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/brillig_retry_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def tune(resume=0, steps_max_log2=26, depth_max=1 << 16, mem_max_log2=22, total_log2=32):
    return dict(resume=resume, steps_max_log2=steps_max_log2, depth_max=depth_max, mem_max_log2=mem_max_log2, total_log2=total_log2)


def lane(msg=0, x0=0, opcode=0, record_cells=8, n_regs=6, prev_col=NONE, n_mem=0, n_cs=0, steps=0, ck_opcode=None, state=5):
    return dict(msg=msg, x0=x0, opcode=opcode, record_cells=record_cells, n_regs=n_regs, prev_col=prev_col, n_mem=n_mem, n_cs=n_cs, steps=steps,
                ck_opcode=opcode if ck_opcode is None else ck_opcode, state=state)


def command(tn, cur, compact, max_regs, lanes, refuse=False):
    head = "plan %d %d %d %d %d %d %d %d %d %d %d %d %d" % (refuse, tn["resume"], tn["steps_max_log2"], tn["depth_max"], tn["mem_max_log2"], tn["total_log2"],
                                                         cur["steps"], cur["depth"], cur["mem_cap"], cur["stride"], compact, max_regs, len(lanes))
    return head + "".join(" %d %d %d %d %d %d %d %d %d %d %d" % (l["msg"], l["x0"], l["opcode"], l["record_cells"], l["n_regs"], l["prev_col"], l["n_mem"], l["n_cs"],
                                                                  l["steps"], l["ck_opcode"], l["state"]) for l in lanes)


def parse(line, n):
    head, rest = line.split(" L")
    lanes_txt, reloc_txt = rest.split(" R")
    h = [int(x) for x in head.split()]
    lv = [int(x) for x in lanes_txt.split()]
    rv = [int(x) for x in reloc_txt.split()]
    assert len(lv) == 6 * n and len(rv) % 5 == 0
    return dict(n_retried=h[0], n_continued=h[1], n_restarted=h[2], steps=h[3], depth=h[4], mem_cap=h[5], stride=h[6], bytes=h[7], relocate=h[8], cells=h[9],
                lanes=[tuple(lv[6 * i:6 * i + 6]) for i in range(n)], reloc=[tuple(rv[5 * i:5 * i + 5]) for i in range(len(rv) // 5)])


def clamp(v, lo, hi):
    return min(max(v, lo), hi)


def model(tn, cur, compact, max_regs, lanes, refuse=False):
    """the restatement. resume = 0: the restart loop (every lane at a limit runs again with the limit raised, or is final at a stated maximum)"""
    max_steps = 1 << clamp(tn["steps_max_log2"], 0, 31)
    max_depth = clamp(tn["depth_max"], 1, 1 << 24)
    max_cells = 1 << clamp(tn["mem_max_log2"], 0, 30)
    total = 1 << clamp(tn["total_log2"], 0, 62)
    resume = tn["resume"] != 0
    out = [(SKIP, NONE, 0, 0, 0, 0)] * len(lanes)
    at_limit = [l for l in lanes if l["msg"] in (MEM, STEPS, DEPTH)]
    cur_cells = cur["mem_cap"] or max([l["record_cells"] for l in at_limit], default=0)
    retried, want = [], 0
    hit = set()
    for t, l in enumerate(lanes):
        if l["msg"] not in (MEM, STEPS, DEPTH):
            continue
        valid = (resume and compact and l["prev_col"] != NONE and l["prev_col"] < cur["stride"] and l["state"] == 5 and l["ck_opcode"] == l["opcode"]
                 and l["n_mem"] <= cur["mem_cap"] and l["n_cs"] <= cur["depth"])
        if l["msg"] == STEPS and ((valid and l["steps"] >= total) if resume else cur["steps"] >= max_steps):
            out[t] = (FINAL, NONE, K_STEPS, total if resume else max_steps, 0, 0)
            continue
        if l["msg"] == DEPTH and cur["depth"] >= max_depth:
            out[t] = (FINAL, NONE, K_DEPTH, max_depth, 0, 0)
            continue
        own = cur["mem_cap"] or l["record_cells"]
        if l["msg"] == MEM and (l["x0"] + 1 > max_cells or own >= max_cells):
            out[t] = (FINAL, NONE, K_MEMORY, max_cells, l["x0"], 0)
            continue
        out[t] = (CONTINUE if valid else RESTART, len(retried), 0, 0, 0, l["steps"] if valid else 0)
        retried.append(t)
        hit.add(l["msg"])
        if l["msg"] == MEM:
            want = max(want, l["x0"] + 1)
    res = dict(n_retried=len(retried), n_continued=sum(out[t][0] == CONTINUE for t in retried), n_restarted=sum(out[t][0] == RESTART for t in retried),
               steps=0, depth=0, mem_cap=0, stride=0, bytes=0, relocate=0, cells=0, lanes=out, reloc=[])
    if not retried:
        return res
    res["steps"] = min(cur["steps"] * 16, max_steps) if STEPS in hit else cur["steps"]
    res["depth"] = min(cur["depth"] * 16, max_depth) if DEPTH in hit else cur["depth"]
    cells = max(cur_cells, 64)
    if MEM in hit:
        cells = min(max(2 * want, 4 * cells), max_cells)
    res["mem_cap"] = cells
    res["stride"] = (len(retried) + 63) // 64 * 64
    res["bytes"] = ((max_regs + cells) * 8 + res["depth"] + cells // 4 + 16) * res["stride"] * 4
    if refuse:
        res["lanes"] = [(FINAL, NONE, K_DEVICE, res["bytes"] >> 20, 0, 0) if o[0] in (CONTINUE, RESTART) else o for o in out]
        res.update(n_retried=0, n_continued=0, n_restarted=0)
        return res
    cont = [t for t in retried if out[t][0] == CONTINUE]
    if cont:
        moved = (res["stride"], res["mem_cap"], res["depth"]) != (cur["stride"], cur["mem_cap"], cur["depth"]) or any(out[t][1] != lanes[t]["prev_col"] for t in cont)
        if moved:
            res["relocate"] = 1
            res["reloc"] = [(lanes[t]["prev_col"], out[t][1], lanes[t]["n_regs"], lanes[t]["n_mem"], lanes[t]["n_cs"]) for t in cont]
            res["cells"] = sum(lanes[t]["n_mem"] for t in cont)
    return res


def check(tool, cases):
    lines = tool([command(*c[:5], **(c[5] if len(c) > 5 else {})) for c in cases])
    for line, c in zip(lines, cases):
        got, want = parse(line, len(c[4])), model(*c[:5], **(c[5] if len(c) > 5 else {}))
        assert got == want, (c, got, want)
    return [parse(line, len(c[4])) for line, c in zip(lines, cases)]


BASE = dict(steps=1 << 22, depth=64, mem_cap=0, stride=0)


def test_caps_are_clamped(tool):
    lines = tool(["caps 26 65536 22 0 32", "caps -3 0 99 7 99", "caps 40 %d -1 1 -5" % (1 << 30)])
    assert lines == ["%d 65536 %d %d 0" % (1 << 26, 1 << 22, 1 << 32), "1 1 %d %d 1" % (1 << 30, 1 << 62), "%d %d 1 1 1" % (1 << 31, 1 << 24)]


def test_resume_off_is_the_restart_loop_on_the_shapes_of_the_device_tests(tool):
    """store_far's rows (memory), counting_loop under steps 2^8 / 2^12 and 2^8 / 2^20, recursion under depth 64 / 128: pass after pass as the loop
    walks them, first from the class scratch, then from the compact one"""
    cases = []
    # memory: pointers 200 .. 300000 against an estimate of 8 cells, default maximum 2^22 and the lowered one 2^12
    for mem_max in (22, 12):
        tn = tune(mem_max_log2=mem_max)
        rows = [lane(MEM, x0=x) for x in (200, 1000, 5000, 70000, 300000, 100000)] + [lane()]
        cases.append((tn, BASE, False, 6, rows))
        for cap in (1 << 12, 1 << 18, 1 << 22):
            cases.append((tn, dict(BASE, mem_cap=cap, stride=64), True, 6, [lane(MEM, x0=x, prev_col=i) for i, x in enumerate((cap, 2 * cap + 1, 300000))]))
    # steps: 2^8 -> 2^12 and then final; 2^8 -> 2^20
    for steps_max in (12, 20):
        tn = tune(steps_max_log2=steps_max)
        for steps in (1 << 8, 1 << 12, 1 << 16, 1 << 20):
            cases.append((tn, dict(BASE, steps=steps, stride=64 if steps > 256 else 0, mem_cap=64 if steps > 256 else 0), steps > 256, 4, [lane(STEPS), lane(), lane(STEPS)]))
    # depth: 64 -> 128 (maximum) -> final; 64 -> 1024 -> 16384 -> 65536
    for depth_max in (128, 1 << 16):
        tn = tune(depth_max=depth_max)
        for depth in (64, 128, 1024, 16384, 65536):
            cases.append((tn, dict(BASE, depth=depth, stride=64 if depth > 64 else 0, mem_cap=64 if depth > 64 else 0), depth > 64, 5, [lane(DEPTH), lane(DEPTH, opcode=1)]))
    got = check(tool, cases)
    assert all(g["n_continued"] == 0 and g["relocate"] == 0 for g in got)
    # (the figures the device tests assert: aux1 of the lanes that are given up)
    assert got[4]["lanes"][5][:5] == (FINAL, NONE, K_MEMORY, 1 << 12, 100000)
    assert any(g["lanes"][0][:4] == (FINAL, NONE, K_STEPS, 1 << 12) for g in got) and any(g["lanes"][0][:4] == (FINAL, NONE, K_DEPTH, 128) for g in got)


def test_the_slice_schedule_and_the_total(tool):
    """under resume a pass is a slice: it grows 16-fold up to 2^steps_max_log2 and stays there; the run ends when the steps behind a lane reach the
    total -- below it the lane continues, at and above it the lane is final with the total as its limit"""
    tn = tune(resume=1, steps_max_log2=8, total_log2=16)
    cur = dict(steps=64, depth=4, mem_cap=64, stride=64)
    first = check(tool, [(tn, dict(steps=64, depth=4, mem_cap=0, stride=0), False, 4, [lane(STEPS)])])[0]
    assert first["lanes"][0][0] == RESTART and first["steps"] == 256  # (64 * 16 cut at the slice)
    total, slice_ = 1 << 16, 256
    cases = [(tn, dict(cur, steps=slice_), True, 4, [lane(STEPS, prev_col=0, n_mem=3, n_cs=1, steps=done)]) for done in (total - slice_ - 1, total - slice_, total - 1, total, total + 1)]
    got = check(tool, cases)
    assert [g["lanes"][0][0] for g in got] == [CONTINUE, CONTINUE, CONTINUE, FINAL, FINAL]
    assert all(g["steps"] == slice_ and g["relocate"] == 0 for g in got[:3])  # the slice stays, nothing moves: no launch
    assert got[3]["lanes"][0][2:4] == (K_STEPS, total)
    # a total above 2^32: the limit is reported as it is (the result word saturates it)
    got = check(tool, [(tune(resume=1, total_log2=40), dict(cur, steps=1 << 26), True, 4, [lane(STEPS, prev_col=0, steps=1 << 40)])])
    assert got[0]["lanes"][0][2:4] == (K_STEPS, 1 << 40)


def test_all_three_limits_in_one_pass(tool):
    tn = tune(resume=1, steps_max_log2=10, depth_max=256, mem_max_log2=12)
    cur = dict(steps=256, depth=16, mem_cap=128, stride=64)
    lanes = [lane(STEPS, prev_col=0, n_mem=5, n_cs=2, steps=700), lane(DEPTH, prev_col=1, n_mem=0, n_cs=16, steps=90), lane(MEM, x0=300, prev_col=2, n_mem=128, n_cs=0, steps=40),
             lane(), lane(MEM, x0=5000, prev_col=3, n_mem=9, steps=1), lane(STEPS, prev_col=NONE), lane(MEM, x0=200, prev_col=5, state=0),
             lane(DEPTH, prev_col=6, ck_opcode=7), lane(DEPTH, prev_col=7, n_cs=17), lane(MEM, x0=130, prev_col=64)]
    g = check(tool, [(tn, cur, True, 9, lanes)])[0]
    assert [l[0] for l in g["lanes"]] == [CONTINUE, CONTINUE, CONTINUE, SKIP, FINAL, RESTART, RESTART, RESTART, RESTART, RESTART]
    assert (g["steps"], g["depth"], g["mem_cap"], g["stride"]) == (1024, 256, 602, 64)
    assert g["relocate"] == 1 and g["cells"] == 5 + 0 + 128 and g["reloc"] == [(0, 0, 6, 5, 2), (1, 1, 6, 0, 16), (2, 2, 6, 128, 0)]
    # the same pass with maxima already reached: depth and memory lanes are final, the step lane goes on
    g = check(tool, [(tune(resume=1, steps_max_log2=8, depth_max=16, mem_max_log2=7), cur, True, 9, lanes[:3])])[0]
    assert [l[0] for l in g["lanes"]] == [CONTINUE, FINAL, FINAL] and g["relocate"] == 0


@pytest.mark.parametrize("n", [63, 64, 65])
def test_lanes_around_a_stride(tool, n):
    """n continuing lanes: the stride is n rounded up to 64; one lane more finishes and the columns behind it move down"""
    tn = tune(resume=1, steps_max_log2=8, total_log2=20)
    cur = dict(steps=256, depth=8, mem_cap=64, stride=(n + 1 + 63) // 64 * 64)
    lanes = [lane(STEPS, prev_col=i, n_mem=i % 7, n_cs=i % 3, steps=1000 + i) for i in range(n + 1)]
    g = check(tool, [(tn, cur, True, 4, lanes)])[0]
    assert g["relocate"] == 0 and g["n_continued"] == n + 1
    lanes[10] = lane()  # it finished
    g = check(tool, [(tn, cur, True, 4, lanes)])[0]
    assert g["stride"] == (n + 63) // 64 * 64 and g["relocate"] == 1 and len(g["reloc"]) == n
    assert [r[:2] for r in g["reloc"]] == [(i, i if i < 10 else i - 1) for i in range(n + 1) if i != 10]
    assert g["cells"] == sum(i % 7 for i in range(n + 1) if i != 10)


def test_a_want_above_the_maximum_and_a_refused_allocation(tool):
    tn = tune(resume=1, mem_max_log2=10)
    cur = dict(steps=256, depth=8, mem_cap=256, stride=64)
    lanes = [lane(MEM, x0=1023, prev_col=0, n_mem=200), lane(MEM, x0=1024, prev_col=1, n_mem=17), lane(MEM, x0=0xFFFFFFFF, prev_col=2)]
    g = check(tool, [(tn, cur, True, 4, lanes)])[0]
    assert [l[0] for l in g["lanes"]] == [CONTINUE, FINAL, FINAL] and g["lanes"][1][2:5] == (K_MEMORY, 1024, 1024) and g["mem_cap"] == 1024
    g = check(tool, [(tn, cur, True, 4, lanes, dict(refuse=True))])[0]
    assert [l[2] for l in g["lanes"]] == [K_DEVICE, K_MEMORY, K_MEMORY] and g["n_retried"] == 0 and g["reloc"] == []
    assert g["lanes"][0][3] == g["bytes"] >> 20


def test_random_passes(tool):
    rng = random.Random(20240611)
    cases = []
    for _ in range(400):
        resume = rng.random() < 0.7
        tn = tune(resume=int(resume), steps_max_log2=rng.choice([6, 8, 12, 26]), depth_max=rng.choice([8, 64, 1 << 16]), mem_max_log2=rng.choice([6, 8, 12, 22]),
                  total_log2=rng.choice([4, 10, 16, 32]))
        compact = rng.random() < 0.8
        n = rng.choice([1, 2, 5, 64, 70])
        cur = dict(steps=1 << rng.choice([4, 6, 8, 12]), depth=rng.choice([4, 8, 64, 1 << 16]), mem_cap=rng.choice([64, 256, 4096]) if compact else 0,
                   stride=(n + 63) // 64 * 64 if compact else 0)
        lanes = []
        for i in range(n):
            lanes.append(lane(msg=rng.choice([0, MEM, STEPS, DEPTH, DEPTH, STEPS, MEM, 5]), x0=rng.choice([0, 63, 64, 300, 5000, 1 << 22]), opcode=rng.randrange(3),
                              record_cells=rng.choice([0, 8, 100]), n_regs=rng.randrange(1, 9), prev_col=i if compact and rng.random() < 0.8 else NONE,
                              n_mem=rng.choice([0, 1, 64, 65, 4096, 4097]), n_cs=rng.choice([0, 3, 4, 5, 64]), steps=rng.choice([0, 15, 16, 1023, 1024, 1 << 16, 1 << 33]),
                              ck_opcode=rng.randrange(3), state=rng.choice([5, 5, 5, 0, 1])))
        cases.append((tn, cur, compact, rng.randrange(1, 12), lanes, dict(refuse=rng.random() < 0.1)))
    check(tool, cases)
