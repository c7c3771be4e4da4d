"""brillig_resume = 1: a lane of the exact path that reaches a device limit of the Brillig VM is CONTINUED from a checkpoint in the next pass, not
started over (csrc/brillig_resume.hpp, csrc/brillig_retry_plan.cpp, csrc/kernels_brillig_resume.hip). The expected results are the oracle's, which
has no limits; the limits are forced small so that a program crosses them several times within a few thousand steps; and the statistics of
acvm_debug_brillig_resume_stats prove that the lanes were continued -- passes, lanes continued and restarted, cells relocated, steps executed --
not merely that the outcomes agree. Step counts come from tests/brillig_steps.py (the Python VM with a counter)."""
import pytest

import acvm_amd
from acvm_amd.acir import Brillig, Circuit, Expression as E
from acvm_amd.synth import values_from_rows
from brillig_steps import count_steps, loop_of, padded_loop
from test_gpu_brillig_limits import others_survive, recursion
from test_gpu_opcodes import run_both

pytestmark = pytest.mark.gpu
W = E.from_witness
SLICE_LOG2 = 8
SLICE = 1 << SLICE_LOG2
SMALL = dict(brillig_resume=1, brillig_steps_log2=6, brillig_steps_max_log2=SLICE_LOG2, brillig_steps_total_log2=16)


def solve_checked(oracle, circ, ids, rows, force_slow=False):
    """run_both of tests/test_gpu_opcodes.py -- every result word, message, assigned set and witness value against the oracle. run_both frees its
    handle, so the handle's resume statistics and results are read as it is freed; the call stacks, which run_both does not compare, are compared
    here frame by frame"""
    seen = {}
    free = acvm_amd.Batch.free

    def free_after_reading(batch):
        seen.update(stats=batch.brillig_resume_stats(), results=batch.results())
        free(batch)

    acvm_amd.Batch.free = free_after_reading
    try:
        ores, stats = run_both(oracle, circ, ids, rows, force_slow=force_slow)
    finally:
        acvm_amd.Batch.free = free
    for j, (g, o) in enumerate(zip(seen["results"], ores)):
        assert list(g.call_stack[:g.n_call_stack]) == list(o.call_stack[:o.n_call_stack]), (j, force_slow)
    return ores, dict(seen["stats"], retries=stats["n_brillig_retries"])


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_programs_longer_than_a_slice_are_continued(oracle, delta):
    """m S - 1, m S, m S + 1 steps for the slice S = 2^8 and m = 1, 2, 7: all longer than the first value, two of three longer than
    2^brillig_steps_max_log2 -- solved as the oracle solves them, continued and not started over"""
    counts = [m * SLICE + delta for m in (1, 2, 7)]
    pad = loop_of(counts[0])[0]
    assert all(loop_of(c)[0] == pad for c in counts)  # (S is a multiple of 4: one program serves the three lengths)
    circ = Circuit(3, [padded_loop(pad), E([], [(1, 2), (-1, 3)], 0)])
    rows = [[loop_of(c)[1]] for c in counts] + [[2]]  # and one that never reaches a limit
    for j, c in enumerate(counts):
        assert count_steps(padded_loop(pad), {1: rows[j][0]})[1] == c
    with acvm_amd.tuning(**SMALL):
        for force in (False, True):
            ores, st = solve_checked(oracle, circ, [1], rows, force)
            assert all(r.status == 0 for r in ores)
            assert st["lanes_continued"] > 0 and st["lanes_restarted"] <= 3, st  # at most one restart per lane
            # the compact passes ran every program from its start, once: its own count, and the base passes (2^6 steps each) are not among them
            assert sum(counts) <= st["steps_executed"] <= sum(counts) + 3 * 64, st
            assert st["passes"] == st["retries"] >= 7, st  # the longest program alone takes seven slices


def test_the_total_budget_ends_one_instance(oracle):
    """exactly 2^total steps are solved; one step more is ACVM_ERR_DEVICE_LIMIT / STEPS with aux1 = 2^total for that instance alone"""
    total_log2 = 12
    total = 1 << total_log2
    pad, n = loop_of(total)
    assert loop_of(total + 4)[0] == pad
    circ = Circuit(3, [padded_loop(pad), E([], [(1, 2), (-1, 3)], 0)])
    assert count_steps(padded_loop(pad), {1: n})[1] == total and count_steps(padded_loop(pad), {1: n + 1})[1] == total + 4
    limits = dict(SMALL, brillig_steps_total_log2=total_log2)
    with acvm_amd.tuning(**limits):
        ores, st = solve_checked(oracle, circ, [1], [[n], [5], [n - 1]])
        assert all(r.status == 0 for r in ores) and st["lanes_continued"] >= 2 * (total // SLICE - 1)
    r = others_survive(oracle, circ, [1], [[n], [n + 1], [5], [0]], over=1, kind=acvm_amd.LIMIT_BRILLIG_STEPS, **limits)
    assert r.aux1 == total
    # 2^total + 1 steps exactly: one more Const behind the loop
    circ1 = Circuit(3, [padded_loop(pad + 1), E([], [(1, 2), (-1, 3)], 0)])
    assert count_steps(padded_loop(pad + 1), {1: n})[1] == total + 1
    r = others_survive(oracle, circ1, [1], [[n - 1], [n], [5]], over=1, kind=acvm_amd.LIMIT_BRILLIG_STEPS, **limits)
    assert r.aux1 == total


def trapping_recursion():
    # f(n): if n == 0 trap; if n == 2: mem[w2] = 1; n -= 1; call f   -- traps at call depth n + 1; the store happens with n - 1 frames on the stack
    bc = [("Const", 2, 0), ("Const", 3, 1), ("Const", 5, 2),
          ("Call", 5), ("Stop",),
          ("BinaryFieldOp", 4, "Equals", 0, 2), ("JumpIf", 4, 13),
          ("BinaryFieldOp", 4, "Equals", 0, 5), ("JumpIfNot", 4, 10),
          ("Store", 1, 3),
          ("BinaryFieldOp", 0, "Sub", 0, 3), ("Call", 5), ("Return",),
          ("Trap",)]
    return Brillig(inputs=[W(1), W(2)], outputs=[3], bytecode=bc)


def test_call_depth_is_continued_and_returns_read_the_relocated_stack(oracle):
    circ = Circuit(3, [recursion(), E([], [(1, 2), (-1, 3)], 0)])
    rows = [[n] for n in (3, 4, 5, 63, 64)]
    with acvm_amd.tuning(brillig_resume=1, brillig_call_depth=4):
        ores, st = solve_checked(oracle, circ, [1], rows)
        assert all(r.status == 0 for r in ores)
        # depth 4 -> 64 (the restart of n = 4, 5, 63, 64; n = 3 fits) -> 1024: the lane of depth 65 continues, and its returns walk the relocated stack down
        assert st["lanes_continued"] == 1 and st["lanes_restarted"] == 4 and st["relocation_launches"] == 1 and st["cells_relocated"] == 0, st
        solve_checked(oracle, circ, [1], rows, force_slow=True)
    # Traps behind two relocations; solve_checked compares every lane's call stack with the oracle's, frame by frame. From a depth of 1 all three
    # lanes restart at their second call (depth 16, 66 cells). Lane 0 traps at depth 20: it stops at its 17th call (relocation 1: depth 256, 16
    # frames move), then with 18 frames on the stack at its store to cell 300 (relocation 2: 602 cells), and traps in the pass after. Lane 1 traps
    # at depth 301: it stops at depth 16 and at depth 256 (depth 4096 with relocation 2), its store fits. Lane 2 traps at depth 3 in the restart pass.
    circ = Circuit(3, [trapping_recursion()])
    with acvm_amd.tuning(brillig_resume=1, brillig_call_depth=1, brillig_mem_cells=64):
        ores, st = solve_checked(oracle, circ, [1, 2], [[19, 300], [300, 300], [2, 10]])
        assert all(r.err == oracle.E_BRILLIG_FAILED for r in ores)
        assert (st["lanes_restarted"], st["lanes_continued"], st["relocation_launches"], st["cells_relocated"]) == (3, 4, 2, 0), st
        assert list(ores[0].call_stack[:ores[0].n_call_stack]) == [3] + [11] * 14 + [13]  # (the result keeps the first 15 frames and the failing pc)
        assert list(ores[2].call_stack[:ores[2].n_call_stack]) == [3, 11, 11, 13]
        solve_checked(oracle, circ, [1, 2], [[19, 300]], force_slow=True)
    # past brillig_call_depth_max the instance is still given up
    circ = Circuit(3, [recursion(), E([], [(1, 2), (-1, 3)], 0)])
    r = others_survive(oracle, circ, [1], [[100], [500], [3], [90]], over=1, kind=acvm_amd.LIMIT_BRILLIG_CALL_DEPTH, brillig_resume=1, brillig_call_depth=4,
                       brillig_call_depth_max=128)
    assert r.aux1 == 128


K = 40


def memory_program():
    """cells 0..K get distinct values, then two stores far past the capacity (w1 < w2), then cells 0 and K, the zero fill below both far cells and
    the far cells are read back into six outputs"""
    bc = [("Const", 2, 0), ("Const", 3, 1), ("Const", 4, K + 1), ("Const", 5, 70000),
          ("BinaryFieldOp", 6, "Add", 2, 5), ("Store", 2, 6),                      # 4, 5: mem[i] = i + 70000
          ("BinaryFieldOp", 2, "Add", 2, 3), ("BinaryFieldOp", 7, "Equals", 2, 4), ("JumpIfNot", 7, 4),
          ("Store", 0, 5), ("Store", 1, 6),                                        # mem[w1] = 70000, mem[w2] = K + 70000
          ("Const", 8, 0), ("Load", 10, 8), ("Const", 8, K), ("Load", 11, 8),
          ("BinaryFieldOp", 8, "Sub", 0, 3), ("Load", 12, 8), ("Load", 13, 0),
          ("BinaryFieldOp", 8, "Sub", 1, 3), ("Load", 14, 8), ("Load", 15, 1),
          ("Mov", 0, 10), ("Mov", 1, 11), ("Mov", 2, 12), ("Mov", 3, 13), ("Mov", 4, 14), ("Mov", 5, 15), ("Stop",)]
    return Brillig(inputs=[W(1), W(2)], outputs=[3, 4, 5, 6, 7, 8], bytecode=bc)


def test_memory_is_relocated_with_its_live_prefix_only(oracle):
    """the capacity is crossed twice: the first far store restarts the lane in the compact scratch (602 cells for cell 300: twice the cell wanted,
    and more than four times the planner's estimate of 64 + K + 1 cells -- a constant below 2^16 counts as a pointer there, which is why the
    programs of this file take their pointers from witnesses), the second one continues it -- and the relocation copies the 301 live cells, not
    the 602 of the capacity"""
    circ = Circuit(8, [memory_program()])
    with acvm_amd.tuning(brillig_resume=1, brillig_mem_cells=64):
        ores, st = solve_checked(oracle, circ, [1, 2], [[300, 5000]])
        assert ores[0].status == 0
        assert (st["lanes_restarted"], st["lanes_continued"], st["relocation_launches"], st["cells_relocated"]) == (1, 1, 1, 301), st
        ores, st = solve_checked(oracle, circ, [1, 2], [[300, 5000], [110, 200], [350, 7000], [50, 60]], force_slow=True)
        assert all(r.status == 0 for r in ores)
        # lanes 0 and 2 stop at their second store in the first compact pass (capacity 702, lane 1 fits there, lane 3 never left its estimate):
        # 301 + 351 live cells move
        assert (st["lanes_restarted"], st["lanes_continued"], st["cells_relocated"]) == (3, 2, 301 + 351), st


FAR = 400
CAP = 2 * (FAR + 1)  # the compact scratch's capacity after a store to cell FAR: twice the cell wanted (four times an estimate of 64 + 64 + 64 + a size is less)


def overlapping_hash(name):
    """mem[FAR] = w2 puts the lane into the compact scratch; mem[CAP - 1] = w2 makes all of its cells live; the message is cells [CAP - 32, CAP)
    and the digest goes to cell w3 -- CAP - 5: INSIDE its own message and across the capacity. Inputs: FAR, a byte, w3, CAP - 1, CAP - 27, CAP - 32"""
    bc = [("Store", 0, 1), ("Store", 3, 1), ("Store", 4, 1), ("Const", 6, 32),
          ("BlackBox", name, 5, 6, 2, 32), ("Mov", 0, 2), ("Stop",)]
    return Brillig(inputs=[W(w) for w in range(1, 7)], outputs=[list(range(7, 39))], bytecode=bc)


@pytest.mark.parametrize("name", ["Sha256", "Blake2s", "Keccak256"])
def test_a_digest_across_the_capacity_leaves_its_message_alone(oracle, name):
    circ = Circuit(38, [overlapping_hash(name)])
    ids, tail = list(range(1, 7)), [CAP - 1, CAP - 27, CAP - 32]
    with acvm_amd.tuning(brillig_resume=1, brillig_mem_cells=64):
        ores, st = solve_checked(oracle, circ, ids, [[FAR, 0xAB, CAP - 5] + tail, [FAR, 0x17, CAP - 32] + tail, [FAR, 0x99, CAP - 4] + tail])
        assert all(r.status == 0 for r in ores)
        # (the digest at CAP - 32 fits; the other two lanes stopped before their first write with all CAP cells live)
        assert st["lanes_restarted"] == 3 and st["lanes_continued"] == 2 and st["cells_relocated"] == 2 * CAP, st
        solve_checked(oracle, circ, ids, [[FAR, 0xAB, CAP - 5] + tail], force_slow=True)


def test_curve_outputs_across_the_capacity(oracle):
    """Pedersen whose two inputs are cells [CAP - 2, CAP) and whose output pair starts at cell CAP - 1; FixedBaseScalarMul at the same place.
    Inputs: FAR, a value, the output pointer, CAP - 2, CAP - 1"""
    ins = [W(w) for w in range(1, 6)]
    ped = Brillig(inputs=ins, outputs=[[6, 7]],
                  bytecode=[("Store", 0, 1), ("Store", 3, 1), ("Store", 4, 1), ("Const", 5, 2), ("Const", 6, 0),
                            ("BlackBox", "Pedersen", 3, 5, 6, 2, 2), ("Mov", 0, 2), ("Stop",)])
    fixed = Brillig(inputs=ins, outputs=[[6, 7]],
                    bytecode=[("Store", 0, 1), ("Const", 5, 0), ("BlackBox", "FixedBaseScalarMul", 1, 5, 2, 2), ("Mov", 0, 2), ("Stop",)])
    with acvm_amd.tuning(brillig_resume=1, brillig_mem_cells=64):
        for br, live in ((ped, CAP), (fixed, FAR + 1)):
            ores, st = solve_checked(oracle, Circuit(7, [br]), [1, 2, 3, 4, 5], [[FAR, 12345, CAP - 1, CAP - 2, CAP - 1], [FAR, 777, 20, CAP - 2, CAP - 1]])
            assert all(r.status == 0 for r in ores)
            assert st["lanes_continued"] == 1 and st["cells_relocated"] == live, st  # (nothing of the pair was written when the lane stopped)


def test_foreign_call_results_across_the_capacity(oracle):
    """results carried by the circuit: a vector destination that crosses the capacity behind a register destination; and destination 0's written
    register is destination 1's pointer -- the sizing walk reads it through the write. Nothing of the instruction is written before the lane
    stops: the live prefix that is relocated is the FAR + 1 cells of before. Inputs: FAR, a value, a pointer"""
    ins = [W(1), W(2), W(3)]
    vec = Brillig(inputs=ins, outputs=[4, [5, 6, 7, 8]],
                  bytecode=[("Store", 0, 1),
                            ("ForeignCall", "f", [("Register", 6), ("HeapVector", 2, 4)], [("Register", 1)]),  # (destinations, then inputs)
                            ("BinaryFieldOp", 0, "Add", 6, 4), ("Mov", 1, 2), ("Stop",)],
                  foreign_call_results=[[41, [1, 2, 3, 4]]])
    alias = Brillig(inputs=ins, outputs=[4, [5, 6, 7]],
                    bytecode=[("Store", 0, 1), ("Mov", 5, 2),
                              ("ForeignCall", "g", [("Register", 5), ("HeapArray", 5, 3)], [("Register", 1)]),
                              ("Mov", 0, 5), ("Mov", 1, 5), ("Stop",)],
                    foreign_call_results=[[CAP - 2, [9, 8, 7]]])
    with acvm_amd.tuning(brillig_resume=1, brillig_mem_cells=64):
        # (vec: the vector goes to cells [CAP - 3, CAP + 1); alias: register 5 holds 7 before the call and CAP - 2 behind destination 0)
        for br, n, ptr in ((vec, 8, CAP - 3), (alias, 7, 7)):
            ores, st = solve_checked(oracle, Circuit(n, [br]), [1, 2, 3], [[FAR, 5, ptr], [FAR, 6, ptr]])
            assert all(r.status == 0 for r in ores) and st["lanes_continued"] == 2 and st["cells_relocated"] == 2 * (FAR + 1), st
            solve_checked(oracle, Circuit(n, [br]), [1, 2, 3], [[FAR, 5, ptr]], force_slow=True)


def test_a_pending_call_behind_a_continuation(oracle):
    """the loop crosses the slice, then the program waits for an answer; the answered opcode runs again from its start (ACVM::solve after
    resolve_pending_foreign_call) and is continued again -- no checkpoint of the first run is picked up"""
    bc = [("Const", 1, 0), ("Const", 2, 1),
          ("BinaryFieldOp", 3, "Equals", 1, 0), ("JumpIf", 3, 6),
          ("BinaryFieldOp", 1, "Add", 1, 2), ("Jump", 2),
          ("ForeignCall", "h", [("Register", 4)], [("Register", 1)]),  # (destinations, then inputs)
          ("BinaryFieldOp", 0, "Add", 1, 4), ("Stop",)]
    circ = Circuit(2, [Brillig(inputs=[W(1)], outputs=[2], bytecode=bc)])
    data, rows = circ.to_bytes(), [[200], [3], [450]]
    with acvm_amd.tuning(**SMALL):
        batch = acvm_amd.Batch(acvm_amd.Circuit(data), len(rows), [1])
        batch.set_initial_witness(values_from_rows(rows))
        assert batch.solve() == 3
        first = batch.brillig_resume_stats()
        assert [r.status for r in batch.results()] == [acvm_amd.STATUS_REQUIRES_FOREIGN_CALL] * 3 and first["lanes_continued"] >= 3 + 7
        for j in range(3):
            fn, inputs = batch.get_pending_foreign_call(j)
            assert fn == "h" and inputs == [[rows[j][0]]]
            batch.resolve_pending_foreign_call(j, [1000 + j])
        assert batch.solve() == 0
        # the answered opcodes ran again from their first instruction -- the two long lanes left the class scratch by a restart once more, the
        # third never reaches a limit -- and were continued again as often as before: no record of the first run was picked up
        second = batch.brillig_resume_stats()
        assert second["lanes_restarted"] == 2 and second["lanes_continued"] == first["lanes_continued"] == 3 + 7, (first, second)
        asg, vals = batch.witness_map()
        assert [int.from_bytes(vals[j, 2].tobytes(), "big") for j in range(3)] == [rows[j][0] + 1000 + j for j in range(3)]
        batch.free()
    for j in range(3):  # (the oracle, one instance at a time)
        a = oracle.ACVM(oracle.Circuit(data), {1: rows[j][0]})
        assert a.solve() == oracle.ST_REQUIRES_FOREIGN_CALL
        a.resolve_pending_foreign_call([1000 + j])
        assert a.solve() == oracle.ST_SOLVED and a.witness_map()[2] == rows[j][0] + 1000 + j


def test_65_lanes_finish_pass_by_pass(oracle):
    """65 lanes with different loop counts: some finish in every pass, so the stride falls from 128 to 64 and the columns move; and two Brillig
    opcodes with different register counts in one circuit, the second one reaching its limit in the pass in which the first finished"""
    second = Brillig(inputs=[W(2)], outputs=[3], bytecode=[("Const", 9, 3)] + [("Const", 1, 0), ("Const", 2, 1),
                                                              ("BinaryFieldOp", 3, "Equals", 1, 0), ("JumpIf", 3, 7),
                                                              ("BinaryFieldOp", 1, "Add", 1, 2), ("Jump", 3),
                                                              ("BinaryFieldOp", 0, "Add", 1, 9), ("Stop",)])
    circ = Circuit(3, [padded_loop(0), second])
    rows = [[20 + 9 * j] for j in range(65)]  # 86 .. 2 390 steps in the first opcode, as many again in the second
    with acvm_amd.tuning(**SMALL):
        ores, st = solve_checked(oracle, circ, [1], rows)
        assert all(r.status == 0 for r in ores)
        assert st["lanes_continued"] > 65 and st["relocation_launches"] >= 2 and st["lanes_restarted"] <= 2 * 65, st
        solve_checked(oracle, circ, [1], rows[::8], force_slow=True)


def test_stepping_one_handle_three_times_and_the_node_driver(oracle):
    circ = Circuit(5, [memory_program_small(), recursion(out=4), E([], [(1, 3), (1, 4), (-1, 5)], 0)])
    rows = [[70, 5], [300, 6], [2, 7]]
    data, values = circ.to_bytes(), values_from_rows(rows)
    ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), [1, 2], values, len(rows))
    with acvm_amd.tuning(brillig_resume=1, brillig_call_depth=4, brillig_mem_cells=64):
        # acvm_batch_solve_opcode: the continuation happens inside the step that executes the opcode
        batch = acvm_amd.Batch(acvm_amd.Circuit(data), len(rows), [1, 2])
        batch.set_initial_witness(values)
        for _ in range(3):
            batch.solve_opcode()
        assert all(r.status == 0 for r in batch.results())
        asg, vals = batch.witness_map()
        assert (asg == oasg[:, :asg.shape[1]]).all() and (vals == ovals[:, :vals.shape[1]]).all()
        assert batch.brillig_resume_stats()["lanes_continued"] >= 2
        batch.free()
        # one handle, three solves: the same statistics every time -- a record of an earlier solve is never picked up
        batch = acvm_amd.Batch(acvm_amd.Circuit(data), len(rows), [1, 2])
        seen = []
        for _ in range(3):
            batch.set_initial_witness(values)
            assert batch.solve() == 0
            asg, vals = batch.witness_map()
            assert (asg == oasg[:, :asg.shape[1]]).all() and (vals == ovals[:, :vals.shape[1]]).all()
            seen.append(batch.brillig_resume_stats())
        assert seen[0] == seen[1] == seen[2] and seen[0]["lanes_continued"] >= 2, seen
        batch.free()
        # the node driver, two lanes on device 0 and tiles of 64: the exact path runs beside the next tile
        many = [[5 + (j % 40), j + 1] for j in range(200)]
        many[77], many[140] = [300, 9], [70, 3]
        mdata = values_from_rows(many)
        mres, masg, mvals = oracle.solve_batch(oracle.Circuit(data), [1, 2], mdata, len(many))
        node = acvm_amd.Node(acvm_amd.Circuit(data), [1, 2], keep=[5], devices=[0, 0], tile=64)
        not_solved, res, kept, asg, dig = node.solve(mdata, len(many))
        node.free()
        assert not_solved == 0
        for j in range(len(many)):
            assert res[j].as_tuple() == mres[j].as_tuple() and asg[j, 0] == 1 and bytes(kept[j, 0]) == bytes(mvals[j][5])


def memory_program_small():
    """store_far of tests/test_gpu_brillig_limits.py with a second far store at three times the pointer: the capacity is crossed twice"""
    bc = [("Store", 0, 1), ("BinaryFieldOp", 6, "Add", 0, 0), ("BinaryFieldOp", 6, "Add", 6, 0), ("Store", 6, 1),
          ("Const", 2, 1), ("BinaryFieldOp", 3, "Sub", 0, 2), ("Load", 4, 3), ("Load", 5, 6),
          ("BinaryFieldOp", 0, "Add", 4, 5), ("Stop",)]
    return Brillig(inputs=[W(1), W(2)], outputs=[3], bytecode=bc)


def test_resume_off_gives_todays_outcomes(oracle):
    """brillig_resume = 0 (the default): the same programs and limits, nobody continues, the statistics stay zero, and past
    2^brillig_steps_max_log2 steps the instance is given up as before -- with the slice as its limit, not the total"""
    pad, n = loop_of(7 * SLICE)
    circ = Circuit(3, [padded_loop(pad), E([], [(1, 2), (-1, 3)], 0)])
    limits = dict(SMALL, brillig_resume=0)
    r = others_survive(oracle, circ, [1], [[10], [n], [40], [0]], over=1, kind=acvm_amd.LIMIT_BRILLIG_STEPS, **limits)
    assert r.aux1 == SLICE
    with acvm_amd.tuning(brillig_resume=0, brillig_call_depth=4, brillig_mem_cells=64):
        ores, st = solve_checked(oracle, Circuit(3, [recursion(), E([], [(1, 2), (-1, 3)], 0)]), [1], [[n] for n in (3, 4, 5, 63, 64)])
        assert all(r.status == 0 for r in ores) and st["retries"] >= 2
        assert {k: v for k, v in st.items() if k != "retries"} == dict(passes=0, lanes_continued=0, lanes_restarted=0, cells_relocated=0, steps_executed=0, relocation_launches=0)
        ores, st = solve_checked(oracle, Circuit(8, [memory_program()]), [1, 2], [[300, 5000]])
        assert ores[0].status == 0 and st["passes"] == 0 and st["retries"] == 2
    assert acvm_amd.tuning_get("brillig_resume") == 0 and acvm_amd.tuning_get("brillig_steps_total_log2") == 32
