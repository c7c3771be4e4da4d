"""The case lists of tests/brillig_cases.py against the CPU oracle (oracle/brillig_vm.c, oracle/pwg.c): status, error kind, failing opcode, failure
text, call stack, pending foreign call and the whole witness map of every row must equal what the Python model of the reference (tests/brillig_ref.py)
expects, and the lists must cover what they are built to cover: every branch label of the model, every outcome kind and every failure text, each at
least twice. No GPU: tests/test_gpu_brillig_edges.py runs the same lists on the device.

Where model and oracle disagreed, the Rust decided:
  * the empty output array behind a register above u64 (acvm/src/pwg/brillig.rs:102-108: to_usize stands inside the loop over the witnesses): the
    ORACLE was wrong (it converted in front of the loop and panicked), and so was the device (op_brillig); both now convert inside the loop.
Where model and oracle agreed and the device did not (tests/test_gpu_brillig_edges.py), the DEVICE was wrong:
  * a foreign-call result of NO values into a HeapVector past the memory's end grows the memory (memory.rs:32-39); brillig_foreign_call wrote cell by
    cell and never grew it, so a Load inside the growth panicked. BrVm::mem_grow does it now. No other write_slice caller can carry zero values.
  * a pending foreign call whose input slice crosses the memory's end, or whose pointer or size is above u64, panics (lib.rs:198-202); the device set the
    waiting status before it resolved the inputs, which made BrVm::panic a no-op, and reported RequiresForeignCall. The status is set last now."""
import collections

import pytest

import brillig_cases as bc
import brillig_ref as br


def oracle_row(oracle, case, j, answers=()):
    """(status, err, opcode_index, message, witness map, call stack, pending) of one row through the oracle's single-instance handle, every pending
    call answered with the next of `answers`"""
    a = oracle.ACVM(oracle.Circuit(case.circuit.to_bytes()), dict(zip(case.ids, case.rows[j])))
    status = a.solve()
    for values in answers:
        if status != oracle.ST_REQUIRES_FOREIGN_CALL:
            break
        a.resolve_pending_foreign_call(values)
        status = a.solve()
    r = a.result()
    return (r.status, r.err, r.opcode_index, r.message, a.witness_map(), list(r.call_stack[:r.n_call_stack]), a.get_pending_foreign_call())


def oracle_rows(oracle, case, answers=None):
    return [oracle_row(oracle, case, j, answers(j) if answers else ()) for j in range(len(case.rows))]


def test_error_codes_are_the_oracles(oracle):
    assert (bc.ST_SOLVED, bc.ST_FAILURE, bc.ST_REQUIRES_FOREIGN_CALL) == (oracle.ST_SOLVED, oracle.ST_FAILURE, oracle.ST_REQUIRES_FOREIGN_CALL)
    assert (bc.E_NONE, bc.E_MISSING_ASSIGNMENT, bc.E_TOO_MANY_UNKNOWNS, bc.E_UNSATISFIED, bc.E_BRILLIG_FAILED, bc.E_PANIC) == (
        oracle.E_NONE, oracle.E_MISSING_ASSIGNMENT, oracle.E_TOO_MANY_UNKNOWNS, oracle.E_UNSATISFIED, oracle.E_BRILLIG_FAILED, oracle.E_PANIC)


@pytest.mark.parametrize("name", bc.NAMES)
def test_oracle_agrees_with_the_model(oracle, name):
    case = bc.case(name)
    bc.compare(case, oracle_rows(oracle, case), "oracle")


def test_oracle_agrees_behind_the_hosts_answers(oracle):
    case = bc.case("foreign call, answered by the host")
    assert all(x.kind == br.REQUIRES_FOREIGN_CALL for x in case.expect)
    expect = bc.answered_expect(case)
    bc.compare(case, oracle_rows(oracle, case, lambda j: [bc.answer_of(j)]), "oracle", expect)
    by_answer = collections.Counter((bc.ANSWERS.index(bc.answer_of(j)), x.kind) for j, x in enumerate(expect))
    assert all(by_answer[(k, br.SOLVED)] >= 2 and by_answer[(k, br.PANIC)] >= 2 for k in range(3)), by_answer
    assert sum(1 for x in expect if "write_zero_len_grows" in x.branches and x.kind == br.SOLVED) >= 2


def test_every_branch_outcome_and_message_is_reached_twice():
    """a condition on the lists, not a measurement: a label that no row reaches fails here"""
    cases = bc.all_cases()
    reached, kinds, messages = collections.Counter(), collections.Counter(), collections.Counter()
    for c in cases:
        for x in list(c.expect) + (bc.answered_expect(c) if c.name == "foreign call, answered by the host" else []):
            reached.update(x.branches)
            kinds[x.kind] += 1
            if x.kind == br.BRILLIG_FAILED:
                messages[br.message_class(x.message)] += 1
    assert len(set(br.LABELS)) == len(br.LABELS)
    assert not set(reached) - set(br.LABELS)
    missing = {label: reached[label] for label in br.LABELS if reached[label] < 2}
    assert not missing, f"branch labels reached by fewer than two rows: {missing}"
    assert all(kinds[k] >= 2 for k in br.KINDS), kinds
    assert set(messages) == set(br.MESSAGES) and all(n >= 2 for n in messages.values()), messages


def test_the_lists_hold_what_they_are_built_around():
    mem = bc.case("memory")
    stores, loads, bases = {r[4] for r in mem.rows}, {r[6] for r in mem.rows}, {r[7] for r in mem.rows}
    far = {bc.U32 - 1, bc.U32, bc.U64 - 1, bc.U64, bc.P - 1}
    assert stores >= {0, 3, 4, 5, bc.MEM_CAP_ESTIMATE - 1, bc.MEM_CAP_ESTIMATE, 1000} and max(stores) < 4096 and loads >= far | {0, 3, 4, 5} and bases >= far | {0, 1}
    # the output array crosses the end at element 0, 1 and 2, and the map holds what was inserted before the panic
    crossed = collections.Counter()
    for x in mem.expect:
        if "out_array_oob" in x.branches:
            crossed[sum(w in x.witnesses for w in (10, 11, 12))] += 1
            assert 9 in x.witnesses and x.kind == br.PANIC
    assert all(crossed[k] >= 2 for k in (0, 1, 2)), crossed
    # the gap behind a Store past the end reads zero
    assert sum(1 for r, x in zip(mem.rows, mem.expect) if "write_gap_zero_fill" in x.branches and x.kind == br.SOLVED and 4 <= r[6] < r[4] and x.witnesses[9] == 0) >= 3
    assert len(bc.case("registers").rows) <= 8
    trap = bc.case("trap at a call depth")
    assert {len(x.call_stack) - 1 for x in trap.expect} >= {0, 1, 14, 15, 16, 17}
    assert all(len(set(x.call_stack[:-1])) == 2 for x in trap.expect if len(x.call_stack) > 2)  # (frames differ: a cut at the wrong end shows)
    for kind in ("Jump", "JumpIf", "JumpIfNot", "Call"):
        c = bc.case(f"{kind} to every target")
        assert [op.bytecode[1][-1] for op in c.circuit.opcodes] == [3, 4, 5, bc.U32 - 1, bc.U32, bc.U64 - 1] and all(len(op.bytecode) == 4 for op in c.circuit.opcodes)
        assert {r[0] for r in c.rows} >= {0, 1, bc.P - 1, bc.U64} and all(x.kind == br.SOLVED for x in c.expect)
        assert bc.n_inlinable(c) == (0 if kind == "Call" else 6)
    # finding 2: the empty output array behind 2^70 solves, and the output behind it is assigned
    io = bc.case("inputs and outputs")
    assert io.rows[1][0] == 1 << 70 and io.expect[1].kind == br.SOLVED and io.expect[1].witnesses[16] == 3
    # finding 1: a vector of no values past the end grows the memory, and a Load inside the growth reads zero
    v0 = bc.case("foreign call, vector of 0")
    assert sum(1 for r, x in zip(v0.rows, v0.expect) if r[3] == 7 and x.kind == br.SOLVED and "write_zero_len_grows" in x.branches and 3 <= r[4] < 7 and x.witnesses[8] == 0) >= 2
    for n in (0, 1, 5):
        assert {r[3] for r in bc.case(f"foreign call, vector of {n}").rows} >= {1, 3, 7}
    pend = bc.case("foreign call, pending inputs")
    assert sum(1 for x in pend.expect if x.kind == br.REQUIRES_FOREIGN_CALL) >= 5 and sum(1 for x in pend.expect if x.kind == br.PANIC) >= 5
    loop = bc.case("foreign call in a loop")
    assert [x.kind for x in loop.expect[:3]] == [br.SOLVED, br.SOLVED, br.REQUIRES_FOREIGN_CALL] and loop.expect[1].witnesses[4] == 30 and loop.expect[2].pending == ("next", [[1], [30]])
    # an unequal size or count in the middle fails the VM, as the last instruction it finishes it; earlier destinations are written, later ones not
    mid, last = bc.case("foreign call, array too long, in the middle"), bc.case("foreign call, array too long, last")
    assert all(x.kind == br.BRILLIG_FAILED and x.message == br.MSG_FC_SIZE and x.call_stack == [0] for x in mid.expect)
    assert all(x.kind == br.SOLVED and (x.witnesses[9], x.witnesses[10]) == (11, 0) and [x.witnesses[w] for w in (4, 5, 6, 7)] == [51, 52, 0, 0] for x in last.expect)
    for h in bc.HASHES:
        c = bc.case(f"black box {h}")
        assert sum(1 for x in c.expect if x.kind == br.SOLVED) >= 12 and sum(1 for x in c.expect if x.kind == br.PANIC) >= 12
        assert any(r[8:] == [0, 8, 0] for r in c.rows) and any(r[8:] == [0, 8, 20] for r in c.rows) and {255, 256, bc.P - 1} <= set(c.rows[0][:8])
    sch = bc.case("black box SchnorrVerify")
    assert collections.Counter(x.witnesses.get(9) for x in sch.expect if x.kind == br.SOLVED) == {1: 4, 0: 2}
    ecd = bc.case("black box EcdsaSecp256k1, verdicts")
    assert [x.witnesses.get(3) for x in ecd.expect] == [1, 0, 1, None, None]
    for name, group, size in bc.ECDSA_SIZES:  # the slice panic comes before the length failure
        c = bc.case(f"black box {name}, array {group} of {size}")
        assert {x.kind for x in c.expect} == {br.BRILLIG_FAILED, br.PANIC}


@pytest.mark.parametrize("name,what", bc.PERTURBATIONS, ids=[w for _, w in bc.PERTURBATIONS])
def test_each_list_bites(oracle, name, what):
    """the oracle passes the list and fails the same list with one expectation changed"""
    case, expect, j = bc.perturbed(name, what)
    assert [k for k, (a, b) in enumerate(zip(case.expect, expect)) if a != b] == [j]
    got = oracle_rows(oracle, case)
    bc.compare(case, got, "oracle")
    with pytest.raises(AssertionError, match=f"row {j} "):
        bc.compare(case, got, "oracle", expect)
