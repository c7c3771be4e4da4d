"""The case lists of tests/mem_cases.py against the CPU oracle (oracle/pwg.c): status, error kind, failing opcode, the aux words, the panic text and the
whole witness map of every row must equal the expectation of the Python model (tests/mem_ref.py); the lists must cover what they are built to cover;
and each list must notice the mistake it is meant to catch (a model variant that is wrong in one way changes the expectation of some row). No GPU:
tests/test_gpu_mem_edges.py runs the same lists on the device."""
import collections

import numpy as np
import pytest

import mem_cases as mc
import mem_ref as mr
from acvm_amd.acir import P, MemoryOp

CALLS = [mc.reentry_case("call", d) for d in (False, True)]
EVERY_CASE = mc.all_cases() + CALLS


def oracle_rows(oracle, case):
    """[(Result.as_tuple(), message, {witness: value})] of the oracle, one per row"""
    B = len(case.rows)
    values = b"".join(v.to_bytes(32, "big") for row in case.rows for v in row)
    res, asg, vals = oracle.solve_batch(oracle.Circuit(case.circuit.to_bytes()), case.ids, values, B)
    return [(res[j].as_tuple(), res[j].message, {int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])}) for j in range(B)]


def same(a, b):
    """two expectations agree in everything a run is compared by"""
    return a[:7] == b[:7] and a.pending == b.pending


def test_codes_are_the_oracles(oracle):
    assert (mr.ST_SOLVED, mr.ST_IN_PROGRESS, mr.ST_FAILURE, mr.ST_REQUIRES_FOREIGN_CALL) == (oracle.ST_SOLVED, oracle.ST_IN_PROGRESS, oracle.ST_FAILURE, oracle.ST_REQUIRES_FOREIGN_CALL)
    assert (mr.E_NONE, mr.E_MISSING_ASSIGNMENT, mr.E_TOO_MANY_UNKNOWNS, mr.E_UNSATISFIED, mr.E_INDEX_OOB, mr.E_BRILLIG_FAILED, mr.E_PANIC) == (
        oracle.E_NONE, oracle.E_MISSING_ASSIGNMENT, oracle.E_TOO_MANY_UNKNOWNS, oracle.E_UNSATISFIED, oracle.E_INDEX_OOB, oracle.E_BRILLIG_FAILED, oracle.E_PANIC)


@pytest.mark.parametrize("case", EVERY_CASE, ids=lambda c: c.name)
def test_oracle_agrees_with_the_model(oracle, case):
    mc.compare(case, oracle_rows(oracle, case), "oracle")


@pytest.mark.parametrize("case", CALLS, ids=lambda c: c.name)
def test_oracle_agrees_behind_the_answers(oracle, case):
    expect = mc.answered_expect(case)
    got = []
    for row, want in zip(case.rows, case.expect):
        a = oracle.ACVM(oracle.Circuit(case.circuit.to_bytes()), dict(zip(case.ids, row)))
        assert a.solve() == oracle.ST_REQUIRES_FOREIGN_CALL and a.get_pending_foreign_call() == want.pending and a.instruction_pointer() == want.opcode_index
        a.resolve_pending_foreign_call(mc.answer_of(row))
        a.solve()
        got.append((a.result().as_tuple(), a.result().message, a.witness_map()))
    assert all(x.status == mr.ST_SOLVED for x in expect)
    mc.compare(case, got, "oracle, answered", expect)


def test_oracle_agrees_on_the_initial_sets(oracle):
    circ, maps, expect, notes = mc.initial_set_case()
    case = mc.Case("H", circ, [], list(maps), list(expect), list(notes), None, None)
    got = []
    for m in maps:
        a = oracle.ACVM(oracle.Circuit(circ.to_bytes()), m)
        a.solve()
        got.append((a.result().as_tuple(), a.result().message, a.witness_map()))
    mc.compare(case, got, "oracle")
    assert collections.Counter(notes) == {"the plain set": 7, "knows the read target": 7, "lacks an init witness": 7}


def test_the_oracle_steps_like_the_model(oracle):
    """the partial map after every solve_opcode of a row that fails in mid-program"""
    case, failing, _ = mc.order_case(mc.ORDER_SEEDS[0])
    for j in (failing[1], failing[4]):
        a = oracle.ACVM(oracle.Circuit(case.circuit.to_bytes()), dict(zip(case.ids, case.rows[j])))
        for k in range(1, len(case.circuit.opcodes) + 1):
            if a.result().status == oracle.ST_IN_PROGRESS:
                a.solve_opcode()
            want = mr.run(case.circuit, dict(zip(case.ids, case.rows[j])), n_opcodes=k)
            assert a.result().status == want.status and a.witness_map() == want.witnesses, (j, k)
            if want.status == mr.ST_IN_PROGRESS:
                assert a.instruction_pointer() == want.opcode_index == k


# ---- what the lists cover
def test_sizes():
    for case in EVERY_CASE:
        assert 0 < len(case.rows) <= 200 and len(case.rows) % 64, case.name
    assert mc.LENGTHS == (1, 6, 33, 67) and [len(c.circuit.opcodes[0].init) for c in mc.lists()["A"]] == list(mc.LENGTHS)
    assert sorted(n for _, n in mc.ORDER_BLOCKS) == [6, 33, 67]


def test_every_branch_outcome_and_panic_text_at_least_twice():
    expects = [x for c in EVERY_CASE for x in c.expect] + list(mc.initial_set_case()[2]) + [x for c in CALLS for x in mc.answered_expect(c)]
    branches = collections.Counter(l for x in expects for l in x.branches)
    assert not [l for l in mr.LABELS if branches[l] < 2], [l for l in mr.LABELS if branches[l] < 2]
    kinds = collections.Counter((x.status, x.err) for x in expects)
    for kind in ((mr.ST_SOLVED, mr.E_NONE), (mr.ST_REQUIRES_FOREIGN_CALL, mr.E_NONE), (mr.ST_FAILURE, mr.E_MISSING_ASSIGNMENT), (mr.ST_FAILURE, mr.E_UNSATISFIED),
                 (mr.ST_FAILURE, mr.E_INDEX_OOB), (mr.ST_FAILURE, mr.E_PANIC)):
        assert kinds[kind] >= 2, kind
    assert set(kinds) <= {(mr.ST_SOLVED, 0), (mr.ST_REQUIRES_FOREIGN_CALL, 0)} | {(mr.ST_FAILURE, e) for e in (mr.E_MISSING_ASSIGNMENT, mr.E_UNSATISFIED, mr.E_INDEX_OOB, mr.E_PANIC)}
    texts = collections.Counter(x.message for x in expects if x.err == mr.E_PANIC)
    assert set(texts) == {mr.MSG_INDEX, mr.MSG_READ_TARGET} and min(texts.values()) >= 2
    # an out-of-bounds error reports the NEW length after a shorter init, and the wrapped index
    oob = {(x.aux0, x.aux1) for c in mc.lists()["E"] for x in c.expect if x.err == mr.E_INDEX_OOB}
    assert {(2, 2), (4, 2), (6, 6), (0, 0), (3, 0), (5, 0), (3, 3), (1, 1)} <= oob, oob
    assert any((x.aux0, x.aux1) == (6, 6) and x.err == mr.E_INDEX_OOB for x in mc.index_case(6).expect)  # 2^32 + len is reported as len


def form_of(e):
    if not e.mul_terms and not e.linear_combinations:
        return "constant"
    if e.mul_terms:
        return "product"
    return "sum of two gate outputs" if len(e.linear_combinations) == 2 else "witness + constant" if e.q_c else "witness"


@pytest.mark.parametrize("n", mc.LENGTHS)
def test_list_a_covers_every_index_class_form_and_predicate(n):
    case = mc.index_case(n)
    ops = case.circuit.opcodes
    executed = collections.defaultdict(set)   # (class, read?) -> {(form, predicate)} of the opcodes that got to the index with the predicate on, or panicked
    skipped = collections.defaultdict(set)    # the same under a zero predicate
    for trace in case.traces:
        for oi, is_read, raw, pred in trace:
            for c in mc.index_classes(raw, n):
                (skipped if pred == 0 else executed)[c, is_read].add((form_of(ops[oi].index), pred))
    panics = ("2^64", "p - 1")
    for c in mc.INDEX_CLASSES:
        for is_read in (True, False):
            seen = executed[c, is_read]
            if c in panics:  # the first MemoryOp of the circuit panics, whatever its predicate: reads at two lengths, writes at the other two
                assert (len(seen) == 1) == (is_read == (mc.LENGTHS.index(n) % 2 == 0)), (c, is_read, seen)
                continue
            assert {f for f, _ in seen} == set(mc.FORMS) | {"constant"}, (c, is_read, seen)
            assert {p for _, p in seen} >= {1, 2, P - 1}, (c, is_read, seen)
            assert {f for f, _ in skipped[c, is_read]} >= set(mc.FORMS), (c, is_read)
        assert any(p == "absent" for is_read in (True, False) for _, p in executed[c, is_read]) or c in panics, c
    # the sum of two gate outputs wraps past p in about half of the rows
    k = n + 5  # position of d = i - t; t follows
    wraps = [row[k - 1] + row[k] >= P for row in case.rows]
    assert sum(wraps) >= 40 and len(wraps) - sum(wraps) >= 40
    # a zero predicate with an index of 2^64 still panics; with an out-of-bounds index it does not, and a read target gets 0
    first = min(oi for oi, op in enumerate(ops) if isinstance(op, MemoryOp))
    assert ops[first].predicate is not None
    for v in (mc.U64, P - 1):
        rows = [j for j, row in enumerate(case.rows) if row[n] == v and not any(row[n + 7:])]
        assert rows and all((case.expect[j].err, case.expect[j].opcode_index, case.expect[j].message) == (mr.E_PANIC, first, mr.MSG_INDEX) for j in rows)
    quiet = [j for j, row in enumerate(case.rows) if row[n] == n + 1 and not any(row[n + 7:])]
    assert quiet and all((case.expect[j].err, case.expect[j].opcode_index) == (mr.E_INDEX_OOB, first + 8) for j in quiet)  # the first opcode WITHOUT a predicate
    assert all(case.expect[j].witnesses[t.value.linear_combinations[0][1]] == 0 for j in quiet for t in ops[first:first + 8] if t.operation.q_c == 0)


def test_list_a_both_kinds_panic_first_somewhere():
    firsts = {next(op for op in mc.index_case(n).circuit.opcodes if isinstance(op, MemoryOp)).operation.q_c for n in mc.LENGTHS}
    assert firsts == {0, 1}


def test_list_b_dual_opcodes_read_in_some_rows_and_write_in_others():
    case, duals = mc.operation_case()
    assert len(duals) == 4
    for oi in duals:
        kinds = collections.Counter(is_read for trace in case.traces for at, is_read, _, _ in trace if at == oi)
        assert kinds[True] >= 2 and kinds[False] >= 2, (oi, kinds)
        outcomes = {(x.err, x.aux0) for x in case.expect if x.status == mr.ST_FAILURE and x.opcode_index == oi}
        unknown_operand = oi in (duals[0], duals[2])
        assert len(outcomes) == 1 and next(iter(outcomes))[0] == (mr.E_MISSING_ASSIGNMENT if unknown_operand else mr.E_PANIC), (oi, outcomes)
    operations = {op.operation.q_c for op in case.circuit.opcodes if isinstance(op, MemoryOp) and mr.is_constant(op.operation)}
    assert operations == {0, 1, 2, P - 1}
    assert {row[7] for row in case.rows} == {0, 1, 7} == {row[8] for row in case.rows}


def test_list_c_every_target_in_every_predicate_mode():
    names = [c.name for c in mc.target_cases()]
    assert len(names) == 1 + 4 + 8 and all(f"C, target {t}, predicate unassigned" in names for t in mc.TARGETS)
    for c in mc.target_cases():
        if c.name.endswith("predicate unassigned"):
            assert all(x.err == mr.E_MISSING_ASSIGNMENT and x.opcode_index == 1 for x in c.expect), c.name
        elif c.name != "C, targets that can be a witness":  # the panic comes first under every predicate
            assert all((x.err, x.message, x.opcode_index) == (mr.E_PANIC, mr.MSG_READ_TARGET, 1) for x in c.expect) and {row[11] for row in c.rows} >= {0, 1, 2, P - 1}, c.name
    can = mc.target_cases()[0]
    at = collections.Counter((x.err, x.opcode_index) for x in can.expect)
    assert at[mr.E_PANIC, 3] >= 2 and at[mr.E_PANIC, 4] >= 2 and at[mr.E_INDEX_OOB, 1] >= 1 and at[mr.E_NONE, 0] >= 2, at
    zero_pred_panics = [j for j, row in enumerate(can.rows) if not any(row[11:]) and can.expect[j].err == mr.E_PANIC]
    assert len(zero_pred_panics) >= 2


def test_list_f_reads_share_levels():
    import acvm_amd
    for seed in mc.ORDER_SEEDS:
        case, failing, trip_at = mc.order_case(seed)
        ops = case.circuit.opcodes
        n_mem = sum(1 for op in ops[3:] if isinstance(op, MemoryOp)) - sum(n for _, n in mc.ORDER_BLOCKS)
        assert n_mem == 120 and 30 <= sum(1 for op in ops if not isinstance(op, MemoryOp) and hasattr(op, "q_c")) <= 50, (seed, n_mem)
        assert all(mr.is_constant(op.operation) for op in ops if isinstance(op, MemoryOp))
        st = acvm_amd.Circuit(case.circuit.to_bytes()).plan_stats(case.ids)
        assert st["truncated_at"] == 0xFFFFFFFF and st["n_levels"] * 3 < len(ops), (seed, st["n_levels"], len(ops))
        assert len(failing) == 5 and sorted(trip_at) == list(trip_at) and trip_at[0] < len(ops) // 3 < trip_at[2] and trip_at[3] == len(ops) - 1
        # behind every tripwire but the last the program still writes
        for k in trip_at[:3]:
            assert any(isinstance(op, MemoryOp) and op.operation.q_c == 1 for op in ops[k:])


# ---- each list bites
BITES = [("readable_is_len", "E"), ("pred_counts_only_as_one", "A"), ("index_not_wrapped", "A"), ("pred_before_to_witness", "C"), ("replay_style", "B"), ("replay_style", "G"),
         ("dynamic_read_writes_back", "G")]


@pytest.mark.parametrize("variant,letter", BITES, ids=[f"{v} on {l}" for v, l in BITES])
def test_each_list_bites(variant, letter):
    """a model that is wrong in one way expects something else of at least one row of the list meant to catch it"""
    changed = 0
    for case in mc.lists()[letter]:
        for row, want in zip(case.rows, case.expect):
            changed += not same(mr.run(case.circuit, dict(zip(case.ids, row)), variant=variant), want)
    assert changed >= 1, (variant, letter)


def test_list_g_catches_a_replay_that_ignores_the_predicate_and_nothing_else():
    """the narrow variant moves exactly the rows of the dynamic circuits whose predicate z is 0 (the cell read back is 0 there, not its value); where
    z = 1, and at the stale key, what such a replay stores is what the cell holds"""
    for form in ("call", "loop"):
        case = mc.reentry_case(form, True)
        want = mc.answered_expect(case) if form == "call" else case.expect
        answers = (lambda row: [mc.answer_of(row)]) if form == "call" else (lambda row: ())
        moved = [not same(mr.run(case.circuit, dict(zip(case.ids, row)), answers=answers(row), variant="dynamic_read_writes_back"), x) for row, x in zip(case.rows, want)]
        assert moved == [row[10] == 0 for row in case.rows] and 40 <= sum(moved) < len(moved)
        static = mc.reentry_case(form, False)
        assert all(same(mr.run(static.circuit, dict(zip(static.ids, row)), variant="dynamic_read_writes_back"), x) for row, x in zip(static.rows, static.expect))
