"""The case lists of tests/arith_cases.py against the CPU oracle (oracle/pwg.c): status, error kind, failing opcode, the aux words, the panic text and the
whole witness map of every row must equal the expectation of the Python model (tests/arith_ref.py); the lists must cover what they are built to cover -- in
the model's branches and, read off the plan (Circuit.gate_records, plan_stats, lin_plan), in the record shapes the planner makes of list C --; and each
list must notice the mistake it is meant to catch (a model variant that is wrong in one way changes the expectation of some row). No GPU:
tests/test_gpu_arith_edges.py runs the same lists on the device."""
import collections
import functools

import numpy as np
import pytest

import acvm_amd
import arith_cases as ac
import arith_ref as ar
from acvm_amd.acir import P

EVERY_CASE = ac.all_cases()
NOT_TRUNCATED = ac.NOT_TRUNCATED


def oracle_rows(oracle, case):
    """[(Result.as_tuple(), message, {witness: value})] of the oracle, one per row"""
    B = len(case.rows)
    values = b"".join(v.to_bytes(32, "big") for row in case.rows for v in row)
    res, asg, vals = oracle.solve_batch(oracle.Circuit(case.circuit.to_bytes()), case.ids, values, B)
    return [(res[j].as_tuple(), res[j].message, {int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])}) for j in range(B)]


def same(a, b):
    """two expectations agree in everything a run is compared by"""
    return a[:7] == b[:7] and a.expression == b.expression


def test_codes_are_the_oracles(oracle):
    assert (ar.ST_SOLVED, ar.ST_IN_PROGRESS, ar.ST_FAILURE, ar.ST_REQUIRES_FOREIGN_CALL) == (oracle.ST_SOLVED, oracle.ST_IN_PROGRESS, oracle.ST_FAILURE, oracle.ST_REQUIRES_FOREIGN_CALL)
    assert (ar.E_NONE, ar.E_MISSING_ASSIGNMENT, ar.E_TOO_MANY_UNKNOWNS, ar.E_UNSATISFIED, ar.E_PANIC) == (
        oracle.E_NONE, oracle.E_MISSING_ASSIGNMENT, oracle.E_TOO_MANY_UNKNOWNS, oracle.E_UNSATISFIED, oracle.E_PANIC)


@pytest.mark.parametrize("letter", sorted(ac.lists()))
def test_oracle_agrees_with_the_model(oracle, letter):
    for case in ac.lists()[letter]:
        ac.compare(case, oracle_rows(oracle, case), "oracle")


def test_oracle_agrees_on_the_initial_sets(oracle):
    circ, maps, expect, notes = ac.initial_set_case()
    case = ac.Case("D", circ, [], list(maps), list(expect), None, list(notes))
    got = []
    for m in maps:
        a = oracle.ACVM(oracle.Circuit(circ.to_bytes()), m)
        a.solve()
        got.append((a.result().as_tuple(), a.result().message, a.witness_map()))
    ac.compare(case, got, "oracle")
    assert collections.Counter(notes) == {"the plain set": 4, "the plain set, d wrong": 3, "lacks d": 7, "brings o, consistent": 7, "brings o, inconsistent": 7}
    by_note = collections.defaultdict(set)
    for x, m, n in zip(expect, maps, notes):
        by_note[n].add((x.status, x.err, x.opcode_index))
        if n == "lacks d":  # the gate the plan of the plain set holds as an ASSERT solved it
            assert x.witnesses[4] == x.witnesses[5]
        if n == "brings o, inconsistent":  # opcode 0 is an assert for this row: the map keeps what the row brought
            assert x.witnesses[5] == m[5] != (m[1] * m[2] + m[3]) % P and 6 not in x.witnesses
    assert by_note == {"the plain set": {(0, 0, 0)}, "the plain set, d wrong": {(2, ar.E_UNSATISFIED, 1)}, "lacks d": {(0, 0, 0)}, "brings o, consistent": {(0, 0, 0)},
                       "brings o, inconsistent": {(2, ar.E_UNSATISFIED, 0)}}


def test_the_oracle_steps_like_the_model(oracle):
    """the partial map after every solve_opcode of rows that end in mid-program"""
    for case in (ac.dyn_cases("an assert solves it")[2], ac.dyn_cases("too many unknowns")[2], ac.order_cases()[0]):
        for j, row in enumerate(case.rows[:8]):
            a = oracle.ACVM(oracle.Circuit(case.circuit.to_bytes()), dict(zip(case.ids, row)))
            for k in range(1, len(case.circuit.opcodes) + 1):
                if a.result().status == oracle.ST_IN_PROGRESS:
                    a.solve_opcode()
                want = ar.run(case.circuit, dict(zip(case.ids, row)), n_opcodes=k)
                assert a.result().status == want.status and a.witness_map() == want.witnesses, (case.name, j, k)


# ---- what the lists cover
def test_sizes():
    for case in EVERY_CASE:
        assert 0 < len(case.rows) <= 135 and len(case.circuit.opcodes) <= 700, case.name
    assert all(3 <= len(c.circuit.opcodes) <= 6 for c in ac.lists()["A"])
    assert sorted({len(c.rows) for f in ac.FOLLOW_UPS for c in ac.dyn_cases(f)}) == [1, 63, 64, 65, 130]
    for f in ac.FOLLOW_UPS:  # the special rows: alone, first / middle / last lane of a wave, in a partial last wave, every other row, every row
        special = [tuple(j for j, n in enumerate(c.notes) if n != "passes") for c in ac.dyn_cases(f)]
        assert special == [s for _, s in ac.PLACEMENTS] and (64,) in special and tuple(range(130)) in special and tuple(range(0, 65, 2)) in special


def all_expects():
    return [x for c in EVERY_CASE for x in c.expect] + list(ac.initial_set_case()[2])


def test_every_branch_outcome_and_panic_text_at_least_twice():
    expects = all_expects()
    branches = collections.Counter(l for x in expects for l in x.branches)
    reachable = [l for l in ar.LABELS if l not in ar.UNREACHABLE]
    assert not [l for l in reachable if branches[l] < 2], [l for l in reachable if branches[l] < 2]
    kinds = collections.Counter((x.status, x.err) for x in expects)
    want = {(ar.ST_SOLVED, ar.E_NONE), (ar.ST_FAILURE, ar.E_MISSING_ASSIGNMENT), (ar.ST_FAILURE, ar.E_TOO_MANY_UNKNOWNS), (ar.ST_FAILURE, ar.E_UNSATISFIED), (ar.ST_FAILURE, ar.E_PANIC)}
    assert set(kinds) == want and min(kinds.values()) >= 2, kinds
    texts = collections.Counter(x.message for x in expects if x.err == ar.E_PANIC)
    assert set(texts) == {ar.MSG_MUL_TERMS} and texts[ar.MSG_MUL_TERMS] >= 2
    # a TooManyUnknowns row carries its evaluated expression, and nobody else does; expressions with a product, with linear terms only, with a folded term
    assert all((x.expression is not None) == (x.err == ar.E_TOO_MANY_UNKNOWNS) for x in expects)
    shapes = collections.Counter((len(x.expression[0]), min(len(x.expression[1]), 3), x.expression[2] != 0) for x in expects if x.expression is not None)
    assert {(1, 0, True), (0, 2, True), (0, 2, False), (1, 1, True)} <= set(shapes), shapes


def test_the_unreachable_arms_are_not_reached():
    """evaluate leaves no witness of the map in the expression: solve_mul_term can only say TooManyUnknowns of a term, no coefficient is zero, and the witness
    a gate assigns is never in the map already"""
    assert len(ar.UNREACHABLE) == 14
    hit = {l for x in all_expects() for l in x.branches}
    assert not hit & set(ar.UNREACHABLE), hit & set(ar.UNREACHABLE)


def test_list_a_has_the_shapes_as_written():
    cases = {c.name: c for c in ac.lists()["A"]}
    ops = lambda name: [e for e in cases["A, " + name].circuit.opcodes if hasattr(e, "mul_terms")]
    assert any(not e.mul_terms and not e.linear_combinations and e.q_c == 0 for e in ops("empty expressions, q_c zero"))
    assert any(not e.mul_terms and not e.linear_combinations and e.q_c for e in ops("empty expressions, q_c nonzero behind two gates"))
    zero_lin = [e for c in cases.values() for e in c.circuit.opcodes if hasattr(e, "mul_terms") and any(c_ == 0 for c_, _ in e.linear_combinations)]
    zero_mul = [e for c in cases.values() for e in c.circuit.opcodes if hasattr(e, "mul_terms") and any(c_ == 0 for c_, _, _ in e.mul_terms)]
    assert len(zero_lin) >= 6 and len(zero_mul) >= 8
    assert any(t[1] == t[2] for e in ops("x x with x unknown") for t in e.mul_terms) and any(t[1] == t[2] for e in ops("x x with x known") for t in e.mul_terms)
    assert any({(l, r) for _, l, r in e.mul_terms} >= {(1, 2), (2, 1)} for e in ops("(c, a, b) with (c', b, a)"))
    assert any([w for _, w in e.linear_combinations] != sorted(w for _, w in e.linear_combinations) for e in ops("terms in unsorted order"))
    # what each shape comes to: an unknown beside a written zero stays unknown; duplicates of an unknown are two unknowns; the panic goes before TooManyUnknowns
    kinds = lambda name: {(x.status, x.err, x.opcode_index) for x in cases["A, " + name].expect}
    assert kinds("one unknown in two linear terms, c and -c") == {(2, ar.E_TOO_MANY_UNKNOWNS, 1)} == kinds("x x with x unknown") == kinds("two residual products, one with coefficient zero")
    for name in ("two residual products", "three residual products, one with coefficient zero", "two residual products beside two unknown linear terms",
                 "three residual products beside a folded and an unknown linear term"):
        assert kinds(name) == {(2, ar.E_PANIC, 1)}, name
    c = cases["A, an unknown under two known partners"]
    outcome = {(row[0] == 0, row[1] == 0): (x.status, x.err, x.opcode_index) for row, x in zip(c.rows, c.expect) if row[2]}
    assert outcome == {(False, False): (2, ar.E_TOO_MANY_UNKNOWNS, 0), (True, False): (0, 0, 0), (False, True): (0, 0, 0), (True, True): (2, ar.E_UNSATISFIED, 0)}, outcome
    assert any(x.status == 2 and x.err == ar.E_TOO_MANY_UNKNOWNS and x.opcode_index == 1 for row, x in zip(c.rows, c.expect) if row[:3] == [0, 0, 0])  # both zero, c = 0: nothing assigned
    c = cases["A, zero coefficient on an unknown linear term"]
    assert all(5 in x.witnesses and x.witnesses[5] == -row[2] % P for row, x in zip(c.rows, c.expect) if x.status == 0) and any(x.status == 0 for x in c.expect)
    for c in cases.values():  # rows of 0, 1 and p - 1 and random ones
        assert {0, 1, P - 1} <= {v for row in c.rows for v in row} and len({v for row in c.rows for v in row}) > 20, c.name


def test_list_b_rows_leave_the_generic_path_in_every_way():
    for f, want in (("an assert solves it", (ar.ST_SOLVED, ar.E_NONE, 0)), ("too many unknowns", (ar.ST_FAILURE, ar.E_TOO_MANY_UNKNOWNS, 2)),
                    ("missing assignment", (ar.ST_FAILURE, ar.E_MISSING_ASSIGNMENT, 2)), ("nobody reads it", (ar.ST_SOLVED, ar.E_NONE, 0))):
        n_zero = 0
        for case in ac.dyn_cases(f):
            st = acvm_amd.Circuit(case.circuit.to_bytes()).plan_stats(case.ids)
            assert st["n_dyn_gates"] == 1 and st["truncated_at"] == NOT_TRUNCATED, case.name
            for note, x, row in zip(case.notes, case.expect, case.rows):
                if note == "zero partner, zero sum":
                    n_zero += 1
                    assert (x.status, x.err, x.opcode_index) == want, (case.name, x[:5])
                    assert (4 in x.witnesses) == (f == "an assert solves it") and (f != "an assert solves it" or x.witnesses[4] == -row[2] % P)
                    if f == "too many unknowns":
                        assert x.expression == ([], [(1, 4), (P - 1, 6)], row[2])
                    if f == "missing assignment":
                        assert x.aux0 == 4
                elif note == "zero partner, nonzero sum":
                    assert (x.status, x.err, x.opcode_index) == (ar.ST_FAILURE, ar.E_UNSATISFIED, 0) and 4 not in x.witnesses
                else:
                    assert x.status == ar.ST_SOLVED and 4 in x.witnesses
        assert n_zero >= 100
    if True:  # the plan of "an assert solves it" holds the follow-up as an ASSERT record
        case = ac.dyn_cases("an assert solves it")[0]
        recs = acvm_amd.Circuit(case.circuit.to_bytes()).gate_records(case.ids)
        assert [r["kind"] for r in sorted(recs, key=lambda r: r["opcode"])] == ["SOLVE_DYN", "ASSERT", "SOLVE"]
    wide = ac.wide_dyn_case()
    st = acvm_amd.Circuit(wide.circuit.to_bytes()).plan_stats(wide.ids)
    assert st["n_dyn_gates"] == ac.WIDE == 260 and acvm_amd.tuning_get("inv_chunk") == 128 and st["n_inverse_slots"] == 260
    recs = acvm_amd.Circuit(wide.circuit.to_bytes()).gate_records(wide.ids)
    assert sum(r["kind"] == "SOLVE_DYN" for r in recs) == 260
    at = {n: (x.status, x.err, x.opcode_index) for n, x in zip(wide.notes, wide.expect)}
    for k in ac.WIDE_ZEROS:
        assert at[f"partner {k} zero, nonzero sum"] == (2, ar.E_UNSATISFIED, k) and at[f"partner {k} zero, zero sum"][0] == (2 if k == 128 else 0)
    assert at["the four partners zero, zero sum"] == (2, ar.E_TOO_MANY_UNKNOWNS, 261) and at["every partner zero, zero sum"] == (2, ar.E_TOO_MANY_UNKNOWNS, 260)
    assert at["both operands of the reader unassigned"] == (2, ar.E_TOO_MANY_UNKNOWNS, 260)
    two, first_a, first_p, early = ac.order_cases()
    both = [x for n, x in zip(two.notes, two.expect) if "opcode 2" in n and "opcode 3" in n]
    assert len(both) >= 2 and all(x.opcode_index == 2 and 8 not in x.witnesses for x in both)
    assert {x.opcode_index for n, x in zip(two.notes, two.expect) if x.status == 2} == {2, 3}
    for case, want in ((first_a, {"a != b zero partner": 0, "zero partner": 1, "a != b": 0}), (first_p, {"a != b zero partner": 0, "zero partner": 0, "a != b": 1})):
        for n, x in zip(case.notes, case.expect):
            if n in want:
                assert (x.status, x.err, x.opcode_index) == (2, ar.E_UNSATISFIED, want[n]), (case.name, n, x[:5])
        assert all(sum(1 for n in case.notes if n == k) >= 2 for k in want) and any(n == "zero partner zero sum" or n.endswith("zero sum") for n in case.notes)
    st = acvm_amd.Circuit(early.circuit.to_bytes()).plan_stats(early.ids)
    assert st["n_levels"] >= 21 and st["truncated_at"] == NOT_TRUNCATED
    bad = [x for x in early.expect if x.status == 2]
    assert len(bad) == 4 and all(x.opcode_index == 20 and max(x.witnesses) == 23 for x in bad)  # nothing of the 40 gates behind the assert is in the map


def test_every_plan_ends_where_the_generic_row_does():
    """truncated_at of every plan is what the lists say (tests/test_gpu_arith_edges.py asserts the same of the handles' statistics)"""
    at = collections.Counter()
    for case in EVERY_CASE:
        st = acvm_amd.Circuit(case.circuit.to_bytes()).plan_stats(case.ids)
        assert st["truncated_at"] == ac.expected_truncation(case), (case.name, st["truncated_at"])
        at[case.name[0], st["truncated_at"] != NOT_TRUNCATED] += 1
    assert at["A", True] >= 10 and at["A", False] >= 10 and at["B", True] == 0 and at["C", True] == 2, at


# ---- list C: the record shapes its plans hold, read off the plan under the default tuning
def reductions(r):
    """Montgomery reductions of a record, as gate_eval pairs its terms"""
    n_mac = r["np_mac"] + r["nl_mac"]
    both = min(r["np_pos"], n_mac)
    return both + (n_mac - both + 1) // 2 + (r["np_pos"] - both + 1) // 2


def side_sum_resets(r):
    """how often gate_h_room brings the side sum down (budget 111: the constant 16, a -1 product 33, a +1 term 16, a -1 term 33; 17 after a reduction)"""
    hw, resets = 16 if r["has_qc"] else 0, 0
    for weight, n in ((33, r["np_neg"]), (16, r["nl_pos"]), (33, r["nl_neg"])):
        for _ in range(n):
            if hw + weight > 111:
                hw, resets = 17, resets + 1
            hw += weight
    return resets


def loop_exits(r):
    """the exits of gate_eval's three pairing loops: how the +1 product / coefficient loop ends, the leftover of the coefficient pairs (with tables or
    without), the leftover of the +1 product pairs"""
    n_mac = r["np_mac"] + r["nl_mac"]
    both = min(r["np_pos"], n_mac)
    mac_left, pos_left = n_mac - both, r["np_pos"] - both
    first = "not entered" if both == 0 else "products ran out" if mac_left else "coefficients ran out" if pos_left else "both ran out"
    parity = lambda n: "none" if n == 0 else "odd" if n % 2 else "even"
    return ("first", first), ("coefficients", "tables" if r["lin_terms"] else "no tables", parity(mac_left)), ("products", parity(pos_left))


@functools.lru_cache(maxsize=None)
def list_c_plans():
    """[(case, plan_stats, gate records, lin_plan)] under the default tuning"""
    out = []
    for case in ac.lists()["C"]:
        gc = acvm_amd.Circuit(case.circuit.to_bytes())
        out.append((case, gc.plan_stats(case.ids), gc.gate_records(case.ids), gc.lin_plan(case.ids)))
    return out


def test_gate_records_decode_the_whole_stream():
    for case, st, recs, lp in list_c_plans():
        assert len(recs) == lp["n_gate_records"] == st["n_fast_gates"] + st["n_dyn_gates"], case.name
        assert sum(1 for r in recs if r["position"] == 0) == lp["n_wave_programs"] and sum(r["tail"] for r in recs) == st["n_gate_pairs"]
        assert collections.Counter(r["out_mode"] for r in recs if r["kind"] != "ASSERT") == collections.Counter(
            {m: st[k] for m, k in (("ASIS", "n_gate_out_asis"), ("WEAK", "n_gate_out_weak"), ("CANON", "n_gate_out_canon")) if st[k]}), case.name
        assert sum(1 for r in recs if r["lin_terms"]) == lp["n_lin_records"] and sum(r["lin_terms"] for r in recs) == lp["n_lin_terms"], case.name
        assert sorted(r["opcode"] for r in recs) == [oi for oi, op in enumerate(case.circuit.opcodes) if hasattr(op, "mul_terms")][:len(recs)], case.name


def test_list_c_reaches_the_record_shapes_it_is_built_for():
    """conditions on the INPUTS (list C grows until they hold), measured on the plan, not on the kernels; NOTEBOOK.md quotes the counts"""
    assert all(acvm_amd.tuning_get(k) == 1 for k in ("scale", "relax", "pairs", "chains", "lin_table"))
    recs = [r for _, _, rs, _ in list_c_plans() for r in rs]
    assert {r["out_mode"] for r in recs} == {None, "ASIS", "WEAK", "CANON"}
    assert {r["sub_k"] for r in recs if r["nl_neg"]} == {1, 2, 3}
    assert sum(r["presum_weak"] for r in recs) >= 2 and all(r["kind"] == "SOLVE_DYN" for r in recs if r["presum_weak"])
    n_red = collections.Counter(reductions(r) for r in recs)
    assert {16, 17, 32, 33} <= set(n_red) and max(n_red) >= 128, sorted(n_red)   # around the periodic reduction of the running sum: once, twice, often
    assert {0, 1, 2} <= {min(side_sum_resets(r), 2) for r in recs}
    for unit, spill in (("nl_pos", "nl_mac"), ("nl_neg", "nl_mac"), ("np_neg", "np_mac"), ("np_pos", "np_mac")):
        full = [r for r in recs if r[unit] == 255]
        assert any(r[spill] == 0 for r in full) and any(r[spill] == 1 for r in full) and any(r[spill] >= 45 for r in full), unit
        assert any(r[unit] == 254 for r in recs), unit
    assert {r["np_mac"] for r in recs} >= {0, 1, 2, 3, 254} and {r["nl_mac"] for r in recs} >= {0, 1, 2, 3, 255}
    assert any(r["tail"] for r in recs) and any(r["set_local"] for r in recs) and any(r["position"] >= 2 for r in recs)
    # the plan ends at the gates of 256 general terms and nowhere else
    for case, st, _, _ in list_c_plans():
        assert st["truncated_at"] == (1 if case.name.startswith("C, 256 general") else NOT_TRUNCATED), case.name
    assert sum(1 for case, _, _, _ in list_c_plans() if case.name.startswith("C, 256 general")) == 2
    # linear tables: records with tables and odd and even numbers of terms; every exit of the three pairing loops
    tabled = [r for r in recs if r["lin_terms"]]
    assert {r["lin_terms"] % 2 for r in tabled} == {0, 1} and {1, 2, 3} <= {r["lin_terms"] for r in tabled} and max(r["lin_terms"] for r in tabled) >= 65
    exits = collections.Counter(e for r in recs for e in loop_exits(r))
    want = {("first", f) for f in ("not entered", "products ran out", "coefficients ran out", "both ran out")} | {("products", p) for p in ("none", "odd", "even")} | {
        ("coefficients", t, p) for t in ("tables", "no tables") for p in ("odd", "even")} | {("coefficients", "no tables", "none")}
    assert set(exits) >= want and min(exits[e] for e in want) >= 2, sorted(want - set(exits))


def test_list_c_as_written_without_projective_scales():
    """scale = 0: the record lists follow from the circuit -- every cell of the grid (np_pos, np_mac, nl_mac) in {0..3}^3 as SOLVE, ASSERT and SOLVE_DYN, and
    the -1 products stay -1 products"""
    grid = next(c for c in ac.lists()["C"] if c.name == "C, the grid of record shapes")
    with acvm_amd.tuning(scale=0):
        recs = acvm_amd.Circuit(grid.circuit.to_bytes()).gate_records(grid.ids)
        cells = {(r["kind"], r["np_pos"], r["np_mac"], r["nl_mac"]) for r in recs}
        assert cells == {(k, a, b, c) for k in ("SOLVE", "ASSERT", "SOLVE_DYN") for a in range(4) for b in range(4) for c in range(4)}
        assert all(r["out_mode"] in (None, "CANON") for r in recs)
        kp = next(c for c in ac.lists()["C"] if c.name == "C, asserts whose sums are k p")
        recs = acvm_amd.Circuit(kp.circuit.to_bytes()).gate_records(kp.ids)
        assert {r["np_neg"] for r in recs} >= {1, 2, 3, 5, 8, 13} and {r["nl_neg"] for r in recs} >= {1, 13} and {r["nl_pos"] for r in recs} >= {2, 14}


def test_list_c_forces_the_values_at_the_limb_boundaries():
    names = dict(ac.forced_values())
    top = P >> 232
    assert {0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, top << 232, (top << 232) - 1, (top << 232) + 1} <= set(names.values())
    assert all(1 << k in names.values() and P - (1 << k) in names.values() for i in range(1, 8) for k in (29 * i, 32 * i)) and 1 << 232 in names.values()
    for store in ac.STORES:
        case = ac.forced_case(store)
        recs = acvm_amd.Circuit(case.circuit.to_bytes()).gate_records(case.ids)
        modes = {r["out_mode"] for r in recs if r["out"] in (7, 8, 9, 10)}
        assert modes == ({"CANON"} if store == "pinned" else {"ASIS"} if store == "operand of an assert" else {"ASIS", "WEAK"}) or store == "relaxed", (store, modes)
        assert sum(1 for n in case.notes if n.endswith("the sum wraps")) >= 10
    kp = next(c for c in ac.lists()["C"] if c.name == "C, asserts whose sums are k p")
    assert all(v == P - 1 for v in kp.rows[0][:8])


# ---- each list bites
BITES = [("unknowns_by_witness", "A"), ("folded_zero_kept", "A"), ("written_zero_counts", "A"), ("too_many_before_panic", "A"), ("zero_partner_assigns_zero", "B"), ("integer_zero_test", "C")]


@pytest.mark.parametrize("variant,letter", BITES, ids=[f"{v} on {l}" for v, l in BITES])
def test_each_list_bites(variant, letter):
    """a model that is wrong in one way expects something else of at least two rows of the list meant to catch it"""
    changed = 0
    for case in ac.lists()[letter]:
        for row, want in zip(case.rows, case.expect):
            changed += not same(ar.run(case.circuit, dict(zip(case.ids, row)), variant=variant), want)
    assert changed >= 2, (variant, letter)


def test_every_variant_is_named():
    assert sorted(v for v, _ in BITES) == sorted(ar.VARIANTS) and len(ar.VARIANTS) == 6
