"""The case lists of tests/sort_cases.py against the CPU oracle (oracle/sorting.c, oracle/pwg.c): status, error kind, failing opcode, the aux words, the
panic text and the whole witness map of every row must equal the expectation of the Python model (tests/sort_ref.py); the model is pinned to the
reference's own known answers and to the network-execution property; the lists must cover what they are built to cover; each list must notice the mistake
it is meant to catch; and the scratch the planner reserves for a sort must cover what op_perm_sort's allocation walk touches. No GPU:
tests/test_gpu_sort_edges.py runs the same lists on the device."""
import collections
import itertools

import pytest

import sort_cases as sc
import sort_ref as sr
from acvm_amd.acir import P, Circuit, Expression as E, PermutationSort
from acvm_amd.synth import values_from_rows
from test_oracle_sorting import execute_network, switch_nb

EVERY_CASE = sc.all_cases()


def oracle_got(oracle, case):
    return oracle.solve_batch(oracle.Circuit(case.circuit.to_bytes()), case.ids, values_from_rows(case.rows), len(case.rows))


def same(a, b):
    return a[:7] == b[:7]


# ---- the model
def test_route_known_answers():
    """sorting.rs:309-383"""
    assert sr.route([1, 2, 3], [1, 2, 3]) == [False, False, False]
    assert sr.route([1, 2, 3], [1, 3, 2]) == [False, False, True]
    assert sr.route([1, 2, 3], [3, 2, 1]) == [True, True, True]
    assert sr.route([0, 1, 2, 3], [2, 3, 0, 1]) == [False, True, True, True, True]
    assert sr.route([0, 1, 2, 3, 4], [0, 3, 4, 2, 1]) == [False, False, False, True, False, True, False, True]


def test_route_executes_to_every_permutation():
    """executing the network with route's bits maps the inputs to the outputs (sorting.rs:256-307), over every permutation of up to seven wires"""
    for n in range(1, 8):
        assert sr.switch_count(n) == switch_nb(n)
        ident = list(range(n))
        for p in itertools.permutations(ident):
            c = sr.route(ident, list(p))
            assert len(c) == switch_nb(n) and execute_network(c, ident) == list(p), p
    assert sr.route([], []) == []


def test_route_is_the_oracles(oracle):
    from test_oracle_sorting import route
    for n in (3, 4, 5, 6, 7, 8, 9, 16, 17, 33, 64, 129):
        for name, keys in sc.structured(n, __import__("random").Random(n)):
            if len(set(keys)) == n:
                assert route(oracle, list(range(n)), keys) == sr.route(list(range(n)), keys), (n, name)


def test_the_sort_is_stable_and_by_canonical_integers():
    circ = Circuit(20, [PermutationSort([[E.from_witness(1 + i)] for i in range(4)], 1, list(range(5, 10)), [0])])
    x, orders = sr.run_traced(circ, {1: P - 1, 2: 1 << 32, 3: 7, 4: 1 << 32})
    assert orders == [(0, [2, 1, 3, 0])]


@pytest.mark.parametrize("case", EVERY_CASE, ids=lambda c: c.name)
def test_oracle_agrees_with_the_model(oracle, case):
    sc.compare(case, oracle_got(oracle, case), "oracle")


# ---- what the lists cover
def test_every_branch_outcome_and_text_at_least_twice():
    expects = [x for c in EVERY_CASE for x in c.expect]
    branches = collections.Counter(l for x in expects for l in x.branches)
    unused = ("gate_solves", "range_passes", "range_fails")   # (the model's other opcodes: no list has them)
    assert not [l for l in sr.LABELS if branches[l] < 2 and l not in unused], [l for l in sr.LABELS if branches[l] < 2]
    kinds = collections.Counter((x.status, x.err) for x in expects)
    assert set(kinds) == {(sr.ST_SOLVED, sr.E_NONE)} | {(sr.ST_FAILURE, e) for e in (sr.E_MISSING_ASSIGNMENT, sr.E_UNSATISFIED, sr.E_PANIC)} and min(kinds.values()) >= 2
    texts = collections.Counter(x.message for x in expects if x.err == sr.E_PANIC)
    assert set(texts) == {sr.msg_index(t + 1, t + 1) for t in (1, 2, 3, 4)} and min(texts.values()) >= 2


def test_list_a_permutations():
    assert sc.SMALL_N == tuple(range(7)) and sc.LARGE_N == (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
    for n in sc.SMALL_N:
        case = sc.every_permutation_case(n)
        assert {tuple(r[:n]) for r in case.rows} == set(itertools.permutations(range(n)))
        for row, x in zip(case.rows, case.expect):   # the bits route the identity to the sorted order
            bits = case.circuit.opcodes[0].bits
            if n >= 2:
                assert execute_network([bool(x.witnesses[w]) for w in bits], list(range(n))) == sorted(range(n), key=lambda i: row[i])
    for n in sc.LARGE_N:
        case = sc.structured_case(n)
        want = {"identity", "reverse", "rotation by +1", "rotation by -1", "first two swapped", "last two swapped", "last to front", "first to last",
                "even / odd riffle", "the riffle's inverse", "all keys equal", "two keys alternating", "random 0", "random 1", "random 2"}
        assert set(case.notes) == want | ({"bit reversal"} if n & (n - 1) == 0 else set()), n
        bits = case.circuit.opcodes[0].bits
        assert len(bits) == switch_nb(n)
        for row, x in zip(case.rows, case.expect):
            assert execute_network([bool(x.witnesses[w]) for w in bits], list(range(n))) == sorted(range(n), key=lambda i: row[i]), (n, row[:8])
        assert any(max(row) >> 224 for row in case.rows)   # keys that reach the top limb


def test_list_b_comparator():
    case = sc.limb_case()
    for limb in range(8):
        rows = [row for row, note in zip(case.rows, case.notes) if f"limb {limb} only" in note]
        assert len(rows) == 2
        for row in rows:
            assert len(set(row)) == 9 and len({v & ~(0xFFFFFFFF << (32 * limb)) for v in row}) == 1
    assert sum(1 for row in case.rows if {0, 1, P - 1, (P - 1) // 2, (P + 1) // 2} <= set(row)) >= 2
    ex = sc.expression_case()
    assert sum(1 for row in ex.rows if row[0] + P - 1000 >= P) >= 5 and sum(1 for row in ex.rows if row[0] + P - 1000 < P) >= 5
    els = ex.circuit.opcodes[0].inputs
    assert sum(1 for el in els if not el[0].mul_terms and not el[0].linear_combinations) == 2 and sum(1 for el in els if el[0].mul_terms) == 2
    assert sum(1 for el in els if any(w == 1 for _, w in el[0].linear_combinations)) >= 3   # one witness in several tuples
    shapes = {(c.circuit.opcodes[0].tuple, tuple(c.circuit.opcodes[0].sort_by)) for c in sc.sort_by_cases()}
    assert shapes == {(t, tuple(s)) for t in (1, 2, 3, 4) for s in sc.sort_by_shapes(t)} and len(sc.sort_by_cases()) == 24
    for t in (1, 2, 3, 4):
        case = sc.past_tuple_case(t)
        assert case.circuit.opcodes[0].sort_by == [0, t + 1]
        assert [x.err for x in case.expect] == [sr.E_NONE, sr.E_PANIC] * 5
        assert all("column_past_the_tuple_not_reached" in x.branches for x in case.expect[0::2])


def test_list_c_bits():
    nb = switch_nb(sc.N_BITS)
    cases = sc.bits_cases()
    assert [len(c.circuit.opcodes[0].bits) for c in cases[:4]] == [0, 1, nb - 1, nb + 3]
    extra = cases[3].circuit.opcodes[0].bits[nb:]
    assert len(extra) == 3 and all(w not in x.witnesses for x in cases[3].expect for w in extra)
    pre = cases[4]
    kinds = collections.Counter(n.split("pre-assigned ")[1] for n in pre.notes)
    assert kinds == {"right": 8, "wrong": 8, "no bit at all": 8}
    assert [x.status for x in pre.expect] == [sr.ST_SOLVED, sr.ST_FAILURE, sr.ST_FAILURE] * 8
    twice = cases[5].circuit.opcodes[0].bits
    assert twice[2] == twice[7] and len(set(twice)) == len(twice) - 1


def test_list_e_neighbours():
    for n_rows in (65, 130):
        case = sc.neighbours_case(n_rows)
        ops = case.circuit.opcodes
        assert len(case.rows) == n_rows and [len(op.inputs) for op in ops if isinstance(op, PermutationSort)] == [33, 129]
        sha = ops[1]
        assert sum((f.num_bits + 7) // 8 for f in sha.args["inputs"]) == 300 and len({f.num_bits for f in sha.args["inputs"]}) >= 6
        assert all(x.status == sr.ST_SOLVED for x in case.expect)


# ---- each list bites
BITES = [("unstable_sort", "A"), ("unstable_sort", "B"), ("switch_y_first", "A"), ("sub_networks_swapped", "A"), ("low_limb_first", "B"), ("panic_unreached", "B")]


@pytest.mark.parametrize("variant,letter", BITES, ids=[f"{v} on {l}" for v, l in BITES])
def test_each_list_bites(variant, letter):
    changed = 0
    for case in sc.lists()[letter]:
        if len(case.rows) > 200:
            continue
        for row, want in zip(case.rows, case.expect):
            changed += not same(sr.run(case.circuit, dict(zip(case.ids, row)), variant=variant), want)
    assert changed >= 2, (variant, letter)


def test_the_panic_variant_moves_exactly_the_rows_without_a_tie():
    for t in (1, 2, 3, 4):
        case = sc.past_tuple_case(t)
        moved = [not same(sr.run(case.circuit, dict(zip(case.ids, row)), variant="panic_unreached"), x) for row, x in zip(case.rows, case.expect)]
        assert moved == [True, False] * 5


# ---- the scratch the planner reserves
SCRATCH_N = sorted(set(range(0, 1026)) | set(sc.SMALL_N) | set(sc.LARGE_N) | {33, 129, sc.N_BITS})


def test_the_walk_stays_inside_the_bounds_the_kernel_assumes():
    """op_perm_sort sizes its switch list n (lg + 1) + 1 words and its stack 72 frames: the walk's switch count and stack depth against them, and its
    high-water mark against the planner's formula, for n = 0 .. 1 025 and every n of the lists, with tuples of 1 .. 4"""
    for n in SCRATCH_N:
        lg = max(n - 1, 0).bit_length()
        for t in (1, 2, 3, 4):
            walk = sr.scratch_walk(n, t)
            assert walk.switches == sr.switch_count(n) <= n * (lg + 1) + 1, n
            assert walk.max_frames <= sr.STACK_FRAMES, (n, walk.max_frames)
            assert walk.high_water <= sr.scratch_reserved_formula(n, t), (n, t, walk.high_water)
    for n in (4095, 4096, 4097, 65535):   # the largest shapes the planner admits (n < 2^16)
        walk = sr.scratch_walk(n, 1)
        assert walk.high_water <= sr.scratch_reserved_formula(n, 1) and walk.max_frames <= sr.STACK_FRAMES and walk.switches <= n * (max(n - 1, 0).bit_length() + 1) + 1, n


def test_the_planner_reserves_what_the_formula_says():
    """the reservation the plan really carries (acvm_debug_record_scratch), for sorts of every n of the lists and the powers of two around them up to 1 025,
    tuples 1 .. 4: the restated formula, and so (above) at least the walk's high-water mark"""
    import acvm_amd
    for t in (1, 2, 3, 4):
        ns = sorted(set(sc.SMALL_N) | set(sc.LARGE_N) | {33, 129, 511, 512, 513, 1023, 1024, 1025})
        ops, first = [], 1
        for n in ns:
            ops.append(PermutationSort([[E.from_witness(first + i * t + k) for k in range(t)] for i in range(n)], t, [], [0]))
            first += n * t
        ids = list(range(1, first))
        got = acvm_amd.Circuit(Circuit(first, ops).to_bytes()).record_scratch(ids)
        assert got == [sr.scratch_reserved_formula(n, t) for n in ns], t
        assert all(sr.scratch_walk(n, t).high_water <= r for n, r in zip(ns, got))
    for case in EVERY_CASE:   # and the circuits of the lists themselves
        got = acvm_amd.Circuit(case.circuit.to_bytes()).record_scratch(case.ids)
        for op, r in zip(case.circuit.opcodes, got):
            if isinstance(op, PermutationSort):
                assert sr.scratch_walk(len(op.inputs), op.tuple).high_water <= r == sr.scratch_reserved_formula(len(op.inputs), op.tuple), case.name
