"""The case lists of tests/int_cases.py against the CPU oracle (oracle/pwg.c, oracle/brillig_vm.c): status, error kind, failing opcode, panic text
and the whole witness map of every row must equal the Python expectation, and the lists must cover what they are built to cover (the minima
below are conditions on the inputs, which the builders meet by construction). No GPU: tests/test_gpu_int_edges.py runs the same lists on the device."""
import collections

import numpy as np
import pytest

import int_cases as ic
from acvm_amd.acir import Expression, P, ToLeRadix


def oracle_rows(oracle, case):
    """[(status, err, opcode_index, message, {witness: value})] of the oracle, one per row"""
    B = len(case.rows)
    values = b"".join(v.to_bytes(32, "big") for row in case.rows for v in row)
    res, asg, vals = oracle.solve_batch(oracle.Circuit(case.circuit.to_bytes()), case.ids, values, B)
    out = []
    for j in range(B):
        wm = {int(w): int.from_bytes(vals[j, w].tobytes(), "big") for w in np.flatnonzero(asg[j])}
        out.append((res[j].status, res[j].err, res[j].opcode_index, res[j].message, wm))
    return out


def test_error_codes_are_the_oracles(oracle):
    assert (ic.ST_SOLVED, ic.ST_FAILURE, ic.E_NONE, ic.E_UNSATISFIED, ic.E_PANIC) == (oracle.ST_SOLVED, oracle.ST_FAILURE, oracle.E_NONE, oracle.E_UNSATISFIED, oracle.E_PANIC)


@pytest.mark.parametrize("case", ic.all_cases(), ids=lambda c: c.name)
def test_oracle_agrees_with_integers(oracle, case):
    ic.compare(case, oracle_rows(oracle, case), "oracle")


def test_quotient_rows_cover_both_division_paths():
    pairs = [(a, b) for a, b, _ in ic.quotient_operands()]
    assert {b for _, b in pairs} >= set(ic.DIVISORS)
    by_shift = collections.Counter(ic.long_shift(a, b) for a, b in pairs)
    for s in ic.SHIFTS:
        assert by_shift[s] >= 3, (s, by_shift[s])
    assert min(s for s in by_shift if s is not None) == 1 and max(s for s in by_shift if s is not None) == 222
    # s with bits(b) = 33 (the narrowest divisor of the long path) and, where a dividend below P leaves room, a wider one
    for s in ic.SHIFTS:
        widths = {b.bit_length() for a, b in pairs if ic.long_shift(a, b) == s}
        assert 33 in widths and (len(widths) > 1 or s == 222), (s, widths)
    for s in ic.SHIFTS:  # the quotient patterns: all ones, the top bit alone, alternating bits
        qs = sorted({a // b for a, b in pairs if ic.long_shift(a, b) == s and a >= b})
        L = [q.bit_length() for q in qs]
        assert any(q == (1 << n) - 1 for q, n in zip(qs, L)) and any(q == 1 << (n - 1) for q, n in zip(qs, L))
        assert s <= 2 or any(q == int("a" * 64, 16) >> (256 - n) for q, n in zip(qs, L))
    small = [(a, b) for a, b in pairs if 0 < b < (1 << 32)]
    long_ = [(a, b) for a, b in pairs if b >= (1 << 32)]
    assert len(small) >= 40 and len(long_) >= 40 and sum(1 for a, b in long_ if ic.long_shift(a, b) is None) >= 5  # (a < b, shorter)
    assert sum(1 for a, b in pairs if b == 0) >= 3
    # quotient bits in every limb, the pre-shift with and without a bit part (bs == 0: s a multiple of 32)
    assert {(a // b).bit_length() - 1 >> 5 for a, b in long_ if a >= b} >= set(range(7))
    assert sum(1 for a, b in long_ if (ic.long_shift(a, b) or 1) % 32 == 0) >= 18


def test_quotient_case_covers_predicates_wraps_and_the_compared_output():
    case = ic.quotient_case()
    assert {row[2] for row in case.rows} == {0, 1, 2, P - 1}
    for pred in (0, 1, 2, P - 1):  # each predicate meets both paths with a nonzero quotient behind it
        assert sum(1 for row in case.rows if row[2] == pred and 0 < row[1] < (1 << 32) and row[0] >= row[1]) >= 10
        assert sum(1 for row in case.rows if row[2] == pred and row[1] >= (1 << 32) and row[0] >= row[1]) >= 10
    wraps = [row[4] + row[3] >= P for row in case.rows]
    assert sum(wraps) >= 100 and len(wraps) - sum(wraps) >= 100
    long_wraps = [ic.long_shift(row[0], row[1]) for row, w in zip(case.rows, wraps) if w]
    assert len({s for s in long_wraps if s is not None}) >= len(ic.SHIFTS) // 2
    failing = [x for x in case.expect if x.status == ic.ST_FAILURE]
    assert len(failing) >= 30 and all(x.err == ic.E_UNSATISFIED and x.opcode_index == 7 and 16 not in x.witnesses for x in failing)
    assert sum(1 for x in case.expect if x.status == ic.ST_SOLVED) >= 300
    for x, row in zip(case.expect, case.rows):  # the quotient of the gate outputs is the quotient of a and b again
        assert (x.witnesses[14], x.witnesses[15]) == (x.witnesses[8], x.witnesses[9]) and x.witnesses[12] == row[0] and x.witnesses[13] == row[1]


def test_radix_cases_cover_every_radix_and_limb_boundary():
    a, b = ic.radix_case_a(), ic.radix_case_b()
    on_input = [op for op in a.circuit.opcodes if isinstance(op, ToLeRadix) and op.a == Expression.from_witness(1)]
    assert a.circuit.opcodes[:19] == on_input and [op.radix for op in on_input] == ic.RADICES and len(b.circuit.opcodes) == len(ic.RADICES) == 19
    values = {row[0] for row in a.rows}
    for r in ic.RADICES:
        for k in (1, 2):
            assert {r ** k - 1, r ** k, r ** k + 1} <= values
        top = max(k for k in range(1, 256) if r ** k + 1 < P)
        assert {r ** top - 1, r ** top, r ** top + 1} <= values
    for m in range(1, 8):
        assert {(1 << 32 * m) - 1, 1 << 32 * m, (1 << 32 * m) + 1} <= values
    assert {0, 1, P - 1, P - 2} <= values
    # the alternating patterns, both phases: complements of each other in every bit below 2^253
    cut = (1 << 253) - 1
    assert {int("aa" * 32, 16) & cut, int("55" * 32, 16) & cut} <= values and (int("aa" * 32, 16) & cut) ^ (int("55" * 32, 16) & cut) == cut
    assert len({int(pat * 32, 16) & cut for pat in ic.ALTERNATING} & values) == len(ic.ALTERNATING) == 4  # (no two patterns collapse into one row)
    # the second group reads a gate output equal to the input, through sums that wrap past P and sums that do not
    behind = [op for op in a.circuit.opcodes if isinstance(op, ToLeRadix) and op not in on_input]
    assert [op.radix for op in behind] == ic.GATE_RADICES and len({op.a.linear_combinations[0][1] for op in behind}) == 1
    wraps = [row[1] + row[2] >= P for row in a.rows]
    assert sum(wraps) >= 50 and len(wraps) - sum(wraps) >= 50
    for op in behind:
        twin = on_input[ic.RADICES.index(op.radix)]
        assert all([x.witnesses[w] for w in op.b] == [x.witnesses[w] for w in twin.b] for x in a.expect)
    # the padding is visible: the two last outputs of every opcode are zero for P - 1, and the one before them is not
    top_row = a.expect[[row[0] for row in a.rows].index(P - 1)]
    for op in on_input + behind:
        assert top_row.witnesses[op.b[-1]] == top_row.witnesses[op.b[-2]] == 0 and top_row.witnesses[op.b[-3]] != 0
    # the digits of a power-of-two radix that straddle two limbs are nonzero somewhere (log2 r of 3, 5, 6, 7)
    for op in on_input + behind:
        log2r = op.radix.bit_length() - 1
        if op.radix & (op.radix - 1) or 32 % log2r == 0:
            continue
        straddling = [i for i in range(len(op.b) - 2) if (i * log2r) // 32 != (i * log2r + log2r - 1) // 32 and i * log2r + log2r <= 253]
        assert len(straddling) == sum(1 for m in range(1, 8) if 32 * m % log2r)  # (every limb boundary a digit can lie across)
        for i in straddling:
            digits = {x.witnesses[op.b[i]] for x in a.expect}
            assert len(digits) >= 3, (op.radix, i, digits)
    # circuit B: every radix passes for some row and is the failing opcode of some row
    failing = collections.Counter(x.opcode_index for x in b.expect if x.status == ic.ST_FAILURE)
    passing = collections.Counter(i for x in b.expect for i in range(x.opcode_index if x.status == ic.ST_FAILURE else len(ic.RADICES)))
    for i, r in enumerate(ic.RADICES):
        assert failing[i] >= 1 and passing[i] >= 1, r
        k, limit = ic.radix_limit(r)
        assert len(b.circuit.opcodes[i].b) == k and r ** (k - 1) <= (1 << 64) < limit
    assert all(x.err == ic.E_UNSATISFIED for x in b.expect if x.status == ic.ST_FAILURE)
    assert [c.circuit.opcodes[1].radix for c in ic.radix_panic_cases()] == [0, 1, 257]


def test_range_cases_cover_every_width_and_every_position():
    shared, own = ic.range_case_shared(), ic.range_case_distinct()
    for case in (shared, own):
        assert sorted(op.args["input"].num_bits for op in case.circuit.opcodes) == list(range(257))
    values = {row[0] for row in shared.rows}
    assert all({(1 << k) - 1, 1 << k} <= values for k in range(254)) and {0, P - 1} <= values
    failed_width, passed_width, positions = set(), set(), set()
    for case in (shared, own):
        widths = [op.args["input"].num_bits for op in case.circuit.opcodes]
        for x in case.expect:
            n = x.opcode_index if x.status == ic.ST_FAILURE else len(widths)
            passed_width.update(widths[:n])
            if x.status == ic.ST_FAILURE:
                assert x.err == ic.E_UNSATISFIED
                failed_width.add(widths[n])
                positions.add(n % 8)
    # a value below P has at most 254 bits: widths 254..256 cannot fail, every other one does; every width passes somewhere
    assert failed_width == set(range(254)) and passed_width == set(range(257))
    assert positions == set(range(8))
    # with one witness, the first failing opcode is decided by the order: the prefix minima of the widths
    widths = [op.args["input"].num_bits for op in shared.circuit.opcodes]
    minima = {i for i, b in enumerate(widths) if b == min(widths[:i + 1])}
    assert {x.opcode_index for x in shared.expect if x.status == ic.ST_FAILURE} == minima - {i for i in minima if widths[i] >= 254}
    # own witnesses: rows where several checks fail. The two lowest failing opcodes lie in one merged record (eight opcodes in program order),
    # in one of its groups of four or one in each, so that the lowest must win inside a group and across the groups
    ops = own.circuit.opcodes
    same_four = across_fours = 0
    for row, x in zip(own.rows, own.expect):
        fails = [i for i, op in enumerate(ops) if row[op.args["input"].witness - 1].bit_length() > op.args["input"].num_bits]
        if len(fails) >= 2:
            assert x.status == ic.ST_FAILURE and x.opcode_index == fails[0] and fails[0] // 8 == fails[1] // 8, fails
            same_four += fails[0] // 4 == fails[1] // 4
            across_fours += fails[0] // 4 != fails[1] // 4
    assert same_four >= 20 and across_fours >= 20, (same_four, across_fours)
    assert any(x.status == ic.ST_SOLVED for x in own.expect) and any(x.status == ic.ST_SOLVED for x in shared.expect)


def test_logic_case_covers_every_width_and_the_reduction():
    case = ic.logic_case()
    assert len(case.circuit.opcodes) == 514 and all(x.status == ic.ST_SOLVED for x in case.expect)
    assert sorted(op.args["lhs"].num_bits for op in case.circuit.opcodes if op.name == "AND") == list(range(257))
    assert sorted(op.args["lhs"].num_bits for op in case.circuit.opcodes if op.name == "XOR") == list(range(257))
    reduced = [row for row in case.rows if row[0] ^ row[1] >= P]
    assert len(reduced) >= 10
    for row, x in zip(case.rows, case.expect):
        for b in (0, 1, 31, 32, 33, 253, 254, 255, 256):  # spot values, written out once more
            assert x.witnesses[3 + b] == (row[0] & row[1]) % (1 << b) % P and x.witnesses[260 + b] == (row[0] ^ row[1]) % (1 << b) % P
    assert {(1 << k) - 1 for k in range(254)} <= {row[0] for row in case.rows}


def test_brillig_cases_cover_the_sign_classes_and_the_panics():
    cases = {c.name: c for c in ic.brillig_cases()}
    assert len(cases) == 8
    for op, widths in ic.INT_WIDTHS.items():
        for bits in widths:
            case = cases[f"{op} at {bits} bits"]
            solved = [x for x in case.expect if x.status == ic.ST_SOLVED]
            panics = [x for x in case.expect if x.status == ic.ST_FAILURE]
            assert len(solved) >= 200 and len(panics) >= 3 and all(x.err == ic.E_PANIC and x.opcode_index == 0 for x in panics)
            assert all(x.witnesses[3] == x.witnesses[4] for x in solved)
            if op == "UnsignedDiv":  # both paths of canon_divrem behind the mask
                m = 1 << bits
                assert sum(1 for a, b in case.rows if 0 < b % m < (1 << 32)) >= 40 and sum(1 for a, b in case.rows if b % m >= (1 << 32) and a % m >= b % m) >= 40
            elif bits < 256:
                for side in (0, 1):
                    classes = collections.Counter(ic.sign_class(row[side], bits) for row in case.rows)
                    assert all(classes[c] >= 3 for c in (0, 1, 2)), (bits, side, classes)
                h = 1 << (bits - 1)
                rows = {tuple(row) for row in case.rows}
                assert {(h, 2 * h - 1), (2 * h - 1, 1), (1, 2 * h - 1), (7, 0), (77, 2 * h)} <= rows
                # signs differ and the quotient is nonzero: the result is 2^bits - q; and the quotient that passes 2^bits panics
                assert sum(1 for row, x in zip(case.rows, case.expect) if x.status == ic.ST_SOLVED and {ic.sign_class(row[0], bits), ic.sign_class(row[1], bits)} == {0, 1}
                           and x.witnesses[3] >= h) >= 5
                assert case.expect[case.rows.index([P - 1, 2 * h - 1])].status == ic.ST_FAILURE
