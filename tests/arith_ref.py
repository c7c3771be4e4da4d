"""Opcode::Arithmetic and the solve loop around it in Python integers, restated from the reference's Rust alone, arm by arm: no oracle, no device and no
product code here. tests/arith_cases.py builds the inputs, tests/test_arith_cases.py runs them through the CPU oracle, tests/test_gpu_arith_edges.py on
the device. tests/mem_ref.py takes evaluate, gate and insert_value from here.

run(circuit, witness map) solves the opcodes in program order (Arithmetic opcodes and RANGE readers) and returns Expect(status, err, opcode_index, aux0,
aux1, message, witnesses, branches, expression): the head as Result.as_tuple() carries it (aux0: the witness of MissingAssignment), the panic text, the WHOLE
witness map the reference leaves behind, the set of branch labels the run passed through (LABELS lists every one, UNREACHABLE the ones no input can
reach), and for a row that ends in ExpressionHasTooManyUnknowns the EVALUATED expression (mul, lin, q_c) the error carries.

The rules and where they stand:
  ArithmeticSolver::solve              acvm/src/pwg/arithmetic.rs:27-127   evaluate FIRST; then solve_mul_term and solve_fan_in_term on the evaluated
                                                                           expression, the mul term first (its panic goes before everything else)
      the six arms of the match        :38-42 TooManyUnknowns | Unsolvable; :43-67 OneUnknown x Solvable (w1 == w2 or not); :68-91 OneUnknown x Satisfied;
                                       :92-102 Solved x Satisfied; :103-125 Solved x Solvable
  solve_mul_term                       :133-144  0 terms: Solved(0); 1 term: the helper; more: panic
  solve_mul_term_helper                :146-161  by PRESENCE in the map: (None, None) TooManyUnknowns, else Solved / OneUnknown(q known, unknown)
  solve_fan_in_term                    :176-209  counts TERMS whose witness is absent (not witnesses); the last one is "the unknown"
  evaluate                             :212-239  product terms first, then linear terms; OneUnknown(v, w) is dropped where v == 0, an unknown product or an
                                                 unknown linear term where c == 0; known parts are summed into q_c; terms of one witness are NOT merged
  insert_value                         acvm/src/pwg/mod.rs:338-357   the map takes the new value FIRST, then the displaced one is compared
  RANGE                                acvm/src/pwg/blackbox/range.rs:7-18
  Display of FieldElement, Expression  acir_field/src/generic_ark.rs:13-74, acir/src/native_types/expression/mod.rs:40-48, circuit/opcodes.rs:88-102

evaluate leaves no witness of the map in the expression, so solve_mul_term_helper can only answer TooManyUnknowns on it and every coefficient it
leaves is non-zero: the arms OneUnknown x Solvable, OneUnknown x Satisfied and `coeff.is_zero()` cannot be reached. Nor can a gate displace a value: the
witness it assigns is one the map does not hold, so insert_value only ever inserts here (the memory opcodes of tests/mem_ref.py reach its other two ends). All
of these are restated all the same and tests/test_arith_cases.py asserts that no row reaches them.

A Variant is the same model wrong in ONE way; tests/test_arith_cases.py uses them to prove that each list of tests/arith_cases.py would notice."""
import collections

from acvm_amd.acir import P, Arithmetic, BlackBoxFuncCall, Expression

ST_SOLVED, ST_IN_PROGRESS, ST_FAILURE, ST_REQUIRES_FOREIGN_CALL = 0, 1, 2, 3  # ACVMStatus and the error kinds as oracle/binding.py numbers them
E_NONE, E_MISSING_ASSIGNMENT, E_TOO_MANY_UNKNOWNS, E_UNSATISFIED, E_INDEX_OOB, E_BRILLIG_FAILED, E_PANIC = 0, 1, 2, 4, 5, 7, 8

MSG_MUL_TERMS = b"Mul term in the arithmetic opcode must contain either zero or one term"  # arithmetic.rs:142

Expect = collections.namedtuple("Expect", "status err opcode_index aux0 aux1 message witnesses branches expression")

LABELS = (
    # evaluate, product terms
    "eval_mul_both_known", "eval_mul_left_unknown", "eval_mul_right_unknown", "eval_mul_folds_to_zero", "eval_mul_both_unknown", "eval_mul_both_unknown_zero_coef",
    # evaluate, linear terms
    "eval_lin_known", "eval_lin_unknown", "eval_lin_unknown_zero_coef", "eval_empty",
    # solve_mul_term
    "mul_none", "mul_one_too_many_unknowns", "mul_one_left_unknown", "mul_one_right_unknown", "mul_one_solved", "mul_panic",
    # solve_fan_in_term
    "fan_in_satisfied", "fan_in_solvable", "fan_in_unsolvable",
    # the arms of solve
    "arm_too_many_unknowns",
    "arm_one_unknown_solvable_same_zero_unsatisfied", "arm_one_unknown_solvable_same_zero_ok", "arm_one_unknown_solvable_same_assigns", "arm_one_unknown_solvable_differ",
    "arm_one_unknown_satisfied_zero_unsatisfied", "arm_one_unknown_satisfied_zero_ok", "arm_one_unknown_satisfied_assigns",
    "arm_solved_satisfied_ok", "arm_solved_satisfied_unsatisfied",
    "arm_solved_solvable_zero_unsatisfied", "arm_solved_solvable_zero_ok", "arm_solved_solvable_assigns",
    # insert_value
    "insert_new", "insert_same", "insert_differs",
    # RANGE
    "range_passes", "range_fails", "range_missing",
)
UNREACHABLE = tuple(l for l in LABELS if l.startswith(("arm_one_unknown_", "arm_solved_solvable_zero_", "mul_one_left", "mul_one_right", "mul_one_solved", "insert_same", "insert_differs")))

# ways in which a Variant is wrong (each names the rule it breaks)
VARIANTS = (
    "unknowns_by_witness",         # solve_fan_in_term merges the terms of one unknown witness (what the `w1 == w2` arm does with q + b): c x - c x is no unknown at all
    "folded_zero_kept",            # evaluate keeps OneUnknown(v, w) where v = c * known == 0
    "written_zero_counts",         # evaluate keeps an unknown term whose WRITTEN coefficient is zero
    "too_many_before_panic",       # the fan-in's verdict is looked at before the mul term's panic
    "zero_partner_assigns_zero",   # c * 0 * x + 0 = 0 assigns x = 0 where the reference assigns nothing
    "integer_zero_test",           # the sum is tested for zero as an integer, not modulo p
)

_SUP = "⁰¹²³⁴⁵⁶⁷⁸⁹"


def field_display(v):
    """impl Display for FieldElement, acir_field/src/generic_ark.rs:13-74, restated with Python integers"""
    v %= P
    if v == 0:
        return "0"
    minus = (P - v) % P
    neg = len(str(minus)) < len(str(v))
    s = minus if neg else v
    out = "-" if neg else ""
    if bin(s).count("1") == 1:
        bit = s.bit_length() - 1
        return out + (str(1 << bit) if bit < 4 else "2" + "".join(_SUP[int(d)] for d in str(bit)))
    for power in (64, 32, 16, 8, 4):
        if s % (1 << power) == 0:
            return out + "2" + "".join(_SUP[int(d)] for d in str(power)) + "×" + str(s >> power)
    return out + str(s)


def expr_display(mul, lin, qc):
    """impl Display for Expression (expression/mod.rs:40-48) over Opcode::Arithmetic's Debug text (circuit/opcodes.rs:88-102)"""
    if not mul and len(lin) == 1 and lin[0][0] % P == 1 and qc % P == 0:
        return f"x{lin[0][1]}"
    return "%EXPR [ " + "".join(f"({field_display(c)}, _{a}, _{b}) " for c, a, b in mul) + "".join(f"({field_display(c)}, _{w}) " for c, w in lin) + field_display(qc) + " ]%"


class Fail(Exception):
    def __init__(self, err, aux0=0, aux1=0, message=None, expression=None):
        self.head = (err, aux0, aux1, message)
        self.expression = expression


def _nothing(label):
    pass


def _mul_term_helper(term, wm):
    """solve_mul_term_helper: by presence in the map alone"""
    c, l, r = term
    if l not in wm and r not in wm:
        return ("TooManyUnknowns",)
    if l in wm and r in wm:
        return ("Solved", c * wm[l] * wm[r] % P)
    if l not in wm:
        return ("OneUnknown", c * wm[r] % P, l)
    return ("OneUnknown", c * wm[l] % P, r)


def evaluate(e, wm, hit=_nothing, variant=None, dropped=None):
    """ArithmeticSolver::evaluate: (mul_terms, linear_combinations, q_c) with every known witness folded into the constant. dropped: a list that takes the
    unknown witnesses of the product terms that folded to zero."""
    mul, lin, qc = [], [], 0
    for c, l, r in e.mul_terms:
        c %= P
        res = _mul_term_helper((c, l, r), wm)
        if res[0] == "OneUnknown":
            _, v, w = res
            hit("eval_mul_left_unknown" if w == l else "eval_mul_right_unknown")
            if v or variant == "folded_zero_kept":
                lin.append((v, w))
            else:
                hit("eval_mul_folds_to_zero")
                if dropped is not None:
                    dropped.append(w)
        elif res[0] == "TooManyUnknowns":
            hit("eval_mul_both_unknown")
            if c or variant == "written_zero_counts":
                mul.append((c, l, r))
            else:
                hit("eval_mul_both_unknown_zero_coef")
        else:
            hit("eval_mul_both_known")
            qc += res[1]
    for c, w in e.linear_combinations:
        c %= P
        if w in wm:
            hit("eval_lin_known")
            qc += c * wm[w] % P
        elif c or variant == "written_zero_counts":
            hit("eval_lin_unknown")
            lin.append((c, w))
        else:
            hit("eval_lin_unknown")
            hit("eval_lin_unknown_zero_coef")
    if not e.mul_terms and not e.linear_combinations:
        hit("eval_empty")
    qc += e.q_c % P
    return mul, lin, (qc if variant == "integer_zero_test" else qc % P)


def insert_value(wm, w, v, hit=_nothing):
    """the map takes the new value FIRST, then the displaced one is compared"""
    old = wm.get(w)
    wm[w] = v
    if old is not None and old != v:
        hit("insert_differs")
        raise Fail(E_UNSATISFIED)
    hit("insert_new" if old is None else "insert_same")


def _solve_mul_term(mul, wm, hit):
    if not mul:
        hit("mul_none")
        return ("Solved", 0)
    if len(mul) == 1:
        res = _mul_term_helper(mul[0], wm)
        hit("mul_one_too_many_unknowns" if res[0] == "TooManyUnknowns" else "mul_one_solved" if res[0] == "Solved" else
            "mul_one_left_unknown" if res[2] == mul[0][1] else "mul_one_right_unknown")
        return res
    hit("mul_panic")
    raise Fail(E_PANIC, message=MSG_MUL_TERMS)


def _solve_fan_in_term(lin, wm, hit, variant=None):
    """("Satisfied", sum) | ("Solvable", sum, (coefficient, witness)) | ("Unsolvable",)"""
    if variant == "unknowns_by_witness":
        merged = {}
        for c, w in lin:
            if w not in wm:
                merged[w] = (merged.get(w, 0) + c) % P
        lin = [t for t in lin if t[1] in wm] + [(c, w) for w, c in merged.items() if c]
    unknown, n_unknown, result = (0, 0), 0, 0
    for c, w in lin:
        if w in wm:
            result = (result + c * wm[w]) % P
        else:
            unknown = (c, w)
            n_unknown += 1
        if n_unknown > 1:
            hit("fan_in_unsolvable")
            return ("Unsolvable",)
    if n_unknown == 0:
        hit("fan_in_satisfied")
        return ("Satisfied", result)
    hit("fan_in_solvable")
    return ("Solvable", result, unknown)


def _is_zero(x, variant):
    return x == 0 if variant == "integer_zero_test" else x % P == 0


def gate(e, wm, hit=_nothing, variant=None):
    """ArithmeticSolver::solve"""
    dropped = []
    ev = evaluate(e, wm, hit, variant, dropped)
    mul, lin, qc = ev
    too_many = Fail(E_TOO_MANY_UNKNOWNS, expression=(list(mul), list(lin), qc % P))
    if variant == "too_many_before_panic" and sum(1 for _, w in lin if w not in wm) > 1:
        raise too_many
    mul_result = _solve_mul_term(mul, wm, hit)
    status = _solve_fan_in_term(lin, wm, hit, variant)

    def zero_or(kind, denominator, total, w):
        """the shape the three solving arms share: a zero denominator is an assert of the sum, else w = -total / denominator"""
        if denominator % P == 0:
            if not _is_zero(total, variant):
                hit(kind + "_zero_unsatisfied")
                raise Fail(E_UNSATISFIED)
            hit(kind + "_zero_ok")
            return
        hit(kind + "_assigns")
        insert_value(wm, w, -total * pow(denominator, -1, P) % P, hit)

    if mul_result[0] == "TooManyUnknowns" or status[0] == "Unsolvable":
        hit("arm_too_many_unknowns")
        raise too_many
    if mul_result[0] == "OneUnknown" and status[0] == "Solvable":
        _, q, w1 = mul_result
        _, a, (b, w2) = status
        if w1 != w2:
            hit("arm_one_unknown_solvable_differ")
            raise too_many
        return zero_or("arm_one_unknown_solvable_same", q + b, a + qc, w1)
    if mul_result[0] == "OneUnknown":
        _, partial_prod, w = mul_result
        return zero_or("arm_one_unknown_satisfied", partial_prod, status[1] + qc, w)
    if status[0] == "Satisfied":
        if not _is_zero(mul_result[1] + status[1] + qc, variant):
            hit("arm_solved_satisfied_unsatisfied")
            raise Fail(E_UNSATISFIED)
        hit("arm_solved_satisfied_ok")
        if variant == "zero_partner_assigns_zero" and len(set(dropped)) == 1:
            insert_value(wm, dropped[0], 0, hit)
        return
    _, partial_sum, (coeff, w) = status
    return zero_or("arm_solved_solvable", coeff, mul_result[1] + partial_sum + qc, w)


def range_check(op, wm, hit=_nothing):
    f = op.args["input"]
    if f.witness not in wm:
        hit("range_missing")
        raise Fail(E_MISSING_ASSIGNMENT, f.witness)
    if wm[f.witness].bit_length() > f.num_bits:
        hit("range_fails")
        raise Fail(E_UNSATISFIED)
    hit("range_passes")


def run(circ, wm, n_opcodes=None, variant=None, snapshots=None):
    """ACVM::solve over the opcodes in program order on a copy of the map wm; n_opcodes: stop after that many solve_opcode steps (a row that has not
    ended by then is InProgress and reports the opcode it stands on); snapshots: a list that takes, per step that succeeds, the (witness, value) pairs
    the step added to the map"""
    assert variant is None or variant in VARIANTS, variant
    wm = dict(wm)
    branches = set()

    def hit(label):
        assert label in LABELS, label
        branches.add(label)

    def end(status, err=E_NONE, at=0, aux0=0, aux1=0, message=None, expression=None):
        return Expect(status, err, at, aux0, aux1, message, wm, frozenset(branches), expression)

    n_seen = len(wm)
    for oi, op in enumerate(circ.opcodes):
        if n_opcodes is not None and oi == n_opcodes:
            return end(ST_IN_PROGRESS, at=oi)
        try:
            if isinstance(op, (Arithmetic, Expression)):
                gate(op.expr if isinstance(op, Arithmetic) else op, wm, hit, variant)
            elif isinstance(op, BlackBoxFuncCall) and op.name == "RANGE":
                range_check(op, wm, hit)
            else:
                raise AssertionError(f"no model for {op!r}")
        except Fail as f:
            err, aux0, aux1, message = f.head
            return end(ST_FAILURE, err, oi, aux0, aux1, message, f.expression)
        if snapshots is not None:
            snapshots.append([(w, wm[w]) for w in list(wm)[n_seen:]])
            n_seen = len(wm)
    return end(ST_SOLVED)
