"""One builder of the inputs that reach every branch of the cheap integer opcodes (acvm_amd/csrc/ops_light.hpp: canon_divrem, op_to_le_radix,
op_range / op_range_multi, op_logic, int_op_core), with every expected outcome in Python integers: no oracle and no device here. Random
operands essentially never reach those branches (two random 254-bit operands leave the restoring division 1-3 steps), so every list below is
built by bit length, by limb boundary or by digit count. tests/test_int_cases.py runs the lists through the CPU oracle and asserts what they
cover; tests/test_gpu_int_edges.py runs them on the device.

A case is (name, circuit, ids, rows, expect, labels, notes): the circuit, its initial witness ids, one list of initial values per instance, and
per instance Expect(status, err, opcode_index, witnesses, message) -- `witnesses` is the WHOLE witness map the reference leaves behind (the
initial witnesses and everything assigned before the failing opcode), `message` the panic text where there is one. labels: witness -> what it
is (for assertion messages), notes: per row, what the row is for.

The rules restated by model() below:
  Arithmetic gates        acvm/src/pwg/arithmetic.rs:27-127 (only the shape used here: every term known but one linear unknown)
  insert_value            acvm/src/pwg/mod.rs:338-357 (an assigned witness takes the new value, then the old one is compared)
  Directive::Quotient     acvm/src/pwg/directives/mod.rs:28-59
  Directive::ToLeRadix    acvm/src/pwg/directives/mod.rs:60-87, num-bigint BigUint::to_radix_le (0 -> [0], radix outside 2..=256 panics)
  RANGE                   acvm/src/pwg/blackbox/range.rs:7-18, acir_field/src/generic_ark.rs:214-221 (num_bits)
  AND / XOR               acvm/src/pwg/blackbox/logic.rs:11-56, acir_field/src/generic_ark.rs:322-355,446-473
  Brillig BinaryIntOp     brillig_vm/src/arithmetic.rs:23-98 (ref_int_op); the VM around it is tests/brillig_ref.py"""
import collections
import functools
import random

from acvm_amd.acir import (P, Arithmetic, BlackBoxFuncCall as BB, Brillig, Circuit, Expression as E, FunctionInput as FI, QuotientDirective,
                           ToLeRadix)

SEED = 20261                      # of every random draw below
ST_SOLVED, ST_FAILURE = 0, 2      # ACVMStatus as oracle/binding.py numbers it (tests/test_int_cases.py asserts that these agree)
E_NONE, E_UNSATISFIED, E_PANIC = 0, 4, 8
RADIX_PANIC = b"The radix must be within 2...256"

Expect = collections.namedtuple("Expect", "status err opcode_index witnesses message")
Case = collections.namedtuple("Case", "name circuit ids rows expect labels notes")


def ref_int_op(op, a, b, bits):
    """evaluate_binary_bigint_op (brillig_vm/src/arithmetic.rs:23-98) with Python integers, then FieldElement::from_be_bytes_reduce: the
    reference's BigUint arithmetic takes ANY bit_size. Returns the field value, or None where the reference panics."""
    m = 1 << bits

    def signed(x):
        return x if x < (1 << (bits - 1)) else x - 2 * (1 << (bits - 1))
    if op == "Add":
        r = (a + b) % m
    elif op == "Sub":
        r = (m + a - b) % m if m + a - b >= 0 else None
    elif op == "Mul":
        r = (a * b) % m
    elif op == "UnsignedDiv":
        r = (a % m) // (b % m) if b % m else None
    elif op == "SignedDiv":
        if bits == 0 or signed(b) == 0:
            return None
        sa, sb = signed(a), signed(b)
        q = abs(sa) // abs(sb) * (1 if (sa < 0) == (sb < 0) else -1)  # BigInt division truncates toward zero
        r = q if q >= 0 else (m + q if m + q >= 0 else None)
    elif op in ("Equals", "LessThan", "LessThanEquals"):
        x, y = a % m, b % m
        r = int(x == y if op == "Equals" else x < y if op == "LessThan" else x <= y)
    elif op in ("And", "Or", "Xor"):
        r = (a & b if op == "And" else a | b if op == "Or" else a ^ b) % m
    else:
        return None
    return None if r is None else r % P


# ---- the reference's rules on a witness map {witness: integer below P}
def sign_class(x, bits):
    """which branch of int_to_signed (ops_light.hpp; to_big_signed, arithmetic.rs:83-90) x takes: 0 below 2^(bits-1), 1 (negative) below
    2^bits, 2 at or above 2^bits (x - 2^bits, non-negative again)"""
    return 0 if x < (1 << (bits - 1)) else 1 if x < (1 << bits) else 2


def to_radix_le(v, radix):
    """BigUint::to_radix_le: little-endian digits, [0] for zero"""
    digits = []
    while v:
        v, d = divmod(v, radix)
        digits.append(d)
    return digits or [0]


def mask_bits(v, num_bits):
    """mask_to_be_bytes (generic_ark.rs:322-326) + mask_vector_le (:446-473) as written: on the little-endian bytes, the bytes below
    num_bits / 8 stay, the one at it keeps its low num_bits % 8 bits, the ones above are cleared"""
    le = bytearray(v.to_bytes(32, "little"))
    at = num_bits // 8
    for i in range(32):
        if i == at:
            le[i] &= (1 << (num_bits % 8)) - 1
        elif i > at:
            le[i] = 0
    return int.from_bytes(le, "little")


def _value(e, wm):
    """get_value (pwg/mod.rs:321-332) of an expression whose witnesses are all assigned"""
    acc = e.q_c
    for c, l, r in e.mul_terms:
        acc += c * wm[l] * wm[r]
    for c, w in e.linear_combinations:
        acc += c * wm[w]
    return acc % P


def _insert(wm, w, v):
    """insert_value (pwg/mod.rs:338-357): the map takes the new value FIRST, then the displaced one is compared; False = UnsatisfiedConstrain"""
    old = wm.get(w)
    wm[w] = v
    return old is None or old == v


def _step(op, wm):
    """one opcode on the witness map: None, or (error kind, message) of the failure"""
    unsat = (E_UNSATISFIED, None)
    if isinstance(op, Arithmetic):
        op = op.expr
    if isinstance(op, E):  # arithmetic.rs:27-127 with at most one unknown, in a linear term
        acc, unknown = op.q_c, []
        for c, l, r in op.mul_terms:
            acc += c * wm[l] * wm[r]
        for c, w in op.linear_combinations:
            if w in wm:
                acc += c * wm[w]
            elif c % P:
                unknown.append((c, w))
        assert len(unknown) <= 1, "the model solves one linear unknown"
        if not unknown:
            return None if acc % P == 0 else unsat
        wm[unknown[0][1]] = -acc * pow(unknown[0][0], -1, P) % P
        return None
    if isinstance(op, QuotientDirective):  # directives/mod.rs:28-59: q is inserted before r
        a, b = _value(op.a, wm), _value(op.b, wm)
        pred = _value(op.predicate, wm) if op.predicate is not None else 1
        q, r = (0, 0) if pred == 0 or b == 0 else divmod(a, b)
        return None if _insert(wm, op.q, q) and _insert(wm, op.r, r) else unsat
    if isinstance(op, ToLeRadix):  # directives/mod.rs:60-87
        v = _value(op.a, wm)
        if not 2 <= op.radix <= 256:
            return (E_PANIC, RADIX_PANIC)
        digits = to_radix_le(v, op.radix)
        if len(op.b) < len(digits):
            return unsat
        for i, w in enumerate(op.b):
            if not _insert(wm, w, digits[i] if i < len(digits) else 0):
                return unsat
        return None
    if isinstance(op, BB) and op.name == "RANGE":  # range.rs:7-18
        f = op.args["input"]
        return unsat if wm[f.witness].bit_length() > f.num_bits else None
    if isinstance(op, BB) and op.name in ("AND", "XOR"):  # logic.rs:11-56
        l, r = op.args["lhs"], op.args["rhs"]
        assert l.num_bits == r.num_bits
        x, y = mask_bits(wm[l.witness], l.num_bits), mask_bits(wm[r.witness], r.num_bits)
        return None if _insert(wm, op.args["output"], (x ^ y if op.name == "XOR" else x & y) % P) else unsat
    if isinstance(op, Brillig):  # the whole VM: tests/brillig_ref.py (imported here: that module takes ref_int_op from this one)
        import brillig_ref
        out = brillig_ref.run(op, wm)
        assert out.kind in (brillig_ref.SOLVED, brillig_ref.PANIC, brillig_ref.UNSATISFIED), out
        return None if out.kind == brillig_ref.SOLVED else (E_PANIC, None) if out.kind == brillig_ref.PANIC else unsat
    raise AssertionError(f"no model for {op!r}")


def model(circ, ids, row):
    """the reference's solve loop (pwg/mod.rs:203-304) over the opcodes in program order"""
    wm = dict(zip(ids, row))
    for oi, op in enumerate(circ.opcodes):
        bad = _step(op, wm)
        if bad:
            return Expect(ST_FAILURE, bad[0], oi, wm, bad[1])
    return Expect(ST_SOLVED, E_NONE, 0, wm, None)


# ---- comparing a run with the expectation
def describe(case, j):
    return f"{case.name} row {j} ({case.notes[j]}), inputs {[hex(v) for v in case.rows[j][:8]]}"


def describe_opcode(case, i):
    """opcode i of the case's circuit by what decides its outcome: the width, the radix, the operation"""
    if not 0 <= i < len(case.circuit.opcodes):
        return f"opcode {i} (none)"
    op = case.circuit.opcodes[i]
    if isinstance(op, BB):
        f = op.args.get("input") or op.args["lhs"]
        what = f"{op.name} of width {f.num_bits} on witness {f.witness}"
    elif isinstance(op, ToLeRadix):
        what = f"ToLeRadix, radix {op.radix}, {len(op.b)} outputs"
    elif isinstance(op, QuotientDirective):
        what = f"Quotient into witnesses {op.q}, {op.r}"
    elif isinstance(op, Brillig):
        what = f"Brillig {op.bytecode[0][2]} at {op.bytecode[0][3]} bits"
    else:
        what = "gate"
    return f"opcode {i} ({what})"


def compare(case, got, who):
    """got: rows as oracle_rows returns them"""
    for j, (want, (status, err, opcode, message, wm)) in enumerate(zip(case.expect, got)):
        at = describe(case, j)
        assert (status, err) == (want.status, want.err), f"{at}: {who} status / error {(status, err)}, want {(want.status, want.err)}"
        if want.status == ST_FAILURE:
            assert opcode == want.opcode_index, f"{at}: {who} fails at {describe_opcode(case, opcode)}, want {describe_opcode(case, want.opcode_index)}"
        if want.message is not None:
            assert message == want.message, f"{at}: {who} message {message!r}, want {want.message!r}"
        for w in sorted(set(wm) | set(want.witnesses)):
            g, x = wm.get(w), want.witnesses.get(w)
            assert g == x, (f"{at}: witness {w} ({case.labels.get(w, 'input')}): {who} " + (hex(g) if g is not None else "unassigned") +
                            ", want " + (hex(x) if x is not None else "unassigned"))


def _case(name, circ, ids, rows, labels, notes):
    assert len(rows) == len(notes) and len(rows) % 64, (name, len(rows))  # (batches stay off the multiples of the wave size)
    assert all(0 <= v < P for row in rows for v in row), name
    return Case(name, circ, ids, rows, [model(circ, ids, row) for row in rows], labels, notes)


def _pad(rows, notes, filler):
    """one more row where the count is a multiple of 64"""
    if len(rows) % 64 == 0:
        rows.append(filler)
        notes.append("filler")


# ---- Quotient
DIVISORS = [0, 1, 2, 3, 255, 256, 1 << 16, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 33) - 1, 1 << 63, 1 << 64, (1 << 64) + 1,
            (1 << 96) - 1, 1 << 128, (1 << 200) + 7, P // 2, P - 1]
SHIFTS = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 221, 222]  # s of canon_divrem's long path


def long_shift(a, b):
    """s = bits(a) - bits(b) + 1 of canon_divrem's restoring division, or None where the pair does not get there (b < 2^32: the 64-by-32
    path; b = 0; a shorter than b)"""
    if b < (1 << 32) or a.bit_length() < b.bit_length():
        return None
    return a.bit_length() - b.bit_length() + 1


@functools.lru_cache(maxsize=None)
def quotient_operands():
    """[(a, b, note)]: every divisor of DIVISORS with dividends around its multiples, then the pairs built by bit length"""
    rng = random.Random(SEED)
    out, seen = [], set()

    def add(a, b, note):
        if 0 <= a < P and (a, b) not in seen:
            seen.add((a, b))
            out.append((a, b, note))

    for b in DIVISORS:
        for k in (1, 3, (1 << 32) - 1, (1 << 64) + 3, (P - 1) // b if b else 0):
            for d in (-1, 0, 1):
                add(k * b + d, b, f"{k:#x} * b {d:+d}")
        for a, note in ((b - 1, "b - 1"), (b, "b"), (b + 1, "b + 1"), (2 * b - 1, "2b - 1"), (P - 1, "P - 1"), (0, "0")):
            add(a, b, note)
    # by bit length: q of s or s - 1 bits times a divisor of nb bits, plus a remainder, until bits(a) - nb + 1 is the s wanted
    for s in SHIFTS:
        widths = sorted({33, min(65, 255 - s), min(130, 255 - s), 255 - s} - set(range(33)))
        for nb in widths:
            for pattern in ("ones", "top bit", "alternating"):
                for attempt in range(400):
                    L = s - (attempt & 1)
                    if L <= 0:
                        continue
                    q = {"ones": (1 << L) - 1, "top bit": 1 << (L - 1), "alternating": int("a" * 64, 16) >> (256 - L)}[pattern]
                    b = rng.randrange(1 << (nb - 1), 1 << nb)
                    a = q * b + rng.randrange(b)
                    if a < P and long_shift(a, b) == s:
                        add(a, b, f"s = {s}, bits(b) = {nb}, quotient {pattern}")
                        break
                else:
                    raise AssertionError(f"no pair for s = {s}, bits(b) = {nb}, {pattern}")
    return tuple(out)


PREDICATES = [1, 1, 2, P - 1, 1, 0, 1, 2]   # by row; 0 switches the division off (directives/mod.rs:41-45)


@functools.lru_cache(maxsize=None)
def quotient_case():
    """Witnesses 1..7 are inputs: a, b, predicate, t, a - t, b - t, the expected q of opcode 7 (or a wrong one). Opcodes: 0 the plain
    quotient; 1 with the predicate; 2-5 gates w12 = w5 + w4, w13 = w6 + w4 (with coefficient 2), w17 = 5 w12 + w13, w18 = w13, whose sums
    wrap past P for about half of the rows; 6 the quotient of w12 by 3 w13 - 2 w18 (= a by b again), witnesses that gates read too; 7 the
    quotient whose q (witness 7) is already assigned: every 9th row carries q + 1 there and fails at opcode 7 with r unassigned."""
    W = E.from_witness
    ops = [QuotientDirective(W(1), W(2), 8, 9),
           QuotientDirective(W(1), W(2), 10, 11, predicate=W(3)),
           E([], [(1, 5), (1, 4), (P - 1, 12)], 0),
           E([], [(2, 6), (2, 4), (P - 2, 13)], 0),
           E([], [(5, 12), (1, 13), (P - 1, 17)], 0),
           E([], [(1, 13), (P - 1, 18)], 0),
           QuotientDirective(E([], [(1, 12)], 0), E([], [(3, 13), (P - 2, 18)], 0), 14, 15),
           QuotientDirective(W(1), W(2), 7, 16)]
    circ = Circuit(18, ops)
    rng = random.Random(SEED + 1)
    rows, notes = [], []
    for j, (a, b, note) in enumerate(quotient_operands()):
        t = rng.randrange(P) if j % 2 else rng.randrange(1 << 16)  # (a random t above a makes a - t + t wrap)
        q = a // b if b else 0
        rows.append([a, b, PREDICATES[j % len(PREDICATES)], t, (a - t) % P, (b - t) % P, (q + 1) % P if j % 9 == 4 else q])
        notes.append(note)
    _pad(rows, notes, [7, 2, 1, 0, 7, 2, 3])
    labels = {8: "q of Quotient(a, b)", 9: "r of Quotient(a, b)", 10: "q of Quotient(a, b, predicate)", 11: "r of Quotient(a, b, predicate)",
              12: "gate a - t + t", 13: "gate b - t + t", 17: "gate 5 w12 + w13", 18: "gate w13", 14: "q of Quotient(gate outputs)",
              15: "r of Quotient(gate outputs)", 7: "q given", 16: "r of Quotient(a, b) with q given"}
    return _case("quotient", circ, [1, 2, 3, 4, 5, 6, 7], rows, labels, notes)


# ---- ToLeRadix
RADICES = [2, 3, 4, 5, 7, 8, 10, 16, 17, 31, 32, 33, 64, 100, 127, 128, 129, 255, 256]


ALTERNATING = ("aa", "55", "f0", "e3")
GATE_RADICES = [8, 10, 32, 64, 128, 255]   # of circuit A's second group, which reads a gate output


def radix_values():
    """[(value, note)] of circuit A"""
    out = [(0, "0"), (1, "1"), (P - 1, "P - 1"), (P - 2, "P - 2")]
    for r in RADICES:
        top = len(to_radix_le(P - 1, r)) - 1
        while r ** top + 1 >= P:
            top -= 1
        for k in (1, 2, top):
            out += [(r ** k + d, f"{r}^{k} {d:+d}") for d in (-1, 0, 1)]
    for m in range(1, 8):  # the limb boundaries of the funnel shift
        out += [((1 << 32 * m) + d, f"2^{32 * m} {d:+d}") for d in (-1, 0, 1)]
    for pat in ALTERNATING:  # (cut by masking, not by shifting: 0xaa.. and 0x55.. stay complements of each other in every limb)
        out.append((int(pat * 32, 16) & ((1 << 253) - 1), f"0x{pat}.. below 2^253"))
    seen, uniq = set(), []
    for v, note in out:
        if v not in seen:
            seen.add(v)
            uniq.append((v, note))
    return uniq


@functools.lru_cache(maxsize=None)
def radix_case_a():
    """Inputs: witness 1 = v, 2 = t, 3 = v - t. Opcodes 0..18: one ToLeRadix per radix on witness 1, each with two outputs more than P - 1 has
    digits: nothing fails, the padding shows. Then the gates g = w3 + w2 (= v again; the sum wraps past P in about half of the rows) and
    h = 3 g + w1, and one ToLeRadix per radix of GATE_RADICES on g, a witness that a gate reads too: by default the planner may store such a
    row relaxed or scaled and must hand the directive the reduced value (tuning relax / scale)."""
    ops, labels, nxt = [], {}, 4

    def radix_op(src, r, what):
        nonlocal nxt
        n_out = len(to_radix_le(P - 1, r)) + 2
        outs = list(range(nxt, nxt + n_out))
        nxt += n_out
        labels.update({w: f"digit {i} in radix {r}{what}" for i, w in enumerate(outs)})
        ops.append(ToLeRadix(E.from_witness(src), outs, r))

    for r in RADICES:
        radix_op(1, r, "")
    g, h = nxt, nxt + 1
    nxt += 2
    labels[g], labels[h] = "gate v - t + t", "gate 3 g + v"
    ops += [E([], [(1, 3), (1, 2), (P - 1, g)], 0), E([], [(3, g), (1, 1), (P - 1, h)], 0)]
    for r in GATE_RADICES:
        radix_op(g, r, " of the gate output")
    rng = random.Random(SEED + 6)
    vals = radix_values()
    rows, notes = [], [n for _, n in vals]
    for j, (v, _) in enumerate(vals):
        t = rng.randrange(v + 1, P) if j % 2 and v < P - 1 else rng.randrange(v + 1)  # odd rows: t above v, so (v - t mod P) + t wraps
        rows.append([v, t, (v - t) % P])
    _pad(rows, notes, [12345, 5, 12340])
    case = _case("radix A", Circuit(nxt - 1, ops), [1, 2, 3], rows, labels, notes)
    assert all(x.status == ST_SOLVED and x.witnesses[g] == row[0] for x, row in zip(case.expect, case.rows))
    return case


def radix_limit(r):
    """(k_r, r^k_r): the digit count of 2^64 in radix r, and the first value with a digit more"""
    k = len(to_radix_le(1 << 64, r))
    return k, r ** k


@functools.lru_cache(maxsize=None)
def radix_case_b():
    """One ToLeRadix per radix with k_r outputs, radix i on input witness 1 + i (of their own: several limits coincide -- 2^65 for 2 and 32,
    2^66 for 4, 8 and 64 -- so with a shared input some radix could never be the first to fail). Rows: every input at its r^k_r - 1 (all pass);
    per radix, its own input at r^k_r (fails there and nowhere else); the same value on every input (the first radix in program order whose
    limit it reaches fails); two inputs over their limits (the lower opcode wins)."""
    n = len(RADICES)
    ids = list(range(1, n + 1))
    ops, labels, nxt = [], {}, n + 1
    for i, r in enumerate(RADICES):
        k = radix_limit(r)[0]
        outs = list(range(nxt, nxt + k))
        nxt += k
        labels.update({w: f"digit {d} in radix {r}" for d, w in enumerate(outs)})
        ops.append(ToLeRadix(E.from_witness(ids[i]), outs, r))
    below = [radix_limit(r)[1] - 1 for r in RADICES]
    rows, notes = [list(below)], ["every input at r^k_r - 1"]
    for i, r in enumerate(RADICES):
        rows.append(below[:i] + [below[i] + 1] + below[i + 1:])
        notes.append(f"radix {r} at r^k_r = {r}^{radix_limit(r)[0]}")
    for v, note in ((0, "0"), (1 << 64, "2^64"), ((1 << 65) - 1, "2^65 - 1"), (1 << 65, "2^65"), (1 << 66, "2^66"), (3 ** 41, "3^41"), (1 << 70, "2^70"), (1 << 72, "2^72"),
                    (P - 1, "P - 1")):
        rows.append([v] * n)
        notes.append(f"{note} on every input")
    for i, k in ((3, 11), (7, 8), (12, 18), (0, 18)):
        row = list(below)
        row[i] += 1
        row[k] = P - 1
        rows.append(row)
        notes.append(f"radices {RADICES[i]} and {RADICES[k]} over their limits")
    _pad(rows, notes, [5] * n)
    return _case("radix B", Circuit(nxt - 1, ops), ids, rows, labels, notes)


@functools.lru_cache(maxsize=None)
def radix_panic_cases():
    """radix 0, 1 and 257: num-bigint's assert, behind a radix that passes"""
    out = []
    for r in (0, 1, 257):
        circ = Circuit(12, [ToLeRadix(E.from_witness(1), [2, 3, 4], 16), ToLeRadix(E.from_witness(1), [5, 6, 7, 8, 9, 10, 11, 12], r)])
        rows = [[0], [1], [255], [256], [4095]]
        case = _case(f"radix {r}", circ, [1], rows, {2: "digit 0 in radix 16", 3: "digit 1 in radix 16", 4: "digit 2 in radix 16"}, ["panics"] * len(rows))
        assert all(x.err == E_PANIC and x.opcode_index == 1 and x.message == RADIX_PANIC for x in case.expect)
        out.append(case)
    return tuple(out)


# ---- RANGE
def range_order(seed):
    order = list(range(257))
    random.Random(seed).shuffle(order)
    return order


@functools.lru_cache(maxsize=None)
def range_case_shared():
    """257 RANGE opcodes, widths 0..256 in a seeded order, all on witness 1: the opcode that fails is the first in program order whose width is
    below the value's bit length, which the order puts at every position of a merged record of eight"""
    order = range_order(SEED + 2)
    circ = Circuit(1, [BB("RANGE", {"input": FI(1, b)}) for b in order])
    rows, notes = [], []
    for k in range(254):
        rows += [[(1 << k) - 1], [1 << k]]
        notes += [f"2^{k} - 1", f"2^{k}"]
    rows += [[P - 1], [0]]
    notes += ["P - 1", "0"]
    _pad(rows, notes, [5])
    return _case("range, one witness", circ, [1], rows, {}, notes)


@functools.lru_cache(maxsize=None)
def range_case_distinct():
    """The same widths in another order, the check of width b on its own witness 1 + b: per width below 254 a row where that check alone
    fails (2^b against width b), rows where two to five checks of one merged record (eight opcodes in program order) fail at once -- the two
    lowest in one of its groups of four, or one in each -- and the lowest opcode must win, and rows where everything passes at 2^b - 1."""
    order = range_order(SEED + 3)
    circ = Circuit(257, [BB("RANGE", {"input": FI(1 + b, b)}) for b in order])
    ids = list(range(1, 258))
    rng = random.Random(SEED + 4)
    full = [min((1 << b) - 1, P - 1) for b in range(257)]  # (by witness: the largest value of its width)
    rows, notes = [list(full), [0] * 257], ["every witness at 2^b - 1", "0"]
    for b in range(254):
        row = list(full) if b % 2 else [0] * 257
        row[b] = 1 << b
        rows.append(row)
        notes.append(f"2^{b} against width {b}")
    for k in range(48):  # opcodes 8 m .. 8 m + 7 are one merged record, which the kernel walks in two groups of four
        at = 8 * rng.randrange(32)
        lo4, hi4 = ([b for b in order[i:i + 4] if b < 254] for i in (at, at + 4))
        if k % 2 and len(lo4) >= 2:   # the two lowest failures in the first group of four
            fail = rng.sample(lo4, 2) + rng.sample(hi4, min(len(hi4), rng.randrange(0, 3)))
        else:                         # one failure in each group: the lowest must win across the groups
            fail = rng.sample(lo4, 1) + rng.sample(hi4, min(len(hi4), rng.randrange(1, 4)))
        row = [rng.randrange(1 << b) if b else 0 for b in range(257)]
        row = [min(v, P - 1) for v in row]
        for b in fail:
            row[b] = min((1 << b) + (rng.randrange(1 << b) if rng.random() < 0.5 else 0), P - 1)
        rows.append(row)
        notes.append(f"widths {sorted(fail)} fail, opcodes {at}..{at + 7}")
    _pad(rows, notes, [0] * 257)
    return _case("range, own witnesses", circ, ids, rows, {}, notes)


# ---- AND / XOR
@functools.lru_cache(maxsize=None)
def logic_case():
    """AND and XOR at every width 0..256 on witnesses 1 and 2: AND of width b into witness 3 + b, XOR into 260 + b"""
    ops, labels = [], {}
    for b in range(257):
        ops.append(BB("AND", {"lhs": FI(1, b), "rhs": FI(2, b), "output": 3 + b}))
        ops.append(BB("XOR", {"lhs": FI(1, b), "rhs": FI(2, b), "output": 260 + b}))
        labels[3 + b], labels[260 + b] = f"AND at width {b}", f"XOR at width {b}"
    circ = Circuit(260 + 256, ops)
    rng = random.Random(SEED + 5)
    rows = [[rng.randrange(P), rng.randrange(P)] for _ in range(24)]
    notes = ["random"] * len(rows)
    for k in range(0, 254):
        rows.append([(1 << k) - 1, rng.randrange(P) if k % 3 else P - 1])
        notes.append(f"2^{k} - 1")
    rows += [[P - 1, P - 1], [0, 0], [P - 1, 0], [0, P - 1]]
    notes += ["P - 1, P - 1", "0, 0", "P - 1, 0", "0, P - 1"]
    # XOR at or above P: from_be_bytes_reduce subtracts (widths 254..256 only; an AND never exceeds its operands)
    for v in (P, P + 1, P + 12345, (1 << 254) - 1, (1 << 254) - 2):
        a = 1 << 253 | rng.randrange(1 << 252)  # below 2^253 + 2^252 < P; a ^ v has bit 253 clear
        b = a ^ v
        assert a < P and b < P and a ^ b == v >= P
        rows += [[a, b], [b, a]]
        notes += [f"XOR = {v:#x} >= P"] * 2
    rows.append([1 << 253, (1 << 253) - 1])
    notes.append("XOR = 2^254 - 1 >= P")
    _pad(rows, notes, [1, 1])
    return _case("logic", circ, [1, 2], rows, labels, notes)


# ---- Brillig BinaryIntOp
INT_WIDTHS = {"UnsignedDiv": [64, 128, 254, 256], "SignedDiv": [8, 64, 128, 256]}


def signed_div_rows(bits):
    """[(a, b, note)]: the ends of two's complement at this width and the operands past it"""
    m, h = 1 << bits, 1 << (bits - 1)
    if m >= P:  # 254 bits and up: -x = 2^bits - x is no field element for small x; at 256 bits every field element is non-negative
        return [(P - 1, 1, "P - 1 over 1"), (P - 1, P - 1, "P - 1 over P - 1"), (1, P - 1, "1 over P - 1"), (P - 1, P - 2, "P - 1 over P - 2"), (7, 0, "zero divisor"),
                (0, 0, "0 over 0"), (0, 5, "0 over 5"), (1 << 253, 3, "2^253 over 3"), (P - 1, 1 << 32, "P - 1 over 2^32")]
    neg = lambda x: m - x  # noqa: E731
    out = [(h % P, neg(1), "minimum over -1"), (neg(1), 1, "-1 over 1"), (1, neg(1), "1 over -1"), (h % P, 1, "minimum over 1"), (h - 1, neg(1), "maximum over -1"),
           (7, 0, "zero divisor"), (0, 0, "0 over 0"), (neg(1), 0, "-1 over 0"), (0, 5, "0 over 5"), (0, neg(5), "0 over -5")]
    for x in (1, 2, 3, 7, h - 1, h // 2 + 1):
        x = max(x, 1)
        out += [(neg(x), x % P, f"-x over x, x = {x:#x}"), (x % P, neg(x), "x over -x"), (neg(x), neg(x), "-x over -x"), (neg(3 * x + 1) if 3 * x + 1 < h else neg(x), x % P, "-(3x + 1) over x")]
    if bits < 254:  # the third class of int_to_signed: at or above 2^bits, read as x - 2^bits
        for a, b, note in ((m, 1, "2^bits over 1"), (m + 9, 2, "2^bits + 9 over 2"), (m + 9, m - 2, "2^bits + 9 over -2"), (77, m, "divisor 2^bits: zero"), (77, m + 7, "77 over 2^bits + 7"),
                           (P - 1, m + 3, "P - 1 over 2^bits + 3"), (P - 1, 3, "P - 1 over 3"), (P - 1, m - 1, "P - 1 over -1: the quotient passes 2^bits"),
                           (m - 6, m + 2, "-6 over 2^bits + 2"), ((m << 1) + 1, m - 1, "2^(bits+1) + 1 over -1"), (m + m - 1, m - 1, "2^bits + 2^bits - 1 over -1")):
            out.append((a % P, b % P, note))
    return out


@functools.lru_cache(maxsize=None)
def brillig_case(op, bits):
    """One division at one width, twice: opcode 0 straight-line (the planner inlines it: op_brillig_sl), opcode 1 with a backward jump behind
    the division (it stays in the VM kernel). A row where the division panics fails at opcode 0."""
    W = E.from_witness
    ops = [Brillig(inputs=[W(1), W(2)], outputs=[3], bytecode=[("BinaryIntOp", 0, op, bits, 0, 1), ("Stop",)]),
           Brillig(inputs=[W(1), W(2)], outputs=[4], bytecode=[("BinaryIntOp", 0, op, bits, 0, 1), ("Const", 1, 0), ("JumpIf", 1, 0), ("Stop",)])]
    pairs = [(a, b, note) for a, b, note in quotient_operands()]
    if op == "SignedDiv":
        pairs = signed_div_rows(bits) + pairs
    rows, notes = [[a, b] for a, b, _ in pairs], [n for _, _, n in pairs]
    _pad(rows, notes, [9, 4])
    return _case(f"{op} at {bits} bits", Circuit(4, ops), [1, 2], rows, {3: f"{op} at {bits} bits, straight-line", 4: f"{op} at {bits} bits, in the VM"}, notes)


def brillig_cases():
    return [brillig_case(op, bits) for op in ("UnsignedDiv", "SignedDiv") for bits in INT_WIDTHS[op]]


def all_cases():
    return [quotient_case(), radix_case_a(), radix_case_b(), *radix_panic_cases(), range_case_shared(), range_case_distinct(), logic_case(), *brillig_cases()]
