"""Directive::PermutationSort and the solve loop around it in Python integers, restated from the reference's Rust alone: no oracle, no device and no product
code in the model. tests/sort_cases.py builds the inputs, tests/test_sort_cases.py runs them through the CPU oracle, tests/test_gpu_sort_edges.py on the device.

run(circuit, witness map) solves the opcodes in program order and returns Expect(status, err, opcode_index, aux0, aux1, message, witnesses, branches): the
head as Result.as_tuple() carries it, the panic text, the WHOLE witness map the reference leaves behind, and the branch labels the run passed through.

The rules and where they stand:
  Directive::PermutationSort            acvm/src/pwg/directives/mod.rs:88-119
      :91-101    get_value of every tuple component, element by element (the first unknown witness ends the opcode); the element's index is appended
      :102-112   slice::sort_by, a STABLE sort; the comparator walks sort_by and compares BigUint::from_bytes_be(to_be_bytes()), the canonical integers;
                 a[*i as usize] on a Vec of tuple + 1 values panics when the comparator REACHES a column past it -- i.e. when two elements it compares tie on
                 every column before (a sort must compare the neighbours of its result, so a tie anywhere is reached; without ties, and with fewer than two
                 elements, the column is never looked at)
      :113-118   route(identity, the sorted indices); bits.iter().zip(control): the shorter list wins; insert_value per bit
  SortingNetwork, route                 acvm/src/pwg/directives/sorting.rs:7-244   result = switch_x, switch_y, route(first halves), route(second halves)
  get_value, insert_value               acvm/src/pwg/mod.rs:321-357 (tests/mem_ref.py, tests/arith_ref.py)

scratch_walk(n, tuple) is the other thing restated here: the allocation walk of acvm_amd/csrc/ops_sort.hpp:29-90 (a function of the sizes alone), whose
high-water mark the planner's reservation must cover.

A Variant is the same model wrong in ONE way; tests/test_sort_cases.py uses them to prove that each list of tests/sort_cases.py would notice."""
import collections
import functools

import arith_ref
import hash_ref
from acvm_amd.acir import P, Arithmetic, BlackBoxFuncCall, Expression, PermutationSort
from arith_ref import ST_SOLVED, ST_IN_PROGRESS, ST_FAILURE, E_NONE, E_MISSING_ASSIGNMENT, E_UNSATISFIED, E_PANIC, Fail as _Fail, insert_value  # noqa: F401
from mem_ref import get_value

Expect = collections.namedtuple("Expect", "status err opcode_index aux0 aux1 message witnesses branches")

LABELS = (
    "input_missing", "n_0", "n_1", "n_2", "n_3_or_more", "sort_by_empty", "sort_by_index_column", "tie_decided_by_stability", "tie_decided_by_a_later_column",
    "column_past_the_tuple_reached", "column_past_the_tuple_not_reached", "order_is_identity", "order_is_no_identity",
    "bits_fewer_than_switches", "bits_more_than_switches", "bits_as_many_as_switches", "bit_new", "bit_same", "bit_conflict",
    "gate_solves", "range_passes", "range_fails",
)

VARIANTS = ("unstable_sort", "switch_y_first", "sub_networks_swapped", "low_limb_first", "panic_unreached")


def msg_index(length, index):
    """core::panicking::panic_bounds_check"""
    return b"index out of bounds: the len is %d but the index is %d" % (length, index)


def switch_count(n):
    return sum((i).bit_length() for i in range(n))   # sum of ceil(log2(i + 1)) for i < n


class SortingNetwork:
    """sorting.rs:7-157; the BTreeMaps are dicts (their order is never used), `free` is a set whose first() is its minimum"""

    def __init__(self, inputs, outputs):
        n = self.n = len(inputs)
        self.x_inputs, self.y_inputs = list(inputs), list(outputs)
        self.x_values = {v: i for i, v in enumerate(inputs)}
        self.y_values = {v: i for i, v in enumerate(outputs)}
        self.switch_x, self.switch_y = [False] * (n // 2), [False] * ((n - 1) // 2)
        self.inner_x, self.inner_y = [0] * n, [0] * n
        self.free = set(range((n - 1) // 2))
        self.inner_y[n - 1] = self.y_inputs[n - 1]
        if n % 2 == 0:
            self.inner_y[n // 2 - 1] = self.y_inputs[n - 2]
        else:
            self.inner_x[n - 1] = self.x_inputs[n - 1]

    def is_single_x(self, a):
        return self.n % 2 == 1 and a == self.n - 1

    def is_single_y(self, a):
        return a >= self.n - 2 + self.n % 2

    def compute_inner(self, idx, switch):
        return idx // 2 + self.n // 2 if switch ^ (idx % 2 == 1) else idx // 2

    def configure_x(self, x, switch, inner):
        self.inner_x[inner] = self.x_inputs[x]
        self.switch_x[x // 2] = switch

    def configure_y(self, y, switch, inner):
        self.inner_y[inner] = self.y_inputs[y]
        self.switch_y[y // 2] = switch

    def route_out_wire(self, y, sub):
        if self.is_single_y(y):
            assert sub
        else:
            s1 = sub ^ (y % 2 != 0)
            self.configure_y(y, s1, self.compute_inner(y, s1))
        x = self.x_values.pop(self.y_inputs[y])
        if not self.is_single_x(x):
            s2 = sub ^ (x % 2 != 0)
            self.configure_x(x, s2, self.compute_inner(x, s2))
        return x

    def route_in_wire(self, x, sub):
        assert not self.is_single_x(x)
        s1 = sub ^ (x % 2 != 0)
        self.configure_x(x, s1, self.compute_inner(x, s1))
        y = self.y_values.pop(self.x_inputs[x])
        if not self.is_single_y(y):
            s2 = sub ^ (y % 2 != 0)
            self.configure_y(y, s2, self.compute_inner(y, s2))
        return y

    def new_start(self):
        if self.free:
            s = min(self.free)
            return s, 2 * s
        return None, 0


def sibling(index):
    return index + 1 - 2 * (index % 2)


def route(inputs, outputs, variant=None):
    """sorting.rs:161-244 (the recursion as the reference has it: its depth is the logarithm of the size)"""
    assert len(inputs) == len(outputs)
    n = len(inputs)
    if n == 0:
        return []
    if n == 1:
        assert inputs[0] == outputs[0]
        return []
    if n == 2:
        if inputs[0] == outputs[0]:
            assert inputs[1] == outputs[1]
            return [False]
        assert inputs[1] == outputs[0] and inputs[0] == outputs[1]
        return [True]
    net = SortingNetwork(inputs, outputs)
    out_idx, start_sub, switch, start = n - 1, True, None, None
    while net.free:
        if switch is not None:
            net.free.discard(switch)
        in_idx = net.route_out_wire(out_idx, start_sub)
        if net.is_single_x(in_idx):
            start_sub = not start_sub
            start, out_idx = net.new_start()
            switch = start
            continue
        out_idx = net.route_in_wire(sibling(in_idx), not start_sub)
        switch = out_idx // 2
        if start == switch or net.is_single_y(out_idx):
            start, out_idx = net.new_start()
            switch = start
        else:
            out_idx = sibling(out_idx)
    n1 = n // 2
    result = net.switch_y + net.switch_x if variant == "switch_y_first" else net.switch_x + net.switch_y
    s1 = route(net.inner_x[:n1], net.inner_y[:n1], variant)
    s2 = route(net.inner_x[n1:], net.inner_y[n1:], variant)
    return result + (s2 + s1 if variant == "sub_networks_swapped" else s1 + s2)


def _low_limb_first(v):
    return tuple((v >> (32 * k)) & 0xFFFFFFFF for k in range(8))


def sort_elements(val_a, sort_by, tuple_, hit, variant=None):
    """val_a.sort_by(..): list.sort is stable like slice::sort_by; the comparator is the reference's"""
    def cmp(a, b):
        for k, col in enumerate(sort_by):
            if col >= len(a):   # a[*i as usize] on the tuple + 1 values of an element
                raise _Fail(E_PANIC, message=msg_index(len(a), col))
            x, y = (a[col], b[col]) if variant != "low_limb_first" else (_low_limb_first(a[col]), _low_limb_first(b[col]))
            if x != y:
                if k > 0:
                    hit("tie_decided_by_a_later_column")
                return -1 if x < y else 1
        if sort_by:
            hit("tie_decided_by_stability")
        return 0

    if variant == "panic_unreached" and len(val_a) >= 2:
        for col in sort_by:
            if col > tuple_:
                raise _Fail(E_PANIC, message=msg_index(tuple_ + 1, col))
    out = sorted(val_a, key=functools.cmp_to_key(cmp))
    if variant == "unstable_sort":   # equal elements in the reverse of their first order
        groups, k = [], 0
        while k < len(out):
            j = k
            while j < len(out) and all(out[j][c] == out[k][c] for c in sort_by if c < tuple_):
                j += 1
            groups += out[k:j][::-1]
            k = j
        out = groups
    if any(col > tuple_ for col in sort_by):
        hit("column_past_the_tuple_not_reached")
    return out


class Model:
    def __init__(self, variant=None):
        assert variant is None or variant in VARIANTS, variant
        self.variant = variant
        self.orders = []  # per sort that got as far: (opcode, the sorted indices)

    def sort(self, op, wm, hit, at):
        n, tuple_ = len(op.inputs), op.tuple
        val_a = []
        for i, element in enumerate(op.inputs):
            assert len(element) == tuple_
            try:
                val_a.append([get_value(e, wm) for e in element] + [i])
            except _Fail:
                hit("input_missing")
                raise
        hit("n_0" if n == 0 else "n_1" if n == 1 else "n_2" if n == 2 else "n_3_or_more")
        if not op.sort_by:
            hit("sort_by_empty")
        if tuple_ in op.sort_by:
            hit("sort_by_index_column")
        try:
            val_a = sort_elements(val_a, op.sort_by, tuple_, hit, self.variant)
        except _Fail:
            hit("column_past_the_tuple_reached")
            raise
        order = [a[-1] for a in val_a]
        self.orders.append((at, order))
        hit("order_is_identity" if order == list(range(n)) else "order_is_no_identity")
        control = route(list(range(n)), order, self.variant)
        assert len(control) == switch_count(n)
        hit("bits_fewer_than_switches" if len(op.bits) < len(control) else "bits_more_than_switches" if len(op.bits) > len(control) else "bits_as_many_as_switches")
        for w, value in zip(op.bits, control):
            old = wm.get(w)
            try:
                insert_value(wm, w, 1 if value else 0)
            except _Fail:
                hit("bit_conflict")
                raise
            hit("bit_new" if old is None else "bit_same")

    def run(self, circ, wm, n_opcodes=None, snapshots=None):
        branches = set()

        def hit(label):
            assert label in LABELS, label
            branches.add(label)

        def end(status, err=E_NONE, at=0, aux0=0, aux1=0, message=None):
            return Expect(status, err, at, aux0, aux1, message, wm, frozenset(branches))

        n_seen = len(wm)
        for oi, op in enumerate(circ.opcodes):
            if n_opcodes is not None and oi == n_opcodes:
                return end(ST_IN_PROGRESS, at=oi)
            try:
                if isinstance(op, PermutationSort):
                    self.sort(op, wm, hit, oi)
                elif isinstance(op, (Arithmetic, Expression)):
                    seen = set()
                    try:
                        arith_ref.gate(op.expr if isinstance(op, Arithmetic) else op, wm, seen.add)
                    finally:
                        if "arm_solved_solvable_assigns" in seen:
                            hit("gate_solves")
                elif isinstance(op, BlackBoxFuncCall) and op.name == "RANGE":
                    arith_ref.range_check(op, wm, lambda l: hit(l) if l != "range_missing" else None)
                elif isinstance(op, BlackBoxFuncCall) and op.name in hash_ref.HASHES:   # the neighbours of list E: the model of tests/hash_ref.py
                    hash_ref.Model().black_box(op, wm, lambda l: None)
                else:
                    raise AssertionError(f"no model for {op!r}")
            except _Fail as f:
                err, aux0, aux1, message = f.head
                return end(ST_FAILURE, err, oi, aux0, aux1, message)
            if snapshots is not None:
                snapshots.append([(w, wm[w]) for w in list(wm)[n_seen:]])
                n_seen = len(wm)
        return end(ST_SOLVED)


def run(circ, wm, n_opcodes=None, variant=None):
    return Model(variant).run(circ, dict(wm), n_opcodes)


def run_traced(circ, wm):
    m = Model()
    return m.run(circ, dict(wm)), m.orders


def run_stepped(circ, wm):
    m, snaps = Model(), []
    return m.run(circ, dict(wm), snapshots=snaps), snaps


# ---------------------------------------------------------------------------------------------------------------- the device's allocation walk
Walk = collections.namedtuple("Walk", "high_water switches max_frames")
STACK_FRAMES = 72


def scratch_reserved_formula(n, tuple_):
    """what plan.cpp reserves for a sort of n tuples, restated (the test compares it with what the planner reports)"""
    lg = max(n - 1, 0).bit_length()
    return 8 * n * tuple_ + 4 * n + n * (lg + 1) + 1 + 3 * STACK_FRAMES + (4 * n + 8) * (lg + 2) + 64


@functools.lru_cache(maxsize=None)
def scratch_walk(n, tuple_):
    """op_perm_sort's use of its per-lane scratch for n tuples (ops_sort.hpp:29-90): values, order, x_values, y_values, then a bump region -- the switch
    list (n (lg + 1) + 1 words), the identity, 72 stack frames of 3 words, and per node of more than two wires 2 m + m / 2 + 2 ((m - 1) / 2) words that are
    never given back. Returns (words the walk touches, switches it emits, frames on the stack at most)."""
    lg = max(n - 1, 0).bit_length()
    bump = 8 * n * tuple_ + 3 * n
    bump += n * (lg + 1) + 1
    bump += n
    bump += 3 * STACK_FRAMES
    stack, switches, max_frames = [n], 0, 1
    while stack:
        m = stack.pop()
        if m <= 1:
            continue
        if m == 2:
            switches += 1
            continue
        nf = (m - 1) // 2
        bump += 2 * m + m // 2 + 2 * nf
        switches += m // 2 + nf
        stack.append(m - m // 2)
        stack.append(m // 2)
        max_frames = max(max_frames, len(stack))
    return Walk(bump, switches, max_frames)
