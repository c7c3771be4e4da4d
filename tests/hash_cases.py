"""One builder of the rows that random inputs never bring to the hash black boxes (acvm_amd/csrc/ops_hash.hpp op_hash, hash_device.hpp, kernels_hash.hip
hash_coop_level_kernel<1> / <4>, the lane-per-instance kernel and the exact path), with every expected outcome from the Python model of the reference
(tests/hash_ref.py: hashlib, tests/keccak_ref.py): no oracle and no device here. tests/test_hash_cases.py runs the lists through the CPU oracle and asserts
what they cover; tests/test_gpu_hash_edges.py runs them on the device.

A list is a tuple of cases; a case is (name, circuit, ids, rows, expect, notes, filler, meta): one list of initial values per row, the model's Expect per
row (rows of equal values share one), what the row is for, a row that passes (for padding a batch; None where the circuit lets no row pass), and what
the case promises about the launches of its byte-message records (meta: see launch_mode).

  A  every length: the prefixes of one input, 1 .. 140 bytes on one level and around 256, 272, 352 and 1 024 bytes, in the four-wave and in the one-wave kernel
  B  chains of four whose successors are shorter than their predecessor by 1, 2 and 3 bytes, in each kernel mode; heads at the launcher's thresholds
  C  widths: 0 .. 256 bits, the widths whose byte count is past the 32 bytes of a field element (those near 2^32 included), runs of byte-wide inputs
  D  Keccak256VariableLength: sizes around the message's length, the rate, 2^32, 2^64, 2^128 and p - 1
  E  HashToField128Security: every quotient of digest / p, compared outputs, an empty message
  F  outputs: wrong counts, pre-assigned outputs, one witness twice among the outputs
  G  initial sets that differ per row (MultiBatch)"""
import collections
import functools
import hashlib
import random

import hash_ref as hr
from acvm_amd.acir import P, BlackBoxFuncCall as BB, Circuit, Expression as E, FunctionInput as FI
from keccak_ref import keccak256

SEED = 20263
COOP = ("SHA256", "Blake2s", "Keccak256")                         # the functions whose byte messages take the cooperative kernel
WITH_OUTPUTS = COOP + ("Keccak256VariableLength",)
NOT_BYTES = (256, (1 << 29) - 1, 1 << 29, (1 << 29) + 5, P - 256, P - 1)
PANIC_WIDTHS = (257, 300, 1 << 31, 0xFFFFFFF8, 0xFFFFFFF9, 0xFFFFFFFF)
WRAPPING_WIDTHS = tuple(w for w in PANIC_WIDTHS if (w + 7) % (1 << 32) // 8 <= 32)   # (num_bits + 7) / 8 in 32 bits says "a few bytes" for these
WIDTHS = (0, 1, 7, 8, 9, 16, 17, 24, 25, 32, 248, 249, 255, 256)

Case = collections.namedtuple("Case", "name circuit ids rows expect notes filler meta")

HASH_OF = {"SHA256": lambda m: hashlib.sha256(m).digest(), "Blake2s": lambda m: hashlib.blake2s(m).digest(), "Keccak256": keccak256}


def launch_mode(n_rows, n_heads, max_words):
    """(waves per item, message buffers) of a launch of n_heads byte-message records (heads of chains counted once) whose longest message, chained
    members included, has max_words 32-bit words -- the rule of kernels_hash.hip launch_hash_coop_level, restated"""
    buf_words = max(max_words, 8)
    items = (n_rows + 63) // 64 * n_heads
    four = items * 4 <= 8192 or buf_words > 32
    n_buf = 2 if four and 2 * buf_words * 256 <= 44 << 10 else 1
    return (4 if four else 1), n_buf


class Builder:
    """opcodes of one circuit; witnesses 1..n_inputs are the inputs, every other one is handed out by new()"""

    def __init__(self, n_inputs):
        self.next, self.ops = n_inputs + 1, []

    def new(self, n=None):
        if n is None:
            self.next += 1
            return self.next - 1
        self.next += n
        return list(range(self.next - n, self.next))

    def gate(self, lin, qc=0, mul=()):
        out = self.new()
        self.ops.append(E(list(mul), list(lin) + [(P - 1, out)], qc % P))
        return out

    def range(self, w, bits=8):
        self.ops.append(BB("RANGE", {"input": FI(w, bits)}))

    def hash(self, name, inputs, outputs=None, size=None, n_out=32):
        """inputs: witnesses (8 bits wide) or (witness, num_bits); returns the outputs (the one output of HashToField128Security)"""
        ins = [FI(*i) if isinstance(i, tuple) else FI(i, 8) for i in inputs]
        if name == "HashToField128Security":
            out = self.new() if outputs is None else outputs
            self.ops.append(BB(name, {"inputs": ins, "output": out}))
            return out
        outs = self.new(n_out) if outputs is None else list(outputs)
        args = {"inputs": ins, "outputs": outs}
        if name == "Keccak256VariableLength":
            args["var_message_size"] = FI(size, 64)
        self.ops.append(BB(name, args))
        return outs

    def circuit(self):
        return Circuit(self.next - 1, self.ops)


def _case(name, circ, ids, rows, notes, filler=None, meta=None, max_rows=200):
    assert len(rows) == len(notes) and 0 < len(rows) <= max_rows, (name, len(rows))
    assert all(len(row) == len(ids) and all(0 <= v < P for v in row) for row in rows), name
    memo = {}
    expect = []
    for row in rows:
        key = tuple(row)
        if key not in memo:
            memo[key] = hr.run(circ, dict(zip(ids, row)))
        expect.append(memo[key])
    if filler is not None:
        assert expect[filler].status == hr.ST_SOLVED, (name, "the filler row does not pass")
    return Case(name, circ, list(ids), [list(r) for r in rows], expect, list(notes), filler, dict(meta or {}))


def padded(case, n):
    """the case with passing rows IN FRONT up to n rows, so that the rows the case is about lie in the last, partial wave"""
    k = n - len(case.rows)
    if k <= 0 or case.filler is None:
        return case
    f = case.filler
    return case._replace(rows=[case.rows[f]] * k + case.rows, expect=[case.expect[f]] * k + case.expect, notes=["filler"] * k + case.notes, filler=0)


def describe(case, j):
    return f"{case.name} row {j} ({case.notes[j]})"


def compare(case, got, who, expect=None):
    """got: (results, assigned [B, nw], values [B, nw, 32] big-endian) as Batch.witness_map and the oracle's solve_batch give them; every field of the
    model's expectation, the whole map included. The expected maps are laid out once per distinct expectation."""
    import numpy as np
    res, asg, vals = got
    expect = expect or case.expect
    nw = asg.shape[1]
    assert nw > case.circuit.current_witness_index
    for j, want in enumerate(expect):
        at = describe(case, j)
        assert tuple(res[j].as_tuple()) == tuple(want[:5]), f"{at}: {who} (status, error, opcode, aux0, aux1) {tuple(res[j].as_tuple())}, want {tuple(want[:5])}"
        if want.message is not None:
            assert res[j].message == want.message, f"{at}: {who} message {res[j].message!r}, want {want.message!r}"
    laid, index = {}, []
    for want in expect:
        if id(want) not in laid:
            a = np.zeros(nw, dtype=np.uint8)
            v = np.zeros((nw, 32), dtype=np.uint8)
            for w, x in want.witnesses.items():
                a[w] = 1
                v[w] = np.frombuffer(x.to_bytes(32, "big"), dtype=np.uint8)
            laid[id(want)] = (len(laid), a, v)
        index.append(laid[id(want)][0])
    order = sorted(laid.values(), key=lambda t: t[0])
    want_asg = np.stack([a for _, a, _ in order])[index]
    bad = np.argwhere((asg != 0) != (want_asg != 0))
    if bad.size == 0:
        want_vals = np.stack([v for _, _, v in order])[index]
        bad = np.argwhere((vals * (want_asg[:, :, None] != 0) != want_vals).any(axis=2))
    if bad.size:
        j, w = (int(x) for x in bad[0])
        g = int.from_bytes(vals[j, w].tobytes(), "big") if asg[j, w] else None
        x = expect[j].witnesses.get(w)
        raise AssertionError(f"{describe(case, j)}: witness {w}: {who} " + (hex(g) if g is not None else "unassigned") + ", want " + (hex(x) if x is not None else "unassigned")
                             + f" ({len(bad)} differ)")


def compare_maps(case, got, who, expect=None):
    """got: per row (Result.as_tuple(), message, {witness: value})"""
    for j, (want, (head, message, wm)) in enumerate(zip(expect or case.expect, got)):
        at = describe(case, j)
        assert tuple(head) == tuple(want[:5]), f"{at}: {who} (status, error, opcode, aux0, aux1) {tuple(head)}, want {tuple(want[:5])}"
        if want.message is not None:
            assert message == want.message, f"{at}: {who} message {message!r}, want {want.message!r}"
        assert wm == want.witnesses, f"{at}: {who}: the maps differ at witnesses {sorted(w for w in set(wm) | set(want.witnesses) if wm.get(w) != want.witnesses.get(w))[:8]}"


# ---------------------------------------------------------------------------------------------------------------- A: every length
LONG_LENGTHS = (0, 255, 256, 257, 258, 271, 272, 273, 274) + tuple(range(351, 359)) + (1023, 1024, 1025)
ONE_WAVE_SUFFIXES = (1, 3, 55, 56, 63, 64, 65, 71, 72, 119, 127, 128)   # twelve more records of at most 128 bytes: with the prefixes 1 .. 128, 140 records


def length_rows(n, count, seed):
    """`count` rows over n byte inputs, cycling through: random bytes; all 0x00; all 0xFF; all 0x80 and all 0x01 (every message ends in a padding byte); each
    value that is no byte in every position, and in the last position of the input alone"""
    rng = random.Random(seed)
    kinds = [("random bytes", [rng.randrange(256) for _ in range(n)]) for _ in range(3)]
    kinds += [(f"all {b:#04x}", [b] * n) for b in (0x00, 0xFF, 0x80, 0x01)]
    kinds += [(f"{v:#x} in every position", [v] * n) for v in NOT_BYTES]
    kinds += [(f"{v:#x} in the last position", [rng.randrange(256) for _ in range(n - 1)] + [v]) for v in NOT_BYTES]
    kinds.append(("random bytes and field elements", [rng.randrange(P) if rng.random() < 0.3 else rng.randrange(256) for _ in range(n)]))
    return [kinds[j % len(kinds)][1] for j in range(count)], [kinds[j % len(kinds)][0] for j in range(count)]


@functools.lru_cache(maxsize=None)
def length_case(name, mode):
    """mode "four waves": the prefixes ids[:n] for n = 1 .. 140 of one 140-byte input, 140 records on one level, 67 rows (2 x 140 items: the four-wave
    kernel). mode "one wave": the prefixes of 1 .. 128 bytes and twelve suffixes of at most 128 bytes, 140 records, 963 rows (16 x 140 = 2 240 items of at
    most 32 words: the one-wave kernel). HashToField128Security takes the lane kernel either way."""
    n = 140
    ids = list(range(1, n + 1))
    b = Builder(n)
    if mode == "four waves":
        slices = [ids[:k] for k in range(1, n + 1)]
        n_rows = 67
    else:
        slices = [ids[:k] for k in range(1, 129)] + [ids[n - k:] for k in ONE_WAVE_SUFFIXES]
        n_rows = 963
    for s in slices:
        b.hash(name, s)
    rows, notes = length_rows(n, n_rows, SEED + len(name) + len(mode))
    meta = {"coop_heads": len(slices), "max_words": (max(len(s) for s in slices) + 3) // 4, "chained": 0} if name in COOP else {}
    return _case(f"A, {name}, {mode}", b.circuit(), ids, rows, notes, filler=0, meta=meta, max_rows=963)


@functools.lru_cache(maxsize=None)
def long_case(name):
    """the prefixes of LONG_LENGTHS bytes of one 1 025-byte input: 0 and 1 025 bytes take the lane kernel, up to 256 bytes the launch of the short messages, the
    others the launch of the long ones (one message buffer: 256 words)"""
    n = 1025
    ids = list(range(1, n + 1))
    b = Builder(n)
    for k in LONG_LENGTHS:
        b.hash(name, ids[:k])
    rows, notes = length_rows(n, 67, SEED + 7 + len(name))
    return _case(f"A, {name}, long", b.circuit(), ids, rows, notes, filler=0)


# ---------------------------------------------------------------------------------------------------------------- B: chains
CHAIN_FUNCS = ("Keccak256", "SHA256", "Blake2s", "Keccak256")
CHAIN_SHORTER_BY = (1, 2, 3)
CHAIN_MODES = {"two buffers": 45, "one buffer": 357, "one wave": 45}     # the head's bytes
N_FILL = 150     # filler records of the one-wave circuit: with 963 rows, 16 x (1 + 150) = 2 416 items


def add_chain(b, pool, head_len, rng, ranges=False):
    """A chain of four on the builder: the head hashes head_len inputs of `pool`; each successor is shorter than its predecessor by 1, 2 and 3 bytes and reads
    the 32 bytes of the predecessor's digest out of order, at 32 positions drawn among its own, between inputs of the pool. ranges: RANGE checks on bytes
    of every digest (8 bits, and 7 bits on one byte of the second digest, which fails for half of the rows) and on inputs of the head. Returns the four digests."""
    head = [pool[k % len(pool)] for k in range(head_len)]
    if ranges:
        for w in head[:6]:
            b.range(w, 8)
        b.range(head[6], 7)
    digests = [b.hash(CHAIN_FUNCS[0], head)]
    n = head_len
    for k, less in enumerate(CHAIN_SHORTER_BY):
        n -= less
        d = digests[-1][:]
        rng.shuffle(d)
        at = set(rng.sample(range(n), 32))
        ins = [d.pop() if pos in at else pool[rng.randrange(len(pool))] for pos in range(n)]
        assert not d and not all(pos in at for pos in range(32))
        if ranges:
            for w in digests[-1][3:6]:
                b.range(w, 8)
            if k == 1:
                b.range(digests[-1][9], 7)
        digests.append(b.hash(CHAIN_FUNCS[k + 1], ins))
    return digests


def byte_rows(n, count, rng, edge=True):
    rows, notes = [], []
    for j in range(count):
        row = [rng.randrange(256) for _ in range(n)]
        note = "random bytes"
        if edge and j % 5 == 3:
            v = NOT_BYTES[(j // 5) % len(NOT_BYTES)]
            row[rng.randrange(n)] = v
            note = f"one input is {v:#x}"
        rows.append(row)
        notes.append(note)
    return rows, notes


@functools.lru_cache(maxsize=None)
def chain_case(mode, ranges=False):
    head_len = CHAIN_MODES[mode]
    n = 64
    ids = list(range(1, n + 1))
    rng = random.Random(SEED + 1000 + head_len + ranges + len(mode))
    b = Builder(n)
    add_chain(b, ids[:48], head_len, rng, ranges)
    n_heads = 1
    if mode == "one wave":
        for k in range(N_FILL):
            b.hash(("SHA256", "Blake2s")[k % 2], [ids[(k + i) % n] for i in range(3 + k % 23)])
        n_heads += N_FILL
    if mode == "one wave":   # few distinct rows, many times
        base, base_notes = byte_rows(n, 23, rng, edge=not ranges)
        rows, notes = [base[j % 23] for j in range(963)], [base_notes[j % 23] for j in range(963)]
    else:
        rows, notes = byte_rows(n, 67, rng, edge=not ranges)
    if ranges:
        for j, row in enumerate(rows):
            row[6] = row[6] % 128 if j % 7 else 128 + row[6] % 128   # the 7-bit check on a head input fails in one row of seven
    filler = next(j for j, row in enumerate(rows) if hr.run(b.circuit(), dict(zip(ids, row))).status == hr.ST_SOLVED)
    meta = {"coop_heads": n_heads, "max_words": (head_len + 3) // 4, "chained": 3}
    return _case(f"B, chain, {mode}" + (", RANGE checks" if ranges else ""), b.circuit(), ids, rows, notes, filler=filler, meta=meta, max_rows=963)


THRESHOLDS = (128, 129, 256, 257, 352, 353)


@functools.lru_cache(maxsize=None)
def threshold_case(head_len):
    """a head of head_len bytes (32 / 33, 64 / 65, 88 / 89 message words) with one successor behind it: 37 bytes, five of them no digest bytes"""
    ids = list(range(1, head_len + 1))
    rng = random.Random(SEED + 2000 + head_len)
    b = Builder(head_len)
    d = b.hash("SHA256", ids)
    b.hash("Keccak256", d[16:] + ids[:5] + d[:16][::-1])
    rows, notes = byte_rows(head_len, 67, rng)
    return _case(f"B, head of {head_len} bytes", b.circuit(), ids, rows, notes, filler=0, meta={"coop_heads": 1, "max_words": (head_len + 3) // 4, "chained": 1})


def second_rows(case):
    """other rows for a second solve on the same handle: every message differs"""
    rng = random.Random(SEED + 2500 + len(case.rows))
    distinct = {}
    rows = []
    for row in case.rows:
        key = tuple(row)
        if key not in distinct:
            distinct[key] = [(v + 1 + rng.randrange(254)) % 256 if v < 256 else rng.randrange(256) for v in row]
        rows.append(distinct[key])
    return _case(case.name + ", second rows", case.circuit, case.ids, rows, case.notes, meta=case.meta, max_rows=963)


# ---------------------------------------------------------------------------------------------------------------- C: widths
def edge_values(rng):
    return [0, 1, P - 1] + [(1 << k) - 1 for k in (8, 16, 24, 32, 248)] + [1 << 8, 1 << 248, (1 << 253) + 255] + [rng.randrange(P) for _ in range(4)]


def _size_for(b, name, n_bytes):
    """the var_message_size witness of a Keccak256VariableLength record that takes the whole message: a gate output"""
    return b.gate([], qc=n_bytes) if name == "Keccak256VariableLength" else None


RUNS = [(k, 8) for k in range(5)] + sum(([(100, 16)] + [(k, 8) for k in range(run)] for run in range(1, 10)), []) + [(100, 16)] + [(k, 8) for k in range(7)]


@functools.lru_cache(maxsize=None)
def width_case(name):
    """Inputs: 1 = a, 2 = x, 3 = c, 4 = s, 5 = t. One record per width of WIDTHS over [a (8 bits), x (that width), c (16 bits)]; one over runs of 1 .. 9 byte-wide
    inputs between 16-bit ones (and a run at either end: both ends of op_hash's four-at-a-time path); one over the gate outputs s + t and x + c, whose sums
    wrap past p in some rows, at 8 and 32 bits."""
    ids = [1, 2, 3, 4, 5]
    b = Builder(5)
    for width in WIDTHS:
        b.hash(name, [(1, 8), (2, width), (3, 16)], size=_size_for(b, name, 1 + (width + 7) // 8 + 2))
    pool = {100: 3, 0: 1, 1: 2, 2: 4, 3: 5, 4: 1, 5: 2, 6: 4, 7: 5, 8: 1}
    b.hash(name, [(pool[w], bits) for w, bits in RUNS], size=_size_for(b, name, sum(bits // 8 for _, bits in RUNS)))
    g1, g2 = b.gate([(1, 4), (1, 5)]), b.gate([(1, 2), (1, 3)])
    b.hash(name, [(g1, 8), (g2, 32), (g1, 32), (g2, 8)], size=_size_for(b, name, 10))
    rng = random.Random(SEED + 3000 + len(name))
    rows, notes = [], []
    for k, x in enumerate(edge_values(rng)):
        s = rng.randrange(1, P)
        t = rng.randrange(P - s, P) if k % 2 else rng.randrange(P - s)
        rows.append([rng.randrange(P) if k % 3 else rng.randrange(256), x, (P - x + rng.randrange(200)) % P if k % 2 else rng.randrange(1 << 16), s, t])
        notes.append(f"x = {x:#x}" + (", both sums wrap" if k % 2 else ""))
    return _case(f"C, widths, {name}", b.circuit(), ids, rows, notes, filler=0)


@functools.lru_cache(maxsize=None)
def panic_cases(name):
    """one circuit per width above 256 bits: the wide input first, in the middle or last among byte-wide ones (by turns); then, at 0xFFFFFFF9 bits, one whose
    last input nobody assigns (the pre-check comes before the panic) and one with 31 outputs (the panic comes before the count)"""
    rng = random.Random(SEED + 3500 + len(name))
    rows = [[rng.randrange(256), x, rng.randrange(P)] for x in (0, 1, P - 1, rng.randrange(P), rng.randrange(256))]
    notes = [f"x = {row[1]:#x}" for row in rows]
    out = []

    def one(width, where, missing=False, n_out=32):
        b = Builder(3)
        ins = [(1, 8), (3, 8), (1, 8), (3, 8)]
        ins.insert({"first": 0, "middle": 2, "last": 4}[where], (2, width))
        nobody = b.new()
        if missing:
            ins.append((nobody, 8))
        b.hash(name, ins, n_out=n_out, size=_size_for(b, name, 1))
        label = f"C, {name}, {width:#x} bits {where}" + (", an unassigned input behind it" if missing else "") + (f", {n_out} outputs" if n_out != 32 else "")
        return _case(label, b.circuit(), [1, 2, 3], rows, notes), nobody

    for k, width in enumerate(PANIC_WIDTHS):
        case, _ = one(width, ("first", "middle", "last")[(k + len(name)) % 3])
        at = len(case.circuit.opcodes) - 1
        assert all((x.err, x.opcode_index, x.message) == (hr.E_PANIC, at, hr.msg_slice((width + 7) // 8)) for x in case.expect), case.name
        out.append(case)
    case, nobody = one(0xFFFFFFF9, "first", missing=True)
    assert all((x.err, x.aux0) == (hr.E_MISSING_ASSIGNMENT, nobody) for x in case.expect)
    out.append(case)
    if name != "HashToField128Security":
        case, _ = one(0xFFFFFFF9, "last", n_out=31)
        assert all(x.err == hr.E_PANIC for x in case.expect)
        out.append(case)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- D: the variable length
VAR_LENGTHS = (0, 1, 135, 136, 137, 272, 300)


def var_sizes(n):
    return sorted({0, max(n - 1, 0), n, n + 1, 135, 136, 137, (1 << 32) - 1, 1 << 32, (1 << 64) + 5, (1 << 64) + n, (1 << 128) + 5, (1 << 128) + (1 << 64) + min(n, 3), P - 1})


@functools.lru_cache(maxsize=None)
def var_case(n):
    """n byte inputs and the size, a witness; a second record takes the size from a gate (size + 0)"""
    ids = list(range(1, n + 2))
    b = Builder(n + 1)
    b.hash("Keccak256VariableLength", ids[:n], size=n + 1)
    g = b.gate([(1, n + 1)])
    b.hash("Keccak256VariableLength", ids[:n], size=g)
    rng = random.Random(SEED + 4000 + n)
    msg = [rng.randrange(256) for _ in range(n)]
    rows = [msg + [s] for s in var_sizes(n)]
    return _case(f"D, {n} bytes", b.circuit(), ids, rows, [f"size {s:#x}" for s in var_sizes(n)], filler=0)


@functools.lru_cache(maxsize=None)
def var_mixed_case():
    """inputs of 8, 32, 16, 256 and 24 bits (42 bytes) under a size that cuts inside each of them; and a circuit whose size nobody assigns"""
    widths = (8, 32, 16, 256, 24)
    b = Builder(6)
    b.hash("Keccak256VariableLength", list(zip(range(1, 6), widths)), size=6)
    rng = random.Random(SEED + 4500)
    sizes = (0, 1, 2, 3, 5, 6, 7, 8, 20, 38, 39, 40, 41, 42, 43, 44, 1 << 32)
    rows = [[rng.randrange(P) for _ in range(5)] + [s] for s in sizes]
    mixed = _case("D, mixed widths", b.circuit(), list(range(1, 7)), rows, [f"size {s}" for s in sizes], filler=0)
    b = Builder(3)
    nobody = b.new()
    b.hash("Keccak256VariableLength", [1, 2, 3], size=nobody)
    rows = [[rng.randrange(256) for _ in range(3)] for _ in range(3)]
    missing = _case("D, the size unassigned", b.circuit(), [1, 2, 3], rows, ["size unassigned"] * 3)
    assert all((x.err, x.aux0) == (hr.E_MISSING_ASSIGNMENT, nobody) for x in missing.expect)
    return mixed, missing


# ---------------------------------------------------------------------------------------------------------------- E: HashToField
@functools.lru_cache(maxsize=None)
def to_field_case():
    """Inputs 1..4 the message (8, 16, 8 and 32 bits), 5 = what the second record's output is compared with. Rows ground until digest / p takes each of its six
    values (floor(2^256 / p) = 5) three times; the compared output is right in two rows of three. A third record hashes no input at all."""
    widths = (8, 16, 8, 32)
    b = Builder(5)
    b.hash("HashToField128Security", list(zip(range(1, 5), widths)))
    b.hash("HashToField128Security", list(zip(range(1, 5), widths)), outputs=5)
    b.hash("HashToField128Security", [])
    rng = random.Random(SEED + 5000)
    found = collections.defaultdict(list)
    tries = 0
    while any(len(found[q]) < 3 for q in range(6)):
        tries += 1
        vals = [rng.randrange(1 << w) for w in widths]
        msg = b"".join(v.to_bytes(w // 8, "little") for v, w in zip(vals, widths))
        d = int.from_bytes(hashlib.blake2s(msg).digest(), "big")
        if len(found[d // P]) < 3:
            found[d // P].append((vals, d % P))
    assert tries < 2000 and (1 << 256) // P == 5
    rows, notes = [], []
    for q in range(6):
        for k, (vals, f) in enumerate(found[q]):
            rows.append(vals + [f if k < 2 else (f + 1) % P])
            notes.append(f"digest / p = {q}, the compared output is " + ("right" if k < 2 else "wrong"))
    return _case("E, HashToField128Security", b.circuit(), [1, 2, 3, 4, 5], rows, notes, filler=0)


# ---------------------------------------------------------------------------------------------------------------- F: outputs
OUTPUT_COUNTS = (0, 31, 33, 64)
POSITIONS = (0, 1, 4, 31)
TWICE = ((0, 1), (31, 0), (0, 4))


@functools.lru_cache(maxsize=None)
def count_cases(name):
    rng = random.Random(SEED + 6000 + len(name))
    out = []
    for n_out in OUTPUT_COUNTS:
        b = Builder(4)
        b.hash(name, [1, 2, 3], n_out=n_out, size=4)
        rows = [[rng.randrange(256) for _ in range(3)] + [3] for _ in range(3)]
        case = _case(f"F, {name}, {n_out} outputs", b.circuit(), [1, 2, 3, 4], rows, [f"{n_out} outputs"] * 3)
        assert all((x.err, x.aux0, x.message) == (hr.E_BLACKBOX_FAILED, hr.FUNC_TAG[name], hr.msg_outputs(n_out)) for x in case.expect)
        out.append(case)
    return tuple(out)


def _digest_of(name, row, ins):
    return HASH_OF[name](b"".join((row[w - 1] % (1 << bits)).to_bytes((bits + 7) // 8, "little") for w, bits in ins))


@functools.lru_cache(maxsize=None)
def preassigned_case(name, width):
    """Inputs 1..6 the message (the last one `width` bits wide: 8 keeps the record in the cooperative kernel, 16 takes the lane kernel), 7..10 the witnesses
    that ARE outputs 0, 1, 4 and 31 of four records over the same message. A row has at most one of them wrong: the outputs before it stay in the map. A fifth record's output 2 is its own first input."""
    ins = [(w, 8) for w in range(1, 6)] + [(6, width)]
    b = Builder(10)
    for k, pos in enumerate(POSITIONS):
        outs = b.new(31)
        outs.insert(pos, 7 + k)
        b.hash(name, ins, outputs=outs)
    outs = b.new(31)
    outs.insert(2, 1)
    own = [(1, 8), (2, 8), (3, 8)]
    b.hash(name, own, outputs=outs)
    rng = random.Random(SEED + 6500 + len(name) + width)
    rows, notes = [], []
    for wrong in (None, 0, 1, 2, 3, None, "own"):
        for _ in range(2):
            while True:   # the fifth record passes where its digest's byte 2 is its first input
                row = [rng.randrange(256) for _ in range(5)] + [rng.randrange(1 << width)]
                if (_digest_of(name, row, own)[2] == row[0]) == (wrong != "own"):
                    break
            d = _digest_of(name, row, ins)
            row += [(d[pos] + (1 if wrong == k else 0)) % 256 for k, pos in enumerate(POSITIONS)]
            rows.append(row)
            notes.append("every pre-assigned output is right" if wrong is None else "the output that is an input is wrong" if wrong == "own" else f"output {POSITIONS[wrong]} is wrong")
    case = _case(f"F, {name}, pre-assigned outputs, last input {width} bits", b.circuit(), list(range(1, 11)), rows, notes, filler=0)
    assert [x.opcode_index for x in case.expect if x.status == hr.ST_FAILURE] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    return case


def add_twice(b, name, pools, width=8):
    """three records, one per pair of TWICE: the record's two positions hold one witness. pools: per record the six inputs it hashes."""
    recs = []
    for (p0, p1), pool in zip(TWICE, pools):
        outs = b.new(31)
        outs.insert(max(p0, p1), outs[min(p0, p1)])
        ins = [(w, 8) for w in pool[:5]] + [(pool[5], width)]
        b.hash(name, ins, outputs=outs)
        recs.append(ins)
    return recs


def grind(name, ins, n_inputs, rng, want):
    """values of the inputs `ins` names such that want(digest) holds; the others are left 0"""
    for _ in range(200000):
        row = [0] * n_inputs
        for w, bits in ins:
            row[w - 1] = rng.randrange(1 << bits)
        if want(_digest_of(name, row, ins)):
            return row
    raise AssertionError("no such message")


def twice_rows(name, recs, n_inputs, rng):
    """Rows: three in which the two bytes coincide at every record (they pass); per record two in which its bytes differ (the row fails there), in one of
    which the byte compared second is 0x00 and the other is not -- what an untouched row of the table reads as; and per record one that passes its record
    with both bytes 0x00."""
    rows, notes = [], []

    def row_of(parts):
        row = [0] * n_inputs
        for part in parts:
            for w in range(n_inputs):
                row[w] = row[w] or part[w]
        return row

    def same(k):
        return grind(name, recs[k], n_inputs, rng, lambda d: d[TWICE[k][0]] == d[TWICE[k][1]])

    for _ in range(3):
        rows.append(row_of([same(k) for k in range(3)]))
        notes.append("the bytes coincide at every record")
    for k, (p0, p1) in enumerate(TWICE):
        first, second = min(p0, p1), max(p0, p1)
        rows.append(row_of([same(i) if i != k else grind(name, recs[k], n_inputs, rng, lambda d: d[first] != d[second]) for i in range(3)]))
        notes.append(f"bytes {first} and {second} differ")
        rows.append(row_of([same(i) if i != k else grind(name, recs[k], n_inputs, rng, lambda d: d[second] == 0 and d[first] != 0) for i in range(3)]))
        notes.append(f"byte {second} is 0x00, byte {first} is not")
    return rows, notes


@functools.lru_cache(maxsize=None)
def twice_case(mode):
    """One witness twice among the 32 outputs, at the positions TWICE, in records shaped for each kernel mode of list B ("two buffers": 6 bytes; "one buffer":
    360 bytes; "one wave": N_FILL filler records on the same level) and for the lane path (a 16-bit input). The planner sends a record with a repeated
    output to the lane kernel whatever its shape (the second occurrence compares with what the first stored, and the cooperative kernel's waves
    store and compare side by side: on the device the rows whose compared byte is 0x00, and the rows of stale_rows, passed where the reference answers
    UnsatisfiedConstrain): meta counts the filler records alone."""
    n = 18
    ids = list(range(1, n + 1))
    rng = random.Random(SEED + 7000 + len(mode))
    name = "SHA256"
    b = Builder(n)
    pools = [ids[0:6], ids[6:12], ids[12:18]]
    if mode == "one buffer":   # the records themselves are longer than 352 bytes: their six inputs, then 60 times over
        recs = []
        for (p0, p1), pool in zip(TWICE, pools):
            outs = b.new(31)
            outs.insert(max(p0, p1), outs[min(p0, p1)])
            ins = [(w, 8) for w in pool] * 60
            b.hash(name, ins, outputs=outs)
            recs.append(ins)
        meta = {}
    else:
        recs = add_twice(b, name, pools, 16 if mode == "lane" else 8)
        meta = {}
    if mode == "one wave":
        for k in range(N_FILL):
            b.hash(("SHA256", "Blake2s")[k % 2], [ids[(k + i) % n] for i in range(3 + k % 23)])
        meta = {"coop_heads": N_FILL, "max_words": 7, "chained": 0}
    rows, notes = twice_rows(name, recs, n, rng)
    if mode == "one wave":   # the three passing rows again and again in front: the others lie in the last, partial wave and the one before it
        rows, notes = [rows[j % 3] for j in range(963 - 9)] + rows, [notes[j % 3] for j in range(963 - 9)] + notes
    case = _case(f"F, one witness twice among the outputs, {mode}", b.circuit(), ids, rows, notes, filler=0, meta=meta, max_rows=963)
    assert [x.status for x in case.expect[-9:]] == [hr.ST_SOLVED] * 3 + [hr.ST_FAILURE] * 6 and [x.opcode_index for x in case.expect[-6:]] == [0, 0, 1, 1, 2, 2]
    return case


TWICE_MODES = ("two buffers", "one buffer", "one wave", "lane")


@functools.lru_cache(maxsize=None)
def stale_rows(mode):
    """Rows for a SECOND solve on the handle that solved twice_case(mode): in row j the first record's byte 1 (compared) is what the first solve left in the
    shared output's row of the table, and its own byte 0 (stored) is another: a compare that reads the row before the store lands passes
    where the reference answers UnsatisfiedConstrain at opcode 0."""
    case = twice_case(mode)
    ins = [(f.witness, f.num_bits) for f in case.circuit.opcodes[0].args["inputs"]]
    rng = random.Random(SEED + 7500 + len(mode))
    rows = []
    shared = case.circuit.opcodes[0].args["outputs"][0]
    for x in case.expect[-9:]:
        left = x.witnesses[shared]   # (byte 0 of a row that passed; of a row that failed at this record, the byte insert_value put in before it compared)
        rows.append(grind("SHA256", ins, len(case.ids), rng, lambda d: d[1] == left and d[0] != left))
    out = _case(case.name + ", stale rows", case.circuit, case.ids, rows, ["byte 1 is the byte 0 of the solve before"] * 9, meta=case.meta)
    assert all((x.err, x.opcode_index) == (hr.E_UNSATISFIED, 0) for x in out.expect)
    return case._replace(rows=case.rows[-9:], expect=case.expect[-9:], notes=case.notes[-9:]), out


# ---------------------------------------------------------------------------------------------------------------- G: initial sets
@functools.lru_cache(maxsize=None)
def initial_set_case():
    """(circuit, maps, expect, notes): a SHA256 of three bytes and a Keccak256 of its digest; one group of maps assigns the three inputs; one also knows output 4
    of the SHA256 (right in some rows, wrong in others); one lacks the second input (MissingAssignment at opcode 0)"""
    b = Builder(3)
    d = b.hash("SHA256", [1, 2, 3])
    b.hash("Keccak256", d)
    circ = b.circuit()
    rng = random.Random(SEED + 8000)
    maps, notes = [], []
    for j in range(21):
        m = {w: rng.randrange(256) for w in (1, 2, 3)}
        if j % 3 == 1:
            byte = hashlib.sha256(bytes(m[w] for w in (1, 2, 3))).digest()[4]
            m[d[4]] = byte if j % 2 else (byte + 1) % 256
            notes.append("knows an output, " + ("right" if j % 2 else "wrong"))
        elif j % 3 == 2:
            del m[2]
            notes.append("lacks an input")
        else:
            notes.append("the plain set")
        maps.append(m)
    expect = [hr.run(circ, m) for m in maps]
    assert {(x.err, x.opcode_index) for x in expect} == {(hr.E_NONE, 0), (hr.E_UNSATISFIED, 0), (hr.E_MISSING_ASSIGNMENT, 0)}
    return circ, tuple(maps), tuple(expect), tuple(notes)


# ---------------------------------------------------------------------------------------------------------------- the lists
ALL = COOP + ("HashToField128Security", "Keccak256VariableLength")


@functools.lru_cache(maxsize=None)
def lists():
    """{letter: the cases that run as plain batches}; the 963-row cases (big_cases) and G's maps have tests of their own"""
    return {"A": tuple(length_case(f, "four waves") for f in COOP + ("HashToField128Security",)) + tuple(long_case(f) for f in COOP),
            "B": tuple(chain_case(m, r) for m in ("two buffers", "one buffer") for r in (False, True)) + tuple(threshold_case(n) for n in THRESHOLDS),
            "C": tuple(width_case(f) for f in ALL) + tuple(c for f in ALL for c in panic_cases(f)),
            "D": tuple(var_case(n) for n in VAR_LENGTHS) + var_mixed_case(),
            "E": (to_field_case(),),
            "F": tuple(c for f in WITH_OUTPUTS for c in count_cases(f)) + tuple(preassigned_case("SHA256", w) for w in (8, 16)) + (preassigned_case("Keccak256", 8),)
                 + tuple(twice_case(m) for m in TWICE_MODES if m != "one wave")}


@functools.lru_cache(maxsize=None)
def big_cases():
    """the cases of 963 rows: more than 2 048 items of at most 32 words in one launch, the one-wave instantiation"""
    return tuple(length_case(f, "one wave") for f in COOP) + (chain_case("one wave"), chain_case("one wave", True), twice_case("one wave"))


def all_cases():
    return [c for cs in lists().values() for c in cs]
