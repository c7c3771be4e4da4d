"""One builder of the inputs that reach the branches of the Grumpkin opcodes (acvm_amd/csrc/ops_grumpkin.hpp, kernels_grumpkin.hip) which random values
never reach, with every expected outcome from the integer model of tests/grumpkin_ref.py: no device and no product code here. The Pedersen generators
have unknown discrete logarithms and a Schnorr challenge is a hash of R, so no opcode input lands on the same-x branches of the additions, on a
boundary of a table window or in a rare class of the scalar split by chance: every list below is built by slice, window, digit or sign class.
tests/test_grumpkin_cases.py runs the lists through the CPU oracle and asserts what they cover; tests/test_gpu_grumpkin_edges.py runs them on the device.

A case is (name, circuit, ids, rows, expect, labels, notes) as in tests/int_cases.py: per instance Expect(status, err, opcode_index, witnesses) with the
WHOLE witness map the reference leaves behind (insert_value, acvm/src/pwg/mod.rs:338-357: an assigned output takes the new value, then the old one is
compared). The rules restated by model():
  Pedersen             acvm/src/pwg/blackbox/pedersen.rs:11-28
  FixedBaseScalarMul   acvm/src/pwg/blackbox/fixed_base_scalar_mul.rs:11-27, barretenberg_blackbox_solver/src/wasm/scalar_mul.rs:17-65
  SchnorrVerify        acvm/src/pwg/blackbox/signature/schnorr.rs:13-35, signature/mod.rs:5-18 (the last byte of each cell),
                       barretenberg_blackbox_solver/src/lib.rs:40-58 (63 cells panic), wasm/schnorr.rs:79-82 (128 + n >= 1024 panics)
The probe lists (formula_items, split_scalars, r_triples) are for acvm_debug_grumpkin_items, which runs one routine of the header per device lane."""
import collections
import functools
import random

import grumpkin_ref as gr
from acvm_amd.acir import P, BlackBoxFuncCall as BB, Circuit, FunctionInput as FI
from curve_table_ref import GRUMPKIN, R_BITS, ec_add, ec_mul
from grumpkin_ref import LAMBDA, Q, G, neg

SEED = 20262
ST_SOLVED, ST_FAILURE = 0, 2      # as oracle/binding.py numbers them (tests/test_grumpkin_cases.py asserts that these agree)
E_NONE, E_UNSATISFIED, E_BLACKBOX_FAILED, E_PANIC = 0, 4, 6, 8
M128 = (1 << 128) - 1
ALL = (1 << 253) - 1              # every bit set that a value below P can have set together with all the lower ones

Expect = collections.namedtuple("Expect", "status err opcode_index witnesses")
Case = collections.namedtuple("Case", "name circuit ids rows expect labels notes")


# ---- the reference's rules on a witness map
def _insert(wm, w, v):
    old = wm.get(w)
    wm[w] = v
    return old is None or old == v


def _step(op, wm):
    """one opcode on the witness map: None, or the error kind of the failure"""
    R, a = gr.ref(), op.args
    if op.name == "Pedersen":
        x, y = R.pedersen([wm[f.witness] for f in a["inputs"]], a["domain_separator"])
        return None if _insert(wm, a["outputs"][0], x) and _insert(wm, a["outputs"][1], y) else E_UNSATISFIED
    if op.name == "FixedBaseScalarMul":
        what, pt = R.fixed_base(wm[a["low"].witness], wm[a["high"].witness])
        if what != gr.FB_OK:
            return E_BLACKBOX_FAILED
        return None if _insert(wm, a["outputs"][0], pt[0]) and _insert(wm, a["outputs"][1], pt[1]) else E_UNSATISFIED
    if op.name == "SchnorrVerify":
        if len(a["signature"]) < 64 or 128 + len(a["message"]) >= 1024:
            return E_PANIC
        sig = bytes(wm[f.witness] & 255 for f in a["signature"][:64])
        msg = bytes(wm[f.witness] & 255 for f in a["message"])
        ok = R.schnorr_verify((wm[a["public_key_x"].witness], wm[a["public_key_y"].witness]), sig, msg)
        return None if _insert(wm, a["output"], int(ok)) else E_UNSATISFIED
    raise AssertionError(f"no model for {op!r}")


def model(circ, ids, row):
    wm = dict(zip(ids, row))
    for oi, op in enumerate(circ.opcodes):
        bad = _step(op, wm)
        if bad:
            return Expect(ST_FAILURE, bad, oi, wm)
    return Expect(ST_SOLVED, E_NONE, 0, wm)


def describe(case, j):
    return f"{case.name} row {j} ({case.notes[j]}), inputs {[hex(v) for v in case.rows[j][:6]]}"


def compare(case, got, who):
    """got: [(status, err, opcode_index, {witness: value})], one per row"""
    assert len(got) == len(case.expect)
    for j, (want, (status, err, opcode, wm)) in enumerate(zip(case.expect, got)):
        at = describe(case, j)
        assert (status, err) == (want.status, want.err), f"{at}: {who} status / error {(status, err)}, want {(want.status, want.err)}"
        if want.status == ST_FAILURE:
            assert opcode == want.opcode_index, f"{at}: {who} fails at opcode {opcode}, want {want.opcode_index}"
        for w in sorted(set(wm) | set(want.witnesses)):
            g, x = wm.get(w), want.witnesses.get(w)
            assert g == x, (f"{at}: witness {w} ({case.labels.get(w, 'input')}): {who} " + (hex(g) if g is not None else "unassigned") +
                            ", want " + (hex(x) if x is not None else "unassigned"))


def _case(name, circ, ids, rows, labels, notes):
    assert len(rows) == len(notes) and len(rows) % 64, (name, len(rows))
    assert all(0 <= v < P for row in rows for v in row) and all(len(row) == len(ids) for row in rows), name
    return Case(name, circ, ids, rows, [model(circ, ids, row) for row in rows], labels, notes)


# ---- Pedersen: values built around the 9-bit slices, the 18-bit slice pairs (ped2) and the 24-bit windows (pedw) the kernels walk
FIELDS = {"slice": (9, 29), "pair": (18, 15), "window": (24, 11)}   # name -> (width, how many cover the 254 bits)


def ones_below_p(lo, width):
    """the longest run of ones from bit `lo`, `width` bits at most, that is a value below P (slice 28, pair 14 and window 10 end above P's top bit)"""
    while (((1 << width) - 1) << lo) >= P:
        width -= 1
    return ((1 << width) - 1) << lo


def field_of(v, kind, i):
    width, _ = FIELDS[kind]
    return (v >> (width * i)) & ((1 << width) - 1)


@functools.lru_cache(maxsize=None)
def pedersen_values():
    """[(value, note)]"""
    out = [(0, "0"), (1, "1"), (P - 1, "P - 1"), (P - 2, "P - 2"), (1 << 253, "2^253"), (ALL, "every slice full below P")]
    for kind, (width, n) in FIELDS.items():
        for i in range(n):
            out.append((ones_below_p(width * i, width), f"{kind} {i} all ones"))
            out.append((ALL & ~(((1 << width) - 1) << (width * i)), f"{kind} {i} zero, every other bit set"))
    for width, n in ((18, 15), (24, 11)):
        for i in range(n):
            out += [((1 << (width * i)) + d, f"2^({width} * {i}) {d:+d}") for d in (-1, 1) if 0 <= (1 << (width * i)) + d]
    seen, uniq = set(), []
    for v, note in out:
        assert 0 <= v < P, note
        if v not in seen:
            seen.add(v)
            uniq.append((v, note))
    return tuple(uniq)


HASH_INDICES = [0, 1, 3, (1 << 32) - 1]
RECORDS = [(1, 1), (2, 3), (4, (1 << 32) - 1), (5, 0), (8, 0), (20, 1)]   # (inputs, hash_index) of the six records of pedersen_records_case
BATCH_SIZES = (67, 130, 321)


@functools.lru_cache(maxsize=None)
def pedersen_single_case():
    """one circuit of one record (one input, hash_index 0) over every value of pedersen_values, filled up to 321 instances -- a partial workgroup -- with
    seeded random values; outputs in witnesses 2, 3"""
    rng = random.Random(SEED)
    circ = Circuit(3, [BB("Pedersen", {"inputs": [FI(1, 254)], "domain_separator": 0, "outputs": [2, 3]})])
    rows, notes = [[v] for v, _ in pedersen_values()], [n for _, n in pedersen_values()]
    assert len(rows) <= 321
    while len(rows) < 321:
        rows.append([rng.randrange(P)])
        notes.append("random")
    return _case("pedersen, one record", circ, [1], rows, {2: "x", 3: "y"}, notes)


@functools.lru_cache(maxsize=None)
def pedersen_records_case():
    """six records with 1, 2, 4, 5, 8 and 20 inputs and the four hash indices in one circuit: with four or more inputs, several records and several blocks
    every wave of the quad kernel takes the serial tail. 20 input witnesses, record r reads them from witness 1 + 3 r on (wrapping); 130 instances (two
    blocks); the values of pedersen_values walk through the rows so that every one of them is an input of some record."""
    rng = random.Random(SEED + 1)
    ids = list(range(1, 21))
    ops, labels, out = [], {}, 20
    for r, (n, hi) in enumerate(RECORDS):
        ops.append(BB("Pedersen", {"inputs": [FI(1 + (3 * r + k) % 20, 254) for k in range(n)], "domain_separator": hi, "outputs": [out + 1, out + 2]}))
        labels[out + 1], labels[out + 2] = f"x of record {r} ({n} inputs, hash_index {hi})", f"y of record {r}"
        out += 2
    vals = [v for v, _ in pedersen_values()]
    rows, notes = [], []
    for j in range(130):
        rows.append([vals[(20 * j + i) % len(vals)] if (j + i) % 3 else rng.randrange(P) for i in range(20)])
        notes.append(f"values {20 * j % len(vals)} on")
    return _case("pedersen, six records", Circuit(out, ops), ids, rows, labels, notes)


@functools.lru_cache(maxsize=None)
def pedersen_compared_case():
    """outputs that are inputs too: record 0 (two inputs) writes its x into witness 3, record 1 (hash_index 3) its y into witness 4. Rows j % 3 == 0 carry
    the right values there, j % 3 == 1 a wrong x (Unsatisfied at opcode 0, y unassigned), j % 3 == 2 a wrong y (Unsatisfied at opcode 1). 67 instances: a
    partial second wave."""
    rng = random.Random(SEED + 2)
    R = gr.ref()
    ops = [BB("Pedersen", {"inputs": [FI(1, 254), FI(2, 254)], "domain_separator": 0, "outputs": [3, 5]}),
           BB("Pedersen", {"inputs": [FI(2, 254)], "domain_separator": 3, "outputs": [6, 4]})]
    vals = [v for v, _ in pedersen_values()]
    rows, notes = [], []
    for j in range(67):
        a, b = vals[(2 * j) % len(vals)], rng.randrange(P) if j % 2 else vals[(2 * j + 1) % len(vals)]
        x, y = R.pedersen([a, b], 0)[0], R.pedersen([b], 3)[1]
        if j % 3 == 1:
            x = (x + 1) % P if j % 2 else rng.randrange(P)
        if j % 3 == 2:
            y = (y - 1) % P
        rows.append([a, b, x, y])
        notes.append(["both right", "x wrong", "y wrong"][j % 3])
    case = _case("pedersen, compared outputs", Circuit(6, ops), [1, 2, 3, 4], rows, {3: "x of record 0 (given)", 4: "y of record 1 (given)", 5: "y of record 0", 6: "x of record 1"}, notes)
    for j, x in enumerate(case.expect):
        want = [(ST_SOLVED, E_NONE, 0), (ST_FAILURE, E_UNSATISFIED, 0), (ST_FAILURE, E_UNSATISFIED, 1)][j % 3]
        assert (x.status, x.err, x.opcode_index) == want and (5 in x.witnesses) == (j % 3 != 1), j
    return case


# ---- FixedBaseScalarMul: every digit of both window widths at its ends, the window boundaries, the ends of the scalar range, the refusals
@functools.lru_cache(maxsize=None)
def fixed_base_scalars():
    """[(low, high, note)]"""
    out = []

    def add(k, note):
        out.append((k & M128, k >> 128, note))

    for w in range(16):
        add(1 << (16 * w), f"16-bit digit {w} = 1")
        if 65535 << (16 * w) < Q:
            add(65535 << (16 * w), f"16-bit digit {w} = 65535")
    add((Q - 1) >> 240 << 240, "16-bit digit 15 at its largest below q")
    for w in range(32):
        add(1 << (8 * w), f"8-bit digit {w} = 1")
        if 255 << (8 * w) < Q:
            add(255 << (8 * w), f"8-bit digit {w} = 255")
    add((Q - 1) >> 248 << 248, "8-bit digit 31 at its largest below q")
    for w in range(1, 16):
        add((1 << (16 * w)) - 1, f"2^(16 * {w}) - 1")
    add(Q - 1, "q - 1")
    add(Q - 2, "q - 2")
    add((Q - 1) // 2, "(q - 1) / 2")
    hi = (Q >> 128) - 1 if (Q & M128) < M128 else Q >> 128
    out.append((M128, hi, "low = 2^128 - 1 with the largest valid high"))
    assert (hi << 128 | M128) < Q <= ((hi + 1) << 128 | M128)
    add(0, "0: the point at infinity, (0, 0)")
    out += [(1 << 128, 0, "low = 2^128"), (P - 1, 0, "low = P - 1"), (0, 1 << 128, "high = 2^128"), (1 << 128, 1 << 128, "both limbs too wide: low is named"),
            (Q & M128, Q >> 128, "k = q"), ((Q + 1) & M128, (Q + 1) >> 128, "k = q + 1"), (0, 1 << 126, "k = 2^254"), (M128, M128, "k = 2^256 - 1")]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fixed_base_case():
    circ = Circuit(4, [BB("FixedBaseScalarMul", {"low": FI(1, 128), "high": FI(2, 128), "outputs": [3, 4]})])
    rows, notes = [[lo, hi] for lo, hi, _ in fixed_base_scalars()], [n for _, _, n in fixed_base_scalars()]
    rng = random.Random(SEED + 3)
    while len(rows) % 64 != 3:
        rows.append([rng.randrange(1 << 128), rng.randrange(Q >> 128)])
        notes.append("random")
    return _case("fixed base", circ, [1, 2], rows, {3: "x", 4: "y"}, notes)


# ---- SchnorrVerify
MSG_LENGTHS = [0, 1, 31, 32, 33, 95, 96, 97, 895]      # 32 + n around Blake2s's 64-byte block, and the longest message that does not panic
SECRET_KEYS = [1, 2, Q - 1, LAMBDA, Q - LAMBDA, 0x1F3C5A7E9B2D4F60718293A4B5C6D7E8F9010B1C2D3E4F5061728394A5B6C7D8 % Q]
NONCES = [1, 2, Q - 1]                                 # and seeded random ones

Signed = collections.namedtuple("Signed", "sk k pk sig msg")


def _message(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def split_class(e):
    """(sign of k2, a digit of magnitude 16 in k1 / in k2, a zero top digit in k1 / in k2) of e mod q"""
    k1, k2 = gr.glv_split(e % Q)
    d1, d2 = gr.signed_windows5(k1), gr.signed_windows5(abs(k2))
    return ((k2 > 0) - (k2 < 0), 16 in d1, 16 in d2, d1[25] == 0, d2[25] == 0)


@functools.lru_cache(maxsize=None)
def signed_messages(n_msg):
    """accepting signatures over messages of n_msg bytes: every secret key of SECRET_KEYS with the nonces in turn; and, for n_msg = 33 (the grinding list),
    seeded nonces ground until every count 0..5 of reduce_mod_q's subtractions on e occurs twice and a digit 16 and a zero top digit occur in both halves
    of the split"""
    R = gr.ref()
    rng = random.Random(SEED + 10 + n_msg)
    out = []
    for i, sk in enumerate(SECRET_KEYS):
        k = NONCES[(i + n_msg) % 4] if (i + n_msg) % 4 < 3 else rng.randrange(1, Q)
        msg = _message(rng, n_msg)
        pk, sig = R.schnorr_sign(sk, k, msg)
        out.append(Signed(sk, k, pk, sig, msg))
    if n_msg == 33:
        need = collections.Counter({("count", c): 2 for c in range(6)})
        need.update({("digit 16", h): 1 for h in (1, 2)})
        need.update({("top zero", h): 1 for h in (1, 2)})
        for s in out:
            need[("count", gr.reduce_count(int.from_bytes(s.sig[32:], "big")))] -= 1
        sk = SECRET_KEYS[5]
        for _ in range(4000):
            if all(v <= 0 for v in need.values()):
                break
            k, msg = rng.randrange(1, Q), _message(rng, n_msg)
            pk, sig = R.schnorr_sign(sk, k, msg)
            e = int.from_bytes(sig[32:], "big")
            _, s1, s2, z1, z2 = split_class(e)
            has = [("count", gr.reduce_count(e))] + [("digit 16", h) for h, f in ((1, s1), (2, s2)) if f] + [("top zero", h) for h, f in ((1, z1), (2, z2)) if f]
            if any(need[x] > 0 for x in has):
                for x in has:
                    need[x] -= 1
                out.append(Signed(sk, k, pk, sig, msg))
        assert all(v <= 0 for v in need.values()), need
    return tuple(out)


def _cell(rng, b, style):
    """a witness whose last big-endian byte is b: the byte itself, 256 + b, or P - 256 + c (P ends in the byte 01)"""
    if style == 0:
        return b
    if style == 1:
        return 256 * rng.randrange(1, 1 << 200) + b
    v = P - 256 + ((b - 1) & 255)
    assert v < P and v & 255 == b
    return v


def schnorr_circuit(n_sig, n_msg, out_is_input=False):
    """witnesses: 1, 2 the public key, then the signature cells, then the message cells, then the output"""
    sig = list(range(3, 3 + n_sig))
    msg = list(range(3 + n_sig, 3 + n_sig + n_msg))
    out = 3 + n_sig + n_msg
    circ = Circuit(out, [BB("SchnorrVerify", {"public_key_x": FI(1, 254), "public_key_y": FI(2, 254), "signature": [FI(w, 8) for w in sig],
                                               "message": [FI(w, 8) for w in msg], "output": out})])
    return circ, [1, 2] + sig + msg + ([out] if out_is_input else []), out


def _row(pk, sig, msg):
    return [pk[0], pk[1]] + list(sig) + list(msg)


def s_variants(sig):
    """the signature with s + m q in place of s, for every m >= 1 that stays below 2^256"""
    s = int.from_bytes(sig[:32], "big")
    return [(s + m * Q).to_bytes(32, "big") + sig[32:] for m in range(1, 6) if s + m * Q < 1 << 256]


@functools.lru_cache(maxsize=None)
def schnorr_accepting_case(n_msg):
    circ, ids, out = schnorr_circuit(64, n_msg)
    rows, notes = [], []
    for i, s in enumerate(signed_messages(n_msg)):
        rows.append(_row(s.pk, s.sig, s.msg))
        notes.append(f"signed, key {i}")
        for m, v in enumerate(s_variants(s.sig), start=1):
            rows.append(_row(s.pk, v, s.msg))
            notes.append(f"signed, key {i}, s + {m} q")
    if len(rows) % 64 == 0:
        rows.append(rows[0])
        notes.append("filler")
    case = _case(f"schnorr accepting, {n_msg} bytes", circ, ids, rows, {out: "verdict"}, notes)
    assert all(x.status == ST_SOLVED and x.witnesses[out] == 1 for x in case.expect), case.name
    return case


@functools.lru_cache(maxsize=None)
def schnorr_rejecting_case():
    """status Solved, output 0, over 33-byte messages (32 + 33 bytes: a second Blake2s block of one byte). The last two groups sit on the exceptional branches
    of the final addition R = e pk + s G: s = e sk makes it a doubling (R = 2 e pk, finite: the digest decides), s = -e sk the point at infinity."""
    R = gr.ref()
    rng = random.Random(SEED + 30)
    circ, ids, out = schnorr_circuit(64, 33)
    rows, notes = [], []

    def add(pk, sig, msg, note):
        rows.append(_row(pk, sig, msg))
        notes.append(note)

    for i, s in enumerate(signed_messages(33)[:6]):
        S, E = int.from_bytes(s.sig[:32], "big"), int.from_bytes(s.sig[32:], "big")
        be = lambda a, b: a.to_bytes(32, "big") + b.to_bytes(32, "big")  # noqa: E731
        add(s.pk, be(S ^ (1 << rng.randrange(253)), E), s.msg, f"key {i}: a bit of s flipped")
        add(s.pk, be(S, E ^ (1 << rng.randrange(256))), s.msg, f"key {i}: a bit of e flipped")
        flipped = bytearray(s.msg)
        flipped[rng.randrange(33)] ^= 1 << rng.randrange(8)
        add(s.pk, s.sig, bytes(flipped), f"key {i}: a bit of the message flipped")
        add(neg(s.pk), s.sig, s.msg, f"key {i}: pk_y negated")
        add((s.pk[0], (s.pk[1] + 1) % P), s.sig, s.msg, f"key {i}: pk off the curve")
        add((0, 0), s.sig, s.msg, f"key {i}: pk = (0, 0)")
        add(s.pk, be(0, E), s.msg, f"key {i}: s = 0")
        add(s.pk, be(Q, E), s.msg, f"key {i}: s = q")
        add(s.pk, be(S, 0), s.msg, f"key {i}: e = 0")
        add(s.pk, be(S, Q), s.msg, f"key {i}: e = q")
        for e in (E, split_scalars()[(7 * i) % len(split_scalars())][0] or 5):   # the signature's own e, and one of a crafted class
            es = e % Q * s.sk % Q
            add(s.pk, be(es, e), s.msg, f"key {i}: s = e sk, the final addition doubles")
            add(s.pk, be(Q - es, e), s.msg, f"key {i}: s = -e sk, R is the point at infinity")
            if es + Q < 1 << 256:
                add(s.pk, be(es + Q, e), s.msg, f"key {i}: s = e sk + q")
    if len(rows) % 64 == 0:
        add((0, 0), bytes(64), bytes(33), "filler")
    case = _case("schnorr rejecting", circ, ids, rows, {out: "verdict"}, notes)
    assert all(x.status == ST_SOLVED and x.witnesses[out] == 0 for x in case.expect)
    return case


@functools.lru_cache(maxsize=None)
def schnorr_cells_case():
    """signature and message cells that are not bytes (only the last byte counts), accepting and rejecting, and the verdict as a compared output: witness
    `out` is an input that holds the right verdict, or (every third row) the wrong one -- Unsatisfied at opcode 0 with the computed verdict in the map"""
    rng = random.Random(SEED + 31)
    circ, ids, out = schnorr_circuit(64, 31, out_is_input=True)
    rows, notes = [], []
    for i, s in enumerate(signed_messages(31)):
        for style in (0, 1, 2):
            for good in (True, False):
                sig = bytearray(s.sig)
                if not good:
                    sig[rng.randrange(64)] ^= 1 << rng.randrange(8)
                cells = [_cell(rng, b, style if k % 2 == 0 or style == 0 else 3 - style) for k, b in enumerate(bytes(sig) + s.msg)]
                verdict = int(good)
                wrong = len(rows) % 3 == 2
                rows.append([s.pk[0], s.pk[1]] + cells + [verdict ^ wrong])
                notes.append(f"key {i}, cells {['bytes', '256 k + b', 'P - 256 + c'][style]}, {'accepting' if good else 'rejecting'}, verdict given {'wrong' if wrong else 'right'}")
    if len(rows) % 64 == 0:
        rows.append(rows[0])
        notes.append("filler")
    case = _case("schnorr cells and compared verdict", circ, ids, rows, {out: "verdict (given)"}, notes)
    for j, x in enumerate(case.expect):
        assert (x.status, x.err) == ((ST_FAILURE, E_UNSATISFIED) if j % 3 == 2 and notes[j] != "filler" else (ST_SOLVED, E_NONE)), j
    return case


@functools.lru_cache(maxsize=None)
def schnorr_panic_cases():
    """63 signature cells (the slice [32..64] panics) and 896 message bytes (the message overruns the scratch space)"""
    s = signed_messages(1)[0]
    circ, ids, _ = schnorr_circuit(63, 1)
    short = _case("schnorr, 63 signature cells", circ, ids, [_row(s.pk, s.sig[:63], s.msg), _row((0, 0), bytes(63), b"\0"), _row(s.pk, s.sig[1:], s.msg)], {}, ["panics"] * 3)
    circ, ids, _ = schnorr_circuit(64, 896)
    long_ = _case("schnorr, 896 message bytes", circ, ids, [_row(s.pk, s.sig, s.msg * 896), _row((0, 0), bytes(64), bytes(896)), _row(s.pk, s.sig, bytes(896))], {}, ["panics"] * 3)
    for case in (short, long_):
        assert all((x.status, x.err, x.opcode_index) == (ST_FAILURE, E_PANIC, 0) for x in case.expect)
    return short, long_


CASE_BUILDERS = collections.OrderedDict(
    [("pedersen, one record", pedersen_single_case), ("pedersen, six records", pedersen_records_case), ("pedersen, compared outputs", pedersen_compared_case),
     ("fixed base", fixed_base_case)] +
    [(f"schnorr accepting, {n} bytes", functools.partial(schnorr_accepting_case, n)) for n in MSG_LENGTHS] +
    [("schnorr rejecting", schnorr_rejecting_case), ("schnorr cells and compared verdict", schnorr_cells_case),
     ("schnorr, 63 signature cells", lambda: schnorr_panic_cases()[0]), ("schnorr, 896 message bytes", lambda: schnorr_panic_cases()[1])])
PEDERSEN_CASES = [n for n in CASE_BUILDERS if n.startswith("pedersen")]
SCHNORR_CASES = [n for n in CASE_BUILDERS if n.startswith("schnorr")]


def case(name):
    c = CASE_BUILDERS[name]()
    assert c.name == name
    return c


# ---- each list must bite: one expected value per list moved, for the comparisons of tests/test_grumpkin_cases.py (oracle) and of the device tests
PERTURBATIONS = [("pedersen, six records", "coordinate"), ("fixed base", "status"), ("schnorr rejecting", "verdict"), ("pedersen, compared outputs", "failing opcode")]


def perturbed(name, what):
    """(row, the case with that row's expectation changed)"""
    c = case(name)

    def change(j, **kw):
        expect = list(c.expect)
        expect[j] = expect[j]._replace(**kw)
        return j, c._replace(expect=expect)

    if what == "coordinate":    # the y of the last record (20 inputs) of the last row
        j, w = len(c.rows) - 1, max(c.expect[-1].witnesses)
        return change(j, witnesses={**c.expect[j].witnesses, w: c.expect[j].witnesses[w] ^ 1})
    if what == "status":        # a refused scalar expected to solve
        return change(next(i for i, x in enumerate(c.expect) if x.err == E_BLACKBOX_FAILED), status=ST_SOLVED, err=E_NONE)
    if what == "verdict":       # the row whose R is the point at infinity expected to accept
        j = next(i for i, n in enumerate(c.notes) if "infinity" in n)
        return change(j, witnesses={**c.expect[j].witnesses, max(c.expect[j].witnesses): 1})
    assert what == "failing opcode"   # a wrong y (opcode 1) expected at opcode 0
    return change(next(i for i, x in enumerate(c.expect) if x.opcode_index == 1), opcode_index=0)


# ---- the probe lists
@functools.lru_cache(maxsize=None)
def split_scalars():
    """[(k, note)], k < q, for glv_split + signed_windows5: the three sign classes that exist (k1 is never negative, grumpkin_ref.glv_split), the ends of
    the range, multiples of lambda, the 2^127 neighbourhood, digits of magnitude 16 and zero top digits in both halves"""
    rng = random.Random(SEED + 40)
    out = [(0, "0"), (1, "1"), (2, "2"), (15, "15"), (16, "16: one digit 16"), (17, "17: the first borrow"), (Q - 1, "q - 1"), (Q - 2, "q - 2"), (LAMBDA, "lambda"),
           (LAMBDA + 1, "lambda + 1"), (LAMBDA - 1, "lambda - 1"), (Q - LAMBDA, "q - lambda"), (2 * LAMBDA % Q, "2 lambda"), (7 * LAMBDA % Q, "7 lambda"),
           ((Q - 3 * LAMBDA) % Q, "-3 lambda"), (1 << 127, "2^127"), ((1 << 127) - 1, "2^127 - 1"), ((1 << 128) + 5, "2^128 + 5"), (1 << 253, "2^253"), (Q // 2, "q / 2"),
           (Q // 3, "q / 3")]
    out += [((1 << b) - 1, f"2^{b} - 1: k2 = 0") for b in (5, 64, 100, 126)] + [(int("1000000000" * 12, 2), "every other digit 16, k2 = 0"), (int("10000" * 25, 2), "every digit 16, k2 = 0")]
    for i in range(12):   # k2 > 0: k A / q a hair above an integer
        m, t = rng.randrange(1, gr.GLV_A - 1), 62 + (i * 5) % 58
        out.append((-(-m * Q // gr.GLV_A) + (1 << t), f"ceil(m q / A) + 2^{t}: k2 > 0"))
    for s in signed_messages(33):
        out.append((int.from_bytes(s.sig[32:], "big") % Q, "e of a signature"))
    out += [(rng.randrange(Q), "random") for _ in range(16)]
    assert all(0 <= k < Q for k, _ in out)
    return tuple(out)


Triple = collections.namedtuple("Triple", "pk e s want note")


@functools.lru_cache(maxsize=None)
def r_triples():
    """R = e pk + s G (s, e below q) with the expected point, None for the point at infinity: s = e sk (the final addition doubles), s = -e sk (it returns
    infinity), each +- 1, for e of every class of split_scalars; s at the ends of the fixed-base windows"""
    R = gr.ref()
    out = []
    sks = SECRET_KEYS + [3]
    es = [k for k, _ in split_scalars() if k] + [Q - 1]
    for i, e in enumerate(es):
        sk = sks[i % len(sks)]
        pk = R.mul_g(sk)
        for what, s in (("e sk", e * sk % Q), ("-e sk", -e * sk % Q)):
            for d in ((0,) if i % 4 else (0, 1, -1)):
                s1 = (s + d) % Q
                out.append(Triple(pk, e, s1, R.mul_g((e * sk + s1) % Q), f"s = {what} {d:+d}, sk {i % len(sks)}, e = {e:#x}"))
    pk = R.mul_g(sks[5])
    for w in range(16):
        for s in (1 << (16 * w), 65535 << (16 * w)):
            if s < Q:
                e = es[(3 * w) % len(es)]
                out.append(Triple(pk, e, s, R.mul_g((e * sks[5] + s) % Q), f"s = {s:#x}, a fixed-base window end"))
    assert sum(1 for t in out if t.want is None) >= 30
    return tuple(out)


# the lazy 29-bit working form: a coordinate v travels as the Montgomery residue v 2^261 mod P, or that plus P ("class A": normalised limbs, value < 2 P)
MONT = (1 << R_BITS) % P
MONT_INV = pow(MONT, -1, P)


def limbs29(v, rep=0):
    """the nine 29-bit limbs of the representative rep (0: in [0, P), 1: in [P, 2 P)) of the coordinate v"""
    m = v * MONT % P + rep * P
    return [(m >> (29 * i)) & 0x1FFFFFFF for i in range(9)]


def from_limbs29(limbs):
    """(the coordinate, the raw value of the limbs)"""
    raw = sum(int(x) << (29 * i) for i, x in enumerate(limbs))
    return raw * MONT_INV % P, raw


def jac(pt, z):
    """the affine point (None: infinity, as Z = 0 with X = Y = 1) with the denominator z"""
    if pt is None:
        return (1, 1, 0)
    return (pt[0] * z * z % P, pt[1] * z * z * z % P, z % P)


def jac_to_affine(X, Y, Z):
    if Z % P == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


Item = collections.namedtuple("Item", "coords reps want note")   # coords: 3 (dbl), 5 (add_aff29: X Y Z x2 y2) or 6 (add) field values; reps: one 0 / 1 per coordinate


def _reps(n, rng, exhaustive):
    return [tuple((m >> i) & 1 for i in range(n)) for m in range(1 << n)] if exhaustive else [tuple(rng.randrange(2) for _ in range(n))]


@functools.lru_cache(maxsize=None)
def formula_items(which):
    """which: "dbl", "add_aff29", "add". Exceptional items carry every coordinate in both representatives (all 2^n combinations); Z = 0 with rep 1 is the
    infinity whose limbs are P's. The points are multiples of G and of a Pedersen generator, so that the model knows every sum."""
    R = gr.ref()
    rng = random.Random(SEED + 50 + len(which))
    pts = [G, R.mul_g(2), R.mul_g(Q - 1), R.D[0], ec_mul(GRUMPKIN, 5, R.D[7]), R.mul_g(rng.randrange(Q))]
    zs = lambda: [1, P - 1, rng.randrange(2, P)]  # noqa: E731
    out = []

    def add(coords, want, note, exhaustive):
        for reps in _reps(len(coords), rng, exhaustive):
            out.append(Item(tuple(coords), reps, want, note))

    if which == "dbl":
        for pt in pts:
            for z in zs():
                add(jac(pt, z), ec_add(GRUMPKIN, pt, pt), "ordinary", z == 1 and pt == pts[0])
        for pt in pts[:3]:
            X, _, Z = jac(pt, rng.randrange(2, P))
            add((X, 0, Z), None, "Y = 0 (mod p): not a curve point, the branch returns infinity", True)
            add((X, rng.randrange(1, P), 0), None, "Z = 0 (mod p): infinity in, infinity out", True)
        add((1, 1, 0), None, "the infinity gj_inf() writes", True)
    elif which == "add_aff29":
        for pt in pts:
            for q in pts:
                for z in zs()[:2 if pt != q else 3]:
                    kind = "doubling" if pt == q else "opposite points" if pt == neg(q) else "ordinary"
                    add(jac(pt, z) + q, ec_add(GRUMPKIN, pt, q), kind, kind != "ordinary" and z != 1 and pt in pts[:2])
        for q in pts[:2]:
            add((rng.randrange(P), rng.randrange(P), 0) + q, q, "P at infinity", True)
    else:
        for pt in pts:
            for q in pts:
                kind = "doubling" if pt == q else "opposite points" if pt == neg(q) else "ordinary"
                z1 = rng.randrange(2, P)
                for za, zb in ((1, 1), (z1, z1), (P - 1, rng.randrange(2, P)), (rng.randrange(2, P), 1)):
                    add(jac(pt, za) + jac(q, zb), ec_add(GRUMPKIN, pt, q), f"{kind}, {'equal' if za == zb else 'different'} Z", kind != "ordinary" and pt == pts[0] and za in (z1, P - 1))
        for pt in pts[:2]:
            inf = (rng.randrange(P), rng.randrange(P), 0)
            add(inf + jac(pt, rng.randrange(2, P)), pt, "P at infinity", True)
            add(jac(pt, rng.randrange(2, P)) + inf, pt, "Q at infinity", True)
        add((1, 1, 0, 5, 7, 0), None, "both at infinity", True)
    if len(out) % 64 == 0:   # (the launch ends inside a wave)
        out.append(out[0])
    return tuple(out)
