"""The rows random values never reach, for the deflating container of the batch-wide wire format (tests/wire_deflate_ref.py): values as 64 hex
digits built so that every match length occurs with each distance that can produce it, ties, runs inside a value, the edge values, keys that
move where the distance-76 run starts, and the entry counts around the kernel's window. tests/test_wire_deflate_cases.py asserts what they
cover; tests/test_wire_deflate_on_host.py and tests/test_gpu_wire_deflate.py run them.

CHAIN is one flat list of values in which the values at 2 i and 2 i + 1 are a (predecessor, entry) pair; ROW_VALUES of them in a row make one
instance's inputs, so pairs never straddle two rows."""
import os
import random
import re

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGITS = "0123456789abcdef"
ROW_VALUES = 20


def window():
    """the kernel's window in list positions, read from the source"""
    return int(re.search(r"WIRE_PLAN_WINDOW = (\d+)", open(os.path.join(ROOT, "acvm_amd", "csrc", "wire_plan.hpp")).read()).group(1))


def _digits(rng, n, prev=None, at=0, before=None, avoid=""):
    """n digits, no two neighbours equal, each unlike prev's digit at its place (prev: 64 digits, at: the place of the first), none of `avoid`;
    the value's first digit is 1 or 2, so that the value is below p"""
    out = []
    for q in range(n):
        banned = set(avoid)
        if out or before:
            banned.add(out[-1] if out else before)
        if prev is not None:
            banned.add(prev[at + q])
            if at + q + 1 < 64 and at + q:
                banned.add(prev[at + q + 1])  # (so that a digit copied from prev behind this one is no repeat)
        pool = "12" if at + q == 0 else DIGITS
        out.append(rng.choice([d for d in pool if d not in banned]))
    return "".join(out)


def _leading(rng, k, prev=None):
    """exactly k leading '0' digits"""
    if k == 64:
        return "0" * 64
    body = _digits(rng, 64 - k, prev, k, before="0", avoid="0" if k else "")
    return "0" * k + body


def _pairs():
    rng = random.Random(0xDEF1A7E0)
    pairs = []
    # k leading zeros behind k' leading zeros: the distance-76 run is 11 header bytes and min(k, k') zeros, a distance-1 run takes the rest
    for kp, ks in [(0, range(65)), (1, range(65)), (5, range(65))] + [(k, [64]) for k in range(65)] + [(k, [k]) for k in range(65)]:
        for k in ks:
            prev = _leading(rng, kp)
            pairs.append((prev, _leading(rng, k, prev)))
    # a stretch of n digits shared with the predecessor inside the value: distance 76, length n, for n below 11 too
    for n in range(3, 65):
        a = (64 - n) // 2
        prev = _digits(rng, 64)
        cur = _digits(rng, a, prev, 0) + prev[a:a + n]
        cur += _digits(rng, 64 - a - n, prev, a + n, before=cur[-1])
        pairs.append((prev, cur))
    # a run of n + 1 equal digits inside the value: distance 1, length n
    for n in range(3, 64):
        a = (63 - n) // 2
        r = "1" if a == 0 else rng.choice(DIGITS[3:])
        prev = _digits(rng, 64, avoid=r)
        cur = _digits(rng, a, prev, 0, avoid=r) + r * (n + 1)
        cur += _digits(rng, 63 - n - a, prev, a + n + 1, before=r, avoid=r)
        pairs.append((prev, cur))
    # ties: the run of n equal digits is also the predecessor's, and the digit in front of it is the same digit
    for n in (3, 4, 10, 17, 40):
        a = 7
        r = rng.choice(DIGITS[3:])
        prev = _digits(rng, a, avoid=r) + r * n
        prev += _digits(rng, 64 - a - n, before=r, avoid=r)
        cur = _digits(rng, a - 1, prev, 0, avoid=r) + r * (n + 1)
        cur += _digits(rng, 64 - a - n, prev, a + n, before=r, avoid=r)
        pairs.append((prev, cur))
    # digits that run, alternate, the edge values
    runs = ["0" + "a" * 63, "0" + "f" * 63, "12" * 32, "0a" * 32, "0" * 64, "%064x" % (P - 1), "%064x" % 1, "2" + "0" * 63]
    for x in runs:
        for y in runs:
            pairs.append((x, y))
    return pairs


PAIRS = _pairs()
CHAIN = [int(v, 16) for pair in PAIRS for v in pair]
while len(CHAIN) % ROW_VALUES:
    CHAIN.append(CHAIN[len(CHAIN) % 7])
assert all(v < P for v in CHAIN)
N_ROWS = len(CHAIN) // ROW_VALUES


def row_values(j):
    """the ROW_VALUES inputs of instance j (any j: the rows repeat)"""
    j %= N_ROWS
    return CHAIN[ROW_VALUES * j:ROW_VALUES * (j + 1)]


def rows(first_key=1):
    """the case rows as maps: row j is {first_key + k: row_values(j)[k]}"""
    return [{first_key + k: v for k, v in enumerate(row_values(j))} for j in range(N_ROWS)]


# keys that move where the distance-76 run starts: w and w + 1 (from byte 1), a carry into byte 1 (from byte 2), w + 256 (byte 0, then from
# byte 2), w + 2^16, w + 2^24 (bytes 0 .. 2, then from byte 4)
KEY_LISTS = [[5, 6], [255, 256], [5, 261], [5, 6, 262, 263], [7, 7 + (1 << 16)], [5, 5 + (1 << 24)], [0x01010101, 0x01010102, 0x02010102]]


def keyed_rows():
    """maps over KEY_LISTS with values of the chain: some pairs equal, so the run goes on into the value"""
    out = []
    for i, keys in enumerate(KEY_LISTS):
        for rot in (0, 1):
            vals = [CHAIN[(2 * i + k // 2 if rot else 2 * i + k) % len(CHAIN)] for k in range(len(keys))]
            out.append(dict(zip(keys, vals)))
        out.append({k: 0 for k in keys})
    return out


def count_rows():
    """entry counts 0, 1, W - 1, W, W + 1, 2 W + 1 and one row of about 600 entries, from keys 1 on: values of the chain, every third a byte"""
    w = window()
    out = []
    for n in (0, 1, w - 1, w, w + 1, 2 * w + 1, 600):
        out.append({1 + k: (CHAIN[(3 * n + k) % len(CHAIN)] if k % 3 else (37 * k + n) % 256) for k in range(n)})
    return out
