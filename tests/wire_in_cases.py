"""Rows for the batch-wide wire import (include/acvm_amd.h acvm_batch_import_device_wire): good rows in every spelling the device form reads --
either letter case, unreduced values, partial maps -- the malformed rows of each finding class, and the device's judgement of a slot restated
in Python (findings). A map is {witness: int}; bytes come from tests/wire_ref.py. Pinned on the CPU by tests/test_wire_in_cases.py against
acvm_amd.decompress_witness."""
import random
import struct
import zlib

import wire_ref
from wire_ref import BINCODE, GZIP_STORED

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
COUNT, LENGTH, HEX, KEY, ORDER, FRAMING, CRC = 1, 2, 3, 4, 5, 6, 7
DIGITS = b"0123456789abcdefABCDEF"


# ---- good rows
def chars(value, case="lower", rng=None):
    """the 64 characters of a 256-bit value (not reduced: a string >= p is legal input)"""
    s = b"%064x" % value
    if case == "upper":
        return s.upper()
    if case == "mixed":
        return bytes(c if rng.random() < 0.5 else ord(chr(c).upper()) for c in s)
    return s


def entry(key, value_chars, length=64):
    return struct.pack("<IQ", key, length) + value_chars


def body_of(entries, count=None):
    return struct.pack("<Q", len(entries) if count is None else count) + b"".join(entries)


def row_of(body, container):
    return wire_ref.member(body) if container == GZIP_STORED else body


def good_row(witness_map, container, case="lower", seed=0):
    """the row of a map, keys ascending; case: lower | upper | mixed"""
    rng = random.Random(seed)
    return row_of(body_of([entry(w, chars(witness_map[w], case, rng)) for w in sorted(witness_map)]), container)


def slots(rows, pitch, fill=wire_ref.FILL, tail=0, rng=None):
    """the rows at a pitch; everything behind a row's length and the tail is `fill`, or random bytes"""
    buf = bytearray(rng.randbytes(len(rows) * pitch + tail)) if rng else bytearray([fill]) * (len(rows) * pitch + tail)
    for j, r in enumerate(rows):
        assert len(r) <= pitch
        buf[j * pitch:j * pitch + len(r)] = r
    return bytes(buf)


# ---- the device's judgement of one slot (the header's rules, in its order)
def _body_from(member, n_bytes):
    return b"".join(member[wire_ref.body_offset(GZIP_STORED, k):wire_ref.body_offset(GZIP_STORED, k) + min(wire_ref.BLOCK, n_bytes - k)] for k in range(0, n_bytes, wire_ref.BLOCK))


def findings(slot, container, ids, length=None):
    """[(class, entry rank)] of the slot's bytes for a handle with the initial ids `ids`; length: what d_lengths says, or None"""
    pitch, at = len(slot), wire_ref.body_offset(container, 0)
    if at + 8 > pitch:
        return [(COUNT, 0)]
    n = struct.unpack_from("<Q", slot, at)[0]
    if n > len(ids) or wire_ref.length(container, n) > pitch or (length is not None and length != wire_ref.length(container, n)):
        return [(COUNT, 0)]
    row = slot[:wire_ref.length(container, n)]
    body = _body_from(row, 8 + 76 * n) if container == GZIP_STORED else row
    out, previous = [], None
    for r in range(n):
        key, ln = struct.unpack_from("<IQ", body, 8 + 76 * r)
        s = body[8 + 76 * r + 12:8 + 76 * (r + 1)]
        cls = LENGTH if ln != 64 else HEX if any(c not in DIGITS for c in s) else KEY if key not in ids else ORDER if r and key <= previous else 0
        if cls:
            out.append((cls, r))
        previous = key
    if container == GZIP_STORED:
        want = wire_ref.member(body)
        frame = lambda m: [m[:16], m[-4:]] + [m[wire_ref.body_offset(GZIP_STORED, b * wire_ref.BLOCK) - 20:wire_ref.body_offset(GZIP_STORED, b * wire_ref.BLOCK)]
                                              for b in range(1, wire_ref.n_blocks(len(body)))]
        if frame(want) != frame(row):
            out.append((FRAMING, 0))
        elif want[-8:-4] != row[-8:-4]:
            out.append((CRC, 0))
    return sorted(out)


def decoded(witness_map):
    """what the handle holds for a good row: the values reduced"""
    return {w: v % P for w, v in witness_map.items()}


# ---- malformed rows
class Bad:
    """name, the finding (cls, rank) the device names for the row, the row's bytes, and what the host reader says of them: `rejected`, or
    `device-only` -- WitnessMap::try_from reads them, the device form's documented rule refuses them"""

    def __init__(self, name, cls, rank, row, host):
        self.name, self.cls, self.rank, self.row, self.host = name, cls, rank, row, host

    def __repr__(self):
        return self.name


def bad_rows(ids, values, container, window):
    """one bad row per planted shape; ids ascending with len(ids) > window, values[k] below p with 64 characters that start with a digit pair"""
    n = len(ids)
    assert n > window and ids == sorted(ids) and ids[-1] + 1 not in ids
    good = [entry(w, chars(v)) for w, v in zip(ids, values)]
    keyed = lambda r, key: entry(key, chars(values[r]))
    put = lambda r, e: good[:r] + [e] + good[r + 1:]
    row = lambda entries, count=None: row_of(body_of(entries, count), container)
    out = [
        Bad("N = 2^63", COUNT, 0, row(good, 1 << 63), "rejected"),
        Bad("N = n_initial + 1", COUNT, 0, row(good, n + 1), "rejected"),
        Bad("a length word 63", LENGTH, 2, row(put(2, entry(ids[2], chars(values[2]), 63))), "rejected"),
        Bad("a g", HEX, 1, row(put(1, entry(ids[1], chars(values[1])[:40] + b"g" + chars(values[1])[41:]))), "rejected"),
        Bad("a 0x prefix", HEX, 3, row(put(3, entry(ids[3], b"0x" + chars(values[3])[2:]))), "device-only"),
        Bad("a key one past an initial id", KEY, n - 1, row(put(n - 1, keyed(n - 1, ids[-1] + 1))), "device-only"),
        Bad("two equal keys", ORDER, 5, row(put(5, keyed(5, ids[4]))), "device-only"),
        Bad("descending keys across a window boundary", ORDER, window,
            row(good[:window - 1] + [keyed(window - 1, ids[window]), keyed(window, ids[window - 1])] + good[window + 1:]), "device-only"),
    ]
    if container == GZIP_STORED:
        member = bytearray(row(good))
        flip = next(k for k in range(16 + 8 + 12, len(member) - 8) if member[k] in b"0123456789")  # (a digit stays a digit: only the CRC can tell)
        member[flip] ^= 1
        out.append(Bad("a flipped body bit under an unchanged CRC", CRC, 0, bytes(member), "rejected"))
        member = bytearray(row(good))
        member[-4] ^= 4
        out.append(Bad("a wrong ISIZE", FRAMING, 0, bytes(member), "rejected"))
        member = bytearray(row(good))
        member[14] ^= 1
        out.append(Bad("a wrong ~LEN", FRAMING, 0, bytes(member), "rejected"))
    return out


def gz(row):
    """a row as decompress_witness takes it: the bincode body inside a gzip stream"""
    return row if row[:2] == b"\x1f\x8b" else wire_ref.member(row)
