"""Rows for the gzip import (include/acvm_amd.h acvm_batch_import_device_wire_gzip): (A) what writers produce -- zlib at every level and strategy,
flushes, every optional head field, the project's own members, the reference's pinned member; (B) what no writer produces, from a small token
writer; (C) rows of every finding class and cause; (D) members that inflate cleanly around bodies that are not canonical. A Case carries its
bytes and -- where the case is about the bound -- the out_cap it is meant for. Judged by tests/wire_inflate_ref.py; pinned on the CPU by
tests/test_wire_inflate_cases.py against zlib."""
import functools
import json
import os
import random
import struct
import zlib
from collections import namedtuple

import wire_deflate_ref
import wire_in_cases as wc
import wire_inflate_ref as ref
import wire_ref

P = wc.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 66000  # the out_cap of the rows that are not about the bound: above the longest output here (a stored block of 65 535), a multiple of 4
Case = namedtuple("Case", "name row cap")
HEAD = bytes.fromhex("1f8b08000000000000ff")


def case(name, row, cap=None):
    return Case(name, bytes(row), cap)


# ---- bits, codes, blocks
class Bits:
    def __init__(self):
        self.acc = self.n = 0

    def put(self, value, bits):
        """LSB first"""
        self.acc |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits

    def code(self, value, bits):
        """a Huffman code: most significant bit first"""
        for k in range(bits - 1, -1, -1):
            self.put(value >> k & 1, 1)

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def raw(self, data):
        self.align()
        for b in data:
            self.put(b, 8)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def codes_of(lengths):
    """{symbol: (code, bits)} of the canonical code (RFC 1951 3.2.2) -- also for sets no decoder takes: the writer does not judge"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def _length_symbol(length):
    s = max(k for k in range(29) if ref.LENGTH_BASE[k] <= length) if length < 258 else 28
    return 257 + s, length - ref.LENGTH_BASE[s], ref.LENGTH_EXTRA[s]


def _dist_symbol(distance):
    s = max(k for k in range(30) if ref.DIST_BASE[k] <= distance)
    return s, distance - ref.DIST_BASE[s], ref.DIST_EXTRA[s]


def put_tokens(w, tokens, lit, dist):
    """tokens: a literal byte, ("m", length, distance), ("lit", symbol) or ("dist", symbol) raw, ("bits", value, n); end-of-block is the caller's"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "m":
            s, extra, n = _length_symbol(t[1])
            w.code(*lit[s])
            w.put(extra, n)
            s, extra, n = _dist_symbol(t[2])
            w.code(*dist[s])
            w.put(extra, n)
        elif t[0] == "bits":
            w.put(t[1], t[2])
        else:
            w.code(*(lit if t[0] == "lit" else dist)[t[1]])


FIXED_LIT, FIXED_DIST = codes_of(ref.FIXED_LIT_LENGTHS), codes_of(ref.FIXED_DIST_LENGTHS)
CLC = [5] * 16 + [2, 3, 3]  # a complete code-length code: 16 x 1/32 + 1/4 + 2 x 1/8


def stored(w, data, final, nlen=None):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
    w.raw(data)


def fixed(w, tokens, final, eob=True):
    w.put(final, 1)
    w.put(1, 2)
    put_tokens(w, tokens + ([("lit", 256)] if eob else []), FIXED_LIT, FIXED_DIST)


def plain_ops(lengths):
    return [(l, 0) for l in lengths]


def dynamic(w, tokens, lit_lengths, dist_lengths, final, ops=None, clc=None, hlit=None, hdist=None, hclen=15, eob=True):
    """ops: the code-length symbols [(symbol, extra)] that describe lit_lengths + dist_lengths (default: one per length)"""
    clc = CLC if clc is None else clc
    w.put(final, 1)
    w.put(2, 2)
    w.put(len(lit_lengths) - 257 if hlit is None else hlit, 5)
    w.put(len(dist_lengths) - 1 if hdist is None else hdist, 5)
    w.put(hclen, 4)
    for k in range(hclen + 4):
        w.put(clc[ref.CLC_ORDER[k]], 3)
    cc = codes_of(clc)
    for s, extra in (plain_ops(lit_lengths + dist_lengths) if ops is None else ops):
        if s in cc:  # (a code-length code that lacks the symbol is one no reader gets past)
            w.code(*cc[s])
            w.put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))
    lit, dist = codes_of(lit_lengths), codes_of(dist_lengths)
    put_tokens(w, tokens + ([("lit", 256)] if eob else []), lit, dist)


def member(deflate, body, head=HEAD, crc=None, isize=None, tail=b""):
    return head + deflate + struct.pack("<II", zlib.crc32(body) if crc is None else crc, len(body) & 0xFFFFFFFF if isize is None else isize) + tail


def head_of(fextra=None, fname=None, fcomment=None, fhcrc=False, ftext=False, hcrc_xor=0, reserved=0):
    flg = (1 if ftext else 0) | (2 if fhcrc else 0) | (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | reserved
    h = bytes([0x1F, 0x8B, 8, flg]) + struct.pack("<IBB", 0x5F5E100, 2, 3)
    if fextra is not None:
        h += struct.pack("<H", len(fextra)) + fextra
    for field in (fname, fcomment):
        if field is not None:
            h += field + b"\x00"
    if fhcrc:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) ^ hcrc_xor)
    return h


def built(build, body=None, **kw):
    """the member around what `build` writes; body None: whatever the blocks inflate to (the model says: list B is judged by zlib as well)"""
    w = Bits()
    build(w)
    if body is None:
        body = ref.inflate(member(w.bytes(), b"")).out
    return member(w.bytes(), body, **kw)


# ---- bodies
def _map(n, kind, seed=0):
    rng = random.Random(0x1F8B0000 + 131 * n + seed)
    values = []
    for k in range(n):
        if kind == "zero":
            values.append(0)
        elif kind == "pm1":
            values.append(P - 1)
        elif kind == "repeat250" and k >= 250:
            values.append(values[k - 250])  # 250 entries are 19 000 bytes: a match more than 16 384 back
        else:
            values.append(rng.randrange(P))
    return {k + 1: v for k, v in enumerate(values)}


@functools.lru_cache(maxsize=None)
def body(n, kind):
    if kind == "upper":
        return wc.good_row(_map(n, "random"), wire_ref.BINCODE, "upper")
    return wire_ref.body(_map(n, kind))


def deflated(data, level=9, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None, wbits=31):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    if flush is None:
        return c.compress(data) + c.flush()
    half = len(data) // 2
    return c.compress(data[:half]) + c.flush(flush) + c.compress(data[half:]) + c.flush()


def pinned():
    """(the reference's own compressed WitnessMap, the map it holds)"""
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")))["acvm_js"]["witness_compression"]
    return bytes(v["expectedCompressedWitnessMap"]), {int(k): int(x, 16) for k, x in v["expectedWitnessMap"].items()}


WRITERS = [("level0", dict(level=0)), ("level1", dict(level=1)), ("level6", dict(level=6)), ("level9", dict(level=9)), ("mem1", dict(level=9, mem=1)),
           ("fixed", dict(strategy=zlib.Z_FIXED)), ("huffman", dict(strategy=zlib.Z_HUFFMAN_ONLY)), ("rle", dict(strategy=zlib.Z_RLE)),
           ("filtered", dict(strategy=zlib.Z_FILTERED)), ("sync", dict(flush=zlib.Z_SYNC_FLUSH)), ("full", dict(flush=zlib.Z_FULL_FLUSH))]
KINDS = ("zero", "pm1", "random", "upper")


@functools.lru_cache(maxsize=None)
def list_a():
    out = []
    for n in (0, 1, 2, 5, 40):
        for kind in KINDS:
            b = body(n, kind)
            for name, kw in WRITERS:
                out.append(case(f"A {n} {kind} {name}", deflated(b, **kw)))
            out.append(case(f"A {n} {kind} own stored", wire_ref.member(b)))
            if kind != "upper":
                out.append(case(f"A {n} {kind} own deflate", wire_deflate_ref.member(b)))
    for kind in ("zero", "repeat250", "upper"):  # 33 448 bytes each
        b = body(440, kind)
        for name, kw in (WRITERS[0], WRITERS[1], WRITERS[3], WRITERS[4], WRITERS[6]):
            out.append(case(f"A 440 {kind} {name}", deflated(b, **kw)))
        out.append(case(f"A 440 {kind} own stored", wire_ref.member(b)))
        if kind != "upper":
            out.append(case(f"A 440 {kind} own deflate", wire_deflate_ref.member(b)))
    b = body(5, "random")
    raw = deflated(b, wbits=-15)
    heads = [("fextra", dict(fextra=b"\x41\x50\x04\x00abcd")), ("empty fextra", dict(fextra=b"")), ("fname", dict(fname=b"witness.gz")), ("fcomment", dict(fcomment=b"a comment")),
             ("fhcrc", dict(fhcrc=True)), ("ftext", dict(ftext=True)),
             ("all four", dict(fextra=b"\x00" * 7, fname=b"n", fcomment=b"", fhcrc=True))]
    for name, kw in heads:
        out.append(case("A head " + name, member(raw, b, head=head_of(**kw))))
    out.append(case("A bytes behind the trailer", deflated(b) + b"\x1f\x8b\x08 and more"))
    out.append(case("A one byte behind the trailer", deflated(body(2, "zero")) + b"\x00"))
    out.append(case("A the reference's member", pinned()[0]))
    return out


# ---- (B) what no writer produces
def _lit_set(symbols_lengths, n=257):
    lengths = [0] * n
    for s, l in symbols_lengths.items():
        lengths[s] = l
    return lengths


FIFTEEN = _lit_set(dict([(256, 1)] + [(65 + k, 2 + k) for k in range(14)] + [(79, 15)]))  # 1/2 + ... + 1/2^15 + 1/2^15: complete
AB = _lit_set({97: 2, 98: 2, 256: 2, 257: 3, 285: 3}, 286)  # a, b, end-of-block, lengths 3 and 258; complete; HLIT = 29


@functools.lru_cache(maxsize=None)
def list_b():
    out = []
    far = bytes(random.Random(0x1F8B0B01).randrange(256) for _ in range(32768))

    def far_match(w):
        stored(w, far, 0)
        fixed(w, [("m", 3, 32768)], 1)
    out.append(case("B distance 32 768 = the bytes written", built(far_match, far + far[:3])))
    def far_match_long(w):
        stored(w, far, 0)
        stored(w, far[:7232], 0)
        fixed(w, [("m", 258, 32768), 33, ("m", 3, 32768)], 1)
    out.append(case("B distance 32 768 twice behind 40 000 bytes", built(far_match_long)))
    out.append(case("B distance 1 = the bytes written", built(lambda w: fixed(w, [97, ("m", 3, 1)], 1), b"aaaa")))
    out.append(case("B length 258 at distance 1", built(lambda w: fixed(w, [98, ("m", 258, 1)], 1), b"b" * 259)))
    out.append(case("B length 258 at distance 2, dynamic", built(lambda w: dynamic(w, [97, 98, ("m", 258, 2)], AB, [0, 1], 1), b"ab" * 130)))
    out.append(case("B a 15-bit code", built(lambda w: dynamic(w, [65, 78, 79, 79, 78], FIFTEEN, [0], 1), b"ANOON")))
    out.append(case("B a one-code distance set", built(lambda w: dynamic(w, [97, ("m", 3, 1)], AB, [1], 1), b"aaaa")))
    out.append(case("B a one-code distance set, the code not the first", built(lambda w: dynamic(w, [97, 98, 97, ("m", 3, 3)], AB, [0, 0, 1], 1), b"abaaba")))
    out.append(case("B an all-zero distance set, literals only", built(lambda w: dynamic(w, [97, 98, 98], AB, [0], 1), b"abb")))
    out.append(case("B a one-code literal/length set", built(lambda w: dynamic(w, [], _lit_set({256: 1}), [0], 1), b"")))
    # a run of zeros from the literal/length lengths (257 .. 259) into the distance lengths (0, 1): 17 with 5
    cross = _lit_set({97: 1, 256: 2, 257: 2}, 260)
    ops = [(18, 97 - 11), (1, 0), (18, 127), (18, 158 - 138 - 11), (2, 0), (2, 0), (17, 4 - 3), (1, 0)]
    out.append(case("B a zero run across the two sets", built(lambda w: dynamic(w, [97, 97, 97, ("m", 3, 3)], cross, [0, 0, 1], 1, ops=ops), b"aaaaaa")))
    # ... and a run of a length (16) across: 256 has 2 bits, and so have 257 and the four codes of a complete distance set
    cross16 = _lit_set({97: 1, 256: 2, 257: 2}, 258)
    ops = [(18, 97 - 11), (1, 0), (18, 127), (18, 158 - 138 - 11), (2, 0), (16, 5 - 3)]
    out.append(case("B a length run across the two sets", built(lambda w: dynamic(w, [97, ("m", 3, 1)], cross16, [2, 2, 2, 2], 1, ops=ops), b"aaaa")))
    full = _lit_set({97: 2, 98: 2, 256: 2, 257: 2}, 286)
    out.append(case("B HLIT = 29 and HDIST = 29", built(lambda w: dynamic(w, [97, 98, ("m", 3, 2)], full, [1, 1] + [0] * 28, 1), b"ababa")))
    out.append(case("B an empty final stored block", built(lambda w: (fixed(w, [120], 0), stored(w, b"", 1)), b"x")))
    big = bytes(random.Random(0x1F8B0B02).randrange(256) for _ in range(65535))
    out.append(case("B a stored block of 65 535 bytes", built(lambda w: stored(w, big, 1), big)))
    out.append(case("B a stored block of 65 535 bytes and a block behind it", built(lambda w: (stored(w, big[::-1], 0), fixed(w, [("m", 4, 65535 - 40000)], 1)))))
    out.append(case("B stored, fixed, dynamic, stored", built(lambda w: (stored(w, b"st", 0), fixed(w, [("m", 3, 2)], 0), dynamic(w, [97, ("m", 3, 5)], AB, [0, 0, 0, 0, 1], 0),
                                                                           stored(w, b"!", 1)))))
    return out


# ---- (C) every finding class and cause, at least twice
@functools.lru_cache(maxsize=None)
def list_c():
    out = []
    small_body = body(2, "random")
    small = deflated(small_body)
    raw = deflated(small_body, wbits=-15)
    # 1 HEAD
    for name, at, value in (("ID1", 0, 0x1E), ("ID2", 1, 0x8C), ("CM 9", 2, 9), ("CM 0", 2, 0), ("FLG bit 5", 3, 0x20), ("FLG bit 7", 3, 0x80), ("FLG bit 6 beside FNAME", 3, 0x48)):
        row = bytearray(small)
        row[at] = value
        out.append(case("C head " + name, row))
    out.append(case("C head a zlib stream", zlib.compress(small_body)))
    out.append(case("C head FHCRC low byte", member(raw, small_body, head=head_of(fhcrc=True, hcrc_xor=0x0001))))
    out.append(case("C head FHCRC high byte", member(raw, small_body, head=head_of(fname=b"x", fhcrc=True, hcrc_xor=0x8000))))
    # 2 BLOCK
    out.append(case("C block type 3 first", built(lambda w: w.put(0b111, 3), b"")))
    out.append(case("C block type 3 behind a block", built(lambda w: (fixed(w, [97], 0), w.put(0b110, 3)), b"a")))
    # 3 STORED
    out.append(case("C stored NLEN = LEN", built(lambda w: stored(w, b"abc", 1, nlen=3), b"abc")))
    out.append(case("C stored NLEN one bit off", built(lambda w: (stored(w, b"", 0), stored(w, b"abc", 1, nlen=0xFFFC ^ 0x100)), b"abc")))
    # 4 CODES
    out.append(case("C codes HLIT 30", built(lambda w: dynamic(w, [], AB, [0], 1, hlit=30), b"")))
    out.append(case("C codes HLIT 31", built(lambda w: dynamic(w, [], AB, [0], 1, hlit=31), b"")))
    out.append(case("C codes HDIST 30", built(lambda w: dynamic(w, [], AB, [0], 1, hdist=30), b"")))
    out.append(case("C codes HDIST 31", built(lambda w: dynamic(w, [], AB, [0], 0, hdist=31), b"")))
    out.append(case("C codes code-length code over-subscribed", built(lambda w: dynamic(w, [], AB, [0], 1, clc=[5] * 16 + [2, 2, 3]), b"")))
    out.append(case("C codes code-length code three of one bit", built(lambda w: dynamic(w, [], AB, [0], 1, clc=[1, 1, 1] + [0] * 16), b"")))
    out.append(case("C codes code-length code incomplete", built(lambda w: dynamic(w, [], AB, [0], 1, clc=[5] * 16 + [2, 3, 4]), b"")))
    out.append(case("C codes code-length code of one code", built(lambda w: dynamic(w, [], AB, [0], 1, clc=[1] + [0] * 18, ops=[]), b"")))
    out.append(case("C codes code-length code all zero", built(lambda w: dynamic(w, [], AB, [0], 1, clc=[0] * 19, ops=[], hclen=0), b"")))
    out.append(case("C codes repeat 16 first", built(lambda w: dynamic(w, [], AB, [0], 1, ops=[(16, 0)]), b"")))
    out.append(case("C codes repeat 16 first, behind a block", built(lambda w: (stored(w, b"q", 0), dynamic(w, [], AB, [0], 1, ops=[(16, 3)])), b"q")))
    n = len(AB) + 1
    out.append(case("C codes repeat 18 past the end", built(lambda w: dynamic(w, [], AB, [0], 1, ops=plain_ops(AB[:n - 20]) + [(18, 21 - 11)]), b"")))
    out.append(case("C codes repeat 16 past the end", built(lambda w: dynamic(w, [], AB, [0], 1, ops=plain_ops(AB[:n - 1]) + [(16, 0)]), b"")))
    out.append(case("C codes repeat 17 past the end", built(lambda w: dynamic(w, [], AB, [0], 1, ops=plain_ops(AB + [0])[:-2] + [(17, 0)]), b"")))
    out.append(case("C codes no end-of-block", built(lambda w: dynamic(w, [], _lit_set({97: 1, 98: 1}), [0], 1, eob=False), b"")))
    out.append(case("C codes no code at all", built(lambda w: dynamic(w, [], [0] * 257, [0], 1, eob=False), b"")))
    out.append(case("C codes literal/length set over-subscribed", built(lambda w: dynamic(w, [], _lit_set({97: 1, 98: 1, 256: 1}), [0], 1, eob=False), b"")))
    out.append(case("C codes literal/length set over-subscribed deep", built(lambda w: dynamic(w, [], _lit_set({97: 1, 98: 2, 99: 3, 100: 3, 256: 3}), [0], 1, eob=False), b"")))
    out.append(case("C codes literal/length set incomplete", built(lambda w: dynamic(w, [], _lit_set({97: 2, 256: 2}), [0], 1), b"")))
    out.append(case("C codes literal/length set of one two-bit code", built(lambda w: dynamic(w, [], _lit_set({256: 2}), [0], 1), b"")))
    out.append(case("C codes distance set over-subscribed", built(lambda w: dynamic(w, [], AB, [1, 1, 1], 1), b"")))
    out.append(case("C codes distance set over-subscribed deep", built(lambda w: dynamic(w, [], AB, [1, 2, 2, 15], 1), b"")))
    out.append(case("C codes distance set incomplete", built(lambda w: dynamic(w, [], AB, [2, 2, 2], 1), b"")))
    out.append(case("C codes distance set of one two-bit code", built(lambda w: dynamic(w, [], AB, [0, 2], 1), b"")))
    # 5 SYMBOL
    out.append(case("C symbol the other bit of a one-code literal/length set", built(lambda w: dynamic(w, [("bits", 0xFFFF, 16)], _lit_set({256: 1}), [0], 1, eob=False), b"")))
    out.append(case("C symbol ... behind output", built(lambda w: (fixed(w, [97], 0), dynamic(w, [("bits", 0xFFFF, 16)], _lit_set({256: 1}), [0], 1, eob=False)), b"a")))
    out.append(case("C symbol a distance of an all-zero set", built(lambda w: dynamic(w, [97, ("lit", 257), ("bits", 0, 16)], AB, [0], 1, eob=False), b"a")))
    out.append(case("C symbol the other bit of a one-code distance set", built(lambda w: dynamic(w, [97, ("lit", 257), ("bits", 0xFFFF, 16)], AB, [1], 1, eob=False), b"a")))
    out.append(case("C symbol 286", built(lambda w: fixed(w, [97, ("lit", 286), ("bits", 0, 16)], 1, eob=False), b"a")))
    out.append(case("C symbol 287", built(lambda w: fixed(w, [("lit", 287), ("bits", 0, 16)], 1, eob=False), b"")))
    out.append(case("C symbol distance 30", built(lambda w: fixed(w, [97, ("lit", 257), ("dist", 30), ("bits", 0, 16)], 1, eob=False), b"a")))
    out.append(case("C symbol distance 31", built(lambda w: fixed(w, [97, ("lit", 285), ("dist", 31), ("bits", 0, 16)], 1, eob=False), b"a")))
    # 6 DISTANCE
    out.append(case("C distance 1 with nothing written", built(lambda w: fixed(w, [("m", 3, 1)], 1), b"")))
    out.append(case("C distance = written + 1", built(lambda w: fixed(w, [97, 98, 99, 100, 101, ("m", 3, 6)], 1), b"abcde")))
    out.append(case("C distance = written + 1 across blocks", built(lambda w: (stored(w, b"abc", 0), dynamic(w, [97, ("m", 3, 5)], AB, [0, 0, 0, 0, 1], 1)), b"abca")))
    # 7 INPUT
    out.append(case("C input a row of length 0", b""))
    for k in range(1, len(small)):
        out.append(case(f"C input truncated at {k} of {len(small)}", small[:k]))
    flushed = deflated(body(5, "zero"), flush=zlib.Z_FULL_FLUSH)
    for k in (len(flushed) - 9, len(flushed) - 1, len(flushed) // 2):
        out.append(case(f"C input a flushed member truncated at {k}", flushed[:k]))
    out.append(case("C input the head's FNAME never ends", head_of(fname=b"n" * 40)[:-1]))
    out.append(case("C input FEXTRA longer than the row", bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 255, 0xFF, 0xFF]) + b"e" * 100))
    for pitch in (4096, 10 + 5 * 7 + 3):  # the termination tripwire: empty stored blocks to the end of the slot, (pitch - 10) // 5 of them
        out.append(case(f"C input {pitch} bytes of empty stored blocks", (HEAD + wire_ref.EMPTY_BLOCK * (pitch // 5 + 1))[:pitch]))
    # 8 OUTPUT: a body of exactly the cap passes, one byte more does not -- stored, fixed (a match across the cap) and dynamic
    b40 = body(40, "random")
    assert len(b40) == 8 + 76 * 40
    out.append(case("C output exactly the cap", deflated(b40), len(b40)))
    out.append(case("C output exactly the cap, stored", wire_ref.member(b40), len(b40)))
    out.append(case("C output the cap + 1", deflated(b40 + b"0"), len(b40)))
    out.append(case("C output the cap + 1, stored", wire_ref.member(b40 + b"0"), len(b40)))
    out.append(case("C output a match across the cap", built(lambda w: fixed(w, [97, ("m", 258, 1)], 1), b"a" * 259), 256))
    out.append(case("C output cap 0", built(lambda w: fixed(w, [97], 1), b"a"), 0))
    out.append(case("C output cap 0, an empty body passes", built(lambda w: fixed(w, [], 1), b""), 0))
    # 9 CRC, 10 ISIZE
    out.append(case("C crc one bit", member(raw, small_body, crc=zlib.crc32(small_body) ^ 0x10000)))
    out.append(case("C crc of another body, ISIZE wrong too", member(raw, small_body, crc=zlib.crc32(small_body[:-1]), isize=len(small_body) - 1)))
    out.append(case("C crc and ISIZE each one off", member(raw, small_body, crc=zlib.crc32(small_body) + 1 & 0xFFFFFFFF, isize=len(small_body) + 1)))
    flipped = bytearray(wire_ref.member(small_body))
    flipped[40] ^= 1
    out.append(case("C crc a stored byte flipped", flipped))
    out.append(case("C isize one more", member(raw, small_body, isize=len(small_body) + 1)))
    out.append(case("C isize 2^32 more is the same", member(raw, small_body, isize=len(small_body))))
    out.append(case("C isize high byte", member(raw, small_body, isize=len(small_body) | 0x80000000)))
    return out


# ---- (D) members that inflate cleanly around bodies the body import refuses (classes 1 .. 5 of wire_in_cases)
def list_d(ids, values, window):
    out = []
    for k, b in enumerate(wc.bad_rows(ids, values, wire_ref.BINCODE, window)):
        out.append((b, deflated(b.row, level=(9, 1, 0)[k % 3])))
    return out


def everything():
    return list_a() + list_b() + list_c()


@functools.lru_cache(maxsize=None)
def judged(row, cap):
    """the model's answer, once per (row, cap)"""
    return ref.inflate(row, cap)


def accepted_small():
    """the accepted rows the mutation sweep starts from: short ones of every block type"""
    return [c.row for c in everything() if c.cap is None and len(c.row) <= 400 and judged(c.row, CAP).cls == 0]


def mutations(n, seed=0x1F8B5EED):
    """n single- and double-byte mutations and truncations of the accepted small rows"""
    rng = random.Random(seed)
    base = accepted_small()
    out = []
    while len(out) < n:
        row = bytearray(rng.choice(base))
        how = rng.randrange(4)
        if how == 3:
            row = row[:rng.randrange(len(row))]
        else:
            for _ in range(1 if how == 0 else 2):
                at = rng.randrange(len(row))
                row[at] = rng.randrange(256) if how == 2 else row[at] ^ (1 << rng.randrange(8))
        out.append(bytes(row))
    return out
