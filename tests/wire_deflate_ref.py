"""The deflating container of the batch-wide WitnessMap wire format (include/acvm_amd.h ACVM_WIRE_GZIP_DEFLATE) restated in Python on top of
tests/wire_ref.py's bodies: one gzip member per map, one dynamic-Huffman block with a code that is a constant of the format, and a token
stream that is a function of the body alone. Pinned by tests/test_wire_deflate_ref.py against zlib's inflater.

The block header's run-length and tie rules (a constant of the format, the same bits in every row):
  - the 278 literal/length lengths and the 13 distance lengths are one sequence of 291 lengths, cut into runs of equal lengths;
  - a run of n zeros: while n >= 11 one symbol 18 over min(n, 138) of them, then while n >= 3 one symbol 17 over min(n, 10), the rest as 0s;
  - a run of n lengths v > 0: v itself, then while 3 or more remain one symbol 16 over min(remaining, 6), the rest as v -- the longest
    repeat first, so 7 remaining are 6 + v, never 4 + 3;
  - the code-length code is not derived from counts but stated: symbol 16 has 1 bit, 9 has 2, 7 has 3, and 1, 5, 10 and 18 have 5 each (Kraft
    sum 1); HCLEN is 14, the 18 entries up to symbol 1 in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1.
The parse's tie rule: where the distance-76 run and the distance-1 run are equally long, distance 76."""
import struct
import zlib

import wire_ref
from wire_ref import ENTRY, FILL, HEADER, body, restrict  # noqa: F401

GZIP_DEFLATE = 8
HEX = b"0123456789abcdef"
N_LITLEN, N_DIST, EOB = 278, 13, 256
MIN_MATCH = 3
LENGTH_BASES = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67]  # symbols 257 .. 277
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CLEN_LENGTHS = {16: 1, 9: 2, 7: 3, 1: 5, 5: 5, 10: 5, 18: 5}
HCLEN = 14


def litlen_lengths():
    out = [0] * N_LITLEN
    others = 0
    for s in range(EOB + 1):
        if s < 256 and s in HEX:
            out[s] = 5
        else:
            out[s] = 9 if others < 103 else 10
            others += 1
    for s in range(257, N_LITLEN):
        out[s] = 7
    assert sum(1 << (15 - n) for n in out if n) == 1 << 15  # complete: zlib rejects an incomplete literal/length code
    return out


def dist_lengths():
    out = [0] * N_DIST
    out[0] = out[12] = 1
    return out


def canonical(lengths):
    """RFC 1951 3.2.2: {symbol: (code, length)}, the code's most significant bit first in the stream"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def reverse(code, n):
    return int(format(code, "0%db" % n)[::-1], 2) if n else 0


class Bits:
    """an LSB-first bit stream"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        assert 0 <= value < 1 << n
        self.acc |= value << self.n
        self.n += n

    def code(self, code_and_length):
        c, n = code_and_length
        self.put(reverse(c, n), n)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def length_symbol(n, extra_shift_at=None):
    """(symbol, extra bit count, extra bits) of match length n"""
    k = max(i for i, b in enumerate(LENGTH_BASES) if b <= n)
    eb = LENGTH_EXTRA[k]
    if extra_shift_at is not None and LENGTH_BASES[k] == extra_shift_at:
        eb += 1
    return 257 + k, eb, n - LENGTH_BASES[k]


class Model:
    """The format; the keyword arguments make the wrong variants tests/test_wire_deflate_ref.py must catch."""

    def __init__(self, tie_to_distance_1=False, min_match=MIN_MATCH, distance_76_at_rank_0=False, wrong_extra_at=None, header_short=False, isize_off=0):
        self.tie_to_distance_1, self.min_match, self.distance_76_at_rank_0 = tie_to_distance_1, min_match, distance_76_at_rank_0
        self.wrong_extra_at, self.header_short, self.isize_off = wrong_extra_at, header_short, isize_off
        self.litlen = canonical(litlen_lengths())
        self.dist = canonical(dist_lengths())

    # ---- the constant block header
    def header_symbols(self):
        """the code-length symbols of the 291 lengths: [(symbol, extra bit count, extra bits)]"""
        seq = litlen_lengths() + dist_lengths()
        out, i = [], 0
        while i < len(seq):
            v, n = seq[i], 1
            while i + n < len(seq) and seq[i + n] == v:
                n += 1
            i += n
            if v == 0:
                while n >= 11:
                    m = min(n, 138)
                    out.append((18, 7, m - 11))
                    n -= m
                while n >= 3:
                    m = min(n, 10)
                    out.append((17, 3, m - 3))
                    n -= m
                out += [(0, 0, 0)] * n
            else:
                out.append((v, 0, 0))
                n -= 1
                while n >= 3:
                    m = min(n, 6)
                    out.append((16, 2, m - 3))
                    n -= m
                out += [(v, 0, 0)] * n
        return out

    def header(self):
        """(the bits as an integer, LSB first; the bit count)"""
        lengths = [CLEN_LENGTHS.get(s, 0) for s in range(19)]
        assert sum(1 << (7 - n) for n in lengths if n) == 1 << 7 and max(i for i, s in enumerate(CLEN_ORDER) if lengths[s]) == HCLEN + 3
        clen = canonical(lengths)
        b = Bits()
        b.put(1, 1)  # BFINAL
        b.put(2, 2)  # BTYPE = 10
        b.put(N_LITLEN - 257, 5)
        b.put(N_DIST - 1, 5)
        b.put(HCLEN, 4)
        for s in CLEN_ORDER[:HCLEN + 4]:
            b.put(lengths[s], 3)
        for s, eb, extra in self.header_symbols():
            b.code(clen[s])
            b.put(extra, eb)
        n = b.n - 1 if self.header_short else b.n
        return b.acc & ((1 << n) - 1), n

    # ---- the token stream
    def parse(self, cur, prev):
        """one entry given its predecessor (None at rank 0): [("lit", byte) | ("match", length, distance)]"""
        tokens, p = [], 0
        while p < ENTRY:
            l76 = l1 = 0
            if prev is not None or self.distance_76_at_rank_0:
                ref = prev if prev is not None else bytes(ENTRY)
                while p + l76 < ENTRY and cur[p + l76] == ref[p + l76]:
                    l76 += 1
            if p:
                while p + l1 < ENTRY and cur[p + l1] == cur[p + l1 - 1]:
                    l1 += 1
            if max(l76, l1) >= self.min_match:
                far = l76 > l1 if self.tie_to_distance_1 else l76 >= l1
                tokens.append(("match", l76, 76) if far else ("match", l1, 1))
                p += max(l76, l1)
            else:
                tokens.append(("lit", cur[p]))
                p += 1
        return tokens

    def token_bits(self, b, token):
        if token[0] == "lit":
            b.code(self.litlen[token[1]])
            return
        _, n, distance = token
        if n == 2:  # (a wrong variant's: below the smallest length code)
            s, eb, extra = 257, 0, 0
        else:
            s, eb, extra = length_symbol(n, self.wrong_extra_at)
        b.code(self.litlen[s])
        b.put(extra & ((1 << eb) - 1), eb)
        if distance == 1:
            b.code(self.dist[0])
        else:
            b.code(self.dist[12])
            b.put(distance - 65, 5)

    def entry_cost(self, cur, prev):
        b = Bits()
        for t in self.parse(cur, prev):
            self.token_bits(b, t)
        return b.n

    def tokens(self, body_bytes):
        """the tokens of a body: its 8 count bytes as literals, then entry by entry"""
        out = [("lit", c) for c in body_bytes[:8]]
        prev = None
        for at in range(8, len(body_bytes), ENTRY):
            cur = body_bytes[at:at + ENTRY]
            out += self.parse(cur, prev)
            prev = cur
        return out

    def block(self, body_bytes):
        """(the block's bytes, zero-padded; its bit count)"""
        b = Bits()
        b.put(*self.header())
        for t in self.tokens(body_bytes):
            self.token_bits(b, t)
        b.code(self.litlen[EOB])
        return b.bytes(), b.n

    def member(self, body_bytes):
        block, _ = self.block(body_bytes)
        return HEADER + block + struct.pack("<II", zlib.crc32(body_bytes), (len(body_bytes) + self.isize_off) & 0xFFFFFFFF)


MODEL = Model()
HEADER_BITS = MODEL.header()[1]


def member(body_bytes):
    return MODEL.member(body_bytes)


def encode(witness_map, container=GZIP_DEFLATE):
    return member(body(witness_map)) if container == GZIP_DEFLATE else wire_ref.encode(witness_map, container)


def bound_bits(n_positions):
    """the block's bits at the most: the header, 8 count literals, per entry 12 + 64 literals at their dearest, end-of-block"""
    return HEADER_BITS + 8 * 10 + n_positions * (12 * 10 + 64 * 5) + 10


def bound(container, n_positions):
    if container != GZIP_DEFLATE:
        return wire_ref.bound(container, n_positions)
    return (len(HEADER) + (bound_bits(n_positions) + 7) // 8 + 8 + 15) // 16 * 16


def slots(maps, container, pitch, tail=0):
    """(the buffer of len(maps) * pitch + tail bytes -- 0xA5 wherever no map's byte lies -- and the lengths)"""
    if container != GZIP_DEFLATE:
        return wire_ref.slots(maps, container, pitch, tail)
    buf = bytearray([FILL]) * (len(maps) * pitch + tail)
    lengths, memo = [], {}
    for i, m in enumerate(maps):
        key = tuple(sorted(m.items()))
        e = memo.get(key)
        if e is None:
            e = memo[key] = encode(m)
        assert len(e) <= pitch
        buf[i * pitch:i * pitch + len(e)] = e
        lengths.append(len(e))
    return bytes(buf), lengths


def inflate(member_bytes):
    """the body, through zlib's gzip reader: it checks the CRC-32 and ISIZE and must end exactly at the member's end"""
    d = zlib.decompressobj(31)
    out = d.decompress(member_bytes)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    return out
