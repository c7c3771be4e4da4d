"""One gzip member (RFC 1952 around RFC 1951) inflated in Python integers, with zlib's acceptance rules (inflate.c, inftrees.c at windowBits 31):
the model of acvm_amd/csrc/wire_inflate.hpp. inflate(row) returns the bytes stored before the reader stopped, the finding's class (0: none)
and the block headers read so far, the CRC-32 of the bytes stored, the names of the branches the row passed through and -- for a finding --
its cause. VARIANTS names six readers that are wrong in one way each; tests/test_wire_inflate_cases.py shows that the case lists catch them."""
import zlib
from collections import namedtuple

HEAD, BLOCK, STORED, CODES, SYMBOL, DISTANCE, INPUT, OUTPUT, CRC, ISIZE = range(1, 11)
CLASS_NAMES = {HEAD: "HEAD", BLOCK: "BLOCK", STORED: "STORED", CODES: "CODES", SYMBOL: "SYMBOL", DISTANCE: "DISTANCE", INPUT: "INPUT", OUTPUT: "OUTPUT",
               CRC: "CRC", ISIZE: "ISIZE"}
VARIANTS = ("repeat_may_not_cross", "distance_limit_off_by_one", "one_bit_incomplete_refused", "isize_before_crc", "fhcrc_skipped", "stored_len_big_endian")
CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENGTHS = [5] * 32

Result = namedtuple("Result", "out cls block crc labels cause")


class _Finding(Exception):
    def __init__(self, cls, cause):
        Exception.__init__(self, cause)
        self.cls, self.cause = cls, cause


def canonical(lengths):
    """(left, max_len, counts[16], symbols in canonical order): left < 0 is an over-subscribed set, > 0 an incomplete one"""
    counts = [0] * 16
    for l in lengths:
        counts[l] += 1
    left, max_len = 1, 0
    for l in range(1, 16):
        left = left * 2 - counts[l]
        if left < 0:
            return -1, 0, counts, []
        if counts[l]:
            max_len = l
    symbols = [s for l in range(1, 16) for s, sl in enumerate(lengths) if sl == l]
    return left, max_len, counts, symbols


class _Reader:
    def __init__(self, row, out_cap, variant):
        self.row, self.out_cap, self.variant = bytes(row), out_cap, variant
        self.pos = self.hold = self.bits = self.block = 0
        self.out = bytearray()
        self.labels = set()
        self.where = "head"

    def byte(self):
        if self.pos >= len(self.row):
            raise _Finding(INPUT, "input." + self.where)
        self.pos += 1
        return self.row[self.pos - 1]

    def take(self, n):
        while self.bits < n:
            self.hold |= self.byte() << self.bits
            self.bits += 8
        v = self.hold & ((1 << n) - 1)
        self.hold >>= n
        self.bits -= n
        return v

    def put(self, b):
        if self.out_cap is not None and len(self.out) >= self.out_cap:
            raise _Finding(OUTPUT, "output")
        self.out.append(b)

    def head(self):
        start = self.pos
        if self.byte() != 0x1F or self.byte() != 0x8B:
            raise _Finding(HEAD, "head.magic")
        if self.byte() != 8:
            raise _Finding(HEAD, "head.method")
        flg = self.byte()
        if flg & 0xE0:
            raise _Finding(HEAD, "head.reserved")
        for _ in range(6):
            self.byte()
        if flg & 4:
            self.labels.add("head.fextra")
            n = self.byte()
            n |= self.byte() << 8
            for _ in range(n):
                self.byte()
        for bit, name in ((8, "head.fname"), (16, "head.fcomment")):
            if flg & bit:
                self.labels.add(name)
                while self.byte():
                    pass
        if flg & 2:
            self.labels.add("head.fhcrc")
            want = zlib.crc32(self.row[start:self.pos]) & 0xFFFF
            got = self.byte()
            got |= self.byte() << 8
            if got != want and self.variant != "fhcrc_skipped":
                raise _Finding(HEAD, "head.fhcrc")

    def decode(self, code, what):
        counts, symbols = code
        value = first = index = 0
        for l in range(1, 16):
            value |= self.take(1)
            if value < first + counts[l]:
                if l == 15:
                    self.labels.add("code.15bit")
                return symbols[index + value - first]
            index += counts[l]
            first = (first + counts[l]) << 1
            value <<= 1
        raise _Finding(SYMBOL, "symbol.nocode_" + what)

    def describe(self):
        hlit, hdist, hclen = self.take(5), self.take(5), self.take(4)
        if hlit > 29:
            raise _Finding(CODES, "codes.hlit")
        if hdist > 29:
            raise _Finding(CODES, "codes.hdist")
        if hlit == 29:
            self.labels.add("codes.hlit29")
        if hdist == 29:
            self.labels.add("codes.hdist29")
        n_lit, n_dist = hlit + 257, hdist + 1
        clc = [0] * 19
        for k in range(hclen + 4):
            clc[CLC_ORDER[k]] = self.take(3)
        left, _, counts, symbols = canonical(clc)
        if left < 0:
            raise _Finding(CODES, "codes.clc_over")
        if left > 0:
            raise _Finding(CODES, "codes.clc_incomplete")
        lengths = []
        while len(lengths) < n_lit + n_dist:
            s = self.decode((counts, symbols), "clc")
            if s < 16:
                lengths.append(s)
                continue
            prev = 0
            if s == 16:
                if not lengths:
                    raise _Finding(CODES, "codes.repeat_first")
                prev = lengths[-1]
                repeat = 3 + self.take(2)
            elif s == 17:
                repeat = 3 + self.take(3)
            else:
                repeat = 11 + self.take(7)
            self.labels.add("repeat.%d" % s)
            if len(lengths) + repeat > n_lit + n_dist:
                raise _Finding(CODES, "codes.repeat_past")
            if len(lengths) < n_lit < len(lengths) + repeat:
                if self.variant == "repeat_may_not_cross":
                    raise _Finding(CODES, "codes.repeat_past")
                self.labels.add("repeat.cross")
            lengths += [prev] * repeat
        if lengths[256] == 0:
            raise _Finding(CODES, "codes.no_eob")
        refuse_one_bit = self.variant == "one_bit_incomplete_refused"
        left, max_len, lcounts, lsymbols = canonical(lengths[:n_lit])
        if left < 0:
            raise _Finding(CODES, "codes.lit_over")
        if left > 0 and (max_len != 1 or refuse_one_bit):
            raise _Finding(CODES, "codes.lit_incomplete")
        if left > 0:
            self.labels.add("lit.onecode")
        left, max_len, dcounts, dsymbols = canonical(lengths[n_lit:])
        if left < 0:
            raise _Finding(CODES, "codes.dist_over")
        if left > 0 and (max_len > 1 or (max_len == 1 and refuse_one_bit)):
            raise _Finding(CODES, "codes.dist_incomplete")
        if max_len == 0:
            self.labels.add("dist.none")
        elif left > 0:
            self.labels.add("dist.onecode")
        return (lcounts, lsymbols), (dcounts, dsymbols)

    def codes(self, lit, dist):
        while True:
            s = self.decode(lit, "lit")
            if s < 256:
                self.put(s)
                continue
            if s == 256:
                return
            if s >= 286:
                raise _Finding(SYMBOL, "symbol.lit286")
            length = LENGTH_BASE[s - 257] + self.take(LENGTH_EXTRA[s - 257])
            d = self.decode(dist, "dist")
            if d >= 30:
                raise _Finding(SYMBOL, "symbol.dist30")
            distance = DIST_BASE[d] + self.take(DIST_EXTRA[d])
            limit = len(self.out) - 1 if self.variant == "distance_limit_off_by_one" else len(self.out)
            if distance > limit:
                raise _Finding(DISTANCE, "distance")
            if distance == len(self.out):
                self.labels.add("dist.all_written")
            if distance > 16384:
                self.labels.add("copy.far")
            if distance == 32768:
                self.labels.add("dist.32768")
            if length == 258:
                self.labels.add("len.258")
            if distance < length:
                self.labels.add("copy.overlap")
            for _ in range(length):
                self.put(self.out[-distance])

    def stored(self):
        self.hold = self.bits = 0
        b = [self.byte() for _ in range(4)]
        n, nlen = b[0] | b[1] << 8, b[2] | b[3] << 8
        if self.variant == "stored_len_big_endian":
            n, nlen = b[0] << 8 | b[1], b[2] << 8 | b[3]
        if n != (~nlen & 0xFFFF):
            raise _Finding(STORED, "stored.nlen")
        self.labels.add("stored.empty" if n == 0 else "stored.full" if n == 65535 else "stored.some")
        for _ in range(n):
            v = self.byte()
            self.put(v)

    def blocks(self):
        while True:
            self.where = "block"
            header = self.take(3)
            self.block += 1
            kind = header >> 1
            if kind == 0:
                self.labels.add("block.stored")
                self.stored()
            elif kind == 1:
                self.labels.add("block.fixed")
                fixed_lit, fixed_dist = canonical(FIXED_LIT_LENGTHS), canonical(FIXED_DIST_LENGTHS)
                self.codes(fixed_lit[2:], fixed_dist[2:])
            elif kind == 2:
                self.labels.add("block.dynamic")
                lit, dist = self.describe()
                self.codes(lit, dist)
            else:
                raise _Finding(BLOCK, "block.type3")
            if header & 1:
                break
        if self.block > 1:
            self.labels.add("blocks.many")

    def trailer(self):
        self.where = "trailer"
        self.hold = self.bits = 0
        words = []
        checks = [(CRC, "crc", lambda: zlib.crc32(bytes(self.out))), (ISIZE, "isize", lambda: len(self.out) & 0xFFFFFFFF)]
        if self.variant == "isize_before_crc":
            pending = []
            for _ in range(2):
                pending.append(sum(self.byte() << (8 * k) for k in range(4)))
            for k in (1, 0):
                if pending[k] != checks[k][2]():
                    raise _Finding(checks[k][0], checks[k][1])
            return
        for cls, cause, want in checks:
            words.append(sum(self.byte() << (8 * k) for k in range(4)))
            if words[-1] != want():
                raise _Finding(cls, cause)
        if self.pos < len(self.row):
            self.labels.add("trailing")


def inflate(row, out_cap=None, variant=None):
    r = _Reader(row, out_cap, variant)
    cls, cause = 0, None
    try:
        r.head()
        r.blocks()
        r.trailer()
    except _Finding as f:
        cls, cause = f.cls, f.cause
    return Result(bytes(r.out), cls, r.block, zlib.crc32(bytes(r.out)), frozenset(r.labels), cause)


def zlib_accepts(row):
    """(accepted, bytes) of zlib's own gzip reader: a member that ends inside the row, whatever lies behind it"""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(bytes(row))
    except zlib.error:
        return False, b""
    return (True, out) if d.eof else (False, b"")
