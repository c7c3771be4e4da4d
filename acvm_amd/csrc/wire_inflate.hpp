// wire_inflate.hpp -- one row's gzip member (RFC 1952 around RFC 1951) inflated by ONE sequential reader: what a lane of kernels_wire_inflate.hip
// runs for its row (include/acvm_amd.h acvm_batch_import_device_wire_gzip), and what the host runs on the same bytes
// (tools/wire_inflate_host_test.hip, tests/test_wire_inflate_on_host.py, `make asan`). The acceptance rules are zlib's (inflate.c, inftrees.c,
// windowBits 31); tests/wire_inflate_ref.py restates them in Python integers.
//
// The reader is templated on
//   In     in(k): input byte k of the row, asked for only with k < n_in
//   Out    out.store(k, byte) with k < out_cap, strictly ascending from 0; out.load(k, n) of a byte stored before, n the bytes stored so far;
//          out.finish(n) once at the end (a sink that gathers bytes into words answers a load from what it still holds, and flushes there)
//   Tab    the row's code tables: tab.get(i) / tab.set(i, v) on INFLATE_TAB_HALFWORDS 16-bit words, tab.len(i) / tab.set_len(i, v) on
//          INFLATE_LEN_NIBBLES 4-bit code lengths
//   Fixed  fixed[i]: the fixed code's table in the same halfword layout (wire_inflate_plan.cpp makes it)
//   Crc    crc[i]: the 256 words of the CRC-32 byte table
//
// Invariants, kept by construction:
//   - Every loop either has a constant bound (16 code lengths, 19 + 320 symbols of a code description) or each of its passes consumes at least
//     one input bit or stores at least one output byte. Input is bounded by 8 * n_in bits and output by out_cap bytes, so a row ends.
//   - Input byte k is fetched only behind the test k < n_in (byte()): no input index at or past the bound is formed.
//   - Output byte k is stored only behind the test k < out_cap (put()), and a back-reference loads written - distance behind the test
//     distance <= written: no output index at or past out_cap, or below 0, is formed.
//   - What the row says sizes no table and no index without a check: HLIT and HDIST are judged before a length is stored, a repeat is judged
//     against HLIT + HDIST + 258 before it is stored, a symbol is judged before it becomes a length or a distance. The tables have their full
//     size whatever the row says.
//
// A row has at most one finding: the reader stops at its first. With it goes the number of block headers read so far (0 inside the head).
#pragma once
#include "wire_encode.hpp"

namespace acvm {

enum : uint32_t {
    INFLATE_HEAD = 1,      // bytes 0..2 are not 1f 8b 08; a reserved FLG bit; FHCRC is not the header's CRC-32 mod 2^16
    INFLATE_BLOCK = 2,     // BTYPE 3
    INFLATE_STORED = 3,    // LEN is not ~NLEN
    INFLATE_CODES = 4,     // a dynamic block's code description that zlib refuses
    INFLATE_SYMBOL = 5,    // bits that are no code of an incomplete set; literal/length symbols 286 / 287; distance symbols 30 / 31
    INFLATE_DISTANCE = 6,  // a distance beyond the bytes written so far
    INFLATE_INPUT = 7,     // the row's readable bytes end before the head, the final block or the trailer do
    INFLATE_OUTPUT = 8,    // more output than out_cap
    INFLATE_CRC = 9,       // the trailer's CRC-32 is not the output's
    INFLATE_ISIZE = 10,    // the trailer's ISIZE is not the output's length mod 2^32
    INFLATE_CLASSES = 11
};

// the row's tables, in 16-bit words: per code the number of codes of each length [16] and the symbols in canonical order (288 and 32: the fixed
// code gives every symbol a code, the two distance symbols no block may use included); OFFS is the construction's scratch. The code-length
// code (19 symbols) is built where the distance code will be: it is done with before that one is made.
enum : uint32_t { INFLATE_LCNT = 0, INFLATE_DCNT = 16, INFLATE_OFFS = 32, INFLATE_LSYM = 48, INFLATE_DSYM = 336, INFLATE_TAB_HALFWORDS = 368, INFLATE_LEN_NIBBLES = 320 };
enum : uint32_t { INFLATE_MAX_LIT = 286, INFLATE_MAX_DIST = 30 };

struct InflateRow {
    uint64_t length;  // bytes stored
    uint32_t cls, block, crc;  // the finding (0: none) and the block headers read; the CRC-32 of the bytes stored
};

// the order the code-length code's lengths come in (RFC 1951 3.2.7), five bits each: no table a lane would index
FR_HD __forceinline__ uint32_t inflate_clc_order(uint32_t k) {
    // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((k < 12u ? lo >> (5u * k) : hi >> (5u * (k - 12u))) & 31u);
}
// length symbol 257 + i (i < 29) and distance symbol d (d < 30): the base and the extra bits (RFC 1951 3.2.5), from the arithmetic of the table
FR_HD __forceinline__ void inflate_length_code(uint32_t i, uint32_t &base, uint32_t &extra) {
    if (i < 8u) { base = 3u + i; extra = 0u; }
    else if (i == 28u) { base = 258u; extra = 0u; }
    else { extra = (i - 4u) >> 2; base = 3u + ((4u + (i & 3u)) << extra); }
}
FR_HD __forceinline__ void inflate_distance_code(uint32_t d, uint32_t &base, uint32_t &extra) {
    if (d < 4u) { base = 1u + d; extra = 0u; }
    else { extra = (d >> 1) - 1u; base = 1u + ((2u + (d & 1u)) << extra); }
}

template <class In, class Out, class Tab, class Fixed, class Crc>
struct WireInflater {
    const In &in;
    const uint64_t n_in;
    Out &out;
    const uint64_t out_cap;
    const Tab &tab;
    const Fixed &fixed;
    const Crc &crc_table;
    uint64_t pos = 0, written = 0;
    uint32_t hold = 0, bits = 0;  // bits < 8 between two calls: a byte is fetched only when a bit of it is asked for
    uint32_t crc = 0xFFFFFFFFu, cls = 0, block = 0;

    FR_HD WireInflater(const In &in_, uint64_t n_in_, Out &out_, uint64_t out_cap_, const Tab &tab_, const Fixed &fixed_, const Crc &crc_)
        : in(in_), n_in(n_in_), out(out_), out_cap(out_cap_), tab(tab_), fixed(fixed_), crc_table(crc_) {}

    FR_HD __forceinline__ bool fail(uint32_t c) { cls = c; return false; }
    FR_HD __forceinline__ uint32_t crc_step(uint32_t c, uint32_t byte) const { return crc_table[(c ^ byte) & 0xffu] ^ (c >> 8); }
    // the next whole byte (the bit buffer is empty: the head, a stored block, the trailer)
    FR_HD __forceinline__ bool byte(uint32_t &v) {
        if (pos >= n_in) return fail(INFLATE_INPUT);
        v = in(pos);
        pos++;
        return true;
    }
    // n <= 16 bits, least significant first
    FR_HD __forceinline__ bool take(uint32_t n, uint32_t &v) {
        while (bits < n) {
            uint32_t b;
            if (!byte(b)) return false;
            hold |= b << bits;
            bits += 8u;
        }
        v = hold & ((1u << n) - 1u);
        hold >>= n;
        bits -= n;
        return true;
    }
    FR_HD __forceinline__ void to_byte_boundary() { hold = 0u; bits = 0u; }
    FR_HD __forceinline__ bool put(uint32_t b) {
        if (written >= out_cap) return fail(INFLATE_OUTPUT);
        out.store(written, b);
        crc = crc_step(crc, b);
        written++;
        return true;
    }

    // ---- RFC 1952: the head
    FR_HD bool head() {
        uint32_t h = 0xFFFFFFFFu, v = 0, flg = 0;
        auto hbyte = [&](uint32_t &x) {
            if (!byte(x)) return false;
            h = crc_step(h, x);
            return true;
        };
        if (!hbyte(v)) return false;
        if (v != 0x1fu) return fail(INFLATE_HEAD);
        if (!hbyte(v)) return false;
        if (v != 0x8bu) return fail(INFLATE_HEAD);
        if (!hbyte(v)) return false;
        if (v != 8u) return fail(INFLATE_HEAD);
        if (!hbyte(flg)) return false;
        if (flg & 0xe0u) return fail(INFLATE_HEAD);
        for (uint32_t k = 0; k < 6u; k++)  // MTIME, XFL, OS
            if (!hbyte(v)) return false;
        if (flg & 4u) {  // FEXTRA
            uint32_t lo, hi;
            if (!hbyte(lo) || !hbyte(hi)) return false;
            for (uint32_t n = lo | hi << 8; n; n--)
                if (!hbyte(v)) return false;
        }
        for (uint32_t field = 8u; field <= 16u; field <<= 1)  // FNAME, FCOMMENT: zero-terminated
            if (flg & field)
                do {
                    if (!hbyte(v)) return false;
                } while (v);
        if (flg & 2u) {  // FHCRC
            uint32_t lo, hi;
            if (!byte(lo) || !byte(hi)) return false;
            if ((lo | hi << 8) != (~h & 0xffffu)) return fail(INFLATE_HEAD);
        }
        return true;
    }

    // ---- canonical codes. A code's table: counts at `cnt`, symbols at `sym`; lengths of its n symbols from nibble `at` on. Returns what is
    // left of the code space (0: complete, above: incomplete) or -1 for an over-subscribed set; max_len: its longest code.
    FR_HD int32_t construct(uint32_t cnt, uint32_t sym, uint32_t at, uint32_t n, uint32_t &max_len) {
        for (uint32_t l = 0; l < 16u; l++) tab.set(cnt + l, 0u);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t l = tab.len(at + i);
            tab.set(cnt + l, tab.get(cnt + l) + 1u);
        }
        int32_t left = 1;
        max_len = 0u;
        for (uint32_t l = 1; l < 16u; l++) {
            const uint32_t c = tab.get(cnt + l);
            left = left * 2 - (int32_t)c;
            if (left < 0) return -1;
            if (c) max_len = l;
        }
        uint32_t offset = 0u;
        for (uint32_t l = 1; l < 16u; l++) {
            tab.set(INFLATE_OFFS + l, offset);
            offset += tab.get(cnt + l);
        }
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t l = tab.len(at + i);
            if (!l) continue;
            const uint32_t o = tab.get(INFLATE_OFFS + l);  // (o < the symbols with a length <= n: inside the code's symbol array)
            tab.set(sym + o, i);
            tab.set(INFLATE_OFFS + l, o + 1u);
        }
        return left;
    }
    // one symbol, a bit at a time, first code of each length against the count of that length
    FR_HD bool decode(bool use_fixed, uint32_t cnt, uint32_t sym, uint32_t &symbol) {
        uint32_t code = 0u, first = 0u, index = 0u;
        for (uint32_t l = 1; l < 16u; l++) {
            uint32_t bit;
            if (!take(1u, bit)) return false;
            code |= bit;
            const uint32_t count = use_fixed ? (uint32_t)fixed[cnt + l] : tab.get(cnt + l);
            if (code < first + count) {
                const uint32_t at = sym + index + (code - first);
                symbol = use_fixed ? (uint32_t)fixed[at] : tab.get(at);
                return true;
            }
            index += count;
            first = (first + count) << 1;
            code <<= 1;
        }
        return fail(INFLATE_SYMBOL);  // 15 bits that are no code of an incomplete set
    }

    // ---- RFC 1951 3.2.7: the description of a dynamic block's codes
    FR_HD bool describe() {
        uint32_t hlit, hdist, hclen, v;
        if (!take(5u, hlit) || !take(5u, hdist) || !take(4u, hclen)) return false;
        if (hlit > 29u || hdist > 29u) return fail(INFLATE_CODES);
        const uint32_t n_lit = hlit + 257u, n_dist = hdist + 1u, total = n_lit + n_dist;
        for (uint32_t i = 0; i < 19u; i++) tab.set_len(i, 0u);
        for (uint32_t k = 0; k < hclen + 4u; k++) {
            if (!take(3u, v)) return false;
            tab.set_len(inflate_clc_order(k), v);
        }
        uint32_t max_len;
        if (construct(INFLATE_DCNT, INFLATE_DSYM, 0u, 19u, max_len) != 0) return fail(INFLATE_CODES);  // over-subscribed or incomplete
        uint32_t n = 0u;
        while (n < total) {
            uint32_t symbol;
            if (!decode(false, INFLATE_DCNT, INFLATE_DSYM, symbol)) return false;
            if (symbol < 16u) {
                tab.set_len(n, symbol);
                n++;
                continue;
            }
            uint32_t length = 0u, repeat;
            if (symbol == 16u) {
                if (!n) return fail(INFLATE_CODES);
                length = tab.len(n - 1u);
                if (!take(2u, v)) return false;
                repeat = 3u + v;
            } else if (symbol == 17u) {
                if (!take(3u, v)) return false;
                repeat = 3u + v;
            } else {
                if (!take(7u, v)) return false;
                repeat = 11u + v;
            }
            if (n + repeat > total) return fail(INFLATE_CODES);
            for (; repeat; repeat--) {
                tab.set_len(n, length);
                n++;
            }
        }
        if (!tab.len(256u)) return fail(INFLATE_CODES);
        int32_t left = construct(INFLATE_LCNT, INFLATE_LSYM, 0u, n_lit, max_len);
        if (left < 0 || (left > 0 && max_len != 1u)) return fail(INFLATE_CODES);
        left = construct(INFLATE_DCNT, INFLATE_DSYM, n_lit, n_dist, max_len);
        if (left < 0 || (left > 0 && max_len > 1u)) return fail(INFLATE_CODES);  // (no distance code at all is legal)
        return true;
    }

    // ---- literals, lengths and distances up to end-of-block
    FR_HD bool codes(bool use_fixed) {
        for (;;) {
            uint32_t symbol, base, extra, v = 0u;
            if (!decode(use_fixed, INFLATE_LCNT, INFLATE_LSYM, symbol)) return false;
            if (symbol < 256u) {
                if (!put(symbol)) return false;
                continue;
            }
            if (symbol == 256u) return true;
            if (symbol >= INFLATE_MAX_LIT) return fail(INFLATE_SYMBOL);
            inflate_length_code(symbol - 257u, base, extra);
            if (extra && !take(extra, v)) return false;
            uint32_t length = base + v;
            if (!decode(use_fixed, INFLATE_DCNT, INFLATE_DSYM, symbol)) return false;
            if (symbol >= INFLATE_MAX_DIST) return fail(INFLATE_SYMBOL);
            inflate_distance_code(symbol, base, extra);
            v = 0u;
            if (extra && !take(extra, v)) return false;
            const uint64_t distance = base + v;
            if (distance > written) return fail(INFLATE_DISTANCE);
            for (; length; length--)  // (an overlapping copy re-reads what it has just stored)
                if (!put(out.load(written - distance, written))) return false;
        }
    }
    FR_HD bool stored() {
        to_byte_boundary();
        uint32_t b[4];
        if (!byte(b[0]) || !byte(b[1]) || !byte(b[2]) || !byte(b[3])) return false;
        const uint32_t len = b[0] | b[1] << 8, nlen = b[2] | b[3] << 8;
        if (len != (~nlen & 0xffffu)) return fail(INFLATE_STORED);
        for (uint32_t k = len; k; k--) {
            uint32_t v;
            if (!byte(v) || !put(v)) return false;
        }
        return true;
    }
    FR_HD bool blocks() {
        for (;;) {
            uint32_t header;
            if (!take(3u, header)) return false;
            if (block != 0xFFFFFFFFu) block++;
            const uint32_t type = header >> 1;
            if (type == 0u) {
                if (!stored()) return false;
            } else if (type == 1u) {
                if (!codes(true)) return false;
            } else if (type == 2u) {
                if (!describe() || !codes(false)) return false;
            } else return fail(INFLATE_BLOCK);
            if (header & 1u) return true;
        }
    }
    // ---- RFC 1952: the trailer at the next byte; what lies behind it is nobody's
    FR_HD bool trailer() {
        to_byte_boundary();
        uint32_t word[2];
        for (uint32_t w = 0; w < 2u; w++) {
            uint32_t b[4];
            if (!byte(b[0]) || !byte(b[1]) || !byte(b[2]) || !byte(b[3])) return false;
            word[w] = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
            if (w == 0u && word[0] != ~crc) return fail(INFLATE_CRC);
        }
        if (word[1] != (uint32_t)written) return fail(INFLATE_ISIZE);
        return true;
    }
    FR_HD InflateRow run() {
        (void)(head() && blocks() && trailer());
        out.finish(written);
        return InflateRow{written, cls, block, ~crc};
    }
};

template <class In, class Out, class Tab, class Fixed, class Crc>
FR_HD __forceinline__ InflateRow wire_inflate_row(const In &in, uint64_t n_in, Out &out, uint64_t out_cap, const Tab &tab, const Fixed &fixed, const Crc &crc_table) {
    return WireInflater<In, Out, Tab, Fixed, Crc>(in, n_in, out, out_cap, tab, fixed, crc_table).run();
}

// the key that names the smallest finding of a batch: ~(instance, class, block), kept with atomicMax so that zero means none
// (wire_decode.hpp wire_in_key's scheme; wire_inflate_plan.cpp admits only batches whose instances fit the 27 bits)
FR_HD __forceinline__ uint64_t inflate_key(uint64_t instance, uint32_t cls, uint32_t block) { return ~((((instance << 4) | cls) << 32) | block); }
FR_HD __forceinline__ uint32_t inflate_key_instance(uint64_t word) { return (uint32_t)(~word >> 36); }
FR_HD __forceinline__ uint32_t inflate_key_class(uint64_t word) { return (uint32_t)(~word >> 32) & 15u; }
FR_HD __forceinline__ uint32_t inflate_key_block(uint64_t word) { return (uint32_t)~word; }

}  // namespace acvm
