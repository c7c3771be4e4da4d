// wire_repitch.hpp -- rows of bytes moved between a PITCHED buffer (row i at i * pitch) and a PACKED one (row i at offsets[i], no byte between
// rows): what a lane of kernels_wire_pack.hip runs (include/acvm_amd.h acvm_batch_witness_maps_wire_packed_device,
// acvm_batch_import_device_wire_packed), and what the host runs on the same bytes (tools/wire_repitch_host_test.hip,
// tests/test_wire_pack_on_host.py, `make asan`). Three pieces: the 64-bit exclusive scan that makes an offsets column from a lengths column,
// the judgement of an untrusted offsets column, and the copy of one 16-byte unit of one row.
//
// The copy works in VIRTUAL addresses: a buffer's base has an alignment 0 .. 15 (src_align, dst_align: its address mod 16), byte `off` of it
// lies at virtual address align + off, and a unit is 16 bytes at a virtual address that is a multiple of 16 -- an aligned 16-byte access of
// the real buffer. A lane owns ONE destination unit of one row:
//   - a unit that lies wholly inside the row is stored as 16 aligned bytes; its source bytes are assembled from the one or two aligned source
//     units they fall into and a byte shift;
//   - the fewer than 16 bytes of a unit the row only partly covers -- at the row's start, at its end -- are loaded and stored byte by byte.
// Rules, kept by construction (in the spirit of record_encode.hpp's record_cover_nibble):
//   - row i's lanes store no byte outside [dst_off(i), dst_off(i) + len(i)); nothing of the destination is loaded, nothing is
//     read-modify-written, no atomic touches either buffer; two rows that share a dword -- or a unit -- each store their own bytes;
//   - no load touches a byte outside [0, src_bytes) of the source: a source unit that crosses either end is assembled from the bytes inside;
//     a packed source may end in mid-dword;
//   - a row with a finding, or one that does not fit the capacity, loads and stores nothing.
// Mem is the memory: load16(off) / store16(off, unit) with align + off a multiple of 16, load8(off) / store8(off, byte).
#pragma once
#include "wire_encode.hpp"

namespace acvm {

// ---- the offsets column of a packed buffer of n_bytes, as the import meets it: untrusted. Row j is [offsets[j], offsets[j + 1]).
enum : uint32_t {
    REPITCH_DESCENDING = 1,  // offsets[j + 1] < offsets[j]
    REPITCH_BEYOND = 2,      // offsets[j + 1] > n_bytes
    REPITCH_LONG = 3,        // the row is longer than the pitch it goes to (or comes from)
    REPITCH_CLASSES = 4
};
FR_HD __forceinline__ uint32_t wire_offsets_class(uint64_t lo, uint64_t hi, uint64_t n_bytes, uint64_t longest) {
    return hi < lo ? REPITCH_DESCENDING : hi > n_bytes ? REPITCH_BEYOND : hi - lo > longest ? REPITCH_LONG : 0u;
}
// the smallest (instance, class) is the largest key: what atomicMax keeps
FR_HD __forceinline__ uint64_t wire_offsets_key(uint64_t instance, uint32_t cls) { return ~((instance << 4) | cls); }
FR_HD __forceinline__ uint64_t wire_offsets_key_instance(uint64_t key) { return ~key >> 4; }
FR_HD __forceinline__ uint32_t wire_offsets_key_class(uint64_t key) { return (uint32_t)~key & 15u; }

// ---- one call of the copy. Source and destination are each pitched (offsets null: row i at i * pitch) or packed (row i at offsets[i]).
// lengths: the rows' lengths where the source is pitched; a packed source's own offsets give them. A packed destination takes row i only
// when dst_offsets[i] + len(i) <= capacity, at dst + dst_offsets[i] - dst_rebase (the host form packs a chunk into a region that starts at
// the chunk's first offset).
struct WireRepitch {
    uint32_t n;
    const uint8_t *src;
    uint64_t src_pitch;
    const uint64_t *src_offsets;
    uint64_t src_bytes;  // the stated end of the source
    uint32_t src_align;
    const uint64_t *lengths;
    uint8_t *dst;
    uint64_t dst_pitch;
    const uint64_t *dst_offsets;
    uint64_t dst_rebase, capacity;
    uint32_t dst_align;
    uint64_t units_per_row;  // wire_repitch_units(the longest row there can be): sizes the grid, a host-known quantity
};
// the destination units a row of up to `longest` bytes can touch at any alignment
FR_HD __forceinline__ uint64_t wire_repitch_units(uint64_t longest) { return (longest + 15u) / 16u + 1u; }

struct RepitchRow {
    uint64_t src_off, dst_off, len;
    uint32_t cls;  // the finding of a packed source's offsets (0: none)
    bool copy;
};
FR_HD __forceinline__ RepitchRow wire_repitch_row(const WireRepitch &a, uint64_t i) {
    RepitchRow r{0u, 0u, 0u, 0u, false};
    if (a.src_offsets) {
        const uint64_t lo = a.src_offsets[i], hi = a.src_offsets[i + 1u];
        r.cls = wire_offsets_class(lo, hi, a.src_bytes, a.dst_offsets ? ~(uint64_t)0 : a.dst_pitch);
        if (r.cls) return r;
        r.src_off = lo;
        r.len = hi - lo;
    } else {
        r.src_off = i * a.src_pitch;
        r.len = a.lengths[i];
        if (r.len > a.src_pitch) { r.cls = REPITCH_LONG; return r; }  // (no exporter writes such a length: nothing past the slot is loaded)
    }
    if (a.dst_offsets) {
        const uint64_t at = a.dst_offsets[i];
        r.dst_off = at - a.dst_rebase;
        r.copy = at >= a.dst_rebase && at + r.len >= at && at + r.len <= a.capacity;
    } else {
        r.dst_off = i * a.dst_pitch;
        r.copy = r.len <= a.dst_pitch;
    }
    return r;
}

struct Unit16 {
    uint32_t w[4];
};
// the aligned source unit at virtual address v: one load where it lies inside the source, else the bytes of it that do (zero elsewhere)
template <class Mem>
FR_HD __forceinline__ Unit16 wire_repitch_load_unit(const Mem &m, const WireRepitch &a, uint64_t v) {
    if (v >= a.src_align && v - a.src_align + 16u <= a.src_bytes) return m.load16(v - a.src_align);
    Unit16 out{{0u, 0u, 0u, 0u}};
    for (uint32_t c = 0; c < 16u; c++) {
        const uint64_t at = v + c;
        if (at >= a.src_align && at - a.src_align < a.src_bytes) out.w[c >> 2] |= (uint32_t)m.load8(at - a.src_align) << (8u * (c & 3u));
    }
    return out;
}
// bytes [shift, shift + 16) of the 32 bytes lo | hi (shift 0 .. 15): selects and funnel shifts, no indexed register
FR_HD __forceinline__ Unit16 wire_repitch_shift(const Unit16 &lo, const Unit16 &hi, uint32_t shift) {
    const uint32_t w[8] = {lo.w[0], lo.w[1], lo.w[2], lo.w[3], hi.w[0], hi.w[1], hi.w[2], hi.w[3]};
    const uint32_t words = shift >> 2, bits = 8u * (shift & 3u);
    Unit16 out;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t x = words == 0u ? w[j] : words == 1u ? w[j + 1u] : words == 2u ? w[j + 2u] : w[j + 3u];
        const uint32_t y = words == 0u ? w[j + 1u] : words == 1u ? w[j + 2u] : words == 2u ? w[j + 3u] : w[j + 4u];
        out.w[j] = bits ? (x >> bits) | (y << (32u - bits)) : x;
    }
    return out;
}
// destination unit u (< units_per_row) of row r
template <class Mem>
FR_HD __forceinline__ void wire_repitch_unit(const Mem &m, const WireRepitch &a, const RepitchRow &r, uint64_t u) {
    if (!r.copy) return;
    const uint64_t d0 = a.dst_align + r.dst_off, d1 = d0 + r.len;  // the row's virtual destination
    const uint64_t lo = ((d0 >> 4) + u) << 4;
    if (lo >= d1) return;  // (a unit beyond its row's length; a row of 0 bytes has none)
    const uint64_t begin = lo > d0 ? lo : d0, end = lo + 16u < d1 ? lo + 16u : d1;
    const uint64_t s0 = a.src_align + r.src_off;  // the virtual source of d0
    if (end - begin == 16u) {
        const uint64_t sv = s0 + (lo - d0);
        const uint32_t shift = (uint32_t)sv & 15u;
        const Unit16 first = wire_repitch_load_unit(m, a, sv - shift);
        // (shift 0: the unit is the source's own; the second one may lie behind the source's end)
        const Unit16 second = shift ? wire_repitch_load_unit(m, a, sv - shift + 16u) : Unit16{{0u, 0u, 0u, 0u}};
        m.store16(lo - a.dst_align, wire_repitch_shift(first, second, shift));
    } else {
        for (uint64_t x = begin; x < end; x++) m.store8(x - a.dst_align, m.load8(s0 + (x - d0) - a.src_align));
    }
}

// ---- the scan: offsets[i + 1] = base + lengths[0] + .. + lengths[i] for the m rows of a chunk, by ONE block of REPITCH_SCAN_THREADS threads in
// tiles of REPITCH_SCAN_TILE rows. A thread owns REPITCH_SCAN_ITEMS consecutive rows of a tile: it sums them (wire_scan_thread_sum), the
// block makes the inclusive sums of the threads' totals in log2(threads) steps over two arrays (wire_scan_step: out[t] from in[t] and
// in[t - d]), and the thread writes its rows' offsets from the sum in front of it (wire_scan_thread_emit), counting those that end at or in
// front of the capacity.
constexpr uint32_t REPITCH_SCAN_THREADS = 256, REPITCH_SCAN_ITEMS = 4, REPITCH_SCAN_TILE = REPITCH_SCAN_THREADS * REPITCH_SCAN_ITEMS;
enum : uint32_t { REPITCH_STATE_BASE = 0, REPITCH_STATE_FIT = 1, REPITCH_STATE_WORDS = 2 };  // the device words that carry a scan from chunk to chunk

FR_HD __forceinline__ uint64_t wire_scan_thread_sum(const uint64_t *lengths, uint64_t m, uint64_t tile0, uint32_t t) {
    uint64_t sum = 0u;
    for (uint32_t k = 0; k < REPITCH_SCAN_ITEMS; k++) {
        const uint64_t i = tile0 + (uint64_t)t * REPITCH_SCAN_ITEMS + k;
        if (i < m) sum += lengths[i];
    }
    return sum;
}
FR_HD __forceinline__ uint64_t wire_scan_step(const uint64_t *in, uint32_t t, uint32_t d) { return in[t] + (t >= d ? in[t - d] : 0u); }
// before: the base and every row in front of this thread's. Returns its rows with offsets[i + 1] <= capacity.
FR_HD __forceinline__ uint32_t wire_scan_thread_emit(const uint64_t *lengths, uint64_t m, uint64_t tile0, uint32_t t, uint64_t before, uint64_t capacity, uint64_t *offsets) {
    uint32_t fit = 0u;
    for (uint32_t k = 0; k < REPITCH_SCAN_ITEMS; k++) {
        const uint64_t i = tile0 + (uint64_t)t * REPITCH_SCAN_ITEMS + k;
        if (i >= m) break;
        before += lengths[i];
        offsets[i + 1u] = before;
        fit += before <= capacity ? 1u : 0u;
    }
    return fit;
}

}  // namespace acvm
