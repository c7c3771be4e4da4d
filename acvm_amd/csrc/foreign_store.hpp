// foreign_store.hpp -- one instance's column of the foreign-call result store (kernels.hpp FcStoreSlot) as the APPENDING side sees it: the mirror of the
// walk in ops_brillig.hpp brillig_foreign_call, which reads what is written here. Descriptor words of instance j lie at desc[w * Bp + j]:
//     [n_results, (n_values, (is_array, n) x n_values) x n_results]
// and its values, in the order of the descriptor, at vals[(2 v + h) * Bp + j] (two 16-byte halves per value, like a row of W). Everything here is
// __host__ __device__ so that the host can run what kernels_foreign.hip runs (tools/foreign_store_host_test.hip, tests/test_foreign_store_on_host.py;
// the per-row form: tools/foreign_rows_store_host_test.hip, tests/test_foreign_rows_on_host.py).
#pragma once
#include "import_decode.hpp"

namespace acvm {

// a result that is no value: the marker of a failing INTERNAL call (batch_exact.cpp upload_fc_tables), nothing follows it
constexpr uint32_t FC_STORE_FAIL_MARKER = 0xFFFFFFF0u;

// where the next result of the instance goes
struct FcAppendPos {
    uint32_t n_results;  // results the column holds
    uint32_t word;       // descriptor word the next result starts at
    uint32_t value;      // values in front of it
};
// limit_words: the slot's descriptor words (FcSlot::desc_words). A column whose words run past it is damaged: the walk stops there and reports
// word == limit_words, which no append fits behind.
FR_HD __forceinline__ FcAppendPos fc_store_walk(const uint32_t *desc, uint64_t Bp, uint64_t j, uint32_t limit_words) {
    FcAppendPos p;
    p.n_results = desc[j];
    p.word = 1u;
    p.value = 0u;
    for (uint32_t r = 0; r < p.n_results; r++) {
        if (p.word >= limit_words) { p.word = limit_words; return p; }
        const uint32_t n_values = desc[(uint64_t)p.word * Bp + j];
        p.word++;
        if (n_values >= FC_STORE_FAIL_MARKER) continue;
        if ((uint64_t)p.word + 2ull * n_values > limit_words) { p.word = limit_words; return p; }
        for (uint32_t v = 0; v < n_values; v++, p.word += 2u) p.value += desc[(uint64_t)(p.word + 1u) * Bp + j];
    }
    return p;
}

// One appended result as words: shape = [n_values, (is_array, n) x n_values], n = 1 for a single value (what upload_fc_tables writes for it).
FR_HD __forceinline__ uint32_t fc_shape_words(uint32_t n_values) { return 1u + 2u * n_values; }
FR_HD __forceinline__ uint32_t fc_shape_total(const uint32_t *shape) {
    uint32_t total = 0;
    for (uint32_t v = 0; v < shape[0]; v++) total += shape[2u + 2u * v];
    return total;
}
// the bound check against the slot's capacity: the result's words and values lie inside the tables
FR_HD __forceinline__ bool fc_store_fits(const FcAppendPos &p, uint32_t shape_words, uint32_t shape_total, uint32_t desc_words, uint32_t vals_cap) {
    return (uint64_t)p.word + shape_words <= desc_words && (uint64_t)p.value + shape_total <= vals_cap;
}
// the shape words behind the column's last result (the count is NOT touched: fc_store_commit, after the values)
FR_HD __forceinline__ void fc_store_write_shape(uint32_t *desc, uint64_t Bp, uint64_t j, const FcAppendPos &p, const uint32_t *shape) {
    const uint32_t n = fc_shape_words(shape[0]);
    for (uint32_t w = 0; w < n; w++) desc[(uint64_t)(p.word + w) * Bp + j] = shape[w];
}
FR_HD __forceinline__ void fc_store_write_value(uint4 *vals, uint64_t Bp, uint64_t j, uint32_t v, const Fr &row) { fr_store(vals, v, Bp, j, row); }
FR_HD __forceinline__ void fc_store_commit(uint32_t *desc, uint64_t j, const FcAppendPos &p) { desc[j] = p.n_results + 1u; }

// One element of the caller's answer buffer as the row x * 2^261, fully reduced (ImportDecoded::row): every 256-bit string is accepted and reduced
// as the per-instance call reduces it; a narrow element is the integer itself.
FR_HD __forceinline__ Fr fc_answer_row(const uint8_t *base, uint32_t encoding, uint32_t layout, uint64_t stride, uint64_t r, uint64_t c) {
    const uint32_t size = export_element_size(encoding);
    const uint8_t *p = base + export_element_offset(layout, stride, r, c, size);
    if (export_enc_is_narrow(encoding)) return import_decode_narrow(import_narrow_read(p, size)).row;
    const uint4 lo = *(const uint4 *)p, hi = *(const uint4 *)(p + 16);
    const Fr m = import_limbs(lo, hi, encoding);
    return import_row(m, encoding == EXPORT_ENC_MONT256_LE ? m : import_reduce(m), encoding);
}

// The whole append of one row, as fc_append_kernel's lane runs it. Returns false, having written nothing, when the result does not fit.
struct FcAnswers {
    const uint8_t *values;  // the caller's buffer
    uint32_t encoding, layout;
    uint64_t stride;
};
FR_HD __forceinline__ bool fc_store_append(uint32_t *desc, uint4 *vals, uint64_t Bp, uint64_t j, uint32_t desc_words, uint32_t vals_cap, const uint32_t *shape,
                                           uint32_t shape_total, const FcAnswers &a, uint64_t r) {
    const FcAppendPos p = fc_store_walk(desc, Bp, j, desc_words);
    if (!fc_store_fits(p, fc_shape_words(shape[0]), shape_total, desc_words, vals_cap)) return false;
    fc_store_write_shape(desc, Bp, j, p, shape);
    for (uint32_t c = 0; c < shape_total; c++) fc_store_write_value(vals, Bp, j, p.value + c, fc_answer_row(a.values, a.encoding, a.layout, a.stride, r, c));
    fc_store_commit(desc, j, p);
    return true;
}

// ---- per-row answers (acvm_batch_resolve_foreign_calls_device_rows): the shape words give n_values and which outputs are arrays; an array output k of
// row r has lens[r * n_values + k] values (lens null: the shape's own n), a single value always 1; answered[r] == 0 (answered non-null) leaves the row out.
struct FcRowAnswers {
    const uint32_t *lens;     // [n_rows][n_values] row-major, or null
    const uint8_t *answered;  // [n_rows], or null: every row
    uint32_t n_columns;       // values per row the caller's buffer holds
};
FR_HD __forceinline__ bool fc_row_answered(const FcRowAnswers &ra, uint64_t r) { return !ra.answered || ra.answered[r] != 0; }
FR_HD __forceinline__ uint32_t fc_row_len(const uint32_t *shape, const FcRowAnswers &ra, uint64_t r, uint32_t k) {
    if (!shape[1u + 2u * k]) return 1u;
    return ra.lens ? ra.lens[r * shape[0] + k] : shape[2u + 2u * k];
}
// the row's number of values, summed in 64 bits
FR_HD __forceinline__ uint64_t fc_row_total(const uint32_t *shape, const FcRowAnswers &ra, uint64_t r) {
    uint64_t total = 0;
    for (uint32_t k = 0; k < shape[0]; k++) total += fc_row_len(shape, ra, r, k);
    return total;
}
// what the sizing launch reduces: 0 for a row that is left out, the row's total, 0xFFFFFFFF for a total of 2^31 or more (refused by the host)
FR_HD __forceinline__ uint32_t fc_row_total_saturated(const uint32_t *shape, const FcRowAnswers &ra, uint64_t r) {
    if (!fc_row_answered(ra, r)) return 0u;
    const uint64_t total = fc_row_total(shape, ra, r);
    return total >= (1ull << 31) ? 0xFFFFFFFFu : (uint32_t)total;
}
enum FcRowAppend : uint32_t { FC_ROW_APPENDED = 0, FC_ROW_LEFT_OUT = 1, FC_ROW_REFUSED = 2 };
// The whole append of one row of the per-row form, as fc_append_rows_kernel's lane runs it. A row that is left out touches nothing. A row whose lengths
// pass the caller's columns or the slot's words or values is refused, having written nothing. The shape words come from the row's own lengths; the
// count word is written last.
FR_HD __forceinline__ FcRowAppend fc_store_append_row(uint32_t *desc, uint4 *vals, uint64_t Bp, uint64_t j, uint32_t desc_words, uint32_t vals_cap, const uint32_t *shape,
                                                      const FcRowAnswers &ra, const FcAnswers &a, uint64_t r) {
    if (!fc_row_answered(ra, r)) return FC_ROW_LEFT_OUT;
    const uint64_t total = fc_row_total(shape, ra, r);
    if (total > ra.n_columns) return FC_ROW_REFUSED;
    const FcAppendPos p = fc_store_walk(desc, Bp, j, desc_words);
    if (!fc_store_fits(p, fc_shape_words(shape[0]), (uint32_t)total, desc_words, vals_cap)) return FC_ROW_REFUSED;
    desc[(uint64_t)p.word * Bp + j] = shape[0];
    for (uint32_t k = 0; k < shape[0]; k++) {
        desc[(uint64_t)(p.word + 1u + 2u * k) * Bp + j] = shape[1u + 2u * k];
        desc[(uint64_t)(p.word + 2u + 2u * k) * Bp + j] = fc_row_len(shape, ra, r, k);
    }
    for (uint32_t c = 0; c < (uint32_t)total; c++) fc_store_write_value(vals, Bp, j, p.value + c, fc_answer_row(a.values, a.encoding, a.layout, a.stride, r, c));
    fc_store_commit(desc, j, p);
    return FC_ROW_APPENDED;
}

// ---- the pending inputs of an exact lane (kernels.hpp FcLanes): pend_desc [n_inputs, len x n_inputs] at pend_desc[w * n_slow + t]
// the lane's number of inputs, never more than the length words the buffer has room for
FR_HD __forceinline__ uint32_t fc_pending_inputs(const uint32_t *pend_desc, uint32_t pend_desc_words, uint64_t t) {
    const uint32_t n_in = pend_desc[t], room = pend_desc_words ? pend_desc_words - 1u : 0u;
    return n_in < room ? n_in : room;
}
FR_HD __forceinline__ uint32_t fc_pending_total(const uint32_t *pend_desc, uint32_t pend_desc_words, uint64_t n_slow, uint64_t t) {
    const uint32_t n_in = fc_pending_inputs(pend_desc, pend_desc_words, t);
    uint32_t total = 0;
    for (uint32_t i = 0; i < n_in; i++) total += pend_desc[(uint64_t)(1u + i) * n_slow + t];
    return total;
}

}  // namespace acvm
