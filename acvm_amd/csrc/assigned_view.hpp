// assigned_view.hpp -- "is witness w assigned for instance j" after a solve, in one place and without a device: plain host code, no HIP include.
// The rule: an instance the level kernels solved (slow_index[j] < 0) has exactly the planner's assigned set, producer[w] != 0xFFFFFFFF; an
// instance of the exact path (lane t = slow_index[j]) has bit w & 31 of word t of row w >> 5 of its bitmap, a row being n_slow words. A witness
// at or beyond n_witnesses is assigned for nobody. An unassigned witness reads as 32 zero bytes. The bitmap lives on the device: the caller
// either hands over all of it or a function that copies one row; a row is asked for once and kept for the life of the view.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <vector>

namespace acvm {

struct AssignedView {
    const uint32_t *producer;   // [n_witnesses]
    uint32_t n_witnesses;
    const int32_t *slow_index;  // per instance: its lane of the exact path, or < 0 (null: the "instances" are the lanes themselves, j is lane j)
    uint32_t n_slow;            // lanes = words per row
    using FetchRow = std::function<bool(uint32_t word, uint32_t *row)>;  // copies row `word` (n_slow words); false: failed, the row reads as unassigned
    enum Lanes { ALL, LEVEL_ONLY };  // LEVEL_ONLY: the instances of the exact path are left untouched
    AssignedView(const uint32_t *producer, uint32_t n_witnesses, const int32_t *slow_index, uint32_t n_slow, FetchRow fetch_row)
        : producer(producer), n_witnesses(n_witnesses), slow_index(slow_index), n_slow(n_slow), fetch_row(std::move(fetch_row)) {}
    // over the whole bitmap, [row][n_slow], already on the host
    AssignedView(const uint32_t *producer, uint32_t n_witnesses, const int32_t *slow_index, uint32_t n_slow, const uint32_t *bitmap)
        : producer(producer), n_witnesses(n_witnesses), slow_index(slow_index), n_slow(n_slow), whole(bitmap) {}

    static bool bit(const uint32_t *row, int32_t t, uint32_t w) { return (row[t] >> (w & 31)) & 1u; }
    bool produced(uint32_t w) const { return w < n_witnesses && producer[w] != 0xFFFFFFFFu; }
    // THE rule, for lane t (< 0: the level kernels) and the row of w's word
    bool has(int32_t t, uint32_t w, const uint32_t *row) const { return t < 0 || w >= n_witnesses ? produced(w) : bit(row, t, w); }
    bool assigned(uint32_t j, uint32_t w) { return has(lane(j), w, lane(j) < 0 || w >= n_witnesses ? nullptr : row(w >> 5)); }
    // flags[i][k] = instance first + i has witness sel[k] (sel null: witness k) and values_be32[i][k] zeroed where it has not, i < n, k < n_sel;
    // either array may be null
    void fill(uint32_t first, uint32_t n, const uint32_t *sel, uint32_t n_sel, uint8_t *flags, uint8_t *values_be32, Lanes lanes = ALL) {
        const std::vector<const uint32_t *> rows = rows_of(first, n, sel, n_sel, lanes);
        std::vector<uint8_t> level(n_sel);  // what every instance of the level kernels has
        for (uint32_t k = 0; k < n_sel; k++) level[k] = produced(sel ? sel[k] : k);
        for (uint32_t i = 0; i < n; i++) {
            const int32_t t = lane(first + i);
            if (t >= 0 && lanes == LEVEL_ONLY) continue;
            uint8_t *f = flags ? flags + (size_t)i * n_sel : nullptr, *v = values_be32 ? values_be32 + (size_t)i * n_sel * 32 : nullptr;
            for (uint32_t k = 0; k < n_sel; k++) {
                const bool a = t < 0 ? level[k] : has(t, sel ? sel[k] : k, rows[k]);
                if (f) f[k] = a;
                if (!a && v) memset(v + (size_t)k * 32, 0, 32);
            }
        }
    }
    // the lowest instance of [first, first + n) that lacks one of the listed witnesses, and the first one it lacks in the list's order; false: none.
    // O(n + n_witnesses x exact lanes of the range)
    bool first_missing(uint32_t first, uint32_t n, const uint32_t *witnesses, uint32_t n_witnesses_listed, uint32_t *instance, uint32_t *witness) {
        const std::vector<const uint32_t *> rows = rows_of(first, n, witnesses, n_witnesses_listed, ALL);
        uint32_t level_k = 0;  // what every instance of the level kernels lacks first
        while (level_k < n_witnesses_listed && produced(witnesses[level_k])) level_k++;
        for (uint32_t i = 0; i < n; i++) {
            const int32_t t = lane(first + i);
            uint32_t k = level_k;
            if (t >= 0)
                for (k = 0; k < n_witnesses_listed && has(t, witnesses[k], rows[k]); k++) {}
            if (k < n_witnesses_listed) { *instance = first + i; *witness = witnesses[k]; return true; }
        }
        return false;
    }

private:
    FetchRow fetch_row;
    const uint32_t *whole = nullptr;
    std::map<uint32_t, std::vector<uint32_t>> kept;  // rows fetched so far
    int32_t lane(uint32_t j) const { return slow_index ? slow_index[j] : (int32_t)j; }
    const uint32_t *row(uint32_t word) {
        if (whole) return whole + (size_t)word * n_slow;
        auto it = kept.find(word);
        if (it == kept.end()) {
            it = kept.emplace(word, std::vector<uint32_t>(n_slow, 0)).first;
            if (!fetch_row(word, it->second.data())) std::fill(it->second.begin(), it->second.end(), 0u);
        }
        return it->second.data();
    }
    // per list position the row of its witness; all null when no instance of the range needs the bitmap
    std::vector<const uint32_t *> rows_of(uint32_t first, uint32_t n, const uint32_t *sel, uint32_t n_sel, Lanes lanes) {
        std::vector<const uint32_t *> rows(n_sel, nullptr);
        bool any = false;
        for (uint32_t i = 0; i < n && !any && lanes == ALL; i++) any = lane(first + i) >= 0;
        for (uint32_t k = 0; k < n_sel && any; k++) {
            const uint32_t w = sel ? sel[k] : k;
            if (w < n_witnesses) rows[k] = row(w >> 5);
        }
        return rows;
    }
};

}  // namespace acvm
