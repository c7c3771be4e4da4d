// foreign_plan.hpp -- the batch-wide foreign-call round trip (include/acvm_amd.h acvm_batch_foreign_call_sites, acvm_batch_foreign_call_inputs_device,
// acvm_batch_resolve_foreign_calls_device), checked and laid out before anything touches a device: what batch_foreign.cpp hands to the kernels of
// kernels_foreign.hip. Pure host code like import_plan.hpp: no HIP call, no handle, no thread-local error text -- the site list, a site's waiting list,
// every refusal with its text, the shape words and the capacity rule of the result store run in a plain C++ program
// (tools/foreign_plan_host_test.cpp, tests/test_foreign_plan_on_host.py, `make asan`; the per-row form acvm_batch_resolve_foreign_calls_device_rows:
// tools/foreign_rows_plan_host_test.cpp, tests/test_foreign_rows_on_host.py).
#pragma once
#include "import_plan.hpp"

namespace acvm {

// What the host knows of one exact lane (acvm_batch: slow_ids, slow_res, fc_lane[t].resolved_new), lane t at index t.
struct FcLaneRecord {
    uint32_t instance = 0;
    uint32_t status = 0;         // ACVM_STATUS_*
    uint32_t opcode_index = 0;   // where it stopped
    uint32_t brillig_index = 0;  // the ForeignCall inside the opcode's bytecode (SlowResult::x0)
    bool resolved_new = false;   // answered since the last solve
};
// What the plan knows of one ForeignCall of the circuit.
struct FcSiteDecl {
    uint32_t opcode_index = 0, brillig_index = 0, n_inputs = 0;
    std::string function;
    bool internal = false;  // answered by the library itself (PLAN_FC_INTERNAL_PREFIX): never listed
};
// one row of a site's waiting list
struct FcRow {
    uint32_t lane = 0, instance = 0;
    bool resolved = false;
};

// The sites at which lanes wait, ascending by (opcode, brillig index), internal ones left out. A waiting lane whose site the plan does not declare is
// listed with n_inputs 0 and an empty name.
std::vector<acvm_foreign_call_site_t> foreign_sites(const std::vector<FcSiteDecl> &decls, const FcLaneRecord *lanes, size_t n_lanes);
// The waiting list of a site: its lanes in ascending instance number (failed, solved and running lanes and those of other sites are not in it; answered
// rows are).
std::vector<FcRow> foreign_waiting_list(const FcLaneRecord *lanes, size_t n_lanes, uint32_t opcode_index, uint32_t brillig_index);

// the words of one ForeignCallResult of that shape as the store holds them -- [n_values, (is_array, n) x n_values], n = 1 for a single value -- and its
// number of values. 0, or ACVM_E_INVALID and the text.
int foreign_shape(uint32_t n_values, const uint8_t *is_array, const uint32_t *lens, std::vector<uint32_t> *words, uint32_t *total, std::string *err);

// What the checks need of a handle.
struct FcHandleView {
    bool solved = false, has_solver = false;
    bool site_internal = false;  // the descriptor's site is one the library answers itself
};
// acvm_batch_foreign_call_inputs_device before its sizing kernel: 0 and *stride as launched, or the code and the text. list: the site's waiting list.
int foreign_check_inputs(const FcHandleView *view, const acvm_foreign_call_inputs_desc_t *d, const std::vector<FcRow> &list, uint64_t *stride, std::string *err);
// ... and behind it: the buffer is wide enough for the longest row
int foreign_check_width(const acvm_foreign_call_inputs_desc_t *d, uint32_t max_values, std::string *err);
// acvm_batch_resolve_foreign_calls_device, everything: 0 with *stride, *words and *total, or the code and the text
int foreign_check_answers(const FcHandleView *view, const acvm_foreign_call_answers_desc_t *d, const std::vector<FcRow> &list, uint64_t *stride, std::vector<uint32_t> *words,
                          uint32_t *total, std::string *err);

// acvm_batch_resolve_foreign_calls_device_rows. The refusals come in this order: the checks of foreign_check_answers up to the buffer (with d_lens the
// host lens are not read, the words of an array output carry length 0 -- the row's own length is the device's -- and the shape's total and the width
// are judged behind the sizing launch); then, with the mask on the host, foreign_mask_resumes; then, with the sizing launch's answer,
// foreign_check_rows_width. Without d_answered the rows that were already answered are refused here, as in foreign_check_answers.
int foreign_check_answers_rows(const FcHandleView *view, const acvm_foreign_call_answers_rows_desc_t *d, const std::vector<FcRow> &list, uint64_t *stride,
                               std::vector<uint32_t> *words, uint32_t *total, std::string *err);
// The lanes a mask resumes: *pairs = (lane, instance) of the rows of [first_row, first_row + n_rows) whose answered[i] is nonzero (answered null: all
// of them), ascending. ACVM_E_STATE when one of those was already answered since the last solve; an answered row that is left out is fine.
int foreign_mask_resumes(const std::vector<FcRow> &list, uint32_t first_row, uint32_t n_rows, const uint8_t *answered, std::vector<uint32_t> *pairs, std::string *err);
// Behind the sizing launch: longest = the largest total among the answered rows (0xFFFFFFFF: 2^31 or more). ACVM_E_INVALID for a total beyond any
// result, for n_columns below the longest row (the text states the needed width), for values without a buffer; else *total = longest, what the
// capacity rule below takes as this call's add_vals.
int foreign_check_rows_width(uint32_t n_columns, uint32_t longest, bool has_values, uint32_t *total, std::string *err);

// The capacity rule of a device-owned slot. A row is answered once between two solves, so a column gains at most ONE result per round, whatever the
// number of calls that answer the round's rows (partial ranges, per-instance resolves): the bounds grow per round, not per call.
//   words / vals:             what any instance's column may hold up to the last solve (descriptor words, count word included; values)
//   round_words / round_vals: the largest result appended since (each maximum on its own: an upper bound of any one result of the round)
struct FcBounds {
    uint32_t words = 1, vals = 0;
    uint32_t round_words = 0, round_vals = 0;
};
// a result of add_words / add_vals was appended to some columns in this round
void foreign_bounds_add(FcBounds *b, uint32_t add_words, uint32_t add_vals);
// a solve has consumed the round's answers: its largest result joins the bounds
void foreign_bounds_fold(FcBounds *b);
// Whether the tables must grow before a result of add_words / add_vals is appended in the current round, and the capacities to allocate then: the
// need -- the bounds plus the larger of the round's largest result and this one -- plus half of it plus 8, so that a round trip of many rounds grows
// a logarithmic number of times. A need beyond 2^31 words or values is refused (ACVM_E_INVALID).
struct FcCapacity {
    uint32_t desc_words = 0, vals_cap = 0;
};
int foreign_capacity(const FcBounds &bounds, uint32_t add_words, uint32_t add_vals, const FcCapacity &have, bool *grow, FcCapacity *want, std::string *err);

}  // namespace acvm
