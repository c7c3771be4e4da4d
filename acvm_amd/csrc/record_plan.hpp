// record_plan.hpp -- the record import (include/acvm_amd.h acvm_batch_import_device_records), checked and laid out before anything touches a
// device: the checks of the caller's field list, the field table as it is uploaded, and the cut of a record into windows. Pure host code like
// import_plan.cpp: no HIP call, no handle (tools/record_plan_host_test.cpp, tests/test_record_plan_on_host.py, `make asan`).
#pragma once
#include "import_plan.hpp"

namespace acvm {

// A WINDOW is a byte range of the record that holds whole fields and that a block of kernels_records.hip stages in LDS for its 64 instances:
// at most RECORD_PLAN_WINDOW_CAP bytes (record_decode.hpp RECORD_WINDOW_CAP; kernels_records.hip asserts that the two agree).
//   - A record of at most that many bytes is ONE window, the whole record [0, pitch): the 64 records of a block are one contiguous span.
//   - A longer record is cut: the fields in ascending offset, a window begins at the first field not yet placed and takes every following
//     field that still ends within the cap. Every field lies whole in exactly one window; bytes no window covers are never loaded.
constexpr uint32_t RECORD_PLAN_WINDOW_CAP = 256u;
// The plan's lists (ImportPlan::lists, the handle's one list buffer on the device): record_windows x RECORD_WINDOW_WORDS words, then per field,
// window by window, RECORD_FIELD_WORDS words.
enum : uint32_t { RECORD_WINDOW_OFFSET_LO = 0, RECORD_WINDOW_OFFSET_HI = 1, RECORD_WINDOW_LENGTH = 2, RECORD_WINDOW_FIRST_FIELD = 3, RECORD_WINDOW_N_FIELDS = 4, RECORD_WINDOW_WORDS = 5 };
// row: of the table (the id, or its slot under slot reuse); plane: the input's byte plane or 0xFFFFFFFF; byte: offset inside the window
enum : uint32_t { RECORD_FIELD_ROW = 0, RECORD_FIELD_PLANE = 1, RECORD_FIELD_ENCODING = 2, RECORD_FIELD_BYTE = 3, RECORD_FIELD_WORDS = 4 };

// acvm_batch_import_device_records: 0 and *out (records = true, no parts, the tables in lists), or ACVM_E_INVALID and the text in *err (*out is
// then untouched). view: null is the null batch; view->B is the live count the null-pointer rule and the size bound are judged by.
int import_plan_records(const ImportView *view, const acvm_record_desc_t *d, const void *d_records, ImportPlan *out, std::string *err);

}  // namespace acvm
