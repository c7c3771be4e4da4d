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

// ---- acvm_batch_import_device_records_masked: a field may name a presence byte of the record. The UNIT of the window cut is then the field
// together with its mask byte, the byte range from the lower of the two to the end of the upper:
//   - near: the unit's span is at most RECORD_PLAN_WINDOW_CAP bytes (always, in a record that is one window). The unit lies whole in one window
//     and the kernel takes the presence from the block's LDS image: RECORD_MFIELD_MASK is the mask byte's offset inside the window.
//   - far: it is not. The unit is the element alone, RECORD_MFIELD_MASK is RECORD_MASK_FAR and RECORD_MFIELD_FAR_LO / _HI carry the mask byte's
//     offset in the RECORD: lane = instance loads that one byte from global memory.
// Either way exactly one window -- one block per 64 instances -- owns an element AND its presence: nobody else writes its row or its bit of the
// missing set. A longer record is cut as the unmasked plan cuts it, over the units in ascending begin.
// The tables are wider than the unmasked ones, which keep their strides: per window RECORD_MWINDOW_WORDS words -- the five of RECORD_WINDOW_* and
// RECORD_MWINDOW_MISS_BASE, the lowest word of the missing set (position >> 5) a field of the window has (record_decode.hpp record_miss_slot) --
// then per field, window by window, RECORD_MFIELD_WORDS words: the four of RECORD_FIELD_*, the position, and the mask words above.
enum : uint32_t { RECORD_MWINDOW_MISS_BASE = 5, RECORD_MWINDOW_WORDS = 6 };
enum : uint32_t { RECORD_MFIELD_POSITION = 4, RECORD_MFIELD_MASK = 5, RECORD_MFIELD_FAR_LO = 6, RECORD_MFIELD_FAR_HI = 7, RECORD_MFIELD_WORDS = 8 };
enum : uint32_t { RECORD_MASK_NONE = 0xFFFFFFFFu, RECORD_MASK_FAR = 0xFFFFFFFEu };  // (a mask byte inside a window is below RECORD_PLAN_WINDOW_CAP)
// Every check of import_plan_records on (pitch, position, encoding, offset), unchanged, in the same order and with the same texts; behind them
// mask_offset >= pitch (ACVM_RECORD_NO_MASK aside) is refused, naming the field. No field with a mask: *out IS import_plan_records' plan, lists
// and all. Otherwise records and record_masks are set: such a plan never compares equal to an unmasked one.
int import_plan_records_masked(const ImportView *view, const acvm_record_masked_desc_t *d, const void *d_records, ImportPlan *out, std::string *err);

}  // namespace acvm
