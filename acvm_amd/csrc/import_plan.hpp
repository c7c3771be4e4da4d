// import_plan.hpp -- one device import, checked and laid out, before anything touches a device: what every import entry point of
// batch_import.cpp (and the two solve_then_import entry points of batch_schedule.cpp) hands to batch_launch_import. Pure host code: no HIP call,
// no handle, no thread-local error text -- the checks of the caller's descriptor, parts, column lists and position lists run in a plain C++
// program (tools/import_plan_host_test.cpp, tests/test_import_plan_on_host.py, `make asan`).
#pragma once
#include "../../include/acvm_amd.h"
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace acvm {

// ---- the checks of a described device buffer, shared with acvm_batch_export_device (batch_export.cpp). Each returns the refusal's text, or an
// empty string; all of them are ACVM_E_INVALID. They are steps because the two callers put checks of their own between them.
uint32_t buffer_element_size(uint32_t encoding);  // bytes per element: 32, or the width of a narrow encoding
// "unknown encoding E" / "unknown layout L" (broadcast: ACVM_LAYOUT_BROADCAST is a layout too -- the parts of an import)
std::string buffer_check_shape(uint32_t encoding, uint32_t layout, bool broadcast);
// the pointer is aligned to the element's size, 16 bytes for the 32-byte encodings
std::string buffer_check_pointer(uint32_t encoding, const void *d_values);
// *stride: the caller's, 0 = dense; comes back as launched. n: instances, n_sel: columns / listed witnesses of the buffer.
std::string buffer_check_stride(uint32_t layout, uint32_t n, uint32_t n_sel, uint64_t *stride);

// What the checks need of a handle.
struct ImportView {
    uint32_t B = 0, n_in = 0;          // live instances, initial witnesses
    const uint32_t *ids = nullptr;     // per position the initial witness (the refusals name it)
    const uint32_t *rows = nullptr;    // per position its row of the table: the id, or its slot under slot reuse
    const uint32_t *planes = nullptr;  // per position its byte plane or NONE; null: the circuit has no planes
};

constexpr size_t IMPORT_NO_LIST = (size_t)-1;
struct ImportPlanPart {
    uint32_t encoding = 0, layout = 0;
    uint32_t elem_size = 32;   // bytes per element
    uint64_t stride = 0;       // as launched: never 0
    uint32_t n = 0;            // inputs this part supplies
    const void *d_values = nullptr;  // the caller's device pointer (not compared)
    // Where the part's lists lie in ImportPlan::lists. resident: a descriptor supplies every initial witness in order, so its rows and planes are
    // the tables the handle keeps on the device anyway (d_init_ids / d_init_rows, d_byte_plane_of_input) and only its column list travels.
    bool resident = false;
    size_t rows_at = IMPORT_NO_LIST, planes_at = IMPORT_NO_LIST, columns_at = IMPORT_NO_LIST;
    bool operator==(const ImportPlanPart &o) const {
        return encoding == o.encoding && layout == o.layout && elem_size == o.elem_size && stride == o.stride && n == o.n && resident == o.resident && rows_at == o.rows_at &&
               planes_at == o.planes_at && columns_at == o.columns_at;
    }
};
// The handle keeps a COPY of the plan it enqueued behind a solve: the following import costs nothing only if pointer and plan are both the same.
struct ImportPlan {
    // BE32, instance-major, dense, no column list, from a descriptor: the one shape of acvm_batch_set_initial_witness_device /
    // acvm_batch_solve_then_import (kernels.hip import_witness_kernel), exempt from the alignment rule
    bool plain = false;
    std::vector<ImportPlanPart> parts;
    std::vector<uint32_t> lists;  // all lists of the call, per part: rows, planes (circuits with byte planes), columns (parts with a list)
    // acvm_batch_import_device_masked: one byte per element in the layout, stride and column list of the (one, resident) part. A plan with a mask
    // never compares equal to one without, and the solve_then_import entry points take none: it never counts as the import that ran behind a
    // solve. (Like d_values the pointer itself is not compared.)
    const uint8_t *d_assigned = nullptr;
    bool masked() const { return d_assigned != nullptr; }
    // acvm_batch_import_device_records (record_plan.hpp import_plan_records): no parts -- lists holds the window table and the field table, one
    // launch reads them (kernels_records.hip). A record plan never compares equal to a plan of another kind, two record plans are equal when
    // pitch, window count and tables are, and the solve_then_import entry points take none: it never counts as the import that ran behind a
    // solve. (Like d_values the pointer d_records is not compared.)
    bool records = false;
    // acvm_batch_import_device_records_masked (record_plan.hpp import_plan_records_masked) with at least one mask byte: a record plan whose
    // tables are the wider masked ones and whose launch is the masked kernel's (kernels_records_masked.hip). Never equal to an unmasked plan.
    bool record_masks = false;
    uint64_t record_pitch = 0;
    uint32_t record_windows = 0;
    const void *d_records = nullptr;
    bool operator==(const ImportPlan &o) const {
        return masked() == o.masked() && plain == o.plain && records == o.records && record_masks == o.record_masks && record_pitch == o.record_pitch && record_windows == o.record_windows && parts == o.parts &&
               lists == o.lists;
    }
};

// the plain plan of a handle with n_in initial witnesses: nothing to check, any pointer
ImportPlan import_plan_plain(uint32_t n_in, const void *d_values);
// A descriptor is a plan of one (resident) part; each part of acvm_batch_import_device_parts one part with lists of its own. Each returns 0 and
// *out, or ACVM_E_INVALID and the text in *err (*out is then untouched). view: null is the null batch, judged behind encoding and layout.
int import_plan_desc(const ImportView *view, const acvm_import_desc_t *d, const void *d_values, ImportPlan *out, std::string *err);
// acvm_batch_import_device_masked: every check of import_plan_desc on d and d_values, unchanged and in the same order; d_assigned (any
// alignment) joins the plan. d_assigned null IS import_plan_desc: the same plan, equal to the unmasked call's.
int import_plan_desc_masked(const ImportView *view, const acvm_import_desc_t *d, const void *d_values, const uint8_t *d_assigned, ImportPlan *out, std::string *err);
int import_plan_parts(const ImportView *view, const acvm_import_part_t *parts, uint32_t n_parts, ImportPlan *out, std::string *err);

}  // namespace acvm
