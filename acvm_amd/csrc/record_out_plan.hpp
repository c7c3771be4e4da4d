// record_out_plan.hpp -- the record export (include/acvm_amd.h acvm_batch_export_device_records), checked and laid out before anything touches
// a device: the checks of the caller's field list, the cut of the covered bytes into windows, each window's cover bitmap and the field table as
// it is uploaded. The twin of record_plan.cpp and pure host code like it: no HIP call, no handle (tools/record_out_plan_host_test.cpp,
// tests/test_record_out_plan_on_host.py, `make asan`).
#pragma once
#include "record_plan.hpp"

namespace acvm {

// A COVERED RANGE is a byte range of the record that the call writes: the element of a field, or its mask byte (a range of one byte). Covered
// ranges never overlap -- a store, unlike the import's load, has one owner per byte -- and every byte outside them is never written.
// The WINDOW cut is record_plan.hpp's, made over the covered ranges: a record of at most RECORD_PLAN_WINDOW_CAP bytes is one window, the record
// itself; a longer one is cut in ascending offset, every covered range whole in exactly one window. A field's element and its mask byte may
// fall into different windows.
// The tables (RecordOutPlan::tables, one device buffer): n_windows x RECORD_OUT_WINDOW_WORDS words -- record_plan.hpp's five window words, then
// the COVER BITMAP of RECORD_PLAN_WINDOW_CAP bits: bit b of the bitmap (bit b & 31 of its word b >> 5) is set when byte b of the window is
// covered -- then per entry, window by window, RECORD_OUT_FIELD_WORDS words.
enum : uint32_t { RECORD_OUT_WINDOW_BITMAP = RECORD_WINDOW_WORDS, RECORD_OUT_BITMAP_WORDS = RECORD_PLAN_WINDOW_CAP / 32u, RECORD_OUT_WINDOW_WORDS = RECORD_WINDOW_WORDS + RECORD_OUT_BITMAP_WORDS };
// witness: the id (the kernel looks up row, producer and scale as the other exports do); byte: of the element inside the window; kind: what the
// entry writes (RECORD_OUT_KIND_*) in bits 0 .. 1, the mask byte's offset inside the window in bits 8 .. 15. The fused kind -- element and mask
// byte in one window, the common case -- costs one row load and one product, not two.
enum : uint32_t { RECORD_OUT_FIELD_WITNESS = 0, RECORD_OUT_FIELD_ENCODING = 1, RECORD_OUT_FIELD_BYTE = 2, RECORD_OUT_FIELD_KIND = 3, RECORD_OUT_FIELD_WORDS = 4 };
enum : uint32_t { RECORD_OUT_KIND_VALUE = 1, RECORD_OUT_KIND_MASK = 2, RECORD_OUT_KIND_BOTH = 3 };

struct RecordOutPlan {
    uint64_t pitch = 0;
    uint32_t first = 0, n = 0;  // output rows [0, n): instances [first, first + n), or the list's entries
    uint32_t n_windows = 0, n_entries = 0;
    bool mont256 = false, plain = false;  // which factor tables the fields take (ACVM_ENC_MONT256_LE / every other encoding)
    std::vector<uint32_t> witnesses;      // the distinct witnesses of the fields, ascending (what the handle's state is judged by)
    std::vector<uint32_t> tables;
};

// 0 and *out, or ACVM_E_INVALID and the text in *err (*out is then untouched). live: null is the null batch, else the live instance count the
// range is judged by. list: the call has an instance list (first must be 0; the entries are the device's to judge). records: the caller's
// buffer, judged for null only.
int record_out_plan(const uint32_t *live, const acvm_record_out_desc_t *d, bool list, const void *records, RecordOutPlan *out, std::string *err);

}  // namespace acvm
