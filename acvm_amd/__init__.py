"""acvm_amd -- MI355X-native batched ACIR witness solver (drop-in for acvm::pwg::ACVM::solve()).

The compute path is libacvm_amd.so (hand-written gfx950 HIP kernels behind the C ABI of
include/acvm_amd.h). This module is only the ctypes view of that ABI for tests and the bench, shaped
like the reference API (acvm/src/pwg/mod.rs:145-304): Circuit.read -> Batch(...).solve() ->
results()/witness_map(). There is no CPU fallback: importing the solver without the built library, or
creating a batch without a gfx950 device, raises.
"""
import ctypes as C
import functools
import os

from . import acir  # noqa: F401  (data model + wire format)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (ACVM_AMD_LIB: another build of the same ABI, for A/B measurements of two library versions on one box: tools/gpu_ab_lib.sh)
LIB_PATH = os.environ.get("ACVM_AMD_LIB") or os.path.join(_HERE, "libacvm_amd.so")

STATUS_SOLVED, STATUS_IN_PROGRESS, STATUS_FAILURE, STATUS_REQUIRES_FOREIGN_CALL = 0, 1, 2, 3
(ERR_NONE, ERR_MISSING_ASSIGNMENT, ERR_TOO_MANY_UNKNOWNS, ERR_UNSUPPORTED_BLACKBOX, ERR_UNSATISFIED, ERR_INDEX_OOB,
 ERR_BLACKBOX_FAILED, ERR_BRILLIG_FAILED, ERR_PANIC, ERR_DEVICE_LIMIT) = range(10)
LIMIT_BRILLIG_STEPS, LIMIT_BRILLIG_CALL_DEPTH, LIMIT_BRILLIG_MEMORY, LIMIT_DEVICE_MEMORY = 1, 2, 3, 4
# acvm_batch_export_device / acvm_batch_import_device: ACVM_ENC_* / ACVM_LAYOUT_*
ENC_BE32, ENC_LE32, ENC_MONT256_LE = 0, 1, 2
ENC_U8, ENC_U16, ENC_U32, ENC_U64, ENC_U128 = 16, 17, 18, 19, 20  # unsigned little-endian integers of 1 .. 16 bytes per element
LAYOUT_INSTANCE_MAJOR, LAYOUT_WITNESS_MAJOR = 0, 1
LAYOUT_BROADCAST = 16  # parts of import_device_parts only: one element per column, the value of every instance

# every symbol include/acvm_amd.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "acvm_last_error", "acvm_abi_version", "acvm_device_count", "acvm_set_device", "acvm_device_synchronize",
    "acvm_device_arch", "acvm_selftest", "acvm_debug_grumpkin", "acvm_debug_grumpkin_items", "acvm_debug_secp", "acvm_circuit_from_bytes", "acvm_circuit_free", "acvm_circuit_num_opcodes",
    "acvm_circuit_num_witnesses", "acvm_circuit_plan_stats", "acvm_batch_new", "acvm_batch_free", "acvm_batch_set_initial_witness",
    "acvm_batch_set_initial_witness_device", "acvm_batch_solve", "acvm_batch_solve_then_import", "acvm_batch_reset", "acvm_batch_set_instances", "acvm_batch_set_force_slow_path",
    "acvm_batch_results", "acvm_batch_witness", "acvm_batch_witness_map", "acvm_batch_stats",
    "acvm_batch_set_profiling", "acvm_batch_pending_foreign_call", "acvm_batch_pending_foreign_call_inputs",
    "acvm_batch_resolve_foreign_call", "acvm_circuit_assert_message", "acvm_circuit_witness_set", "acvm_batch_error_string",
    "acvm_batch_extract_witnesses", "acvm_batch_digest", "acvm_witness_map_decode", "acvm_witness_map_encode", "acvm_batch_witness_map_bytes",
    "acvm_device_malloc", "acvm_device_free", "acvm_device_upload", "acvm_batch_solve_opcode", "acvm_bb_stubbed", "acvm_bb_dummy",
    "acvm_new", "acvm_free", "acvm_solve", "acvm_solve_opcode", "acvm_get_status", "acvm_instruction_pointer", "acvm_witness_map", "acvm_finalize",
    "acvm_get_pending_foreign_call", "acvm_pending_foreign_call_inputs", "acvm_resolve_pending_foreign_call",
    "acvm_multi_new", "acvm_multi_free", "acvm_multi_num_groups", "acvm_multi_solve", "acvm_multi_results", "acvm_multi_num_witnesses",
    "acvm_multi_witness_map", "acvm_multi_locate", "acvm_debug_modmul_rate", "acvm_debug_secp_rate", "acvm_batch_new_ex", "acvm_circuit_plan_stats_ex",
    "acvm_tuning_set", "acvm_tuning_get", "acvm_tuning_key",
    "acvm_device_release_tables", "acvm_circuit_opcode_kinds", "acvm_batch_error_expression", "acvm_debug_stream_rate", "acvm_node_new", "acvm_node_free", "acvm_node_tile_instances", "acvm_node_num_devices", "acvm_node_solve", "acvm_node_stats",
    "acvm_debug_cpulist", "acvm_debug_device_locality", "acvm_debug_plan_fingerprint", "acvm_circuit_plans_built", "acvm_circuit_check_schedule", "acvm_batch_digest_blake2s",
    "acvm_batch_export_device", "acvm_device_download", "acvm_debug_fr", "acvm_debug_inverse_batch", "acvm_debug_inverse_batch_shared",
    "acvm_batch_import_device", "acvm_batch_solve_then_import_ex",
    "acvm_batch_import_device_parts", "acvm_debug_import_list_copies",
    "acvm_batch_import_device_masked", "acvm_batch_set_initial_witness_masked", "acvm_debug_import_missing",
    "acvm_debug_table_info", "acvm_debug_table_read", "acvm_debug_batch_tables",
    "acvm_batch_outcomes_device", "acvm_batch_export_device_list", "acvm_debug_export_h2d_bytes", "acvm_debug_select",
    "acvm_node_solve_device", "acvm_debug_node_io_bytes",
    "acvm_batch_foreign_call_sites", "acvm_batch_foreign_call_inputs_device", "acvm_batch_resolve_foreign_calls_device", "acvm_debug_foreign_call_stats", "acvm_debug_brillig_resume_stats",
    "acvm_batch_resolve_foreign_calls_device_rows",
    "acvm_node_set_foreign_call_handler", "acvm_node_foreign_stats",
    "acvm_batch_import_device_records", "acvm_batch_set_initial_witness_records", "acvm_node_solve_records",
    "acvm_batch_export_device_records", "acvm_batch_witness_records",
    "acvm_batch_wire_bound", "acvm_batch_witness_maps_wire_device", "acvm_batch_witness_maps_wire",
    "acvm_batch_import_device_records_masked", "acvm_batch_set_initial_witness_records_masked", "acvm_debug_import_state",
    "acvm_debug_lin_add", "acvm_debug_lin_plan", "acvm_debug_bundle_plan",
    "acvm_batch_import_device_wire", "acvm_batch_set_initial_witness_maps_wire",
    "acvm_batch_import_device_wire_gzip", "acvm_batch_set_initial_witness_maps_gzip", "acvm_debug_inflate_rows",
    "acvm_batch_witness_maps_wire_packed_device", "acvm_batch_witness_maps_wire_packed", "acvm_batch_import_device_wire_packed", "acvm_debug_wire_repitch",
    "acvm_debug_gate_records", "acvm_debug_record_scratch",
]


class AcvmError(RuntimeError):
    pass


class ExpressionHead(C.Structure):
    _fields_ = [("n_mul", C.c_uint32), ("n_lin", C.c_uint32), ("opcode_index", C.c_uint32), ("q_c", C.c_uint8 * 32)]


class ExportDesc(C.Structure):
    """acvm_export_desc_t"""
    _fields_ = [("encoding", C.c_uint32), ("layout", C.c_uint32), ("first", C.c_uint32), ("n", C.c_uint32), ("witnesses", C.POINTER(C.c_uint32)),
                ("n_witnesses", C.c_uint32), ("stride", C.c_uint64)]


class OutcomesDesc(C.Structure):
    """acvm_outcomes_desc_t (the pointers are device addresses, 0 / None = NULL)"""
    _fields_ = [("first", C.c_uint32), ("n", C.c_uint32), ("d_status", C.c_void_p), ("d_err", C.c_void_p), ("d_opcode_index", C.c_void_p),
                ("select_mask", C.c_uint32), ("d_selected", C.c_void_p)]


class ImportDesc(C.Structure):
    """acvm_import_desc_t"""
    _fields_ = [("encoding", C.c_uint32), ("layout", C.c_uint32), ("columns", C.POINTER(C.c_uint32)), ("n_columns", C.c_uint32), ("stride", C.c_uint64)]


class ImportPart(C.Structure):
    """acvm_import_part_t"""
    _fields_ = [("d_values", C.c_void_p), ("encoding", C.c_uint32), ("layout", C.c_uint32), ("positions", C.POINTER(C.c_uint32)),
                ("columns", C.POINTER(C.c_uint32)), ("n", C.c_uint32), ("n_columns", C.c_uint32), ("stride", C.c_uint64)]


class RecordField(C.Structure):
    """acvm_record_field_t: initial witness `position` is the element of `encoding` at byte `offset` of every record (any alignment)"""
    _fields_ = [("position", C.c_uint32), ("encoding", C.c_uint32), ("offset", C.c_uint64)]


class RecordDesc(C.Structure):
    """acvm_record_desc_t"""
    _fields_ = [("pitch", C.c_uint64), ("fields", C.POINTER(RecordField)), ("n_fields", C.c_uint32)]


def record_desc(pitch, fields):
    """(RecordDesc, the array its field pointer refers to) from the bytes between two records and (position, encoding, offset) triples or
    RecordField objects"""
    fl = [f if isinstance(f, RecordField) else RecordField(*f) for f in fields]
    arr = (RecordField * max(len(fl), 1))(*fl)
    return RecordDesc(pitch=pitch, fields=arr, n_fields=len(fl)), arr


RECORD_NO_MASK = (1 << 64) - 1


class RecordOutField(C.Structure):
    """acvm_record_out_field_t: `witness` leaves as the element of `encoding` at byte `offset` of every record (any alignment), its mask byte at
    byte `mask_offset` (RECORD_NO_MASK: none)"""
    _fields_ = [("witness", C.c_uint32), ("encoding", C.c_uint32), ("offset", C.c_uint64), ("mask_offset", C.c_uint64)]


class RecordOutDesc(C.Structure):
    """acvm_record_out_desc_t"""
    _fields_ = [("pitch", C.c_uint64), ("fields", C.POINTER(RecordOutField)), ("n_fields", C.c_uint32), ("first", C.c_uint32), ("n", C.c_uint32)]


def record_out_desc(pitch, fields, first, n):
    """(RecordOutDesc, the array its field pointer refers to) from the bytes between two records and (witness, encoding, offset) or (witness,
    encoding, offset, mask_offset) tuples (mask_offset None: no mask byte) or RecordOutField objects"""
    fl = []
    for f in fields:
        if not isinstance(f, RecordOutField):
            f = tuple(f)
            f = RecordOutField(f[0], f[1], f[2], RECORD_NO_MASK if len(f) < 4 or f[3] is None else f[3])
        fl.append(f)
    arr = (RecordOutField * max(len(fl), 1))(*fl)
    return RecordOutDesc(pitch=pitch, fields=arr, n_fields=len(fl), first=first, n=n), arr


WIRE_BINCODE, WIRE_GZIP_STORED, WIRE_GZIP_DEFLATE = 0, 1, 8  # ACVM_WIRE_* (DEFLATE: export only; the value is gzip's CM byte)


class WireDesc(C.Structure):
    """acvm_wire_desc_t"""
    _fields_ = [("container", C.c_uint32), ("first", C.c_uint32), ("n", C.c_uint32), ("witnesses", C.POINTER(C.c_uint32)), ("n_witnesses", C.c_uint32),
                ("pitch", C.c_uint64)]


def wire_desc(container, first, n, witnesses=None, pitch=0):
    """(WireDesc, the array its witness pointer refers to); witnesses None: the whole map"""
    desc = WireDesc(container=container, first=first, n=n, pitch=pitch)
    arr = None
    if witnesses is not None:
        ws = list(witnesses)
        arr = (C.c_uint32 * max(len(ws), 1))(*ws)
        desc.witnesses, desc.n_witnesses = arr, len(ws)
    return desc, arr


class WireInDesc(C.Structure):
    """acvm_wire_in_desc_t"""
    _fields_ = [("container", C.c_uint32), ("pitch", C.c_uint64)]


class RecordMaskedField(C.Structure):
    """acvm_record_masked_field_t: RecordField with the byte `mask_offset` of the record saying whether the instance holds the element at all
    (1: yes, 0: no; RECORD_NO_MASK: always). The layout of RecordOutField, witness -> position."""
    _fields_ = [("position", C.c_uint32), ("encoding", C.c_uint32), ("offset", C.c_uint64), ("mask_offset", C.c_uint64)]


class RecordMaskedDesc(C.Structure):
    """acvm_record_masked_desc_t"""
    _fields_ = [("pitch", C.c_uint64), ("fields", C.POINTER(RecordMaskedField)), ("n_fields", C.c_uint32)]


def record_masked_desc(pitch, fields):
    """(RecordMaskedDesc, the array its field pointer refers to) from the bytes between two records and (position, encoding, offset) or (position,
    encoding, offset, mask_offset) tuples (mask_offset None: no mask byte) or RecordMaskedField objects"""
    fl = []
    for f in fields:
        if not isinstance(f, RecordMaskedField):
            f = tuple(f)
            f = RecordMaskedField(f[0], f[1], f[2], RECORD_NO_MASK if len(f) < 4 or f[3] is None else f[3])
        fl.append(f)
    arr = (RecordMaskedField * max(len(fl), 1))(*fl)
    return RecordMaskedDesc(pitch=pitch, fields=arr, n_fields=len(fl)), arr


def record_masked_fields_from_out(out_fields, position_of):
    """The masked import list of the next circuit from the field list of a record export: out_fields as record_out_desc takes them -- (witness,
    encoding, offset[, mask_offset]) -- and position_of {witness of the exporting circuit: position among the importing circuit's initial ids}.
    A field whose witness the map does not name is padding to the import; a witness exported in several fields is imported from the first."""
    fields, seen = [], set()
    for f in out_fields:
        f = (f.witness, f.encoding, f.offset, None if f.mask_offset == RECORD_NO_MASK else f.mask_offset) if isinstance(f, RecordOutField) else tuple(f)
        if f[0] in position_of and f[0] not in seen:
            seen.add(f[0])
            fields.append((position_of[f[0]], f[1], f[2], f[3] if len(f) > 3 else None))
    return fields


def record_fields_from_dtype(dtype, positions):
    """The (pitch, fields) of a numpy structured dtype, as record_desc and the *_records calls take them. positions: {field name: position, list
    of positions, or (positions, encoding)}. A field's bytes are divided evenly among its positions, in order: ("msg", np.uint8, 64) with 64
    positions is 64 ENC_U8 elements, ("root", "V32") with one position one 32-byte element. The element's width chooses the encoding -- 1, 2, 4,
    8, 16 bytes: ENC_U8 .. ENC_U128, 32 bytes: ENC_BE32 -- unless one is given. Names that positions does not list are padding."""
    import numpy as np
    dtype = np.dtype(dtype)
    by_size = {1: ENC_U8, 2: ENC_U16, 4: ENC_U32, 8: ENC_U64, 16: ENC_U128, 32: ENC_BE32}
    fields = []
    for name, want in positions.items():
        sub, offset = dtype.fields[name][0], dtype.fields[name][1]
        encoding = None
        if isinstance(want, tuple):
            want, encoding = want
        plist = [want] if isinstance(want, int) else list(want)
        if not plist or sub.itemsize % len(plist):
            raise ValueError(f"field {name}: {sub.itemsize} bytes do not divide among {len(plist)} positions")
        size = sub.itemsize // len(plist)
        if encoding is None:
            if size not in by_size:
                raise ValueError(f"field {name}: no encoding for elements of {size} bytes")
            encoding = by_size[size]
        if element_size(encoding) != size:
            raise ValueError(f"field {name}: the encoding takes {element_size(encoding)} bytes, an element of the field has {size}")
        fields += [(pos, encoding, offset + k * size) for k, pos in enumerate(plist)]
    return dtype.itemsize, fields


class NodeLaneIo(C.Structure):
    """acvm_node_lane_io_t (the d_* fields are device addresses, 0 / None = NULL)"""
    _fields_ = [("n", C.c_uint64), ("d_values", C.c_void_p), ("in_", ImportDesc), ("d_kept", C.c_void_p), ("d_kept_assigned", C.c_void_p),
                ("kept_encoding", C.c_uint32), ("kept_layout", C.c_uint32), ("kept_stride", C.c_uint64), ("d_status", C.c_void_p), ("d_err", C.c_void_p),
                ("d_opcode_index", C.c_void_p), ("d_digests32", C.c_void_p), ("select_mask", C.c_uint32), ("d_selected", C.c_void_p),
                ("n_selected", C.c_uint64), ("not_solved", C.c_uint64)]


class ForeignCallSite(C.Structure):
    """acvm_foreign_call_site_t"""
    _fields_ = [("opcode_index", C.c_uint32), ("brillig_index", C.c_uint32), ("n_inputs", C.c_uint32), ("n_waiting", C.c_uint32), ("n_resolved", C.c_uint32),
                ("function", C.c_char * 64)]


class ForeignCallInputsDesc(C.Structure):
    """acvm_foreign_call_inputs_desc_t (the d_* fields are device addresses, 0 / None = NULL)"""
    _fields_ = [("opcode_index", C.c_uint32), ("brillig_index", C.c_uint32), ("first_row", C.c_uint32), ("n_rows", C.c_uint32), ("encoding", C.c_uint32),
                ("layout", C.c_uint32), ("n_columns", C.c_uint32), ("stride", C.c_uint64), ("d_instances", C.c_void_p), ("d_lens", C.c_void_p),
                ("d_values", C.c_void_p), ("d_mask", C.c_void_p)]


class ForeignCallAnswersDesc(C.Structure):
    """acvm_foreign_call_answers_desc_t"""
    _fields_ = [("opcode_index", C.c_uint32), ("brillig_index", C.c_uint32), ("first_row", C.c_uint32), ("n_rows", C.c_uint32), ("n_values", C.c_uint32),
                ("is_array", C.c_char_p), ("lens", C.POINTER(C.c_uint32)), ("encoding", C.c_uint32), ("layout", C.c_uint32), ("n_columns", C.c_uint32),
                ("stride", C.c_uint64), ("d_values", C.c_void_p)]


class ForeignCallAnswersRowsDesc(C.Structure):
    """acvm_foreign_call_answers_rows_desc_t"""
    _fields_ = ForeignCallAnswersDesc._fields_ + [("d_lens", C.c_void_p), ("d_answered", C.c_void_p)]


SPACE_DEVICE, SPACE_HOST = 0, 1


class NodeForeignRound(C.Structure):
    """acvm_node_foreign_round_t (rows, lens, values and mask are addresses in the handler's memory space)"""
    _fields_ = [("lane", C.c_uint32), ("device", C.c_int), ("tile", C.c_uint32), ("round", C.c_uint32), ("site", ForeignCallSite), ("n_rows", C.c_uint32),
                ("max_values", C.c_uint32), ("row_base", C.c_uint64), ("rows", C.c_void_p), ("lens", C.c_void_p), ("values", C.c_void_p), ("mask", C.c_void_p)]


class NodeForeignAnswer(C.Structure):
    """acvm_node_foreign_answer_t"""
    _fields_ = [("n_values", C.c_uint32), ("is_array", C.c_void_p), ("lens", C.c_void_p), ("encoding", C.c_uint32), ("layout", C.c_uint32), ("n_columns", C.c_uint32),
                ("stride", C.c_uint64), ("values", C.c_void_p), ("row_lens", C.c_void_p), ("answered", C.c_void_p)]


_NODE_FOREIGN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(NodeForeignRound), C.POINTER(NodeForeignAnswer))


class NodeForeignHandler(C.Structure):
    """acvm_node_foreign_handler_t"""
    _fields_ = [("fn", _NODE_FOREIGN_FN), ("user", C.c_void_p), ("space", C.c_uint32), ("in_encoding", C.c_uint32), ("in_layout", C.c_uint32), ("max_rounds", C.c_uint32)]


class NodeForeignStats(C.Structure):
    """acvm_node_foreign_stats_t"""
    _fields_ = [("rounds", C.c_uint32), ("handler_calls", C.c_uint32), ("rows_answered", C.c_uint64), ("rows_declined", C.c_uint64), ("rows_left_waiting", C.c_uint64),
                ("handler_ms", C.c_double), ("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64)]


class ForeignRound:
    """What a node's foreign-call handler is asked (acvm_node_foreign_round_t): lane, device, tile, round, opcode_index, brillig_index, function, n_inputs,
    n_rows, max_values, row_base, in_encoding, in_layout, space, and the addresses rows, lens, values, mask -- device addresses for SPACE_DEVICE (the
    lane's device is current: device_download reads them), host addresses for SPACE_HOST, which rows_list / lens_list / values_bytes / mask_bytes read."""

    def __init__(self, r, space, in_encoding, in_layout):
        self.lane, self.device, self.tile, self.round = r.lane, r.device, r.tile, r.round
        self.opcode_index, self.brillig_index, self.n_inputs, self.function = r.site.opcode_index, r.site.brillig_index, r.site.n_inputs, r.site.function.decode()
        self.n_rows, self.max_values, self.row_base = r.n_rows, r.max_values, r.row_base
        self.rows, self.lens, self.values, self.mask = r.rows, r.lens, r.values, r.mask
        self.space, self.in_encoding, self.in_layout = space, in_encoding, in_layout

    def _read(self, ptr, size):
        if not size:
            return b""
        return C.string_at(ptr, size) if self.space == SPACE_HOST else device_download(ptr, size)

    def rows_list(self):
        """the rows' instance numbers inside the tile, ascending; the caller's number of row i is row_base + rows_list()[i]"""
        return list(memoryview(self._read(self.rows, 4 * self.n_rows)).cast("I"))

    def lens_list(self):
        flat = list(memoryview(self._read(self.lens, 4 * self.n_rows * self.n_inputs)).cast("I"))
        return [flat[i * self.n_inputs:(i + 1) * self.n_inputs] for i in range(self.n_rows)]

    def values_bytes(self) -> bytes:
        return self._read(self.values, self.n_rows * self.max_values * element_size(self.in_encoding))

    def mask_bytes(self) -> bytes:
        return self._read(self.mask, self.n_rows * self.max_values)


def device_download(ptr: int, size: int) -> bytes:
    """`size` bytes at a device address of the current device (acvm_device_download)"""
    out = C.create_string_buffer(max(size, 1))
    _check(lib().acvm_device_download(out, ptr, size))
    return out.raw[:size]


def element_size(encoding):
    """bytes per element of an ACVM_ENC_*: 32, or the width of a narrow integer"""
    return 1 << (encoding - ENC_U8) if ENC_U8 <= encoding <= ENC_U128 else 32


class Result(C.Structure):
    _fields_ = [("status", C.c_uint32), ("err", C.c_uint32), ("opcode_index", C.c_uint32), ("aux0", C.c_uint32),
                ("aux1", C.c_uint32), ("n_call_stack", C.c_uint32), ("call_stack", C.c_uint32 * 16),
                ("message", C.c_char * 200)]

    def as_tuple(self):
        return (self.status, self.err, self.opcode_index, self.aux0, self.aux1)


_SCHNORR_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8),
                          C.c_size_t, C.POINTER(C.c_uint8), C.c_void_p, C.c_size_t)
_PEDERSEN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                           C.c_void_p, C.c_size_t)
_FIXED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_void_p,
                        C.c_size_t)


_SCHNORR_BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t,
                                C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_void_p, C.c_size_t)
_PEDERSEN_BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.c_uint32, C.POINTER(C.c_uint8),
                                 C.POINTER(C.c_uint8), C.c_void_p, C.c_size_t)
_FIXED_BATCH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_void_p, C.c_size_t)


class BbSolver(C.Structure):
    """acvm_bb_solver_t: the BlackBoxFunctionSolver trait (blackbox_solver/src/lib.rs:27-45) as a vtable; the *_batch members
    are optional (NULL: the per-instance functions are called once per instance)."""
    _fields_ = [("ctx", C.c_void_p), ("schnorr_verify", _SCHNORR_FN), ("pedersen", _PEDERSEN_FN), ("fixed_base_scalar_mul", _FIXED_FN),
                ("schnorr_verify_batch", _SCHNORR_BATCH_FN), ("pedersen_batch", _PEDERSEN_BATCH_FN), ("fixed_base_scalar_mul_batch", _FIXED_BATCH_FN)]


def make_solver(schnorr_verify, pedersen, fixed_base_scalar_mul):
    """Wrap three Python callables as an acvm_bb_solver_t.
    schnorr_verify(pkx: int, pky: int, sig: bytes, msg: bytes) -> bool
    pedersen(inputs: list[int], domain_separator: int) -> (x, y)
    fixed_base_scalar_mul(low: int, high: int) -> (x, y)
    Raising BlackBoxFailed(msg) reports BlackBoxResolutionError::Failed, BlackBoxUnsupported reports Unsupported."""
    def be(ptr, n=32):
        return int.from_bytes(bytes(ptr[:n]), "big")

    def put(ptr, v):
        for i, byte in enumerate(int(v).to_bytes(32, "big")):
            ptr[i] = byte

    def guard(fn, err, err_len):
        try:
            fn()
            return 0
        except BlackBoxFailed as e:
            msg = str(e).encode()[: max(err_len - 1, 0)]
            if err:
                C.memmove(err, msg + b"\0", len(msg) + 1)
            return 1
        except BlackBoxUnsupported:
            return 2

    def c_schnorr(ctx, pkx, pky, sig, sig_len, msg, msg_len, ok, err, err_len):
        def run():
            ok[0] = 1 if schnorr_verify(be(pkx), be(pky), bytes(sig[:sig_len]), bytes(msg[:msg_len])) else 0
        return guard(run, err, err_len)

    def c_pedersen(ctx, inputs, n, ds, x, y, err, err_len):
        def run():
            vals = [int.from_bytes(bytes(inputs[32 * i:32 * i + 32]), "big") for i in range(n)]
            rx, ry = pedersen(vals, ds)
            put(x, rx)
            put(y, ry)
        return guard(run, err, err_len)

    def c_fixed(ctx, low, high, x, y, err, err_len):
        def run():
            rx, ry = fixed_base_scalar_mul(be(low), be(high))
            put(x, rx)
            put(y, ry)
        return guard(run, err, err_len)

    s = BbSolver(None, _SCHNORR_FN(c_schnorr), _PEDERSEN_FN(c_pedersen), _FIXED_FN(c_fixed))
    return s


def make_batched_solver(pedersen_batch=None, fixed_base_batch=None, schnorr_batch=None, fallback: "BbSolver" = None):
    """An acvm_bb_solver_t whose *_batch members are Python callables over the whole batch (one call per opcode):
    pedersen_batch(inputs: list[list[int]], domain_separator) -> list[(x, y)]
    fixed_base_batch(pairs: list[(low, high)]) -> list[(x, y)]
    schnorr_batch(items: list[(pkx, pky, sig: bytes, msg: bytes)]) -> list[bool]
    The per-instance members come from `fallback` (default: the stubbed vtable, so a missing batch member panics)."""
    fb = fallback if fallback is not None else bb_stubbed()

    def put(ptr, off, v):
        for i, byte in enumerate(int(v).to_bytes(32, "big")):
            ptr[off + i] = byte

    def c_ped(ctx, n, inputs, k, ds, xy, rc, err, stride):
        rows = [[int.from_bytes(bytes(inputs[(q * k + i) * 32:(q * k + i + 1) * 32]), "big") for i in range(k)] for q in range(n)]
        for q, (x, y) in enumerate(pedersen_batch(rows, ds)):
            put(xy, 64 * q, x)
            put(xy, 64 * q + 32, y)
            rc[q] = 0
        return 0

    def c_fixed(ctx, n, lh, xy, rc, err, stride):
        pairs = [(int.from_bytes(bytes(lh[64 * q:64 * q + 32]), "big"), int.from_bytes(bytes(lh[64 * q + 32:64 * q + 64]), "big")) for q in range(n)]
        for q, (x, y) in enumerate(fixed_base_batch(pairs)):
            put(xy, 64 * q, x)
            put(xy, 64 * q + 32, y)
            rc[q] = 0
        return 0

    def c_schnorr(ctx, n, pk, sig, sig_len, msg, msg_len, ok, rc, err, stride):
        items = [(int.from_bytes(bytes(pk[64 * q:64 * q + 32]), "big"), int.from_bytes(bytes(pk[64 * q + 32:64 * q + 64]), "big"),
                  bytes(sig[q * sig_len:(q + 1) * sig_len]), bytes(msg[q * msg_len:(q + 1) * msg_len])) for q in range(n)]
        for q, v in enumerate(schnorr_batch(items)):
            ok[q] = 1 if v else 0
            rc[q] = 0
        return 0

    s = BbSolver(None, fb.schnorr_verify, fb.pedersen, fb.fixed_base_scalar_mul,
                 _SCHNORR_BATCH_FN(c_schnorr) if schnorr_batch else _SCHNORR_BATCH_FN(), _PEDERSEN_BATCH_FN(c_ped) if pedersen_batch else _PEDERSEN_BATCH_FN(),
                 _FIXED_BATCH_FN(c_fixed) if fixed_base_batch else _FIXED_BATCH_FN())
    s._keep = fb
    return s


def bb_stubbed() -> "BbSolver":
    """StubbedBackend (acvm/tests/solver.rs:20-46) as shipped by the library."""
    return C.cast(lib().acvm_bb_stubbed(), C.POINTER(BbSolver)).contents


def bb_dummy() -> "BbSolver":
    """DummyBlackBoxSolver (brillig_vm/src/lib.rs:392-420) as shipped by the library."""
    return C.cast(lib().acvm_bb_dummy(), C.POINTER(BbSolver)).contents


class BlackBoxFailed(Exception):
    pass


class BlackBoxUnsupported(Exception):
    pass


class ForeignCallInfo(C.Structure):
    _fields_ = [("opcode_index", C.c_uint32), ("brillig_index", C.c_uint32), ("n_inputs", C.c_uint32), ("n_values", C.c_uint32),
                ("function", C.c_char * 64)]


class Stats(C.Structure):
    _fields_ = [("n_opcodes", C.c_uint32), ("n_witnesses", C.c_uint32), ("n_levels", C.c_uint32),
                ("n_fast_gates", C.c_uint32), ("n_dyn_gates", C.c_uint32), ("max_level_width", C.c_uint32),
                ("n_kernel_launches", C.c_uint32), ("n_slow_instances", C.c_uint32),
                ("algorithmic_bytes_per_instance", C.c_uint64), ("arith_algorithmic_bytes_per_instance", C.c_uint64),
                ("plan_ms", C.c_double), ("solve_device_ms", C.c_double), ("arith_kernel_ms", C.c_double),
                ("slow_path_ms", C.c_double), ("dyn_kernel_ms", C.c_double),
                ("dyn_algorithmic_bytes_per_instance", C.c_uint64), ("n_other_records", C.c_uint32), ("truncated_at", C.c_uint32),
                ("class_algorithmic_bytes_per_instance", C.c_uint64 * 4), ("class_kernel_ms", C.c_double * 4),
                ("n_gate_pairs", C.c_uint32), ("n_inverse_slots", C.c_uint32),
                ("n_scaled_witnesses", C.c_uint32), ("n_arith_launches", C.c_uint32),
                ("n_table_rows", C.c_uint32), ("n_digest_segments", C.c_uint32), ("n_brillig_inlined", C.c_uint32), ("n_brillig_retries", C.c_uint32),
                ("n_hash_chained", C.c_uint32),
                ("n_gate_out_asis", C.c_uint32), ("n_gate_out_weak", C.c_uint32), ("n_gate_out_canon", C.c_uint32), ("max_gate_bound", C.c_uint32),
                ("n_byte_planes", C.c_uint32), ("n_byte_plane_reads", C.c_uint32),
                ("n_stream_launches", C.c_uint32 * 6), ("n_stream_waits", C.c_uint32)]

    def as_dict(self):
        return {f: (list(getattr(self, f)) if f.startswith("class_") or f == "n_stream_launches" else getattr(self, f)) for f, _ in self._fields_}


_lib = None


def lib():
    """Load libacvm_amd.so. Raises if it has not been built (python -m acvm_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AcvmError(f"{LIB_PATH} is missing: build it with `python -m acvm_amd.build` (no CPU fallback exists)")
    L = C.CDLL(LIB_PATH)
    L.acvm_last_error.restype = C.c_char_p
    L.acvm_device_arch.argtypes = [C.c_char_p, C.c_size_t]
    L.acvm_selftest.argtypes = [C.c_uint32, C.c_uint64]
    L.acvm_debug_grumpkin.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p]
    if hasattr(L, "acvm_debug_grumpkin_items"):  # (an older build loaded through ACVM_AMD_LIB for an A/B run has no such probe)
        L.acvm_debug_grumpkin_items.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    if hasattr(L, "acvm_debug_secp"):  # (an older build loaded through ACVM_AMD_LIB for an A/B run has no such probe)
        L.acvm_debug_secp.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p]
    L.acvm_circuit_from_bytes.restype = C.c_void_p
    L.acvm_circuit_from_bytes.argtypes = [C.c_char_p, C.c_size_t]
    L.acvm_circuit_free.argtypes = [C.c_void_p]
    L.acvm_circuit_num_opcodes.restype = C.c_uint32
    L.acvm_circuit_num_opcodes.argtypes = [C.c_void_p]
    L.acvm_circuit_num_witnesses.restype = C.c_uint32
    L.acvm_circuit_num_witnesses.argtypes = [C.c_void_p]
    L.acvm_circuit_plan_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(Stats)]
    L.acvm_circuit_plan_stats_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(Stats)]
    L.acvm_debug_plan_fingerprint.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32]
    L.acvm_debug_gate_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.acvm_debug_record_scratch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.acvm_circuit_plans_built.restype = C.c_uint64
    L.acvm_circuit_plans_built.argtypes = [C.c_void_p]
    L.acvm_circuit_check_schedule.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
    if hasattr(L, "acvm_debug_bundle_plan"):  # (likewise)
        L.acvm_debug_bundle_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    if hasattr(L, "acvm_debug_lin_plan"):  # (an older build loaded through ACVM_AMD_LIB for an A/B run has neither)
        L.acvm_debug_lin_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_char_p, C.c_size_t]
        L.acvm_debug_lin_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.acvm_batch_new.restype = C.c_void_p
    L.acvm_batch_new.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.acvm_batch_new_ex.restype = C.c_void_p
    L.acvm_batch_new_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
    L.acvm_batch_free.argtypes = [C.c_void_p]
    L.acvm_batch_set_initial_witness.argtypes = [C.c_void_p, C.c_void_p]
    L.acvm_batch_set_initial_witness_device.argtypes = [C.c_void_p, C.c_void_p]
    L.acvm_batch_solve.argtypes = [C.c_void_p]
    L.acvm_batch_solve_then_import.argtypes = [C.c_void_p, C.c_void_p]
    L.acvm_batch_reset.argtypes = [C.c_void_p]
    L.acvm_batch_set_instances.argtypes = [C.c_void_p, C.c_uint32]
    L.acvm_batch_set_force_slow_path.argtypes = [C.c_void_p, C.c_int]
    L.acvm_batch_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.acvm_batch_results.argtypes = [C.c_void_p, C.c_void_p]
    L.acvm_batch_witness.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.acvm_batch_witness_map.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.acvm_batch_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.acvm_batch_pending_foreign_call.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(ForeignCallInfo)]
    L.acvm_batch_pending_foreign_call_inputs.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.acvm_batch_resolve_foreign_call.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p, C.c_char_p]
    L.acvm_circuit_assert_message.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
    L.acvm_circuit_witness_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
    L.acvm_batch_error_string.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]
    L.acvm_batch_extract_witnesses.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.acvm_batch_digest.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.acvm_batch_digest_blake2s.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    for f in (L.acvm_witness_map_decode, L.acvm_witness_map_encode, L.acvm_batch_witness_map_bytes):
        f.restype = C.c_longlong
    L.acvm_witness_map_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32]
    L.acvm_witness_map_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_size_t]
    L.acvm_batch_witness_map_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
    L.acvm_debug_modmul_rate.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    if hasattr(L, "acvm_debug_fr"):  # (an older build loaded through ACVM_AMD_LIB for an A/B run has no such probes)
        L.acvm_debug_fr.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.acvm_debug_inverse_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint32)]
    if hasattr(L, "acvm_debug_inverse_batch_shared"):
        L.acvm_debug_inverse_batch_shared.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.acvm_debug_secp_rate.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.acvm_circuit_opcode_kinds.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.acvm_batch_error_expression.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ExpressionHead), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    L.acvm_device_release_tables.restype = C.c_longlong
    L.acvm_device_release_tables.argtypes = [C.c_int]
    L.acvm_node_new.restype = C.c_void_p
    L.acvm_node_new.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.acvm_node_free.restype = None
    L.acvm_node_free.argtypes = [C.c_void_p]
    L.acvm_node_tile_instances.argtypes = [C.c_void_p]
    L.acvm_node_tile_instances.restype = C.c_uint32
    L.acvm_node_num_devices.argtypes = [C.c_void_p]
    L.acvm_node_num_devices.restype = C.c_uint32
    L.acvm_node_solve.restype = C.c_longlong
    L.acvm_node_solve.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.acvm_node_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.acvm_debug_stream_rate.argtypes = [C.c_size_t, C.POINTER(C.c_double)]
    L.acvm_tuning_set.argtypes = [C.c_char_p, C.c_longlong]
    L.acvm_tuning_get.argtypes = [C.c_char_p, C.POINTER(C.c_longlong)]
    L.acvm_tuning_key.restype = C.c_char_p
    L.acvm_tuning_key.argtypes = [C.c_uint]
    L.acvm_device_malloc.restype = C.c_void_p
    L.acvm_device_malloc.argtypes = [C.c_size_t]
    L.acvm_device_free.argtypes = [C.c_void_p]
    L.acvm_device_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.acvm_device_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.acvm_batch_export_device.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.c_void_p, C.c_void_p]
    if hasattr(L, "acvm_batch_import_device"):  # (an older build loaded through ACVM_AMD_LIB for an A/B run has neither)
        L.acvm_batch_import_device.argtypes = [C.c_void_p, C.POINTER(ImportDesc), C.c_void_p]
        L.acvm_batch_solve_then_import_ex.argtypes = [C.c_void_p, C.POINTER(ImportDesc), C.c_void_p]
    if hasattr(L, "acvm_batch_import_device_parts"):
        L.acvm_batch_import_device_parts.argtypes = [C.c_void_p, C.POINTER(ImportPart), C.c_uint32]
        L.acvm_debug_import_list_copies.restype = C.c_uint64
        L.acvm_debug_import_list_copies.argtypes = [C.c_void_p]
    if hasattr(L, "acvm_batch_import_device_masked"):
        L.acvm_batch_import_device_masked.argtypes = [C.c_void_p, C.POINTER(ImportDesc), C.c_void_p, C.c_void_p]
        L.acvm_batch_set_initial_witness_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.acvm_debug_import_missing.restype = C.c_uint64
        L.acvm_debug_import_missing.argtypes = [C.c_void_p]
    if hasattr(L, "acvm_batch_import_device_records"):
        L.acvm_batch_import_device_records.argtypes = [C.c_void_p, C.POINTER(RecordDesc), C.c_void_p]
        L.acvm_batch_set_initial_witness_records.argtypes = [C.c_void_p, C.POINTER(RecordDesc), C.c_void_p]
        L.acvm_node_solve_records.restype = C.c_longlong
        L.acvm_node_solve_records.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(RecordDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "acvm_batch_import_device_records_masked"):
        L.acvm_batch_import_device_records_masked.argtypes = [C.c_void_p, C.POINTER(RecordMaskedDesc), C.c_void_p]
        L.acvm_batch_set_initial_witness_records_masked.argtypes = [C.c_void_p, C.POINTER(RecordMaskedDesc), C.c_void_p]
        L.acvm_debug_import_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "acvm_batch_export_device_records"):
        L.acvm_batch_export_device_records.argtypes = [C.c_void_p, C.POINTER(RecordOutDesc), C.c_void_p, C.c_void_p]
        L.acvm_batch_witness_records.argtypes = [C.c_void_p, C.POINTER(RecordOutDesc), C.c_void_p]
    if hasattr(L, "acvm_batch_wire_bound"):
        L.acvm_batch_wire_bound.restype = C.c_longlong
        L.acvm_batch_wire_bound.argtypes = [C.c_void_p, C.POINTER(WireDesc)]
        L.acvm_batch_witness_maps_wire_device.argtypes = [C.c_void_p, C.POINTER(WireDesc), C.c_void_p, C.c_void_p, C.c_void_p]
        L.acvm_batch_witness_maps_wire.argtypes = [C.c_void_p, C.POINTER(WireDesc), C.c_void_p, C.c_void_p]
    if hasattr(L, "acvm_batch_import_device_wire"):
        L.acvm_batch_import_device_wire.argtypes = [C.c_void_p, C.POINTER(WireInDesc), C.c_void_p, C.c_void_p]
        L.acvm_batch_set_initial_witness_maps_wire.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    if hasattr(L, "acvm_batch_import_device_wire_gzip"):
        L.acvm_batch_import_device_wire_gzip.argtypes = [C.c_void_p, C.POINTER(WireInDesc), C.c_void_p, C.c_void_p]
        L.acvm_batch_set_initial_witness_maps_gzip.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.acvm_debug_inflate_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "acvm_batch_witness_maps_wire_packed_device"):
        L.acvm_batch_witness_maps_wire_packed_device.argtypes = [C.c_void_p, C.POINTER(WireDesc), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.acvm_batch_witness_maps_wire_packed.argtypes = [C.c_void_p, C.POINTER(WireDesc), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.acvm_batch_import_device_wire_packed.argtypes = [C.c_void_p, C.POINTER(WireInDesc), C.c_void_p, C.c_uint64, C.c_void_p]
        L.acvm_debug_wire_repitch.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32,
                                              C.c_void_p, C.c_void_p]
    if hasattr(L, "acvm_batch_outcomes_device"):
        L.acvm_batch_outcomes_device.argtypes = [C.c_void_p, C.POINTER(OutcomesDesc), C.POINTER(C.c_uint32)]
        L.acvm_batch_export_device_list.argtypes = [C.c_void_p, C.POINTER(ExportDesc), C.c_void_p, C.c_void_p, C.c_void_p]
        L.acvm_debug_export_h2d_bytes.restype = C.c_uint64
        L.acvm_debug_export_h2d_bytes.argtypes = [C.c_void_p]
        L.acvm_debug_select.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
    if hasattr(L, "acvm_node_solve_device"):
        L.acvm_node_solve_device.restype = C.c_longlong
        L.acvm_node_solve_device.argtypes = [C.c_void_p, C.POINTER(NodeLaneIo), C.c_uint32]
        L.acvm_debug_node_io_bytes.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(L, "acvm_batch_foreign_call_sites"):
        L.acvm_batch_foreign_call_sites.argtypes = [C.c_void_p, C.POINTER(ForeignCallSite), C.c_uint32]
        L.acvm_batch_foreign_call_inputs_device.argtypes = [C.c_void_p, C.POINTER(ForeignCallInputsDesc), C.POINTER(C.c_uint32)]
        L.acvm_batch_resolve_foreign_calls_device.argtypes = [C.c_void_p, C.POINTER(ForeignCallAnswersDesc)]
        L.acvm_debug_foreign_call_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                     C.POINTER(C.c_uint64)]
    if hasattr(L, "acvm_debug_brillig_resume_stats"):
        L.acvm_debug_brillig_resume_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    if hasattr(L, "acvm_batch_resolve_foreign_calls_device_rows"):
        L.acvm_batch_resolve_foreign_calls_device_rows.argtypes = [C.c_void_p, C.POINTER(ForeignCallAnswersRowsDesc)]
    if hasattr(L, "acvm_node_set_foreign_call_handler"):
        L.acvm_node_set_foreign_call_handler.argtypes = [C.c_void_p, C.POINTER(NodeForeignHandler)]
        L.acvm_node_foreign_stats.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(NodeForeignStats)]
    if hasattr(L, "acvm_debug_table_read"):
        L.acvm_debug_table_info.argtypes = [C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.acvm_debug_table_read.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.acvm_debug_batch_tables.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.acvm_batch_solve_opcode.argtypes = [C.c_void_p]
    L.acvm_bb_stubbed.restype = C.c_void_p
    L.acvm_bb_dummy.restype = C.c_void_p
    L.acvm_new.restype = C.c_void_p
    L.acvm_new.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32]
    for f in (L.acvm_free, L.acvm_solve, L.acvm_solve_opcode):
        f.argtypes = [C.c_void_p]
    L.acvm_free.restype = None
    L.acvm_get_status.argtypes = [C.c_void_p, C.POINTER(Result)]
    L.acvm_instruction_pointer.restype = C.c_uint32
    L.acvm_instruction_pointer.argtypes = [C.c_void_p]
    for f in (L.acvm_witness_map, L.acvm_finalize):
        f.restype = C.c_longlong
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.acvm_get_pending_foreign_call.argtypes = [C.c_void_p, C.POINTER(ForeignCallInfo)]
    L.acvm_pending_foreign_call_inputs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.acvm_resolve_pending_foreign_call.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_char_p]
    L.acvm_multi_new.restype = C.c_void_p
    L.acvm_multi_new.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p]
    L.acvm_multi_free.restype = None
    L.acvm_multi_free.argtypes = [C.c_void_p]
    L.acvm_multi_num_groups.restype = C.c_uint32
    L.acvm_multi_num_groups.argtypes = [C.c_void_p]
    L.acvm_multi_num_witnesses.restype = C.c_uint32
    L.acvm_multi_num_witnesses.argtypes = [C.c_void_p]
    L.acvm_multi_solve.argtypes = [C.c_void_p]
    L.acvm_multi_results.argtypes = [C.c_void_p, C.c_void_p]
    L.acvm_multi_witness_map.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.acvm_multi_locate.restype = C.c_void_p
    L.acvm_multi_locate.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        raise AcvmError(f"acvm_amd error {rc}: {lib().acvm_last_error().decode()}")
    return rc


def device_count():
    return lib().acvm_device_count()


_current_device = 0


def set_device(i):
    """hipSetDevice for the calling thread (HIP's current device is per thread: helper threads call this with current_device())"""
    global _current_device
    _check(lib().acvm_set_device(i))
    _current_device = i


def current_device():
    return _current_device


def synchronize():
    _check(lib().acvm_device_synchronize())


def selftest(n=1 << 16, seed=1):
    return _check(lib().acvm_selftest(n, seed))


def parse_cpulist(text):
    """a sysfs cpulist ("0-15,32-47") as the node driver reads it (host only)"""
    buf = (C.c_uint32 * 4096)()
    n = lib().acvm_debug_cpulist(text.encode(), buf, 4096)
    _check(n)
    return list(buf[:min(n, 4096)])


def device_locality(pci_root, bus_id):
    """(NUMA node, local CPUs) of a PCI device from a sysfs-shaped tree (host only): what a lane of the node driver pins its threads to"""
    buf = (C.c_uint32 * 4096)()
    node = C.c_int(-1)
    n = lib().acvm_debug_device_locality(pci_root.encode(), bus_id.encode(), C.byref(node), buf, 4096)
    _check(n)
    return node.value, list(buf[:min(n, 4096)])


def tuning_keys():
    """every planner / scheduler mode and device limit of the library (csrc/tuning.hpp)"""
    out, i = [], 0
    while True:
        k = lib().acvm_tuning_key(i)
        if not k:
            return out
        out.append(k.decode())
        i += 1


def tuning_get(key):
    v = C.c_longlong()
    _check(lib().acvm_tuning_get(key.encode(), C.byref(v)))
    return v.value


def tuning_set(key, value):
    _check(lib().acvm_tuning_set(key.encode(), int(value)))


class tuning:
    """with acvm_amd.tuning(scale=0, pairs=0): ... -- the modes hold for batches CREATED inside the block"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: tuning_get(k) for k in self.kv}
        for k, v in self.kv.items():
            tuning_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            tuning_set(k, v)
        return False


def release_tables(device=0):
    """acvm_device_release_tables: frees the lookup tables of `device` (bytes given back); AcvmError while a handle of the device still uses them"""
    r = lib().acvm_device_release_tables(device)
    if r < 0:
        raise AcvmError(lib().acvm_last_error().decode())
    return r


def stream_rate(nbytes=4 << 30):
    """GB/s moved by a two-rows-in, one-row-out stream of nbytes per row (the gate kernel's access shape): the measured streaming ceiling
    beside the spec peak of the HBM roofline"""
    r = C.c_double()
    _check(lib().acvm_debug_stream_rate(nbytes, C.byref(r)))
    return r.value


def modmul_rate(iters=400, waves_per_simd=8):
    """(modmul/s, products per launch) of the back-to-back fr29_mul probe: the peak of the ALU roofline"""
    r, n = C.c_double(), C.c_uint64()
    _check(lib().acvm_debug_modmul_rate(iters, waves_per_simd, C.byref(r), C.byref(n)))
    return r.value, n.value


def secp_rate(curve, iters=400, waves_per_simd=8):
    """(products/s, products per launch) of the back-to-back sp_mul / sp_sqr probe of secp256k1 (0) / secp256r1 (1): the peak of the ECDSA kernels' ALU roofline"""
    r, n = C.c_double(), C.c_uint64()
    _check(lib().acvm_debug_secp_rate(curve, iters, waves_per_simd, C.byref(r), C.byref(n)))
    return r.value, n.value


def modmul_probe_cus():
    """compute units the probe's grid is sized by (blocks = CUs x waves_per_simd): products per launch / (256 x waves x iters x 2)"""
    _, n = modmul_rate(1, 1)
    return n // 512


def device_arch():
    buf = C.create_string_buffer(64)
    _check(lib().acvm_device_arch(buf, 64))
    return buf.value.decode()


def debug_grumpkin(what, param, inputs=()):
    """Component probe of the Grumpkin kernels (see include/acvm_amd.h); returns (x, y) as ints."""
    out = C.create_string_buffer(64)
    data = b"".join(int(v).to_bytes(32, "big") for v in inputs)
    _check(lib().acvm_debug_grumpkin(what, param, data, len(inputs), out))
    return int.from_bytes(out.raw[:32], "big"), int.from_bytes(out.raw[32:], "big")


# acvm_debug_grumpkin_items: u32 words per item (in, out) of every `what` (acvm_amd/csrc/kernels_grumpkin.hip grumpkin_items_words)
GRUMPKIN_ITEM_WORDS = ((27, 27), (45, 36), (54, 27), (27, 17), (8, 62), (8, 17), (32, 17), (32, 17))


def debug_grumpkin_items(what, items, param=0):
    """One routine of the Grumpkin device header per call, one device lane per item (see include/acvm_amd.h): items = an array [n][words in] of raw u32
    words; returns the raw result words as a uint32 array [n][words out]."""
    import numpy as np
    if not 0 <= what < len(GRUMPKIN_ITEM_WORDS):
        _check(lib().acvm_debug_grumpkin_items(what, param, None, 0, None))
    wi, wo = GRUMPKIN_ITEM_WORDS[what]
    a = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1, wi)
    out = np.zeros((a.shape[0], wo), dtype=np.uint32)
    _check(lib().acvm_debug_grumpkin_items(what, param, a.ctypes.data, a.shape[0], out.ctypes.data))
    return out


# acvm_debug_table_info / _read: the lookup tables by number; acvm_debug_batch_tables: the bits of the mask
TABLE_PED, TABLE_WIN, TABLE_SMALL, TABLE_SKEW, TABLE_PED2, TABLE_WIN16, TABLE_PEDW, TABLE_ECDSA_K1, TABLE_ECDSA_R1 = range(9)
TABLE_BIT_PED2, TABLE_BIT_WIN16, TABLE_BIT_PEDW, TABLE_BIT_ECDSA = 1, 2, 4, 8


def debug_table_info(table):
    """(number of entries, whether the current device holds the table now) of one lookup table (see include/acvm_amd.h)"""
    n, built = C.c_uint64(), C.c_int()
    _check(lib().acvm_debug_table_info(table, C.byref(n), C.byref(built)))
    return n.value, bool(built.value)


def debug_table_read(table, entries):
    """The raw 16 words of the given entries of one lookup table, as a uint32 array [n][16] (builds the table if the device does not hold it)"""
    import numpy as np
    idx = np.ascontiguousarray(entries, dtype=np.uint64).reshape(-1)
    out = np.zeros((idx.size, 16), dtype=np.uint32)
    _check(lib().acvm_debug_table_read(table, idx.ctypes.data, idx.size, out.ctypes.data))
    return out


SECP_PROBE_WORDS = ((2, 1), (1, 1), (2, 1), (2, 1), (1, 1), (1, 1), (3, 3), (5, 3), (1, 1), (2, 1), (2, 1), (1, 1),
                    (2, 1), (1, 1), (1, 4), (4, 3), (6, 2))


def debug_secp(curve, what, items):
    """Component probe of the ECDSA kernels (see include/acvm_amd.h): items = tuples of ints (values < p; 12..16: below 2^256); returns one tuple of ints per item."""
    wi, wo = SECP_PROBE_WORDS[what]
    assert all(len(it) == wi for it in items)
    data = b"".join(int(v).to_bytes(32, "big") for it in items for v in it)
    out = C.create_string_buffer(32 * wo * max(len(items), 1))
    _check(lib().acvm_debug_secp(curve, what, data, len(items), out))
    raw = out.raw
    return [tuple(int.from_bytes(raw[32 * (wo * i + k):32 * (wo * i + k + 1)], "big") for k in range(wo)) for i in range(len(items))]


# acvm_debug_fr: u32 words per item (in, out) of every `what` (acvm_amd/csrc/fr_probe.hpp)
FR_PROBE_WORDS = ((16, 8), (16, 8), (8, 8), (16, 8), (16, 8), (8, 8), (8, 8), (8, 8), (8, 8), (8, 2), (8, 2), (1, 8), (8, 9), (9, 8), (18, 9), (18, 9), (9, 9),
                  (9, 1), (9, 9), (10, 9), (9, 9), (9, 9), (9, 9), (9, 9), (19, 9), (18, 9), (9, 9), (9, 1), (18, 9), (36, 9), (54, 9), (27, 9), (45, 9), (27, 9),
                  (45, 9), (18, 9), (36, 9), (27, 9))


def debug_fr(what, items, uniform=None):
    """Component probe of the BN254-Fr device library (see include/acvm_amd.h): items = an array [n][words in] of raw u32 limbs, uniform = the 18 words
    of the two wave-uniform factors of what 35..37; returns the raw result limbs as a uint32 array [n][words out]."""
    import numpy as np
    wi, wo = FR_PROBE_WORDS[what]
    a = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1, wi)
    out = np.zeros((a.shape[0], wo), dtype=np.uint32)
    u = None if uniform is None else np.ascontiguousarray(uniform, dtype=np.uint32).reshape(18)
    _check(lib().acvm_debug_fr(what, a.ctypes.data, a.shape[0], None if u is None else u.ctypes.data, out.ctypes.data))
    return out


def debug_lin_add(n_terms, coef, rows, h):
    """fr29_lin_add<1 / 2> on the device (acvm_debug_lin_add): n_terms = uint32 [n_groups], coef = uint32 [n_groups][2][8] canonical little-endian words,
    rows = uint32 [n][2][8], h = uint32 [n][9]; the 64 items of a group share their coefficients. Returns (tables [n_groups][2][81], result limbs [n][9])."""
    import numpy as np
    nt = np.ascontiguousarray(n_terms, dtype=np.uint32).reshape(-1)
    r = np.ascontiguousarray(rows, dtype=np.uint32)
    n = r.shape[0]
    n_groups = (n + 63) // 64
    cf = np.ascontiguousarray(coef, dtype=np.uint32)
    hh = np.ascontiguousarray(h, dtype=np.uint32)
    assert nt.shape == (n_groups,) and cf.shape == (n_groups, 2, 8) and r.shape == (n, 2, 8) and hh.shape == (n, 9)
    tables, out = np.zeros((n_groups, 2, 81), dtype=np.uint32), np.zeros((n, 9), dtype=np.uint32)
    _check(lib().acvm_debug_lin_add(nt.ctypes.data, cf.ctypes.data, r.ctypes.data, hh.ctypes.data, n, tables.ctypes.data, out.ctypes.data))
    return tables, out


def debug_inverse_batch(den, inv_chunk, slot_of=None, inv_share=None):
    """The shipped inversion batch on denominators of the caller's (see include/acvm_amd.h): den = uint32 [n_jobs][B][8], canonical storage form.
    inv_share: the waves that share one field inversion (None: the process-wide tuning's).
    Returns (inverse-table rows [n_jobs][B][8], row slot_of[k] for job k; event words [B]; the device's count of flagged instances; the host counter)."""
    import numpy as np
    d = np.ascontiguousarray(den, dtype=np.uint32)
    n_jobs, B = d.shape[0], d.shape[1]
    assert d.shape == (n_jobs, B, 8)
    s = None if slot_of is None else np.ascontiguousarray(slot_of, dtype=np.uint32).reshape(n_jobs)
    inv, ev = np.zeros((n_jobs, B, 8), dtype=np.uint32), np.zeros(B, dtype=np.uint32)
    dc, hc = C.c_uint32(), C.c_uint32()
    if inv_share is None:
        _check(lib().acvm_debug_inverse_batch(d.ctypes.data, n_jobs, B, inv_chunk, None if s is None else s.ctypes.data, inv.ctypes.data, ev.ctypes.data,
                                              C.byref(dc), C.byref(hc)))
    else:
        _check(lib().acvm_debug_inverse_batch_shared(d.ctypes.data, n_jobs, B, inv_chunk, inv_share, None if s is None else s.ctypes.data, inv.ctypes.data,
                                                     ev.ctypes.data, C.byref(dc), C.byref(hc)))
    return inv, ev, dc.value, hc.value


def debug_inflate_rows(rows, out_cap, fill=0, pitch=None, lengths=None):
    """The shipped inflater on gzip members of the caller's, no handle (acvm_debug_inflate_rows): rows is a list of bytes objects, row i placed
    at i * pitch (default: the longest row, at least 1) with lengths[i] (default: len(rows[i])) readable bytes -- or, with pitch given, one bytes
    object of len * pitch bytes and lengths a sequence or None (= pitch). out_cap: a multiple of 4. Returns (out uint8 [n][out_cap], which started
    as `fill` everywhere; lengths uint64 [n]; findings uint32 [n][2] = class, block; crcs uint32 [n])."""
    import numpy as np
    if isinstance(rows, (bytes, bytearray)):
        buf = np.frombuffer(bytes(rows), dtype=np.uint8).copy()
        n = buf.size // pitch
        assert buf.size == n * pitch
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint64)
    else:
        rows = [bytes(r) for r in rows]
        n = len(rows)
        pitch = pitch or max([len(r) for r in rows] + [1])
        buf = np.zeros(n * pitch, dtype=np.uint8)
        for i, r in enumerate(rows):
            buf[i * pitch:i * pitch + min(len(r), pitch)] = np.frombuffer(r[:pitch], dtype=np.uint8)
        lens = np.array([len(r) for r in rows] if lengths is None else lengths, dtype=np.uint64)
    assert lens is None or lens.shape == (n,)
    out = np.full((n, out_cap), fill, dtype=np.uint8)
    out_lengths, findings, crcs = np.zeros(n, dtype=np.uint64), np.zeros((n, 2), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    _check(lib().acvm_debug_inflate_rows(buf.ctypes.data if buf.size else None, pitch, None if lens is None else lens.ctypes.data, n, out_cap,
                                         out.ctypes.data if out.size else None, out_lengths.ctypes.data, findings.ctypes.data, crcs.ctypes.data))
    return out, out_lengths, findings, crcs


def debug_wire_repitch(rows=None, packed=None, offsets=None, pitch=None, displacement=0, capacity=None, scan_chunk=0, fill=0xA5, lengths=None):
    """The shipped scan and repitch kernels on rows of the caller's, no handle (acvm_debug_wire_repitch); any bytes at any lengths, zero included.
    Pack (rows: a list of bytes objects): row i lies at i * pitch (default: the longest row, at least 1) with lengths[i] (default: len(rows[i]))
    bytes; the packed buffer has `packed` bytes (an int; default: their sum) of `fill`, at device address `displacement` mod 16; a row is
    copied when it ends at or in front of `capacity` (default: the buffer's size); the scan runs in chunks of scan_chunk rows (0: one).
    Returns (packed uint8 [packed], offsets uint64 [n + 1], total, n_fit).
    Unpack (rows None): `packed` is a bytes object, `offsets` n + 1 numbers, pitch the slots' pitch. Returns (rows uint8 [n][pitch], which started
    as `fill` everywhere; lengths uint64 [n]; findings uint32 [n], the class or 0; count; key = ~(instance << 4 | class) of the smallest)."""
    import numpy as np
    result = np.zeros(2, dtype=np.uint64)
    if rows is not None:
        rows = [bytes(r) for r in rows]
        n = len(rows)
        pitch = pitch or max([len(r) for r in rows] + [1])
        lens = np.array([len(r) for r in rows] if lengths is None else lengths, dtype=np.uint64).reshape(n)
        buf = np.zeros(n * pitch, dtype=np.uint8)
        for i, r in enumerate(rows):
            buf[i * pitch:i * pitch + min(len(r), pitch)] = np.frombuffer(r[:pitch], dtype=np.uint8)
        size = int(lens.sum()) if packed is None else int(packed)
        out = np.full(size, fill, dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.uint64)
        _check(lib().acvm_debug_wire_repitch(0, n, pitch, buf.ctypes.data if buf.size else None, lens.ctypes.data if n else None, out.ctypes.data if size else None, size, displacement,
                                             offs.ctypes.data, size if capacity is None else capacity, scan_chunk, None, result.ctypes.data))
        return out, offs, int(result[0]), int(result[1])
    offs = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    n = offs.size - 1
    buf = np.frombuffer(bytes(packed), dtype=np.uint8).copy()
    out = np.full((n, pitch), fill, dtype=np.uint8)
    lens, findings = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint32)
    _check(lib().acvm_debug_wire_repitch(1, n, pitch, out.ctypes.data if out.size else None, lens.ctypes.data, buf.ctypes.data if buf.size else None, buf.size, displacement,
                                         offs.ctypes.data, 0, 0, findings.ctypes.data, result.ctypes.data))
    return out, lens[:n], findings[:n], int(result[0]), int(result[1])


def debug_select(status, select_mask, out=None, want_list=True):
    """The shipped selection kernels on a status array of the caller's (acvm_debug_select): status = uint8 [n]. Returns (list, count): list = uint32 [n],
    of which [0, count) are the selected indices in ascending order and the rest is what `out` (default: zeros) held; None with want_list=False."""
    import numpy as np
    st = np.ascontiguousarray(status, dtype=np.uint8).reshape(-1)
    n = st.shape[0]
    lst = None
    if want_list:
        lst = np.zeros(n, dtype=np.uint32) if out is None else np.ascontiguousarray(out, dtype=np.uint32).reshape(n).copy()
    count = C.c_uint32()
    _check(lib().acvm_debug_select(st.ctypes.data if n else None, n, select_mask, lst.ctypes.data if lst is not None and n else None, C.byref(count)))
    return lst, count.value


def decompress_witness(data: bytes) -> dict:
    """WitnessMap::try_from(&[u8]) (witness_map.rs:135-146; acvm_js decompressWitness): {witness index: int}."""
    n = _check(lib().acvm_witness_map_decode(data, len(data), None, None, 0))
    ids = (C.c_uint32 * max(n, 1))()
    vals = C.create_string_buffer(32 * max(n, 1))
    _check(lib().acvm_witness_map_decode(data, len(data), ids, vals, n))
    return {ids[i]: int.from_bytes(vals.raw[32 * i:32 * i + 32], "big") for i in range(n)}


def compress_witness(witness_map: dict) -> bytes:
    """Vec<u8>::try_from(WitnessMap) (witness_map.rs:108-119; acvm_js compressWitness)."""
    items = sorted(witness_map.items())
    ids = (C.c_uint32 * max(len(items), 1))(*[k for k, _ in items])
    vals = b"".join(int(v).to_bytes(32, "big") for _, v in items)
    n = _check(lib().acvm_witness_map_encode(ids, vals, len(items), None, 0))
    out = C.create_string_buffer(max(n, 1))
    _check(lib().acvm_witness_map_encode(ids, vals, len(items), out, n))
    return out.raw[:n]


class Circuit:
    """acir::circuit::Circuit::read (circuit/mod.rs:154-161)."""

    def __init__(self, data: bytes):
        self._h = lib().acvm_circuit_from_bytes(data, len(data))
        if not self._h:
            raise AcvmError(lib().acvm_last_error().decode())
        self.num_opcodes = lib().acvm_circuit_num_opcodes(self._h)
        self.num_witnesses = lib().acvm_circuit_num_witnesses(self._h)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.acvm_circuit_free(self._h)
            self._h = None

    LOCATION_ACIR = 0xFFFFFFFF
    SETS = {"private_parameters": 0, "public_parameters": 1, "return_values": 2, "public_inputs": 3, "circuit_arguments": 4}

    def opcode_kinds(self):
        """ACVM::opcodes seen through the ABI: [(Opcode variant, sub-kind)] per opcode (acvm_circuit_opcode_kinds)"""
        import numpy as np
        n = lib().acvm_circuit_num_opcodes(self._h)
        k = np.zeros((max(n, 1), 2), dtype=np.uint32)
        _check(lib().acvm_circuit_opcode_kinds(self._h, 0, n, k.ctypes.data))
        return [(int(a), int(b)) for a, b in k[:n]]

    def get_assert_message(self, acir_index: int, brillig_index: int = None):
        """Circuit::get_assert_message (circuit/mod.rs:43-51) for OpcodeLocation::Acir / ::Brillig; None if there is none."""
        buf = C.create_string_buffer(4096)
        n = lib().acvm_circuit_assert_message(self._h, acir_index, self.LOCATION_ACIR if brillig_index is None else brillig_index, buf, 4096)
        return None if n < 0 else buf.value.decode()

    def witness_set(self, which: str):
        """private_parameters / public_parameters / return_values / public_inputs() / circuit_arguments() (circuit/mod.rs:25-32,109-121)."""
        n = _check(lib().acvm_circuit_witness_set(self._h, self.SETS[which], None, 0))
        arr = (C.c_uint32 * max(n, 1))()
        _check(lib().acvm_circuit_witness_set(self._h, self.SETS[which], arr, n))
        return list(arr[:n])

    def plan_stats(self, initial_ids, fold_digest=False, reuse_slots=False, keep=()) -> dict:
        """Host-only levelisation (no device): statistics of the static plan; raises if an opcode has no kernel."""
        ids = list(initial_ids)
        arr = (C.c_uint32 * max(len(ids), 1))(*ids)
        keep = list(keep)
        karr = (C.c_uint32 * max(len(keep), 1))(*keep)
        s = Stats()
        _check(lib().acvm_circuit_plan_stats_ex(self._h, arr, len(ids), (1 if fold_digest else 0) | (2 if reuse_slots else 0), karr, len(keep), C.byref(s)))
        return s.as_dict()

    def plans_built(self) -> int:
        """how often this circuit handle has been levelised (handles of equal options share one plan)"""
        return int(lib().acvm_circuit_plans_built(self._h))

    def check_schedule(self, initial_ids, n_instances=4096, fold_digest=False, reuse_slots=False, keep=(), host_solver=False, drop_wait=None) -> dict:
        """Host-only hazard check of the level schedule a handle of these options would enqueue (acvm_circuit_check_schedule): every
        launch's reads and writes derived from the record words, happens-before from stream order + events. drop_wait = k leaves the
        k-th cross-stream wait out (mutation testing). Returns {ok, n_launches, n_waits, n_accesses, n_records, n_findings, report}."""
        ids = list(initial_ids)
        arr = (C.c_uint32 * max(len(ids), 1))(*ids)
        keep = list(keep)
        karr = (C.c_uint32 * max(len(keep), 1))(*keep)
        counts = (C.c_uint64 * 8)()
        text = C.create_string_buffer(1 << 14)
        rc = lib().acvm_circuit_check_schedule(self._h, arr, len(ids), (1 if fold_digest else 0) | (2 if reuse_slots else 0) | (0x100 if host_solver else 0),
                                               karr, len(keep), n_instances, 0xFFFFFFFF if drop_wait is None else drop_wait, counts, text, len(text))
        _check(rc)
        return {"ok": rc == 0, "n_launches": counts[0], "n_waits": counts[1], "n_accesses": counts[2], "n_records": counts[3], "n_findings": counts[4],
                "report": text.value.decode()}

    def lin_plan(self, initial_ids, n_instances=4096, fold_digest=False, reuse_slots=False, keep=(), mutation=0) -> dict:
        """Host-only: the plan's linear tables under the hazard checker, after mutation 1 (two tables change places) or 2 (a wave program's offset
        moves by one) of a copy of the plan if asked (acvm_debug_lin_plan). Returns {ok, n_wave_programs, n_programs_with_tables, n_gate_records,
        n_lin_records, n_lin_terms, n_findings, report}."""
        ids = list(initial_ids)
        arr = (C.c_uint32 * max(len(ids), 1))(*ids)
        keep = list(keep)
        karr = (C.c_uint32 * max(len(keep), 1))(*keep)
        counts = (C.c_uint64 * 8)()
        text = C.create_string_buffer(1 << 14)
        rc = lib().acvm_debug_lin_plan(self._h, arr, len(ids), (1 if fold_digest else 0) | (2 if reuse_slots else 0), karr, len(keep), n_instances, mutation,
                                       counts, text, len(text))
        _check(rc)
        return {"ok": rc == 0, "n_wave_programs": counts[0], "n_programs_with_tables": counts[1], "n_gate_records": counts[2], "n_lin_records": counts[3],
                "n_lin_terms": counts[4], "n_findings": counts[5], "report": text.value.decode()}

    SHARED_NONE = 0xFFFFFFFE

    def bundle_plan(self, initial_ids, n_instances=4096, fold_digest=False, reuse_slots=False, keep=(), mutation=0) -> dict:
        """Host-only: the bundles of the static plan (acvm_debug_bundle_plan; csrc/gate_record.hpp "bundles"): per gate launch -- one level -- the wave
        programs one wave runs one after the other and the operand row they share. Returns {launches: per level a list of (programs, row) with the
        programs as `gate_records` numbers them and row None where nothing is shared, n_bundles, n_shared_bundles, n_shared_loads_saved (row loads per
        instance), n_findings (of the hazard checker, after mutation 1 -- a wave program named twice in a copy of the plan -- if asked)}."""
        ids = list(initial_ids)
        arr = (C.c_uint32 * max(len(ids), 1))(*ids)
        keep = list(keep)
        karr = (C.c_uint32 * max(len(keep), 1))(*keep)
        flags = (1 if fold_digest else 0) | (2 if reuse_slots else 0)
        n = _check(lib().acvm_debug_bundle_plan(self._h, arr, len(ids), flags, karr, len(keep), n_instances, mutation, None, 0))
        out = (C.c_uint32 * n)()
        assert _check(lib().acvm_debug_bundle_plan(self._h, arr, len(ids), flags, karr, len(keep), n_instances, mutation, out, n)) == n
        n_levels, n_bundles, n_prog = out[0], out[1], out[2]
        at = 6
        level_start = out[at:at + n_levels + 1]; at += n_levels + 1
        start = out[at:at + n_bundles + 1]; at += n_bundles + 1
        row = out[at:at + n_bundles]; at += n_bundles
        prog = out[at:at + n_prog]
        launches = [[(list(prog[start[b]:start[b + 1]]), None if row[b] == self.SHARED_NONE else row[b]) for b in range(level_start[L], level_start[L + 1])]
                    for L in range(n_levels)]
        return {"launches": launches, "n_bundles": n_bundles, "n_shared_bundles": out[3], "n_shared_loads_saved": out[4], "n_findings": out[5]}

    def plan_fingerprint(self, initial_ids, fold_digest=False, reuse_slots=False, keep=(), host_solver=False) -> list:
        """Host-only: 64-bit fingerprints of the static plan, one per component (acvm_debug_plan_fingerprint)."""
        ids = list(initial_ids)
        arr = (C.c_uint32 * max(len(ids), 1))(*ids)
        keep = list(keep)
        karr = (C.c_uint32 * max(len(keep), 1))(*keep)
        out = (C.c_uint64 * 128)()
        n = lib().acvm_debug_plan_fingerprint(self._h, arr, len(ids), (1 if fold_digest else 0) | (2 if reuse_slots else 0) | (0x100 if host_solver else 0),
                                              karr, len(keep), out, 128)
        _check(n)
        return list(out[:n])

    GATE_KINDS = ("ASSERT", "SOLVE", "SOLVE_DYN")
    GATE_OUT_MODES = ("ASIS", "WEAK", "CANON")

    def record_scratch(self, initial_ids, fold_digest=False, reuse_slots=False, keep=()) -> list:
        """Host-only: the per-lane scratch words the static plan reserves for each opcode's record, in program order (acvm_debug_record_scratch)"""
        ids = list(initial_ids)
        arr = (C.c_uint32 * max(len(ids), 1))(*ids)
        keep = list(keep)
        karr = (C.c_uint32 * max(len(keep), 1))(*keep)
        flags = (1 if fold_digest else 0) | (2 if reuse_slots else 0)
        n = _check(lib().acvm_debug_record_scratch(self._h, arr, len(ids), flags, karr, len(keep), None, 0))
        out = (C.c_uint32 * max(n, 1))()
        assert _check(lib().acvm_debug_record_scratch(self._h, arr, len(ids), flags, karr, len(keep), out, n)) == n
        return list(out[:n])

    def gate_records(self, initial_ids, fold_digest=False, reuse_slots=False, keep=()) -> list:
        """Host-only: the gate records of the static plan in stream order (acvm_debug_gate_records), decoded after csrc/gate_record.hpp. One dict per
        record: program (its wave program), position (0: the host of the wave program), kind ("ASSERT" / "SOLVE" / "SOLVE_DYN"), opcode, out,
        np_mac, nl_mac, np_pos, np_neg, nl_pos, nl_neg (the lengths of its six term lists), tail (another record follows in its wave), set_local,
        out_mode ("ASIS" / "WEAK" / "CANON"; None for an ASSERT), sub_k, presum_weak, has_qc, lin_terms (terms that take the table form: 0 where the
        wave program has no tables or the record does not qualify), words, operands (the operand rows in the order of the term lists; 0xFFFFFFFF =
        the wave's forwarded value)."""
        ids = list(initial_ids)
        arr = (C.c_uint32 * max(len(ids), 1))(*ids)
        keep = list(keep)
        karr = (C.c_uint32 * max(len(keep), 1))(*keep)
        flags = (1 if fold_digest else 0) | (2 if reuse_slots else 0)
        n = _check(lib().acvm_debug_gate_records(self._h, arr, len(ids), flags, karr, len(keep), None, 0))
        out = (C.c_uint32 * n)()
        assert _check(lib().acvm_debug_gate_records(self._h, arr, len(ids), flags, karr, len(keep), out, n)) == n
        n_prog, n_words = out[0], out[1]
        offsets, lin, stream = out[2:2 + n_prog], out[2 + n_prog:2 + 2 * n_prog], out[2 + 2 * n_prog:n]
        assert len(stream) == n_words
        records = []
        for q in range(n_prog):
            pos, k = offsets[q], 0
            while True:
                w0, w5 = stream[pos], stream[pos + 5]
                kind, np_mac, nl_mac = w0 & 0xff, (w0 >> 8) & 0xff, (w0 >> 16) & 0xff
                np_pos, np_neg, nl_pos, nl_neg = w5 & 0xff, (w5 >> 8) & 0xff, (w5 >> 16) & 0xff, w5 >> 24
                words = 6 + 10 * np_mac + 9 * nl_mac + 2 * (np_pos + np_neg) + nl_pos + nl_neg
                tabled = lin[q] != 0xFFFFFFFF and np_mac == 0 and np_pos == 0
                t = pos + 6
                operands = [stream[t + 10 * i + k] for i in range(np_mac) for k in (8, 9)] + [stream[t + 10 * np_mac + 9 * i + 8] for i in range(nl_mac)]
                operands += stream[t + 10 * np_mac + 9 * nl_mac:pos + words]
                records.append({"program": q, "position": k, "kind": self.GATE_KINDS[kind], "opcode": stream[pos + 1], "out": stream[pos + 2] if kind else None,
                                "np_mac": np_mac, "nl_mac": nl_mac, "np_pos": np_pos, "np_neg": np_neg, "nl_pos": nl_pos, "nl_neg": nl_neg,
                                "tail": bool(w0 & 1 << 24), "set_local": bool(w0 & 1 << 25), "out_mode": self.GATE_OUT_MODES[(w0 >> 26) & 3] if kind else None,
                                "sub_k": (w0 >> 28) & 3, "presum_weak": bool(w0 & 1 << 30), "has_qc": stream[pos + 3] != 0xFFFFFFFD,
                                "lin_terms": nl_mac if tabled else 0, "words": words, "operands": operands})
                if not w0 & 1 << 24:
                    break
                pos += words
                k += 1
        return records


class NodeOpts(C.Structure):
    _fields_ = [("n_devices", C.c_uint32), ("devices", C.POINTER(C.c_int)), ("tile_instances", C.c_uint32), ("batch_flags", C.c_uint32)]


class NodeStats(C.Structure):
    _fields_ = [("n_devices", C.c_uint32), ("tile_instances", C.c_uint32), ("n_instances", C.c_uint64), ("total_ms", C.c_double),
                ("device", C.c_int * 16), ("async_exact", C.c_uint32 * 16), ("tiles", C.c_uint32 * 16), ("exact_instances", C.c_uint32 * 16),
                ("lane_ms", C.c_double * 16), ("solve_device_ms", C.c_double * 16), ("h2d_wait_ms", C.c_double * 16), ("export_ms", C.c_double * 16),
                ("numa_node", C.c_int * 16), ("n_cpus_pinned", C.c_uint32 * 16), ("first_cpu", C.c_int * 16),
                ("plans_built", C.c_uint32), ("create_ms", C.c_double), ("plan_ms", C.c_double), ("host_rss_bytes", C.c_uint64)]


class Node:
    """acvm_node_*: one call solves a global batch on every listed device (one handle + one host thread per device, tiles inside a
    device, pinned double-buffered uploads, the exact path of a tile beside the next one). The caller loop it replaces:
    acvm_js/src/execute.rs:60-119 once per instance."""

    def __init__(self, circuit: "Circuit", initial_ids, keep=(), devices=None, tile=0, fold_digest=False, reuse_slots=False, solver: "BbSolver" = None):
        self.ids, self.keep = list(initial_ids), list(keep)
        self._solver = solver
        arr = (C.c_uint32 * max(len(self.ids), 1))(*self.ids)
        karr = (C.c_uint32 * max(len(self.keep), 1))(*self.keep)
        opts = NodeOpts()
        if devices is not None:
            self._dev = (C.c_int * len(devices))(*devices)
            opts.n_devices, opts.devices = len(devices), self._dev
        opts.tile_instances = tile
        opts.batch_flags = (Batch.FOLD_DIGEST if fold_digest else 0) | (Batch.REUSE_SLOTS if reuse_slots else 0)
        self._h = lib().acvm_node_new(circuit._h, C.byref(solver) if solver is not None else None, arr, len(self.ids), karr, len(self.keep), C.byref(opts))
        if not self._h:
            raise AcvmError(lib().acvm_last_error().decode())
        self.tile = lib().acvm_node_tile_instances(self._h)
        self.n_devices = lib().acvm_node_num_devices(self._h)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.acvm_node_free(self._h)
            self._h = None

    def free(self):
        self.__del__()

    def solve(self, values_be, n_instances: int, results=True, kept=True, digests=True):
        """values_be: n_instances * len(ids) * 32 bytes (bytes or a uint8 array). Returns (not_solved, results or None, kept uint8
        [n][len(keep)][32] or None, kept_assigned uint8 [n][len(keep)] or None, digests uint8 [n][32] or None)."""
        import numpy as np
        buf = np.frombuffer(values_be, dtype=np.uint8) if not isinstance(values_be, np.ndarray) else values_be
        if buf.size != n_instances * len(self.ids) * 32:
            raise ValueError("values_be has the wrong size")
        res = (Result * max(n_instances, 1))() if results else None
        nk = len(self.keep)
        kv = np.zeros((n_instances, nk, 32), dtype=np.uint8) if kept and nk else None
        ka = np.zeros((n_instances, nk), dtype=np.uint8) if kept and nk else None
        dg = np.zeros((n_instances, 32), dtype=np.uint8) if digests else None
        rc = lib().acvm_node_solve(self._h, n_instances, buf.ctypes.data if buf.size else None, C.cast(res, C.c_void_p) if res is not None else None,
                                   kv.ctypes.data if kv is not None else None, ka.ctypes.data if ka is not None else None, dg.ctypes.data if dg is not None else None)
        self._finish_call(rc)
        return rc, res, kv, ka, dg

    def solve_records(self, records, n_instances: int, pitch: int, fields, results=True, kept=True, digests=True):
        """solve with the inputs as host records (acvm_node_solve_records): records holds n_instances * pitch bytes (bytes or a uint8 array),
        fields as Batch.import_device_records takes them. Returns what solve returns."""
        import numpy as np
        buf = np.frombuffer(records, dtype=np.uint8) if not isinstance(records, np.ndarray) else records.view(np.uint8).reshape(-1)
        if buf.size != n_instances * pitch:
            raise ValueError("records has the wrong size")
        desc, _keep = record_desc(pitch, fields)
        res = (Result * max(n_instances, 1))() if results else None
        nk = len(self.keep)
        kv = np.zeros((n_instances, nk, 32), dtype=np.uint8) if kept and nk else None
        ka = np.zeros((n_instances, nk), dtype=np.uint8) if kept and nk else None
        dg = np.zeros((n_instances, 32), dtype=np.uint8) if digests else None
        rc = lib().acvm_node_solve_records(self._h, n_instances, C.byref(desc), buf.ctypes.data if buf.size else None, C.cast(res, C.c_void_p) if res is not None else None,
                                           kv.ctypes.data if kv is not None else None, ka.ctypes.data if ka is not None else None,
                                           dg.ctypes.data if dg is not None else None)
        self._finish_call(rc)
        return rc, res, kv, ka, dg

    def solve_device(self, lanes):
        """acvm_node_solve_device: one dict per handle of the node with the fields of acvm_node_lane_io_t -- n, d_values, encoding, layout, columns,
        n_columns, stride (the inputs, as import_device's keywords), d_kept, d_kept_assigned, kept_encoding, kept_layout, kept_stride, d_status,
        d_err, d_opcode_index, d_digests32, select_mask, d_selected; device addresses, absent / 0 / None = NULL. Returns one
        (not_solved, n_selected) per lane; last_not_solved holds their total as the call returned it."""
        arr = (NodeLaneIo * max(len(lanes), 1))()
        keep = []
        for q, lane in enumerate(lanes):
            io = arr[q]
            io.n, io.d_values = lane.get("n", 0), lane.get("d_values") or None
            io.in_.encoding, io.in_.layout, io.in_.stride = lane.get("encoding", ENC_BE32), lane.get("layout", LAYOUT_INSTANCE_MAJOR), lane.get("stride", 0)
            if lane.get("columns") is not None:
                cols = list(lane["columns"])
                if len(cols) != len(self.ids):
                    raise ValueError("columns needs one entry per initial witness")
                c_arr = (C.c_uint32 * max(len(cols), 1))(*cols)
                keep.append(c_arr)
                io.in_.columns, io.in_.n_columns = c_arr, lane["n_columns"] if lane.get("n_columns") is not None else len(cols)
            io.kept_encoding, io.kept_layout, io.kept_stride = lane.get("kept_encoding", ENC_BE32), lane.get("kept_layout", LAYOUT_INSTANCE_MAJOR), lane.get("kept_stride", 0)
            for f in ("d_kept", "d_kept_assigned", "d_status", "d_err", "d_opcode_index", "d_digests32", "d_selected"):
                setattr(io, f, lane.get(f) or None)
            io.select_mask = lane.get("select_mask", 0)
        self.last_not_solved = self._finish_call(lib().acvm_node_solve_device(self._h, arr, len(lanes)))  # (the call's own return value: the total)
        return [(arr[q].not_solved, arr[q].n_selected) for q in range(len(lanes))]

    def _finish_call(self, rc):
        """a Python exception of the foreign-call handler left the node call as a negative return: it is raised again here, in front of the call's own error"""
        raised = getattr(self, "_fc_raised", None)
        if raised:
            exc = raised[0]
            del raised[:]
            raise exc
        return _check(rc)

    def set_foreign_call_handler(self, fn, space=SPACE_DEVICE, in_encoding=ENC_BE32, in_layout=LAYOUT_INSTANCE_MAJOR, max_rounds=0):
        """acvm_node_set_foreign_call_handler: fn(ForeignRound) is called on a lane's thread once per tile, round and site (lanes call it concurrently).
        It returns a dict -- shape (one entry per output: None for a single value, otherwise an array's length; with row_lens any non-None entry), values,
        and optionally encoding, layout, n_columns (default: the shape's total), stride, row_lens, answered -- or False to decline the site for this
        tile, or a negative int to abort the node call. values / row_lens / answered: device addresses (int) for SPACE_DEVICE; bytes-like objects (or
        None) for SPACE_HOST. A Python exception aborts the node call and is raised again by solve / solve_device. fn None: no handler."""
        if fn is None:
            _check(lib().acvm_node_set_foreign_call_handler(self._h, None))
            self._fc = None
            return
        raised, keep = [], {}

        def address(lane, what, x):
            if x is None:
                return None
            if isinstance(x, int):
                return x
            buf = (C.c_char * max(len(x), 1)).from_buffer_copy(bytes(x) if len(x) else b"\0")
            keep[lane].append(buf)
            return C.addressof(buf)

        def trampoline(user, r_ptr, out_ptr):
            try:
                r, out = r_ptr.contents, out_ptr.contents
                ans = fn(ForeignRound(r, space, in_encoding, in_layout))
                if ans is False:
                    return 1
                if isinstance(ans, int):
                    return ans
                keep[r.lane] = []  # (what the previous answer of this lane pointed at may go now)
                shape = list(ans["shape"])
                is_arr = (C.c_uint8 * max(len(shape), 1))(*[0 if n is None else 1 for n in shape])
                lens = (C.c_uint32 * max(len(shape), 1))(*[1 if n is None else n for n in shape])
                keep[r.lane] += [is_arr, lens]
                out.n_values, out.is_array, out.lens = len(shape), C.addressof(is_arr), C.addressof(lens)
                out.encoding, out.layout = ans.get("encoding", ENC_BE32), ans.get("layout", LAYOUT_INSTANCE_MAJOR)
                total = sum(1 if n is None else n for n in shape)
                out.n_columns, out.stride = ans["n_columns"] if ans.get("n_columns") is not None else total, ans.get("stride", 0)
                out.values = address(r.lane, "values", ans.get("values"))
                out.row_lens = address(r.lane, "row_lens", ans.get("row_lens"))
                out.answered = address(r.lane, "answered", ans.get("answered"))
                return 0
            except BaseException as e:  # nothing unwinds through the library
                raised.append(e)
                return -1  # (ACVM_E_INVALID)

        cb = _NODE_FOREIGN_FN(trampoline)
        h = NodeForeignHandler(fn=cb, user=None, space=space, in_encoding=in_encoding, in_layout=in_layout, max_rounds=max_rounds)
        _check(lib().acvm_node_set_foreign_call_handler(self._h, C.byref(h)))
        self._fc, self._fc_raised = (cb, keep), raised  # the callback lives as long as the node may call it

    def foreign_stats(self, lane: int) -> dict:
        """acvm_node_foreign_stats: the foreign-call loop of this lane during the last solve / solve_device"""
        st = NodeForeignStats()
        _check(lib().acvm_node_foreign_stats(self._h, lane, C.byref(st)))
        return {f: getattr(st, f) for f, _ in NodeForeignStats._fields_}

    def io_bytes(self, lane: int):
        """(host-to-device, device-to-host) bytes the device form has copied for this lane so far (acvm_debug_node_io_bytes)"""
        h2d, d2h = C.c_uint64(0), C.c_uint64(0)
        _check(lib().acvm_debug_node_io_bytes(self._h, lane, C.byref(h2d), C.byref(d2h)))
        return h2d.value, d2h.value

    def stats(self):
        st = NodeStats()
        _check(lib().acvm_node_stats(self._h, C.byref(st)))
        n = st.n_devices
        return {"n_devices": n, "tile_instances": st.tile_instances, "n_instances": st.n_instances, "total_ms": st.total_ms,
                "plans_built": st.plans_built, "create_ms": st.create_ms, "plan_ms": st.plan_ms, "host_rss_bytes": st.host_rss_bytes,
                **{f: list(getattr(st, f))[:n] for f in ("device", "async_exact", "tiles", "exact_instances", "lane_ms", "solve_device_ms", "h2d_wait_ms", "export_ms", "numa_node", "n_cpus_pinned",
                                                              "first_cpu")}}


class Batch:
    """ACVM::new / solve / witness_map for n_instances instances of one circuit."""

    FOLD_DIGEST, REUSE_SLOTS = 1, 2

    def __init__(self, circuit: Circuit, n_instances: int, initial_ids, solver: "BbSolver" = None, fold_digest=False, reuse_slots=False, keep=()):
        """fold_digest: the map digests are computed during the solve; reuse_slots: witness-slot liveness reuse (only the initial
        witnesses and `keep` can be read back afterwards, plus results and digests): acvm_batch_new_ex"""
        self.circuit = circuit
        self.B = n_instances
        self.ids = list(initial_ids)
        self._solver = solver  # keeps the callbacks alive: the vtable must outlive the batch
        arr = (C.c_uint32 * max(len(self.ids), 1))(*self.ids)
        keep = list(keep)
        karr = (C.c_uint32 * max(len(keep), 1))(*keep)
        flags = (self.FOLD_DIGEST if fold_digest else 0) | (self.REUSE_SLOTS if reuse_slots else 0)
        self._h = lib().acvm_batch_new_ex(circuit._h, C.byref(solver) if solver is not None else None, n_instances, arr, len(self.ids), flags, karr, len(keep))
        if not self._h:
            raise AcvmError(lib().acvm_last_error().decode())
        self.nw = self.stats()["n_witnesses"]

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.acvm_batch_free(self._h)
            self._h = None

    def free(self):
        self.__del__()

    def set_initial_witness(self, values_be: bytes):
        """values_be: B * len(ids) * 32 bytes, instance-major canonical big-endian."""
        import numpy as np
        buf = np.frombuffer(values_be, dtype=np.uint8)
        if buf.size != self.B * len(self.ids) * 32:
            raise ValueError("initial witness buffer has the wrong size")
        _check(lib().acvm_batch_set_initial_witness(self._h, buf.ctypes.data))

    def solve(self, then_import: int = 0, then_import_desc=None) -> int:
        """ACVM::solve for every instance; then_import: device pointer of the NEXT tile's inputs, imported behind the solve when no instance
        left the generic path (acvm_batch_solve_then_import). then_import_desc: how that buffer is to be read, as a dict of import_device's
        keywords (encoding, layout, columns, n_columns, stride): acvm_batch_solve_then_import_ex"""
        if then_import and then_import_desc is not None:
            desc, _keep = self._import_desc(**then_import_desc)
            return _check(lib().acvm_batch_solve_then_import_ex(self._h, C.byref(desc), then_import))
        if then_import:
            return _check(lib().acvm_batch_solve_then_import(self._h, then_import))
        return _check(lib().acvm_batch_solve(self._h))

    def solve_opcode(self) -> int:
        """ACVM::solve_opcode for the batch (see include/acvm_amd.h): one opcode, returns the number of instances not Solved."""
        return _check(lib().acvm_batch_solve_opcode(self._h))

    def set_initial_witness_device(self, d_ptr: int):
        """values already resident on the device (same layout as set_initial_witness), e.g. a slice of a DeviceBuffer."""
        _check(lib().acvm_batch_set_initial_witness_device(self._h, d_ptr))

    def _import_desc(self, encoding=ENC_BE32, layout=LAYOUT_INSTANCE_MAJOR, columns=None, n_columns=None, stride=0):
        """(acvm_import_desc_t, the array its column pointer refers to)"""
        desc = ImportDesc(encoding=encoding, layout=layout, n_columns=0, stride=stride)
        arr = None
        if columns is not None:
            cols = list(columns)
            if len(cols) != len(self.ids):
                raise ValueError("columns needs one entry per initial witness")
            arr = (C.c_uint32 * max(len(cols), 1))(*cols)
            desc.columns, desc.n_columns = arr, len(cols) if n_columns is None else n_columns
        return desc, arr

    def _with_d_assigned(unmasked):
        """import_device(..., d_assigned=None): the keyword routes to import_device_masked. The positional parameters stay exactly those of the
        unmasked call -- solve(then_import_desc=...) and import_device_parts take them as a dict, and d_assigned is none of theirs."""
        @functools.wraps(unmasked)
        def import_device(self, d_ptr, *args, d_assigned=None, **keywords):
            if d_assigned is None:
                return unmasked(self, d_ptr, *args, **keywords)
            return self.import_device_masked(d_ptr, d_assigned, *args, **keywords)
        return import_device

    @_with_d_assigned
    def import_device(self, d_ptr: int, encoding=ENC_BE32, layout=LAYOUT_INSTANCE_MAJOR, columns=None, n_columns=None, stride=0):
        """The initial witnesses read from device memory at d_ptr (acvm_batch_import_device), the mirror image of export_device: 32 bytes per
        element in `encoding` (ENC_U8 .. ENC_U128: the integer's 1 .. 16 bytes, little-endian, d_ptr aligned to that size), element (instance i, column c) where `layout` and `stride` (in elements, 0 = dense) put it; columns: per initial
        witness (in the order of the ids the batch was created with) the column of the buffer that holds it, None = column k; n_columns: the
        buffer's width in columns (default: len(columns)). The defaults are set_initial_witness_device."""
        desc, _keep = self._import_desc(encoding, layout, columns, n_columns, stride)
        _check(lib().acvm_batch_import_device(self._h, C.byref(desc), d_ptr))

    del _with_d_assigned

    def import_device_masked(self, d_ptr: int, d_assigned: int, encoding=ENC_BE32, layout=LAYOUT_INSTANCE_MAJOR, columns=None, n_columns=None, stride=0):
        """import_device for instances that do not all hold every initial witness (acvm_batch_import_device_masked). d_assigned: device pointer of
        one byte per element in the values' layout, stride and column list -- what export_device writes into its d_assigned: 0 = the instance does
        not hold that initial witness, 1 = it does. Any other byte raises, and the batch is then without initial witnesses until another import.
        import_device(..., d_assigned=ptr) is this call; d_assigned=None is import_device."""
        if d_assigned is None:
            return self.import_device(d_ptr, encoding, layout, columns, n_columns, stride)
        desc, _keep = self._import_desc(encoding, layout, columns, n_columns, stride)
        _check(lib().acvm_batch_import_device_masked(self._h, C.byref(desc), d_ptr, d_assigned))

    def set_initial_witness_masked(self, values_be: bytes, assigned: bytes):
        """set_initial_witness with a mask (acvm_batch_set_initial_witness_masked): assigned holds B * len(ids) bytes, instance-major, 0 = the
        instance does not hold that initial witness (its 32 value bytes are ignored), 1 = it does."""
        import numpy as np
        buf, mask = np.frombuffer(values_be, dtype=np.uint8), np.frombuffer(bytes(assigned), dtype=np.uint8)
        if buf.size != self.B * len(self.ids) * 32:
            raise ValueError("initial witness buffer has the wrong size")
        if mask.size != self.B * len(self.ids):
            raise ValueError("assigned needs one byte per instance and initial witness")
        _check(lib().acvm_batch_set_initial_witness_masked(self._h, buf.ctypes.data, mask.ctypes.data))

    def import_missing(self) -> int:
        """instances with at least one absent input after the last import (acvm_debug_import_missing); 0 after any unmasked import"""
        return lib().acvm_debug_import_missing(self._h)

    def import_device_parts(self, parts):
        """One import from several device buffers (acvm_batch_import_device_parts). parts: dicts with d_ptr, positions (which initial witnesses,
        as positions in the ids the batch was created with, the part supplies) and import_device's keywords encoding, layout (LAYOUT_BROADCAST
        too: one element per column, the value of every instance), columns, n_columns, stride. Every initial witness needs exactly one part."""
        arr = (ImportPart * max(len(parts), 1))()
        keep = []
        for q, part in enumerate(parts):
            pos = list(part["positions"])
            p_arr = (C.c_uint32 * max(len(pos), 1))(*pos)
            keep.append(p_arr)
            arr[q].d_values, arr[q].encoding, arr[q].layout = part["d_ptr"], part.get("encoding", ENC_BE32), part.get("layout", LAYOUT_INSTANCE_MAJOR)
            arr[q].positions, arr[q].n, arr[q].n_columns, arr[q].stride = p_arr, len(pos), 0, part.get("stride", 0)
            if part.get("columns") is not None:
                cols = list(part["columns"])
                if len(cols) != len(pos):
                    raise ValueError("columns needs one entry per position of the part")
                c_arr = (C.c_uint32 * max(len(cols), 1))(*cols)
                keep.append(c_arr)
                arr[q].columns, arr[q].n_columns = c_arr, len(cols) if part.get("n_columns") is None else part["n_columns"]
        _check(lib().acvm_batch_import_device_parts(self._h, arr, len(parts)))

    def import_device_records(self, d_ptr: int, pitch: int, fields):
        """The initial witnesses read from an array of structs in device memory (acvm_batch_import_device_records): instance i reads the record at
        d_ptr + i * pitch; fields: (position, encoding, offset) triples or RecordField objects -- initial witness `position` (in the order of the
        ids the batch was created with) is the element of `encoding` at byte `offset` of the record. Pointer, pitch and offsets of any alignment;
        every position exactly once; bytes no field covers are padding. record_fields_from_dtype makes (pitch, fields) of a numpy dtype. (The
        descriptor is built per call, about 0.3 us per field: a loop that minds builds record_desc once and calls the C entry point.)"""
        desc, _keep = record_desc(pitch, fields)
        _check(lib().acvm_batch_import_device_records(self._h, C.byref(desc), d_ptr))

    def set_initial_witness_records(self, records, pitch: int, fields):
        """import_device_records from host memory (acvm_batch_set_initial_witness_records): records holds B * pitch bytes (bytes, or a numpy
        array -- a structured one too)"""
        import numpy as np
        buf = np.frombuffer(records, dtype=np.uint8) if not isinstance(records, np.ndarray) else np.ascontiguousarray(records).view(np.uint8).reshape(-1)
        if buf.size != self.B * pitch:
            raise ValueError("records has the wrong size")
        desc, _keep = record_desc(pitch, fields)
        _check(lib().acvm_batch_set_initial_witness_records(self._h, C.byref(desc), buf.ctypes.data if buf.size else None))

    def import_device_records_masked(self, d_ptr: int, pitch: int, fields):
        """import_device_records for instances that do not all hold every initial witness (acvm_batch_import_device_records_masked). fields:
        (position, encoding, offset, mask_offset) tuples or RecordMaskedField objects -- byte `mask_offset` of the record is 1 where the instance
        holds the element and 0 where it does not (None, or a triple: always held). Several fields may share a mask byte. Any other byte raises,
        and the batch is then without initial witnesses until another import. With no mask at all this is import_device_records.
        record_masked_fields_from_out makes the list from the field list of another circuit's export_device_records."""
        desc, _keep = record_masked_desc(pitch, fields)
        _check(lib().acvm_batch_import_device_records_masked(self._h, C.byref(desc), d_ptr))

    def set_initial_witness_records_masked(self, records, pitch: int, fields):
        """import_device_records_masked from host memory (acvm_batch_set_initial_witness_records_masked): records as
        set_initial_witness_records takes them"""
        import numpy as np
        buf = np.frombuffer(records, dtype=np.uint8) if not isinstance(records, np.ndarray) else np.ascontiguousarray(records).view(np.uint8).reshape(-1)
        if buf.size != self.B * pitch:
            raise ValueError("records has the wrong size")
        desc, _keep = record_masked_desc(pitch, fields)
        _check(lib().acvm_batch_set_initial_witness_records_masked(self._h, C.byref(desc), buf.ctypes.data if buf.size else None))

    def import_device_wire(self, d_ptr: int, container, pitch: int, d_lengths=None):
        """The initial witnesses read from serialised WitnessMaps in device memory (acvm_batch_import_device_wire): instance j's map -- the
        bincode body (WIRE_BINCODE) or the stored-block gzip member around it (WIRE_GZIP_STORED), what witness_maps_wire_device writes -- is the
        slot at d_ptr + j * pitch (d_ptr 16-byte aligned, pitch a multiple of 16). An initial witness a row does not name is absent, as under a
        mask byte 0 of import_device_masked. d_lengths: device pointer of B uint64 lengths, or None = each row's count word gives its length.
        Bytes that are no such map raise, and the batch is then without initial witnesses until another import."""
        desc = WireInDesc(container=container, pitch=pitch)
        _check(lib().acvm_batch_import_device_wire(self._h, C.byref(desc), d_ptr, d_lengths))

    def set_initial_witness_maps_wire(self, maps):
        """One serialised WitnessMap per instance from host memory (acvm_batch_set_initial_witness_maps_wire): maps is a list of B bytes objects,
        each what compress_witness / compressWitness writes (any gzip stream) or the raw bincode body. Everything decompress_witness reads is
        accepted with the same meaning; every key must be one of the ids the batch was created with. A row that does not parse raises naming its
        instance, and the batch keeps the initial witnesses it had."""
        import numpy as np
        maps = [bytes(m) for m in maps]
        if len(maps) != self.B:
            raise ValueError("one serialised map per instance")
        lengths = np.array([len(m) for m in maps], dtype=np.uint64)
        pitch = max([len(m) for m in maps] + [1])
        buf = np.zeros(self.B * pitch, dtype=np.uint8)
        for j, m in enumerate(maps):
            buf[j * pitch:j * pitch + len(m)] = np.frombuffer(m, dtype=np.uint8)
        _check(lib().acvm_batch_set_initial_witness_maps_wire(self._h, buf.ctypes.data if buf.size else None, pitch, lengths.ctypes.data if self.B else None))

    def import_device_wire_gzip(self, d_ptr: int, pitch: int, d_lengths=None):
        """The initial witnesses read from gzip members in device memory, inflated on the device (acvm_batch_import_device_wire_gzip): instance
        j's member -- any deflate stream around its bincode body: what witness_maps_wire_device(WIRE_GZIP_DEFLATE or WIRE_GZIP_STORED) or
        compressWitness writes -- is the slot at d_ptr + j * pitch (d_ptr 16-byte aligned, pitch a multiple of 16), of which row j reads
        min(d_lengths[j], pitch) bytes (d_lengths: device pointer of B uint64, or None = pitch). A member that does not inflate raises
        ("wire inflate: ...") and the batch keeps the initial witnesses it had; a body that is no canonical map raises as import_device_wire does."""
        desc = WireInDesc(container=WIRE_GZIP_DEFLATE, pitch=pitch)
        _check(lib().acvm_batch_import_device_wire_gzip(self._h, C.byref(desc), d_ptr, d_lengths))

    def set_initial_witness_maps_gzip(self, maps):
        """One gzip member per instance from host memory, uploaded compressed and inflated on the device
        (acvm_batch_set_initial_witness_maps_gzip): maps is a list of B bytes objects, each starting 1f 8b. The inflated body must be in canonical
        shape (what every BTreeMap serialiser writes); set_initial_witness_maps_wire takes the others."""
        import numpy as np
        maps = [bytes(m) for m in maps]
        if len(maps) != self.B:
            raise ValueError("one serialised map per instance")
        lengths = np.array([len(m) for m in maps], dtype=np.uint64)
        pitch = max([len(m) for m in maps] + [1])
        buf = np.zeros(self.B * pitch, dtype=np.uint8)
        for j, m in enumerate(maps):
            buf[j * pitch:j * pitch + len(m)] = np.frombuffer(m, dtype=np.uint8)
        _check(lib().acvm_batch_set_initial_witness_maps_gzip(self._h, buf.ctypes.data if buf.size else None, pitch, lengths.ctypes.data if self.B else None))

    def import_state(self) -> dict:
        """what the last import left on the device (acvm_debug_import_state), as uint32 arrays: rows [n_initial][2][B][4], planes [n_initial][B],
        events [2 + B], missing [ceil(n_initial / 32)][B]"""
        import numpy as np
        n = len(self.ids)
        out = {"rows": np.zeros((n, 2, self.B, 4), dtype=np.uint32), "planes": np.zeros((n, self.B), dtype=np.uint32),
               "events": np.zeros(2 + self.B, dtype=np.uint32), "missing": np.zeros(((n + 31) // 32, self.B), dtype=np.uint32)}
        _check(lib().acvm_debug_import_state(self._h, *(out[k].ctypes.data for k in ("rows", "planes", "events", "missing"))))
        return out

    def import_list_copies(self) -> int:
        """host-to-device copies of the imports' lists -- a descriptor's column list, the lists of import_device_parts -- this handle has made
        (acvm_debug_import_list_copies)"""
        return lib().acvm_debug_import_list_copies(self._h)

    def tables(self):
        """the device-built lookup tables this handle's kernels read, as a mask of TABLE_BIT_* (acvm_debug_batch_tables)"""
        m = C.c_uint32()
        _check(lib().acvm_debug_batch_tables(self._h, C.byref(m)))
        return m.value

    def reset(self):
        _check(lib().acvm_batch_reset(self._h))

    def set_instances(self, n):
        """from the next set_initial_witness on the handle covers instances [0, n), n <= the size it was created with"""
        _check(lib().acvm_batch_set_instances(self._h, n))
        self.B = n

    def set_force_slow_path(self, on: bool):
        _check(lib().acvm_batch_set_force_slow_path(self._h, int(on)))

    def set_profiling(self, on: bool):
        _check(lib().acvm_batch_set_profiling(self._h, int(on)))

    def results(self):
        out = (Result * max(self.B, 1))()
        _check(lib().acvm_batch_results(self._h, C.cast(out, C.c_void_p)))
        return out

    def witness(self, w: int):
        import numpy as np
        vals = np.zeros((self.B, 32), dtype=np.uint8)
        asg = np.zeros((self.B,), dtype=np.uint8)
        _check(lib().acvm_batch_witness(self._h, w, vals.ctypes.data, asg.ctypes.data))
        return vals, asg

    def witness_map(self, first=0, n=None):
        import numpy as np
        n = self.B - first if n is None else n
        asg = np.zeros((n, self.nw), dtype=np.uint8)
        vals = np.zeros((n, self.nw, 32), dtype=np.uint8)
        _check(lib().acvm_batch_witness_map(self._h, first, n, asg.ctypes.data, vals.ctypes.data))
        return asg, vals

    def error_string(self, instance: int) -> str:
        """The string acvm_js reports for a failed instance (execute.rs:79-108): assert message or the error's Display text."""
        buf = C.create_string_buffer(1024)
        _check(lib().acvm_batch_error_string(self._h, self.circuit._h, instance, buf, 1024))
        return buf.value.decode()

    def error_expression(self, instance: int):
        """ExpressionHasTooManyUnknowns(Expression) of a failed instance as data (acvm_batch_error_expression): None if the instance did not fail
        that way, else {"opcode_index", "mul": [(coef, wl, wr)], "lin": [(coef, w)], "q_c"} with coefficients as integers"""
        import numpy as np
        head = ExpressionHead()
        cap = 64
        while True:
            mc, mw = np.zeros((cap, 32), dtype=np.uint8), np.zeros((cap, 2), dtype=np.uint32)
            lc, lw = np.zeros((cap, 32), dtype=np.uint8), np.zeros(cap, dtype=np.uint32)
            rc = _check(lib().acvm_batch_error_expression(self._h, self.circuit._h, instance, C.byref(head), mc.ctypes.data, mw.ctypes.data, cap,
                                                          lc.ctypes.data, lw.ctypes.data, cap))
            if rc == 0:
                return None
            if max(head.n_mul, head.n_lin) <= cap:
                break
            cap = max(head.n_mul, head.n_lin)
        be = lambda a: int.from_bytes(bytes(a), "big")
        return {"opcode_index": head.opcode_index, "q_c": be(head.q_c),
                "mul": [(be(mc[i]), int(mw[i, 0]), int(mw[i, 1])) for i in range(head.n_mul)],
                "lin": [(be(lc[i]), int(lw[i])) for i in range(head.n_lin)]}

    def extract(self, witnesses, first=0, n=None):
        """extract_indices (public_witness.rs:10-21) for instances [first, first + n): uint8 array [n][len(witnesses)][32];
        raises if a witness is unassigned. Use with Circuit.witness_set("return_values" | "public_parameters" | "public_inputs")."""
        import numpy as np
        n = self.B - first if n is None else n
        ws = list(witnesses)
        arr = (C.c_uint32 * max(len(ws), 1))(*ws)
        vals = np.zeros((n, len(ws), 32), dtype=np.uint8)
        _check(lib().acvm_batch_extract_witnesses(self._h, arr, len(ws), first, n, vals.ctypes.data))
        return vals

    def export_device(self, d_ptr: int, encoding=ENC_BE32, layout=LAYOUT_INSTANCE_MAJOR, witnesses=None, first=0, n=None, stride=0, d_assigned=None):
        """The map of instances [first, first + n) written into device memory at d_ptr (acvm_batch_export_device): 32 bytes per element in
        `encoding` (ENC_U8 .. ENC_U128: the low 1 .. 16 bytes of the value, little-endian; mask 2 = the value does not fit), element (instance i, list position k) where `layout` and `stride` (in elements, 0 = dense) put it; witnesses: list of
        indices, None = the whole map; d_assigned: device pointer of the mask bytes (0 / 1, for a narrow encoding 0 / 1 / 2), or None. Nothing is copied to the host."""
        n = self.B - first if n is None else n
        desc = ExportDesc(encoding=encoding, layout=layout, first=first, n=n, stride=stride)
        if witnesses is not None:
            ws = list(witnesses)
            arr = (C.c_uint32 * max(len(ws), 1))(*ws)
            desc.witnesses, desc.n_witnesses = arr, len(ws)
        _check(lib().acvm_batch_export_device(self._h, C.byref(desc), d_ptr, d_assigned))

    def export_device_list(self, d_instances: int, n: int, d_ptr: int, encoding=ENC_BE32, layout=LAYOUT_INSTANCE_MAJOR, witnesses=None, stride=0, d_assigned=None):
        """export_device for LISTED instances (acvm_batch_export_device_list): row i of the output is instance d_instances[i], a device array of n absolute
        instance numbers (any order, repeats allowed; an entry beyond the batch reads as an instance that assigned nothing). Everything else as export_device."""
        desc = ExportDesc(encoding=encoding, layout=layout, first=0, n=n, stride=stride)
        if witnesses is not None:
            ws = list(witnesses)
            arr = (C.c_uint32 * max(len(ws), 1))(*ws)
            desc.witnesses, desc.n_witnesses = arr, len(ws)
        _check(lib().acvm_batch_export_device_list(self._h, C.byref(desc), d_instances, d_ptr, d_assigned))

    def export_device_records(self, d_ptr: int, pitch: int, fields, first=0, n=None, d_instances=None):
        """The map as an array of structs in device memory (acvm_batch_export_device_records): output row i writes the record at d_ptr + i * pitch;
        fields: (witness, encoding, offset) or (witness, encoding, offset, mask_offset) tuples or RecordOutField objects -- the element of
        `encoding` that export_device writes for that witness goes to byte `offset` of the record, its mask byte (0 / 1, narrow 0 / 1 / 2) to byte
        `mask_offset`. Pointer, pitch and offsets of any alignment; no byte that no field covers is written. Row i is instance first + i, or --
        d_instances: a device array of n absolute instance numbers -- instance d_instances[i] as export_device_list reads it (n is then the
        list's length and first must be 0). Nothing is copied to the host."""
        if n is None:
            if d_instances is not None:
                raise ValueError("a list export needs n, the list's length")
            n = self.B - first
        desc, _keep = record_out_desc(pitch, fields, first, n)
        _check(lib().acvm_batch_export_device_records(self._h, C.byref(desc), d_instances, d_ptr))

    def witness_records(self, pitch: int, fields, first=0, n=None):
        """export_device_records into host memory (acvm_batch_witness_records): a uint8 array [n][pitch]; the bytes no field covers are zero."""
        import numpy as np
        n = self.B - first if n is None else n
        desc, _keep = record_out_desc(pitch, fields, first, n)
        out = np.zeros((n, pitch), dtype=np.uint8)
        _check(lib().acvm_batch_witness_records(self._h, C.byref(desc), out.ctypes.data if out.size else None))
        return out

    def wire_bound(self, container=WIRE_GZIP_STORED, witnesses=None) -> int:
        """The bytes of the longest map witness_maps_wire_device can write for this container and witness list (None: the whole map), rounded up
        to 16 (acvm_batch_wire_bound): the smallest pitch it accepts. For WIRE_GZIP_DEFLATE it is what the map costs when nothing matches, about
        0.72 of WIRE_GZIP_STORED's."""
        desc, _keep = wire_desc(container, 0, 0, witnesses)
        return _check(lib().acvm_batch_wire_bound(self._h, C.byref(desc)))

    def witness_maps_wire_device(self, d_ptr: int, container=WIRE_GZIP_STORED, witnesses=None, first=0, n=None, pitch=0, d_instances=None, d_lengths=None):
        """The WitnessMap of every output row in the reference's wire format, written on the device (acvm_batch_witness_maps_wire_device): row i's
        map goes to d_ptr + i * pitch (d_ptr 16-byte aligned; pitch a multiple of 16, 0 = wire_bound) -- WIRE_BINCODE: the bincode body,
        WIRE_GZIP_STORED: one gzip member of stored blocks around it, what decompress_witness and every inflater read,
        WIRE_GZIP_DEFLATE: one gzip member of one dynamic-Huffman block whose code and parse are fixed by the format, for the same readers at a
        fraction of the size (import_device_wire refuses it; import_device_wire_gzip reads it). One entry per witness the instance assigned, of the whole map
        or of `witnesses` (strictly ascending). d_lengths: device pointer of uint64 [n] that receives each row's length, or None; nothing at or behind a row's length is written. Row i is instance first + i, or instance d_instances[i] of a
        device array of n absolute instance numbers as export_device_list reads it. Nothing is copied to the host."""
        if n is None:
            if d_instances is not None:
                raise ValueError("a list export needs n, the list's length")
            n = self.B - first
        desc, _keep = wire_desc(container, first, n, witnesses, pitch)
        _check(lib().acvm_batch_witness_maps_wire_device(self._h, C.byref(desc), d_instances, d_ptr, d_lengths))

    def witness_maps_wire(self, container=WIRE_GZIP_STORED, witnesses=None, first=0, n=None):
        """witness_maps_wire_device into host memory (acvm_batch_witness_maps_wire): a list of n bytes objects, one serialised map per instance;
        WIRE_GZIP_DEFLATE rows are what set_initial_witness_maps_wire and decompress_witness read."""
        import numpy as np
        n = self.B - first if n is None else n
        pitch = self.wire_bound(container, witnesses)
        desc, _keep = wire_desc(container, first, n, witnesses, pitch)
        out = np.zeros(max(n * pitch, 1), dtype=np.uint8)
        lengths = np.zeros(max(n, 1), dtype=np.uint64)
        _check(lib().acvm_batch_witness_maps_wire(self._h, C.byref(desc), out.ctypes.data, lengths.ctypes.data))
        return [out[i * pitch:i * pitch + int(lengths[i])].tobytes() for i in range(n)]

    def witness_maps_wire_packed_device(self, d_ptr, capacity: int, d_offsets: int, container=WIRE_GZIP_STORED, witnesses=None, first=0, n=None, d_instances=None):
        """witness_maps_wire_device into a PACKED buffer (acvm_batch_witness_maps_wire_packed_device): row i occupies bytes [offsets[i],
        offsets[i + 1]) of d_ptr (16-byte aligned), no byte between rows; d_offsets: device pointer of uint64 [n + 1], always written. Rows
        that end at or in front of `capacity` are written complete, nothing at or behind the end of the last of them. d_ptr None with capacity 0
        is the sizing call. Returns (total, n_fit): offsets[n] and the leading rows that fit. A packed buffer of gzip members is one
        multi-member .gz file. Nothing per instance is copied to the host."""
        if n is None:
            if d_instances is not None:
                raise ValueError("a list export needs n, the list's length")
            n = self.B - first
        desc, _keep = wire_desc(container, first, n, witnesses, 0)
        total, n_fit = C.c_uint64(), C.c_uint32()
        _check(lib().acvm_batch_witness_maps_wire_packed_device(self._h, C.byref(desc), d_instances, d_ptr, capacity, d_offsets, C.byref(total), C.byref(n_fit)))
        return total.value, n_fit.value

    def witness_maps_wire_packed(self, container=WIRE_GZIP_STORED, witnesses=None, first=0, n=None, capacity=None):
        """witness_maps_wire_packed_device into host memory (acvm_batch_witness_maps_wire_packed): (bytes, offsets) -- the packed rows and
        uint64 [n + 1]. capacity None: a sizing call first, then every row; else the rows that end at or in front of it: len(bytes) is the end
        of the last of them."""
        import numpy as np
        n = self.B - first if n is None else n
        desc, _keep = wire_desc(container, first, n, witnesses, 0)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        total, n_fit = C.c_uint64(), C.c_uint32()
        if capacity is None:
            _check(lib().acvm_batch_witness_maps_wire_packed(self._h, C.byref(desc), None, 0, offsets.ctypes.data, C.byref(total), C.byref(n_fit)))
            capacity = total.value
        out = np.zeros(max(capacity, 1), dtype=np.uint8)
        _check(lib().acvm_batch_witness_maps_wire_packed(self._h, C.byref(desc), out.ctypes.data, capacity, offsets.ctypes.data, C.byref(total), C.byref(n_fit)))
        return out[:int(offsets[n_fit.value])].tobytes(), offsets

    def import_device_wire_packed(self, d_ptr: int, n_bytes: int, d_offsets: int, container, pitch: int):
        """The initial witnesses read from a PACKED buffer of serialised WitnessMaps in device memory (acvm_batch_import_device_wire_packed):
        instance j's map is bytes [offsets[j], offsets[j + 1]) of d_ptr (16-byte aligned, n_bytes long; d_offsets: device pointer of uint64
        [B + 1]), in any of the three containers -- what witness_maps_wire_packed_device writes. pitch: the staging pitch, a nonzero multiple of
        16 and the longest row accepted; B * pitch bytes of device memory are taken. Offsets that are no rows of the buffer raise
        ("wire offsets: ...") and the batch keeps the initial witnesses it had; then import_device_wire / import_device_wire_gzip run."""
        desc = WireInDesc(container=container, pitch=pitch)
        _check(lib().acvm_batch_import_device_wire_packed(self._h, C.byref(desc), d_ptr, n_bytes, d_offsets))

    def outcomes_device(self, first=0, n=None, d_status=None, d_err=None, d_opcode_index=None, select_mask=0, d_selected=None, count=True):
        """The outcomes of instances [first, first + n) as device columns (acvm_batch_outcomes_device): d_status / d_err uint8 [n], d_opcode_index uint32 [n],
        each a device pointer or None; d_selected: device pointer of uint32 [n] that receives the ascending absolute numbers of the instances whose
        status has its bit set in select_mask (1 << STATUS_SOLVED ...). Returns the number selected (None with count=False)."""
        n = self.B - first if n is None else n
        desc = OutcomesDesc(first=first, n=n, d_status=d_status, d_err=d_err, d_opcode_index=d_opcode_index, select_mask=select_mask, d_selected=d_selected)
        got = C.c_uint32()
        _check(lib().acvm_batch_outcomes_device(self._h, C.byref(desc), C.byref(got) if count else None))
        return got.value if count else None

    def export_h2d_bytes(self) -> int:
        """bytes the device exports and outcomes_device have copied host-to-device for this handle so far (acvm_debug_export_h2d_bytes)"""
        return lib().acvm_debug_export_h2d_bytes(self._h)

    def digest(self, first=0, n=None):
        """Per-instance 32-byte digest of the witness map (acvm_batch_digest): uint8 array [n][32]."""
        import numpy as np
        n = self.B - first if n is None else n
        out = np.zeros((n, 32), dtype=np.uint8)
        _check(lib().acvm_batch_digest(self._h, first, n, out.ctypes.data))
        return out

    def digest_blake2s(self, first=0, n=None):
        """Per-instance Blake2s tree digest of the witness map's BYTES (acvm_batch_digest_blake2s): uint8 array [n][32]."""
        import numpy as np
        n = self.B - first if n is None else n
        out = np.zeros((n, 32), dtype=np.uint8)
        _check(lib().acvm_batch_digest_blake2s(self._h, first, n, out.ctypes.data))
        return out

    def witness_map_bytes(self, instance: int) -> bytes:
        """The instance's WitnessMap in the reference's wire format (finalize() + compressWitness)."""
        n = _check(lib().acvm_batch_witness_map_bytes(self._h, instance, None, 0))
        out = C.create_string_buffer(max(n, 1))
        _check(lib().acvm_batch_witness_map_bytes(self._h, instance, out, n))
        return out.raw[:n]

    def get_pending_foreign_call(self, instance: int):
        """ACVM::get_pending_foreign_call: None, or (function, [[int, ...] per input])."""
        info = ForeignCallInfo()
        if _check(lib().acvm_batch_pending_foreign_call(self._h, instance, C.byref(info))) == 0:
            return None
        lens = (C.c_uint32 * max(info.n_inputs, 1))()
        vals = C.create_string_buffer(32 * max(info.n_values, 1))
        _check(lib().acvm_batch_pending_foreign_call_inputs(self._h, instance, lens, vals))
        out, k = [], 0
        for i in range(info.n_inputs):
            out.append([int.from_bytes(vals.raw[32 * (k + c):32 * (k + c + 1)], "big") for c in range(lens[i])])
            k += lens[i]
        return info.function.decode(), out

    def resolve_pending_foreign_call(self, instance: int, values):
        """values: list of int (Single) or list[int] (Array), like ForeignCallResult."""
        is_arr = bytes(0 if isinstance(v, int) else 1 for v in values)
        lens = (C.c_uint32 * max(len(values), 1))(*[1 if isinstance(v, int) else len(v) for v in values])
        flat = b"".join(int(v).to_bytes(32, "big") if isinstance(v, int) else b"".join(int(x).to_bytes(32, "big") for x in v) for v in values)
        _check(lib().acvm_batch_resolve_foreign_call(self._h, instance, len(values), is_arr, lens, flat))

    def foreign_call_sites(self):
        """The sites at which instances wait (acvm_batch_foreign_call_sites), ascending by (opcode, brillig index): a list of dicts with opcode_index,
        brillig_index, n_inputs, n_waiting, n_resolved, function. Host only."""
        n = _check(lib().acvm_batch_foreign_call_sites(self._h, None, 0))
        arr = (ForeignCallSite * max(n, 1))()
        n = min(n, _check(lib().acvm_batch_foreign_call_sites(self._h, arr, n)))
        return [dict(opcode_index=s.opcode_index, brillig_index=s.brillig_index, n_inputs=s.n_inputs, n_waiting=s.n_waiting, n_resolved=s.n_resolved,
                     function=s.function.decode()) for s in arr[:n]]

    def foreign_call_inputs_device(self, opcode_index: int, brillig_index: int, first_row=0, n_rows=None, d_values=None, encoding=ENC_BE32,
                                   layout=LAYOUT_INSTANCE_MAJOR, n_columns=0, stride=0, d_instances=None, d_lens=None, d_mask=None) -> int:
        """The pending inputs of rows [first_row, first_row + n_rows) of the site's waiting list into device memory (acvm_batch_foreign_call_inputs_device):
        d_values / d_mask hold n_columns elements per row in `encoding`, `layout` and `stride` (in elements, 0 = dense) as export_device writes witnesses;
        d_instances uint32 [n_rows], d_lens uint32 [n_rows][n_inputs]; each a device pointer or None. Returns the largest number of values of a row --
        with no pointer given that is the sizing call. n_rows None: to the end of the list. No value is copied to the host."""
        if n_rows is None:
            here = [s for s in self.foreign_call_sites() if (s["opcode_index"], s["brillig_index"]) == (opcode_index, brillig_index)]
            n_rows = max((here[0]["n_waiting"] if here else 0) - first_row, 0)
        desc = ForeignCallInputsDesc(opcode_index=opcode_index, brillig_index=brillig_index, first_row=first_row, n_rows=n_rows, encoding=encoding, layout=layout,
                                     n_columns=n_columns, stride=stride, d_instances=d_instances, d_lens=d_lens, d_values=d_values, d_mask=d_mask)
        longest = C.c_uint32()
        _check(lib().acvm_batch_foreign_call_inputs_device(self._h, C.byref(desc), C.byref(longest)))
        return longest.value

    def resolve_foreign_calls_device(self, opcode_index: int, brillig_index: int, shape, d_values: int, first_row=0, n_rows=None, encoding=ENC_BE32,
                                     layout=LAYOUT_INSTANCE_MAJOR, n_columns=None, stride=0):
        """ACVM::resolve_pending_foreign_call for rows [first_row, first_row + n_rows) of the site's waiting list at once
        (acvm_batch_resolve_foreign_calls_device). shape: one entry per output of the ForeignCallResult, None for a single value or the length of an
        array -- the same for every row; d_values: device pointer, the row's values back to back in columns 0 .. total - 1, read as import_device
        reads a buffer (n_columns None: the shape's total). No value is copied from the host."""
        shape = list(shape)
        if n_rows is None:
            here = [s for s in self.foreign_call_sites() if (s["opcode_index"], s["brillig_index"]) == (opcode_index, brillig_index)]
            n_rows = max((here[0]["n_waiting"] if here else 0) - first_row, 0)
        is_arr = bytes(0 if n is None else 1 for n in shape)
        lens = (C.c_uint32 * max(len(shape), 1))(*[1 if n is None else n for n in shape])
        total = sum(1 if n is None else n for n in shape)
        desc = ForeignCallAnswersDesc(opcode_index=opcode_index, brillig_index=brillig_index, first_row=first_row, n_rows=n_rows, n_values=len(shape), is_array=is_arr,
                                      lens=lens, encoding=encoding, layout=layout, n_columns=total if n_columns is None else n_columns, stride=stride, d_values=d_values)
        _check(lib().acvm_batch_resolve_foreign_calls_device(self._h, C.byref(desc)))

    def resolve_foreign_calls_device_rows(self, opcode_index: int, brillig_index: int, shape, d_values, first_row=0, n_rows=None, encoding=ENC_BE32,
                                          layout=LAYOUT_INSTANCE_MAJOR, n_columns=None, stride=0, d_lens=None, d_answered=None):
        """resolve_foreign_calls_device with per-row answers (acvm_batch_resolve_foreign_calls_device_rows). d_lens: device pointer, uint32
        [n_rows][len(shape)] row-major, the length of array output k of row i (None: the lengths of `shape` hold for every row; with d_lens an array
        entry of `shape` only has to be not None); d_answered: device pointer, one byte per row, 0 = the row is not answered and keeps waiting (None:
        every row is answered). n_columns None: the shape's total."""
        shape = list(shape)
        if n_rows is None:
            here = [s for s in self.foreign_call_sites() if (s["opcode_index"], s["brillig_index"]) == (opcode_index, brillig_index)]
            n_rows = max((here[0]["n_waiting"] if here else 0) - first_row, 0)
        is_arr = bytes(0 if n is None else 1 for n in shape)
        lens = (C.c_uint32 * max(len(shape), 1))(*[1 if n is None else n for n in shape])
        total = sum(1 if n is None else n for n in shape)
        desc = ForeignCallAnswersRowsDesc(opcode_index=opcode_index, brillig_index=brillig_index, first_row=first_row, n_rows=n_rows, n_values=len(shape),
                                          is_array=is_arr, lens=lens, encoding=encoding, layout=layout, n_columns=total if n_columns is None else n_columns,
                                          stride=stride, d_values=d_values, d_lens=d_lens, d_answered=d_answered)
        _check(lib().acvm_batch_resolve_foreign_calls_device_rows(self._h, C.byref(desc)))

    def foreign_call_stats(self) -> dict:
        """bytes both forms of the foreign-call round trip copied over PCIe for this handle so far, and the device times of the last batch-wide kernels
        and the device bytes of the result store's tables
        (acvm_debug_foreign_call_stats)"""
        h2d, d2h, t_in, t_app, store = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double(), C.c_uint64()
        _check(lib().acvm_debug_foreign_call_stats(self._h, C.byref(h2d), C.byref(d2h), C.byref(t_in), C.byref(t_app), C.byref(store)))
        return dict(h2d_bytes=h2d.value, d2h_bytes=d2h.value, inputs_kernel_ms=t_in.value, append_kernel_ms=t_app.value, store_bytes=store.value)

    def brillig_resume_stats(self) -> dict:
        """what the Brillig retry passes of the last solve did under tuning(brillig_resume=1), all zero otherwise (acvm_debug_brillig_resume_stats)"""
        out = (C.c_uint64 * 6)()
        _check(lib().acvm_debug_brillig_resume_stats(self._h, out))
        return dict(zip(("passes", "lanes_continued", "lanes_restarted", "cells_relocated", "steps_executed", "relocation_launches"), (int(v) for v in out)))

    def stats(self) -> dict:
        s = Stats()
        _check(lib().acvm_batch_stats(self._h, C.byref(s)))
        return s.as_dict()


class DeviceBuffer:
    """hipMalloc'd bytes on the current device (acvm_device_malloc): inputs a caller keeps resident in HBM."""

    def __init__(self, data: bytes = None, size: int = None):
        self.size = len(data) if data is not None else size
        self.ptr = lib().acvm_device_malloc(self.size)
        if not self.ptr:
            raise AcvmError(lib().acvm_last_error().decode())
        if data is not None:
            self.upload(data)

    def upload(self, data, offset=0):
        import numpy as np
        buf = np.frombuffer(data, dtype=np.uint8)
        if offset + buf.size > self.size:
            raise ValueError("upload past the end of the device buffer")
        _check(lib().acvm_device_upload(self.ptr + offset, buf.ctypes.data, buf.size))

    def download(self, size=None, offset=0) -> bytes:
        """`size` bytes from `offset` on (default: to the end of the buffer), copied to the host (acvm_device_download)"""
        size = self.size - offset if size is None else size
        if offset < 0 or size < 0 or offset + size > self.size:
            raise ValueError("download past the end of the device buffer")
        out = C.create_string_buffer(max(size, 1))
        _check(lib().acvm_device_download(out, self.ptr + offset, size))
        return out.raw[:size]

    def free(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.acvm_device_free(self.ptr)
            self.ptr = None

    __del__ = free


class Acvm:
    """struct ACVM (acvm/src/pwg/mod.rs:129-304) for one instance: the acvm_new / acvm_solve / acvm_finalize shim."""

    def __init__(self, circuit: Circuit, initial_witness: dict, backend: "BbSolver" = None):
        self.circuit = circuit
        self._backend = backend
        items = list(initial_witness.items())
        ids = (C.c_uint32 * max(len(items), 1))(*[k for k, _ in items])
        vals = b"".join(int(v % (1 << 256)).to_bytes(32, "big") for _, v in items)
        self._h = lib().acvm_new(circuit._h, C.byref(backend) if backend is not None else None, ids, vals, len(items))
        if not self._h:
            raise AcvmError(lib().acvm_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.acvm_free(self._h)
            self._h = None

    def solve(self) -> int:
        return _check(lib().acvm_solve(self._h))

    def solve_opcode(self) -> int:
        return _check(lib().acvm_solve_opcode(self._h))

    def status(self) -> Result:
        r = Result()
        _check(lib().acvm_get_status(self._h, C.byref(r)))
        return r

    def instruction_pointer(self) -> int:
        return lib().acvm_instruction_pointer(self._h)

    def _pairs(self, fn):
        n = fn(self._h, None, None, 0)
        if n < 0:
            raise AcvmError(f"acvm_amd error {n}: {lib().acvm_last_error().decode()}")
        ids = (C.c_uint32 * max(n, 1))()
        vals = C.create_string_buffer(32 * max(n, 1))
        _check(fn(self._h, ids, vals, n))
        return {ids[i]: int.from_bytes(vals.raw[32 * i:32 * i + 32], "big") for i in range(n)}

    def witness_map(self) -> dict:
        return self._pairs(lib().acvm_witness_map)

    def finalize(self) -> dict:
        """ACVM::finalize: raises unless the status is Solved (the reference panics)."""
        return self._pairs(lib().acvm_finalize)

    def get_pending_foreign_call(self):
        info = ForeignCallInfo()
        if _check(lib().acvm_get_pending_foreign_call(self._h, C.byref(info))) == 0:
            return None
        lens = (C.c_uint32 * max(info.n_inputs, 1))()
        vals = C.create_string_buffer(32 * max(info.n_values, 1))
        _check(lib().acvm_pending_foreign_call_inputs(self._h, lens, vals))
        out, k = [], 0
        for i in range(info.n_inputs):
            out.append([int.from_bytes(vals.raw[32 * (k + c):32 * (k + c + 1)], "big") for c in range(lens[i])])
            k += lens[i]
        return info.function.decode(), out

    def resolve_pending_foreign_call(self, values):
        is_arr = bytes(0 if isinstance(v, int) else 1 for v in values)
        lens = (C.c_uint32 * max(len(values), 1))(*[1 if isinstance(v, int) else len(v) for v in values])
        flat = b"".join(int(v).to_bytes(32, "big") if isinstance(v, int) else b"".join(int(x).to_bytes(32, "big") for x in v) for v in values)
        _check(lib().acvm_resolve_pending_foreign_call(self._h, len(values), is_arr, lens, flat))


class MultiBatch:
    """acvm_multi_*: instances whose initial witness maps assign different id sets (list of {witness: int} dicts)."""

    def __init__(self, circuit: Circuit, initial_maps, solver: "BbSolver" = None):
        import numpy as np
        self.circuit = circuit
        self._solver = solver
        self.n = len(initial_maps)
        offsets = np.zeros(self.n + 1, dtype=np.uint64)
        ids, vals = [], []
        for i, m in enumerate(initial_maps):
            for k, v in m.items():
                ids.append(k)
                vals.append(int(v % (1 << 256)).to_bytes(32, "big"))
            offsets[i + 1] = len(ids)
        ids_arr = np.asarray(ids if ids else [0], dtype=np.uint32)
        self._h = lib().acvm_multi_new(circuit._h, C.byref(solver) if solver is not None else None, self.n, offsets.ctypes.data, ids_arr.ctypes.data,
                                       b"".join(vals))
        if not self._h:
            raise AcvmError(lib().acvm_last_error().decode())
        self.n_groups = lib().acvm_multi_num_groups(self._h)
        self.nw = lib().acvm_multi_num_witnesses(self._h)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.acvm_multi_free(self._h)
            self._h = None

    def solve(self) -> int:
        return _check(lib().acvm_multi_solve(self._h))

    def results(self):
        out = (Result * max(self.n, 1))()
        _check(lib().acvm_multi_results(self._h, C.cast(out, C.c_void_p)))
        return out

    def witness_map(self, instance: int):
        import numpy as np
        asg = np.zeros((self.nw,), dtype=np.uint8)
        vals = np.zeros((self.nw, 32), dtype=np.uint8)
        _check(lib().acvm_multi_witness_map(self._h, instance, asg.ctypes.data, vals.ctypes.data))
        return asg, vals
