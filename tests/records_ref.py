"""What tests/test_gpu_records.py and tests/test_gpu_node_records.py share: packed records as bytes and the meaning of their elements, by Python
integers and index arithmetic only, and the record shapes both use. A field is (position, encoding, offset) as acvm_record_field_t."""
import numpy as np

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BE32, LE32, MONT = 0, 1, 2
U8, U16, U32, U64, U128 = 16, 17, 18, 19, 20
PATTERN = 0xA5


def size_of(encoding):
    return 1 << (encoding - U8) if U8 <= encoding <= U128 else 32


def meaning(raw, encoding):
    """the field element the element's bytes, as they lie in memory, mean: every string is valid"""
    if encoding == BE32:
        return int.from_bytes(raw, "big") % P
    if encoding == MONT:
        return int.from_bytes(raw, "little") * pow(1 << 256, -1, P) % P
    return int.from_bytes(raw, "little") % P


def element(v, encoding):
    """the bytes an exporter writes for the value v (below p; below 2^width for a narrow encoding)"""
    if encoding == BE32:
        return int(v).to_bytes(32, "big")
    if encoding == MONT:
        return ((int(v) << 256) % P).to_bytes(32, "little")
    return int(v).to_bytes(size_of(encoding), "little")


def build_records(B, pitch, fields, raws, lead=0, pattern=PATTERN):
    """raws[j][position]: the bytes of that element of instance j. The whole buffer: `lead` bytes, then B records of `pitch` bytes; every byte
    that belongs to no field holds `pattern`. Exactly lead + B * pitch bytes."""
    buf = np.full(lead + B * pitch, pattern, dtype=np.uint8)
    for j in range(B):
        for position, encoding, offset in fields:
            raw = raws[j][position]
            assert len(raw) == size_of(encoding) and offset + len(raw) <= pitch
            at = lead + j * pitch + offset
            buf[at:at + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return buf.tobytes()


def values_of(raws, fields, n_in):
    """vals[j][position]: the value every input holds after the import"""
    enc = {position: encoding for position, encoding, _ in fields}
    return [[meaning(r[k], enc[k]) for k in range(n_in)] for r in raws]


# fn main(msg: [u8; 8], a: Field, b: Field, root: Field) of tests/test_gpu_typed_io.py as one packed 108-byte record per instance: seven bytes, the
# eighth as a u16 (so that a record can hold 256 there and fail its RANGE check), a at an odd offset, three bytes of padding in front of root
MIXED_STRUCT_PITCH = 108
MIXED_STRUCT_FIELDS = [(k, U8, k) for k in range(7)] + [(7, U16, 7), (8, BE32, 9), (9, MONT, 41), (10, LE32, 76)]


def mixed_struct_raws(rows):
    """rows[j]: the 11 values of instance j (the first eight below 256 resp. 65536)"""
    enc = {position: encoding for position, encoding, _ in MIXED_STRUCT_FIELDS}
    return [[element(v, enc[k]) for k, v in enumerate(r)] for r in rows]
