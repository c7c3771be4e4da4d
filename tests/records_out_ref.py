"""What tests/test_gpu_records_out.py builds its expected buffers with: the bytes the record export writes, by Python integers and index
arithmetic only, on top of tests/records_ref.py. An out field is (witness, encoding, offset, mask offset or None) as acvm_record_out_field_t."""
import numpy as np

import records_ref as rr
from records_ref import PATTERN, size_of

TAIL = 64  # bytes behind the last record that lie inside the allocation: a stray store is seen, not faulted on


def element_and_mask(value, assigned, encoding):
    """the element's bytes and its mask byte: an unassigned element is zero bytes and mask 0; a narrow element holds the low bytes of the value
    whether it fits (mask 1) or not (mask 2)"""
    size = size_of(encoding)
    if not assigned:
        return bytes(size), 0
    if size == 32:
        return rr.element(value, encoding), 1
    return (value % (1 << (8 * size))).to_bytes(size, "little"), 1 if value < (1 << (8 * size)) else 2


def expected_buffer(lead, pitch, fields, rows, asg, vals, padding=PATTERN, tail=TAIL):
    """The whole buffer after an export into lead + len(rows) * pitch + tail bytes of `padding`. rows[i]: the instance output row i holds (an
    index into asg / vals, the arrays of Batch.witness_map), or None for an instance that assigned nothing. A witness beyond the arrays' width is
    unassigned."""
    buf = np.full(lead + len(rows) * pitch + tail, padding, dtype=np.uint8)
    nw = asg.shape[1]
    for i, j in enumerate(rows):
        for w, encoding, offset, mask_offset in fields:
            assigned = j is not None and w < nw and bool(asg[j, w])
            value = int.from_bytes(vals[j, w].tobytes(), "big") if assigned else 0
            raw, mask = element_and_mask(value, assigned, encoding)
            at = lead + i * pitch + offset
            buf[at:at + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
            if mask_offset is not None:
                buf[lead + i * pitch + mask_offset] = mask
    return buf


def covered(pitch, fields):
    """which bytes of a record a field or a mask byte covers"""
    c = np.zeros(pitch, dtype=bool)
    for w, encoding, offset, mask_offset in fields:
        assert not c[offset:offset + size_of(encoding)].any()
        c[offset:offset + size_of(encoding)] = True
        if mask_offset is not None:
            assert not c[mask_offset]
            c[mask_offset] = True
    return c
