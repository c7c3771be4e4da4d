"""The batch-wide WitnessMap wire format (include/acvm_amd.h acvm_batch_witness_maps_wire_device) restated in Python: the bincode body, the
stored-block gzip member with its exact framing, and the slots of many maps at a pitch in a buffer of 0xA5. A map is {witness: int}. Pinned
by tests/test_wire_ref.py against acvm_amd.compress_witness / decompress_witness and Python's inflaters."""
import struct
import zlib

BINCODE, GZIP_STORED = 0, 1
ENTRY, BLOCK = 76, 65532
HEADER = bytes.fromhex("1f 8b 08 08 00 00 00 00 00 ff 00")  # deflate, FNAME with an empty name, MTIME 0, XFL 0, OS 255
EMPTY_BLOCK = bytes.fromhex("000000ffff")
FILL = 0xA5


def body(witness_map):
    """u64le N, then per entry in ascending order u32le witness, u64le 64, 64 lowercase hex characters of the big-endian value"""
    out = [struct.pack("<Q", len(witness_map))]
    for w in sorted(witness_map):
        out.append(struct.pack("<IQ", w, 64) + b"%064x" % witness_map[w])
    return b"".join(out)


def n_blocks(body_len):
    return (body_len + BLOCK - 1) // BLOCK


def member(body_bytes):
    """one gzip member of stored blocks of 65 532 bytes around the body, three empty stored blocks in front of every block header but the first"""
    L = len(body_bytes)
    out = [HEADER]
    for k in range(n_blocks(L)):
        chunk = body_bytes[k * BLOCK:(k + 1) * BLOCK]
        final = 1 if (k + 1) * BLOCK >= L else 0
        if k:
            out.append(EMPTY_BLOCK * 3)
        out.append(struct.pack("<BHH", final, len(chunk), len(chunk) ^ 0xFFFF) + chunk)
    out.append(struct.pack("<II", zlib.crc32(body_bytes), L & 0xFFFFFFFF))
    return b"".join(out)


def encode(witness_map, container):
    b = body(witness_map)
    return member(b) if container == GZIP_STORED else b


def length(container, n_entries):
    L = 8 + ENTRY * n_entries
    return 16 + L + 20 * (n_blocks(L) - 1) + 8 if container == GZIP_STORED else L


def bound(container, n_positions):
    return (length(container, n_positions) + 15) // 16 * 16


def body_offset(container, k):
    """where body byte k lies in the slot"""
    return 16 + k + 20 * (k // BLOCK) if container == GZIP_STORED else k


def slots(maps, container, pitch, tail=0):
    """(the buffer of len(maps) * pitch + tail bytes -- 0xA5 wherever no map's byte lies -- and the lengths)"""
    buf = bytearray([FILL]) * (len(maps) * pitch + tail)
    lengths = []
    for i, m in enumerate(maps):
        e = encode(m, container)
        assert len(e) <= pitch
        buf[i * pitch:i * pitch + len(e)] = e
        lengths.append(len(e))
    return bytes(buf), lengths


def restrict(witness_map, witnesses):
    """the entries of a map that a witness list names"""
    return {w: witness_map[w] for w in witnesses if w in witness_map}
