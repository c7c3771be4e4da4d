"""The gzip import (acvm_batch_import_device_wire_gzip) measured in one process at B = 2^16 for handles of 8, 64 and 440 initial witnesses. The
rows are 256 distinct maps of random field elements, repeated over the batch, written (a) by zlib at level 9 -- what compressWitness's
GzEncoder / Compression::best() is -- and (b) by this library's own ACVM_WIRE_GZIP_DEFLATE export. Timed, wall time of the synchronous call:

  gzip device     the new device form on device-resident rows, (a) and (b)
  bincode device  acvm_batch_import_device_wire(ACVM_WIRE_BINCODE) of the same bodies: the floor, stage 2 alone
  old host form   acvm_batch_set_initial_witness_maps_wire of rows (a) in host memory: every row inflated by zlib on one host thread, the
                  inflated bodies uploaded. Its code is untouched: this is the parent commit's path, in the same process.
  new host form   acvm_batch_set_initial_witness_maps_gzip of the same host rows: uploaded compressed, inflated on the device

with the bytes each host form sends over PCIe (the staged slots; the tables of a few KiB are left out). No ratio is asserted.
    python tools/t_wire_inflate.py [--log2-tile 16] [--sizes 8,64,440] [--turns 5] [--host-turns 2] [--no-host]"""
import argparse
import os
import random
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd.acir import P, Circuit, Expression as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-tile", type=int, default=16)
ap.add_argument("--sizes", default="8,64,440")
ap.add_argument("--turns", type=int, default=5)
ap.add_argument("--host-turns", type=int, default=2)
ap.add_argument("--no-host", action="store_true", help="the device forms only")
args = ap.parse_args()
B = 1 << args.log2_tile
DISTINCT = min(256, B)
L = acvm_amd.lib()
BINCODE, DEFLATE = acvm_amd.WIRE_BINCODE, acvm_amd.WIRE_GZIP_DEFLATE


def wall_ms(fn):
    t0 = time.perf_counter()
    rc = fn()
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, L.acvm_last_error()
    return ms


def median(fn, turns):
    ms = sorted(wall_ms(fn) for _ in range(turns))
    return ms[len(ms) // 2], ms[0], ms[-1]


def body(n_in, rng):
    out = [n_in.to_bytes(8, "little")]
    for w in range(1, n_in + 1):
        out.append(w.to_bytes(4, "little") + (64).to_bytes(8, "little") + b"%064x" % rng.randrange(P))
    return b"".join(out)


def tiled(rows, pitch):
    """(the B slots -- the distinct rows repeated -- as one array, the B lengths)"""
    block = np.zeros((len(rows), pitch), dtype=np.uint8)
    for k, r in enumerate(rows):
        block[k, :len(r)] = np.frombuffer(r, dtype=np.uint8)
    lengths = np.array([len(r) for r in rows], dtype=np.uint64)
    return np.tile(block, (B // len(rows), 1)), np.tile(lengths, B // len(rows))


def measure(n_in):
    rng = random.Random(0x1F8B7000 + n_in)
    ids = list(range(1, n_in + 1))
    circuit = acvm_amd.Circuit(Circuit(n_in + 1, [E([], [(1, 1), (P - 1, n_in + 1)], 1)]).to_bytes())
    bodies = [body(n_in, rng) for _ in range(DISTINCT)]
    members = []
    for b in bodies:
        c = zlib.compressobj(9, zlib.DEFLATED, 31)
        members.append(c.compress(b) + c.flush())
    body_pitch = (len(bodies[0]) + 15) // 16 * 16
    zlib_pitch = (max(len(m) for m in members) + 15) // 16 * 16
    h_bodies, h_body_len = tiled(bodies, body_pitch)
    h_zlib, h_zlib_len = tiled(members, zlib_pitch)
    d_bodies, d_body_len = acvm_amd.DeviceBuffer(h_bodies.tobytes()), acvm_amd.DeviceBuffer(h_body_len.tobytes())
    d_zlib, d_zlib_len = acvm_amd.DeviceBuffer(h_zlib.tobytes()), acvm_amd.DeviceBuffer(h_zlib_len.tobytes())
    # (b): the same maps through a first handle, written by the export in its own deflating container
    first = acvm_amd.Batch(circuit, B, ids)
    first.import_device_wire(d_bodies.ptr, BINCODE, body_pitch, d_body_len.ptr)
    first.solve()
    own_pitch = first.wire_bound(DEFLATE, ids)
    d_own, d_own_len = acvm_amd.DeviceBuffer(size=B * own_pitch), acvm_amd.DeviceBuffer(size=B * 8)
    first.witness_maps_wire_device(d_own.ptr, DEFLATE, ids, n=B, pitch=own_pitch, d_lengths=d_own_len.ptr)
    own_bytes = int(np.frombuffer(d_own_len.download(), dtype=np.uint64).sum())
    first.free()
    second = acvm_amd.Batch(circuit, B, ids)
    gz = lambda pitch: acvm_amd.WireInDesc(container=DEFLATE, pitch=pitch)
    bin_desc, zlib_desc, own_desc = acvm_amd.WireInDesc(container=BINCODE, pitch=body_pitch), gz(zlib_pitch), gz(own_pitch)
    calls = {
        "bincode device (floor)": lambda: L.acvm_batch_import_device_wire(second._h, bin_desc, d_bodies.ptr, d_body_len.ptr),
        "gzip device, zlib level 9": lambda: L.acvm_batch_import_device_wire_gzip(second._h, zlib_desc, d_zlib.ptr, d_zlib_len.ptr),
        "gzip device, own deflate": lambda: L.acvm_batch_import_device_wire_gzip(second._h, own_desc, d_own.ptr, d_own_len.ptr),
    }
    body_bytes, zlib_bytes = int(h_body_len.sum()), int(h_zlib_len.sum())
    print(f"{n_in} initial witnesses, B = 2^{args.log2_tile}: bodies {body_bytes / 1e6:.1f} MB, zlib-9 members {zlib_bytes / 1e6:.1f} MB ({zlib_bytes / body_bytes:.3f}), "
          f"own deflate members {own_bytes / 1e6:.1f} MB ({own_bytes / body_bytes:.3f})", flush=True)
    state = {}
    for k, fn in calls.items():
        assert fn() == 0, L.acvm_last_error()  # warm-up, and what each leaves
        if B * n_in <= 1 << 22:
            state[k] = second.import_state()
    if state:
        floor = state["bincode device (floor)"]
        print("  the three leave the same state:", all(np.array_equal(floor[key], s[key]) for s in state.values() for key in floor), flush=True)
    med = {}
    for k, fn in calls.items():
        med[k], lo, hi = median(fn, args.turns)
        print(f"  {k:28s} ms median {med[k]:9.3f} min {lo:9.3f} max {hi:9.3f} | {body_bytes / med[k] / 1e6:7.2f} GB/s of inflated body", flush=True)
    for k in list(calls)[1:]:
        print(f"  {k}: {med[k] / med['bincode device (floor)']:.2f} x the floor", flush=True)
    if args.no_host:
        for x in (d_bodies, d_body_len, d_zlib, d_zlib_len, d_own, d_own_len, second):
            x.free()
        return
    # ---- from host memory
    host_calls = {
        "old host form (zlib on one host thread)": lambda: L.acvm_batch_set_initial_witness_maps_wire(second._h, h_zlib.ctypes.data, zlib_pitch, h_zlib_len.ctypes.data),
        "new host form (inflated on the device)": lambda: L.acvm_batch_set_initial_witness_maps_gzip(second._h, h_zlib.ctypes.data, zlib_pitch, h_zlib_len.ctypes.data),
    }
    pcie = {"old host form (zlib on one host thread)": B * body_pitch, "new host form (inflated on the device)": B * (zlib_pitch + 8)}
    hmed = {}
    for k, fn in host_calls.items():
        assert fn() == 0, L.acvm_last_error()
        hmed[k], lo, hi = median(fn, args.host_turns)
        print(f"  {k:40s} ms median {hmed[k]:10.2f} min {lo:10.2f} max {hi:10.2f} | {pcie[k] / 1e6:8.1f} MB over PCIe", flush=True)
    old, new = (hmed[k] for k in host_calls)
    print(f"  new host form / old host form: {new / old:.3f} of the time ({old / new:.1f} x), {pcie['new host form (inflated on the device)'] / pcie['old host form (zlib on one host thread)']:.3f} of the bytes", flush=True)
    for x in (d_bodies, d_body_len, d_zlib, d_zlib_len, d_own, d_own_len, second):
        x.free()


for size in args.sizes.split(","):
    measure(int(size))
