"""The deflating container of the batch-wide wire format (ACVM_WIRE_GZIP_DEFLATE) measured against ACVM_WIRE_GZIP_STORED in one process:
the same rows leave as stored members (A) and as deflated members (B), A-B-A-B after a warm-up call of each, on

 1. the metric's circuit with its own values: the whole map of a range of instances, and a 64-witness list of the whole tile;
 2. a read-back circuit (outputs 3 x + 1) fed bits, bytes and u32s: the whole map of a range, and a 64-witness list of the whole tile.

Per case: wall time of the synchronous calls (tools/t_wire.py says what that includes), bytes written and the rate as a fraction of the HBM
peak given by --hbm-gbs, the deflated bytes against zlib level 1 and level 9 over a sample of 256 rows, and the time zlib takes for those rows
on one host core scaled to the rows of the call. For the kernel's time alone run under `rocprofv3 --kernel-trace --stats` and read
wire_deflate_kernel.
    python tools/t_wire_deflate.py [--gates 10000] [--log2-tile 17] [--log2-range 14] [--turns 5] [--inputs 128] [--hbm-gbs 8000]"""
import argparse
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd import synth  # noqa: E402
from acvm_amd.acir import P, Circuit, Expression as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gates", type=int, default=10000)
ap.add_argument("--log2-tile", type=int, default=17)
ap.add_argument("--log2-range", type=int, default=14)
ap.add_argument("--turns", type=int, default=5)
ap.add_argument("--inputs", type=int, default=128)
ap.add_argument("--hbm-gbs", type=float, default=8000.0)
args = ap.parse_args()
B = 1 << args.log2_tile
STORED, DEFLATE, BINCODE = acvm_amd.WIRE_GZIP_STORED, acvm_amd.WIRE_GZIP_DEFLATE, acvm_amd.WIRE_BINCODE
L = acvm_amd.lib()
SAMPLE = 256


def wall_ms(fn):
    t0 = time.perf_counter()
    rc = fn()
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, L.acvm_last_error()
    return ms


def measure(batch, what, first, n, witnesses):
    pitch = {c: batch.wire_bound(c, witnesses) for c in (STORED, DEFLATE)}
    d_wire = acvm_amd.DeviceBuffer(size=n * pitch[STORED])
    d_len = acvm_amd.DeviceBuffer(size=n * 8)
    keep = {c: acvm_amd.wire_desc(c, first, n, witnesses, pitch[c]) for c in (STORED, DEFLATE)}
    calls = {c: (lambda c=c: L.acvm_batch_witness_maps_wire_device(batch._h, keep[c][0], None, d_wire.ptr, d_len.ptr)) for c in (STORED, DEFLATE)}
    written = {}
    for c in (STORED, DEFLATE):  # the warm-up, and the bytes
        calls[c]()
        written[c] = int(np.frombuffer(d_len.download(), dtype=np.uint64).sum())
    times = {c: [] for c in calls}
    for _ in range(args.turns):
        for c in (STORED, DEFLATE):
            times[c].append(wall_ms(calls[c]))
    med = {c: sorted(t)[len(t) // 2] for c, t in times.items()}
    print(f"{what}: {n} rows, slots of {pitch[STORED]} / {pitch[DEFLATE]} bytes", flush=True)
    for c, name in ((STORED, "A GZIP_STORED "), (DEFLATE, "B GZIP_DEFLATE")):
        gbs = written[c] / med[c] / 1e6
        print(f"  {name} ms median {med[c]:9.3f} min {min(times[c]):9.3f} max {max(times[c]):9.3f} | {written[c] / 1e6:10.2f} MB written, {gbs:8.1f} GB/s, "
              f"{gbs / args.hbm_gbs:.3f} of the HBM peak | {med[c] * 1e3 / n:8.3f} us per row", flush=True)
    print(f"  B / A: time {med[DEFLATE] / med[STORED]:.2f}, bytes {written[DEFLATE] / written[STORED]:.4f}; the {(written[STORED] - written[DEFLATE]) / 1e6:.1f} MB saved "
          f"take {(written[STORED] - written[DEFLATE]) / 64e9 * 1e3:.2f} ms at 64 GB/s of PCIe, the deflate export {med[DEFLATE] - med[STORED]:+.2f} ms more than the stored one", flush=True)
    # a sample of rows: the device's members against zlib
    m = min(SAMPLE, n)
    bodies = batch.witness_maps_wire(BINCODE, witnesses, first=first, n=m)
    ours = batch.witness_maps_wire(DEFLATE, witnesses, first=first, n=m)
    assert all(zlib.decompress(o, 31) == b for o, b in zip(ours, bodies))
    total = sum(len(b) for b in bodies)
    line = f"  {m} rows, {total} body bytes: the device {sum(len(o) for o in ours) / total:.4f}"
    for level in (1, 9):
        t0 = time.perf_counter()
        size = sum(len(zlib.compress(b, level)) for b in bodies)
        s = time.perf_counter() - t0
        line += f"; zlib level {level} {size / total:.4f} in {s * 1e3:.1f} ms, {s * n / m * 1e3:.0f} ms for the {n} rows on one core"
    print(line, flush=True)
    d_wire.free()
    d_len.free()


def readback(n_in):
    ops = [E([], [(3, k), (P - 1, n_in + k)], 1) for k in range(1, n_in + 1)]
    return acvm_amd.Circuit(Circuit(2 * n_in, ops).to_bytes())


n = 1 << args.log2_range
circ, ids = synth.arithmetic_circuit(args.gates, seed=0xAC1D0002)
batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
batch.set_initial_witness(synth.witness_batch(B, seed=0xAC1D0002))
batch.solve()
print(f"metric circuit, {args.gates} gates, tile 2^{args.log2_tile}, {batch.nw} witnesses", flush=True)
measure(batch, "1a the circuit's own values, the whole map", B - n, n, None)
measure(batch, "1b the circuit's own values, 64 witnesses", 0, B, list(range(1, batch.nw, max(1, batch.nw // 64)))[:64])
batch.free()

rng = np.random.default_rng(0xDEF1A7E)
n_in = args.inputs
bits = [1, 8, 32]
values = np.zeros((B, n_in, 32), dtype=np.uint8)
for k in range(n_in):  # input k holds bits, bytes or u32s, big-endian in 32 bytes
    width = bits[k % 3]
    v = rng.integers(0, 1 << width, size=B, dtype=np.uint64)
    for b in range(4):
        values[:, k, 31 - b] = (v >> (8 * b)) & 0xff
batch = acvm_amd.Batch(readback(n_in), B, list(range(1, n_in + 1)))
batch.set_initial_witness(values.tobytes())
assert batch.solve() == 0
print(f"read-back circuit, {n_in} inputs of 1, 8 and 32 bits, {batch.nw} witnesses", flush=True)
measure(batch, "2a bit / byte / u32 inputs, the whole map", B - n, n, None)
measure(batch, "2b bit / byte / u32 inputs, 64 witnesses", 0, B, list(range(1, 65)))
batch.free()
