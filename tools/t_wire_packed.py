"""Packed wire buffers (acvm_batch_witness_maps_wire_packed_device / _packed) measured against the pitched export of the same commit, one
process, on two shapes: config 3's circuit (synth.hash_circuit(), byte inputs) and a 1 000-witness arithmetic circuit. Per container

 1. the device forms: the pitched export (A) and the packed one (B), A-B-A-B after a warm-up call of each -- wall time of the synchronous
    calls, the bytes written, and the device bytes each needs (A: rows x pitch; B: the packed bytes, the offsets and the staging arena's chunk);
 2. the pack pass: B - A is what the scan, the repitch kernel and the chunking add; the repitch kernel loads and stores every written byte
    once, so 2 x bytes / (B - A) is a LOWER bound on its rate, given against tools/copybench.hip's streaming figure (--copy-gbs);
 3. the host forms: today's (rows x pitch bytes copied down per chunk, then one memcpy per row) and the packed one (the packed range copied
    down per chunk, straight into the caller's buffer) -- wall time and bytes copied down.

For the kernels' own time run under `rocprofv3 --kernel-trace --stats` and read wire_repitch_kernel and wire_scan_kernel.
    python tools/t_wire_packed.py [--log2-rows 16] [--turns 5] [--witnesses 1000] [--copy-gbs 6300] [--max-gib 12]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-rows", type=int, default=16)
ap.add_argument("--turns", type=int, default=5)
ap.add_argument("--witnesses", type=int, default=1000)
ap.add_argument("--copy-gbs", type=float, default=6300.0)
ap.add_argument("--max-gib", type=float, default=12.0)
args = ap.parse_args()
L = acvm_amd.lib()
NAMES = {acvm_amd.WIRE_BINCODE: "BINCODE", acvm_amd.WIRE_GZIP_STORED: "GZIP_STORED", acvm_amd.WIRE_GZIP_DEFLATE: "GZIP_DEFLATE"}
CHUNK_BYTES = 64 << 20


def wall_ms(fn):
    t0 = time.perf_counter()
    rc = fn()
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, L.acvm_last_error()
    return ms


def median(xs):
    return sorted(xs)[len(xs) // 2]


def measure(batch, what):
    B = batch.B
    print(f"{what}: {B} rows, {batch.nw} witnesses", flush=True)
    for container, name in NAMES.items():
        pitch = batch.wire_bound(container)
        n = B
        while n * pitch > args.max_gib * (1 << 30):  # (a pitched buffer of the whole tile does not fit what --max-gib allows: fewer rows, said so)
            n //= 2
        pitched, keep_a = acvm_amd.wire_desc(container, 0, n, None, pitch)
        packed, keep_b = acvm_amd.wire_desc(container, 0, n, None, 0)
        d_off = acvm_amd.DeviceBuffer(size=8 * (n + 1))
        d_len = acvm_amd.DeviceBuffer(size=8 * n)
        total, fit = C.c_uint64(), C.c_uint32()
        assert L.acvm_batch_witness_maps_wire_packed_device(batch._h, packed, None, None, 0, d_off.ptr, C.byref(total), C.byref(fit)) == 0, L.acvm_last_error()  # sizing
        size = total.value
        d_a, d_b = acvm_amd.DeviceBuffer(size=n * pitch), acvm_amd.DeviceBuffer(size=size)
        calls = {"A": lambda: L.acvm_batch_witness_maps_wire_device(batch._h, pitched, None, d_a.ptr, d_len.ptr),
                 "B": lambda: L.acvm_batch_witness_maps_wire_packed_device(batch._h, packed, None, d_b.ptr, size, d_off.ptr, C.byref(total), C.byref(fit))}
        for k in ("A", "B"):
            calls[k]()
        assert fit.value == n and int(np.frombuffer(d_len.download(), dtype=np.uint64).sum()) == size
        times = {"A": [], "B": []}
        for _ in range(args.turns):
            for k in ("A", "B"):
                times[k].append(wall_ms(calls[k]))
        a, b = median(times["A"]), median(times["B"])
        chunk = min(n, max(64, CHUNK_BYTES // pitch // 64 * 64))
        print(f"  {name}: {n} rows, pitch {pitch}, {size / 1e6:.2f} MB written = {size / (n * pitch):.3f} of the slots", flush=True)
        print(f"    device: A pitched {a:9.3f} ms (min {min(times['A']):.3f}), {n * pitch / 1e6:10.2f} MB of device memory | B packed {b:9.3f} ms (min {min(times['B']):.3f}), "
              f"{(size + 8 * (n + 1) + chunk * (pitch + 8)) / 1e6:10.2f} MB (the rows, the offsets, a chunk of {chunk} slots) | B / A {b / a:.2f}", flush=True)
        if b > a:
            gbs = 2 * size / (b - a) / 1e6
            print(f"    the pack pass: B - A = {b - a:.3f} ms for 2 x {size / 1e6:.2f} MB: at least {gbs:.0f} GB/s = {gbs / args.copy_gbs:.3f} of the streaming figure ({args.copy_gbs:.0f} GB/s)", flush=True)
        else:
            print(f"    the pack pass: B is not slower than A ({b - a:+.3f} ms): the chunks' slots stay in the caches", flush=True)
        for x in (d_a, d_b, d_len, d_off):
            x.free()
        # the host forms
        out_a, lengths = np.zeros(n * pitch, dtype=np.uint8), np.zeros(n, dtype=np.uint64)
        out_b, offsets = np.zeros(max(size, 1), dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
        host = {"A": lambda: L.acvm_batch_witness_maps_wire(batch._h, pitched, out_a.ctypes.data, lengths.ctypes.data),
                "B": lambda: L.acvm_batch_witness_maps_wire_packed(batch._h, packed, out_b.ctypes.data, size, offsets.ctypes.data, C.byref(total), C.byref(fit))}
        for k in ("A", "B"):
            host[k]()
        times = {"A": [], "B": []}
        for _ in range(max(args.turns // 2, 1)):
            for k in ("A", "B"):
                times[k].append(wall_ms(host[k]))
        a, b = median(times["A"]), median(times["B"])
        j = n - 1
        assert out_b[int(offsets[j]):int(offsets[j + 1])].tobytes() == out_a[j * pitch:j * pitch + int(lengths[j])].tobytes()
        print(f"    host:   A today's {a:9.3f} ms, {n * pitch / 1e6:10.2f} MB copied down | B packed {b:9.3f} ms, {(size + 8 * (n + 1)) / 1e6:10.2f} MB copied down | B / A {b / a:.2f}", flush=True)


B = 1 << args.log2_rows
circ, ids = synth.hash_circuit()
batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
batch.set_initial_witness(synth.byte_batch(B, len(ids)))
batch.solve()
measure(batch, "config 3's shape")
batch.free()
circ, ids = synth.arithmetic_circuit(args.witnesses - 16)  # (16 inputs and one witness a gate)
batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
batch.set_initial_witness(synth.witness_batch(B))
batch.solve()
measure(batch, f"arithmetic circuit of {args.witnesses - 16} gates")
batch.free()
