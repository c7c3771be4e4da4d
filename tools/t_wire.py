"""The batch-wide wire format (acvm_batch_witness_maps_wire_device) measured on the metric's circuit at one tile, one process: a range of
instances leaves as

 A. ACVM_WIRE_BINCODE bodies, the whole map;
 B. ACVM_WIRE_GZIP_STORED members, the whole map;
 C. acvm_batch_export_device, ACVM_ENC_BE32 instance-major, the whole map: the comparator that reads the same rows and writes 32 bytes per
    element where A and B write 76 per entry;
 D. a loop of acvm_batch_witness_map_bytes over a few instances (one gather, one copy down, hex and zlib level 9 on the host per instance),
    reported per instance.

A-B-C in turns after a warm-up call of each. Wall time of the synchronous call -- the launches, the small table copies and a stream
synchronisation, tens of microseconds of which are not the kernels' -- the way tools/t_outcomes.py times its calls; at milliseconds per call
that is the kernels' time. For kernel times alone run under `rocprofv3 --kernel-trace --stats` and read wire_entries_kernel / export_device_im_kernel.
    python tools/t_wire.py [--gates 10000] [--log2-tile 17] [--log2-range 14] [--turns 5] [--one-instance-calls 64]"""
import argparse
import gzip
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gates", type=int, default=10000)
ap.add_argument("--log2-tile", type=int, default=17)
ap.add_argument("--log2-range", type=int, default=14)
ap.add_argument("--turns", type=int, default=5)
ap.add_argument("--one-instance-calls", type=int, default=64)
args = ap.parse_args()
B, n = 1 << args.log2_tile, 1 << args.log2_range
BINCODE, GZIP = acvm_amd.WIRE_BINCODE, acvm_amd.WIRE_GZIP_STORED


def wall_ms(fn):
    t0 = time.perf_counter()
    rc = fn()
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, acvm_amd.lib().acvm_last_error()
    return ms


circ, ids = synth.arithmetic_circuit(args.gates, seed=0xAC1D0002)
batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
batch.set_initial_witness(synth.witness_batch(B, seed=0xAC1D0002))
batch.solve()
nw = batch.nw
first = B - n  # (the edge-case instances of the exact path are instances 0 .. 7: the range holds generic instances, as almost every range does)
L = acvm_amd.lib()
pitch = {c: batch.wire_bound(c) for c in (BINCODE, GZIP)}
d_wire = acvm_amd.DeviceBuffer(size=n * pitch[GZIP])
d_len = acvm_amd.DeviceBuffer(size=n * 8)
d_be = acvm_amd.DeviceBuffer(size=n * nw * 32)
desc = {c: acvm_amd.wire_desc(c, first, n, None, pitch[c])[0] for c in (BINCODE, GZIP)}
bdesc = acvm_amd.ExportDesc(encoding=acvm_amd.ENC_BE32, layout=acvm_amd.LAYOUT_INSTANCE_MAJOR, first=first, n=n, stride=0)
calls = {
    "A BINCODE": lambda: L.acvm_batch_witness_maps_wire_device(batch._h, desc[BINCODE], None, d_wire.ptr, d_len.ptr),
    "B GZIP_STORED": lambda: L.acvm_batch_witness_maps_wire_device(batch._h, desc[GZIP], None, d_wire.ptr, d_len.ptr),
    "C export_device BE32": lambda: L.acvm_batch_export_device(batch._h, bdesc, d_be.ptr, None),
}
written = {}
for c, name in ((BINCODE, "A BINCODE"), (GZIP, "B GZIP_STORED")):
    calls[name]()
    written[name] = int(np.frombuffer(d_len.download(), dtype=np.uint64).sum())
calls["C export_device BE32"]()
entries = (written["A BINCODE"] // n - 8) // 76
written["C export_device BE32"] = n * nw * 32
print(f"metric circuit, {args.gates} gates, tile 2^{args.log2_tile}, instances [{first}, {first + n}), {nw} witnesses, {entries} entries per map; "
      f"slots of {pitch[BINCODE]} / {pitch[GZIP]} bytes", flush=True)
times = {k: [] for k in calls}
for turn in range(args.turns):
    for k, fn in calls.items():
        times[k].append(wall_ms(fn))
rate = {}
for k, ms in times.items():
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    rate[k] = written[k] / med / 1e6
    print(f"  {k:22s} ms median {med:8.2f} min {ms[0]:8.2f} max {ms[-1]:8.2f} | {written[k] / 1e9:7.2f} GB written, {rate[k]:7.1f} GB/s | "
          f"{med * 1e3 / n:8.2f} us per instance", flush=True)
for k in ("A BINCODE", "B GZIP_STORED"):
    print(f"  {k}: written bytes per second are {rate[k] / rate['C export_device BE32']:.2f} of the instance-major export's", flush=True)
# D: the one-instance call
m = args.one_instance_calls
batch.witness_map_bytes(first)
t0 = time.perf_counter()
blobs = [batch.witness_map_bytes(first + i) for i in range(m)]
one_ms = (time.perf_counter() - t0) * 1e3 / m
print(f"  D witness_map_bytes: {one_ms:8.2f} ms per instance over {m} calls ({sum(len(x) for x in blobs) / m / 1e3:.0f} KB each); "
      f"A costs {sorted(times['A BINCODE'])[args.turns // 2] / n:.5f} ms per instance, B {sorted(times['B GZIP_STORED'])[args.turns // 2] / n:.5f}: "
      f"{one_ms / (sorted(times['B GZIP_STORED'])[args.turns // 2] / n):.0f} x", flush=True)
# the forms hold the same maps
calls["B GZIP_STORED"]()
lengths = np.frombuffer(d_len.download(), dtype=np.uint64)
if m:
    head = np.zeros(pitch[GZIP], dtype=np.uint8)  # (the first slot alone: the buffer is gigabytes)
    assert L.acvm_device_download(head.ctypes.data, d_wire.ptr, head.size) == 0
    print(f"  the first GZIP_STORED slot inflates to the body of witness_map_bytes({first}): "
          f"{gzip.decompress(head[:int(lengths[0])].tobytes()) == gzip.decompress(blobs[0])}", flush=True)
for x in (d_wire, d_len, d_be, batch):
    x.free()
