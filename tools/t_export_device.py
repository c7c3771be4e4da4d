"""The device-resident witness export (acvm_batch_export_device) on the metric's circuit at one tile: wall time of the synchronous call and
bytes (table rows read + output and mask written, from the shapes) of the whole-map export for each encoding x layout, against the streaming
ceiling of acvm_debug_stream_rate; then the new kernels against the host export's kernel on the same selections, alternating A-B-A-B in one
process: the return witnesses of the whole tile, and the whole map of a 2048-instance slice (the host export also copies to the host, so only
its KERNEL time compares: run under `rocprofv3 --kernel-trace` and read the launches of export_* in the order this tool prints).
    python tools/t_export_device.py [--gates 10000] [--log2-tile 17] [--rounds 5]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gates", type=int, default=10000)
ap.add_argument("--log2-tile", type=int, default=17)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
B = 1 << args.log2_tile
ENC = {"be32": acvm_amd.ENC_BE32, "le32": acvm_amd.ENC_LE32, "mont256": acvm_amd.ENC_MONT256_LE}
LAY = {"instance-major": acvm_amd.LAYOUT_INSTANCE_MAJOR, "witness-major": acvm_amd.LAYOUT_WITNESS_MAJOR}

circ, ids = synth.arithmetic_circuit(args.gates, seed=0xAC1D0002)
gc = acvm_amd.Circuit(circ.to_bytes())
batch = acvm_amd.Batch(gc, B, ids)
batch.set_initial_witness(synth.witness_batch(B, seed=0xAC1D0002, edge_cases=False))  # (extract refuses a map with an unassigned return witness)
batch.solve()
st = batch.stats()
nw = batch.nw
print(f"circuit: {args.gates} gates, {nw} witnesses, {B} instances, {st['n_slow_instances']} on the exact path", flush=True)
ceiling = max(acvm_amd.stream_rate(1 << 30) for _ in range(3))
print(f"streaming ceiling (acvm_debug_stream_rate, 3 x 1 GiB): {ceiling:.0f} GB/s", flush=True)


def timed(fn, rounds):
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)


d_vals = acvm_amd.DeviceBuffer(size=B * nw * 32)
d_mask = acvm_amd.DeviceBuffer(size=B * nw)
moved = B * nw * (32 + 32 + 1)
print(f"whole map: {B * nw * 32 / 1e9:.2f} GB out, {moved / 1e9:.2f} GB moved per export", flush=True)
for lname, layout in LAY.items():
    for ename, enc in ENC.items():
        ms = timed(lambda: batch.export_device(d_vals.ptr, encoding=enc, layout=layout, d_assigned=d_mask.ptr), args.rounds)
        med = ms[len(ms) // 2]
        print(f"whole map {lname:15s} {ename:8s} wall ms median {med:9.3f} min {ms[0]:9.3f} max {ms[-1]:9.3f} | {moved / med / 1e6:7.0f} GB/s = "
              f"{moved / med / 1e6 / ceiling:.2f} of the ceiling", flush=True)

ret = gc.witness_set("return_values")
print(f"A-B-A-B, return witnesses {ret} of {B} instances: A = export_device (be32, instance-major), B = extract (export_witness_kernel + D2H)", flush=True)
for r in range(args.rounds):
    a = timed(lambda: batch.export_device(d_vals.ptr, witnesses=ret), 1)[0]
    b = timed(lambda: batch.extract(ret), 1)[0]
    print(f"  round {r}: A {a:8.3f} ms   B {b:8.3f} ms (wall)", flush=True)
n_slice = min(B, 2048)
batch.export_device(d_vals.ptr, n=1, d_assigned=d_mask.ptr)
everything = [w for w, a in enumerate(d_mask.download(nw)) if a]  # (extract refuses an unassigned witness: witness 0 is no witness of the circuit)
print(f"A-B-A-B, the {len(everything)} assigned witnesses of instances [0, {n_slice}): A = export_device (be32, instance-major), B = extract", flush=True)
for r in range(args.rounds):
    a = timed(lambda: batch.export_device(d_vals.ptr, witnesses=everything, n=n_slice), 1)[0]
    b = timed(lambda: batch.extract(everything, 0, n_slice), 1)[0]
    print(f"  round {r}: A {a:8.3f} ms   B {b:8.3f} ms (wall)", flush=True)
d_vals.free()
d_mask.free()
batch.free()
