"""Device-resident outcomes on the metric's circuit at one tile: (1) acvm_batch_export_device_list against acvm_batch_export_device -- the identity
list, and a list with one instance in 64 removed, against the range export of the whole tile, whole map, Montgomery-256, both layouts, alternating
in one process; wall time of the synchronous calls, bytes moved (table rows read + output and mask written, from the shapes; the list and the lane
map add 8 bytes per row) and the host-to-device bytes the handle counted; (2) acvm_batch_outcomes_device against acvm_batch_results, a host
clock around each call (both end in a synchronisation), with 0 and with 64 instances on the exact path.
    python tools/t_outcomes.py [--gates 10000] [--log2-tile 17] [--rounds 5]"""
import argparse
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
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
B = 1 << args.log2_tile
LAY = {"instance-major": acvm_amd.LAYOUT_INSTANCE_MAJOR, "witness-major": acvm_amd.LAYOUT_WITNESS_MAJOR}
ENC = acvm_amd.ENC_MONT256_LE


def ms_of(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(xs):
    xs = sorted(xs)
    return f"median {xs[len(xs) // 2]:9.3f} min {xs[0]:9.3f} max {xs[-1]:9.3f}"


circ, ids = synth.arithmetic_circuit(args.gates, seed=0xAC1D0002)
gc = acvm_amd.Circuit(circ.to_bytes())
batch = acvm_amd.Batch(gc, B, ids)
values = np.frombuffer(synth.witness_batch(B, seed=0xAC1D0002, edge_cases=False), dtype=np.uint8).reshape(B, len(ids), 32).copy()
nw = batch.nw
d_vals = acvm_amd.DeviceBuffer(size=B * nw * 32)
d_mask = acvm_amd.DeviceBuffer(size=B * nw)
identity = np.arange(B, dtype=np.uint32)
thinned = identity[identity % 64 != 63]
d_identity, d_thinned = acvm_amd.DeviceBuffer(identity.tobytes()), acvm_amd.DeviceBuffer(thinned.tobytes())
d_status, d_err = acvm_amd.DeviceBuffer(size=B), acvm_amd.DeviceBuffer(size=B)
d_opcode, d_selected = acvm_amd.DeviceBuffer(size=4 * B), acvm_amd.DeviceBuffer(size=4 * B)

for n_exact in (0, 64):
    v = values.copy()
    if n_exact:
        v[np.arange(n_exact) * (B // n_exact)] = 0  # all-zero inputs: a zero denominator sends the instance to the exact path
    batch.set_initial_witness(v.tobytes())
    batch.solve()
    n_slow = batch.stats()["n_slow_instances"]
    print(f"circuit: {args.gates} gates, {nw} witnesses, {B} instances, {n_slow} on the exact path", flush=True)
    # (2) outcomes
    batch.results()
    batch.outcomes_device(d_status=d_status.ptr, d_err=d_err.ptr, d_opcode_index=d_opcode.ptr, select_mask=1, d_selected=d_selected.ptr)
    res, out = [], []
    h0 = batch.export_h2d_bytes()
    for _ in range(args.rounds):
        res.append(ms_of(batch.results))
        out.append(ms_of(lambda: batch.outcomes_device(d_status=d_status.ptr, d_err=d_err.ptr, d_opcode_index=d_opcode.ptr, select_mask=1 << acvm_amd.STATUS_SOLVED,
                                                       d_selected=d_selected.ptr)))
    up = (batch.export_h2d_bytes() - h0) // args.rounds
    n_sel = batch.outcomes_device(select_mask=1 << acvm_amd.STATUS_SOLVED, d_selected=d_selected.ptr)
    print(f"  acvm_batch_results          wall ms {stats(res)} | {B * 300 / 1e6:.1f} MB written on the host", flush=True)
    print(f"  acvm_batch_outcomes_device  wall ms {stats(out)} | {up} B up, 4 B back, {n_sel} of {B} selected", flush=True)
    # (1) list export against range export, A-B-C per round
    if n_exact:
        continue
    for lname, layout in LAY.items():
        rng_ms, id_ms, th_ms = [], [], []
        h0 = batch.export_h2d_bytes()
        for _ in range(args.rounds):
            rng_ms.append(ms_of(lambda: batch.export_device(d_vals.ptr, encoding=ENC, layout=layout, d_assigned=d_mask.ptr)))
            id_ms.append(ms_of(lambda: batch.export_device_list(d_identity.ptr, B, d_vals.ptr, encoding=ENC, layout=layout, d_assigned=d_mask.ptr)))
            th_ms.append(ms_of(lambda: batch.export_device_list(d_thinned.ptr, thinned.size, d_vals.ptr, encoding=ENC, layout=layout, d_assigned=d_mask.ptr)))
        up = batch.export_h2d_bytes() - h0
        med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
        moved = lambda n: n * nw * (32 + 32 + 1)  # noqa: E731
        print(f"  whole map mont256 {lname}: {up} B host-to-device over {3 * args.rounds} exports", flush=True)
        print(f"    range export            wall ms {stats(rng_ms)} | {moved(B) / 1e9:.2f} GB moved", flush=True)
        print(f"    list export, identity   wall ms {stats(id_ms)} | {(moved(B) + 8 * B) / 1e9:.2f} GB moved | x{med(id_ms) / med(rng_ms):.3f} of the range export", flush=True)
        print(f"    list export, 63 of 64   wall ms {stats(th_ms)} | {(moved(thinned.size) + 8 * thinned.size) / 1e9:.2f} GB moved | x{med(th_ms) / med(rng_ms):.3f} of the range export, "
              f"x{med(th_ms) / med(id_ms) * B / thinned.size:.3f} per row of the identity list", flush=True)
for x in (d_vals, d_mask, d_identity, d_thinned, d_status, d_err, d_opcode, d_selected):
    x.free()
batch.free()
