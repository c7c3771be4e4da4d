"""tools/t_node_device.py [gates=10000] [total_log2=20] [tile_log2=17] [rounds=5] -- the metric's circuit through the node-level driver on ONE GPU,
host form (acvm_node_solve: pageable host buffers in, kept witnesses and digests back on the host) and device form (acvm_node_solve_device:
inputs, kept witnesses, mask, status column and digests resident on the device) in turn in one process, return witnesses kept, digests on.
Prints median (min - max) witnesses/s of each over the rounds, the bytes the device form copied, and whether both forms gave the same kept
witnesses and digests. A library without the device form (an older build loaded through ACVM_AMD_LIB for an A/B run) times the host form alone."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd
from acvm_amd import synth

gates = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
total = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 20)
tile = 1 << (int(sys.argv[3]) if len(sys.argv) > 3 else 17)
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
circ, ids = synth.arithmetic_circuit(gates, seed=0xAC1D0002)
gc = acvm_amd.Circuit(circ.to_bytes())
ret = gc.witness_set("return_values")
values = synth.witness_batch(total, seed=0xAC1D0002)
node = acvm_amd.Node(gc, ids, keep=ret, devices=[0], tile=tile)
has_device_form = hasattr(acvm_amd.lib(), "acvm_node_solve_device")
warm = min(tile, total)
node.solve(values[: warm * len(ids) * 32], warm, results=False)  # staging buffers touched, tables built, clocks up
if has_device_form:
    d_in = acvm_amd.DeviceBuffer(values)
    d_kept, d_mask = acvm_amd.DeviceBuffer(size=total * len(ret) * 32), acvm_amd.DeviceBuffer(size=total * len(ret))
    d_status, d_dig = acvm_amd.DeviceBuffer(size=total), acvm_amd.DeviceBuffer(size=total * 32)
    lane = dict(n=total, d_values=d_in.ptr, d_kept=d_kept.ptr, d_kept_assigned=d_mask.ptr, d_status=d_status.ptr, d_digests32=d_dig.ptr)
    node.solve_device([dict(lane, n=warm)])
host, device, same = [], [], None
for rnd in range(rounds):
    t0 = time.perf_counter()
    not_solved, _, kept, asg, dig = node.solve(values, total, results=False)
    host.append(total / (time.perf_counter() - t0))
    if has_device_form:
        t0 = time.perf_counter()
        got = node.solve_device([lane])
        device.append(total / (time.perf_counter() - t0))
        if rnd == rounds - 1:
            same = bool(got[0][0] == not_solved and np.array_equal(np.frombuffer(d_kept.download(), dtype=np.uint8), kept.reshape(-1)) and
                        np.array_equal(np.frombuffer(d_mask.download(), dtype=np.uint8), asg.reshape(-1)) and
                        np.array_equal(np.frombuffer(d_dig.download(), dtype=np.uint8), dig.reshape(-1)))


def summary(xs):
    return None if not xs else {"median": round(statistics.median(xs)), "min": round(min(xs)), "max": round(max(xs)), "runs": [round(x) for x in xs]}


st = node.stats()
print(json.dumps({"gates": gates, "instances": total, "tile": tile, "rounds": rounds, "unit": "witnesses/s", "host_form": summary(host), "device_form": summary(device),
                  "device_form_io_bytes": list(node.io_bytes(0)) if has_device_form else None, "forms_agree": same, "async_exact": st["async_exact"],
                  "exact_instances_last_call": st["exact_instances"]}))
for name, xs in (("host form  ", host), ("device form", device)):
    if xs:
        print(f"{name}: {statistics.median(xs) / 1e6:.3f} M witnesses/s median ({min(xs) / 1e6:.3f} - {max(xs) / 1e6:.3f}) over {len(xs)} rounds")
