"""The batch-wide wire import (acvm_batch_import_device_wire) measured at one tile, one process, on two input sets: the metric's circuit (16
field-element inputs per instance) and config 3's byte inputs (96 per instance). Per set a first handle solves and writes every instance's
map of the initial witnesses with acvm_batch_witness_maps_wire_device; a second handle of the same circuit then reads

 A. those ACVM_WIRE_BINCODE slots,
 B. those ACVM_WIRE_GZIP_STORED slots,
 C. acvm_batch_import_device_masked of the same values: BE32 instance-major plus one mask byte per element, all ones -- the comparator that
    moves 33 bytes per element where A and B move 76 per entry,

A-B-C in turns after a warm-up call of each. Wall time of the synchronous call -- the launches, the small table copies, the few result words
and a stream synchronisation, tens of microseconds of which are not the kernels' -- the way tools/t_wire.py times its calls. Bytes moved are
what the call must read and write (the slots' lengths or 33 bytes per element in, 32 bytes per element out); the fraction is of the streaming
ceiling tools/copybench.hip measures for a copy kernel (--copy-ceiling-gbs, read plus written bytes per second). No ratio is asserted.

Then the host form on a smaller handle: acvm_batch_set_initial_witness_maps_wire of the maps as gzip members in host memory, against the
four-step host route -- decompress_witness per row, a [B][n_initial] value array and a mask array, acvm_batch_set_initial_witness_masked.
    python tools/t_wire_in.py [--gates 10000] [--log2-tile 17] [--log2-host 13] [--turns 7] [--copy-ceiling-gbs 6300]"""
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
ap.add_argument("--log2-host", type=int, default=13)
ap.add_argument("--turns", type=int, default=7)
ap.add_argument("--copy-ceiling-gbs", type=float, default=6300.0)
args = ap.parse_args()
B = 1 << args.log2_tile
BINCODE, GZIP = acvm_amd.WIRE_BINCODE, acvm_amd.WIRE_GZIP_STORED
L = acvm_amd.lib()


def wall_ms(fn):
    t0 = time.perf_counter()
    rc = fn()
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, L.acvm_last_error()
    return ms


def measure(name, circuit, ids, values):
    n_in = len(ids)
    dc = acvm_amd.Circuit(circuit.to_bytes())
    first = acvm_amd.Batch(dc, B, ids)
    first.set_initial_witness(values)
    first.solve()
    pitch = {c: first.wire_bound(c, ids) for c in (BINCODE, GZIP)}
    d_wire = {c: acvm_amd.DeviceBuffer(size=B * pitch[c]) for c in (BINCODE, GZIP)}
    d_len = {c: acvm_amd.DeviceBuffer(size=B * 8) for c in (BINCODE, GZIP)}
    moved = {}
    for c, k in ((BINCODE, "A BINCODE"), (GZIP, "B GZIP_STORED")):
        first.witness_maps_wire_device(d_wire[c].ptr, c, ids, n=B, pitch=pitch[c], d_lengths=d_len[c].ptr)
        moved[k] = int(np.frombuffer(d_len[c].download(), dtype=np.uint64).sum()) + B * n_in * 32
    d_be, d_mask = acvm_amd.DeviceBuffer(values), acvm_amd.DeviceBuffer(np.ones(B * n_in, dtype=np.uint8).tobytes())
    moved["C import_device_masked BE32"] = B * n_in * (33 + 32)
    second = acvm_amd.Batch(dc, B, ids)
    in_desc = {c: acvm_amd.WireInDesc(container=c, pitch=pitch[c]) for c in (BINCODE, GZIP)}
    be_desc, _keep = second._import_desc(acvm_amd.ENC_BE32, acvm_amd.LAYOUT_INSTANCE_MAJOR, None, None, 0)
    calls = {
        "A BINCODE": lambda: L.acvm_batch_import_device_wire(second._h, in_desc[BINCODE], d_wire[BINCODE].ptr, d_len[BINCODE].ptr),
        "B GZIP_STORED": lambda: L.acvm_batch_import_device_wire(second._h, in_desc[GZIP], d_wire[GZIP].ptr, d_len[GZIP].ptr),
        "C import_device_masked BE32": lambda: L.acvm_batch_import_device_masked(second._h, be_desc, d_be.ptr, d_mask.ptr),
    }
    for fn in calls.values():
        assert fn() == 0, L.acvm_last_error()
    print(f"{name}: tile 2^{args.log2_tile}, {n_in} initial witnesses per instance; slots of {pitch[BINCODE]} / {pitch[GZIP]} bytes", flush=True)
    times = {k: [] for k in calls}
    for _ in range(args.turns):
        for k, fn in calls.items():
            times[k].append(wall_ms(fn))
    med = {}
    for k, ms in times.items():
        ms = sorted(ms)
        med[k] = ms[len(ms) // 2]
        rate = moved[k] / med[k] / 1e6
        print(f"  {k:28s} ms median {med[k]:8.3f} min {ms[0]:8.3f} max {ms[-1]:8.3f} | {moved[k] / 1e6:8.1f} MB moved, {rate:7.1f} GB/s, "
              f"{rate / args.copy_ceiling_gbs:.3f} of the copy ceiling | {med[k] * 1e6 / (B * n_in):7.2f} ns per element", flush=True)
    for k in ("A BINCODE", "B GZIP_STORED"):
        print(f"  {k}: {med[k] / med['C import_device_masked BE32']:.2f} x the time of the masked column import", flush=True)
    # the two forms leave the same handle
    calls["B GZIP_STORED"]()
    wire_state = second.import_state() if B * n_in <= 1 << 22 else None
    calls["C import_device_masked BE32"]()
    if wire_state is not None:
        same = all(np.array_equal(wire_state[key], v) for key, v in second.import_state().items())
        print(f"  the wire import and the masked column import leave the same state: {same}", flush=True)
    # ---- the host form, on a smaller handle
    n = min(B, 1 << args.log2_host)
    maps = first.witness_maps_wire(GZIP, ids, first=0, n=n)
    host = acvm_amd.Batch(dc, n, ids)
    host.set_initial_witness_maps_wire(maps)

    def four_steps():
        vals, mask = np.zeros((n, n_in, 32), dtype=np.uint8), np.zeros((n, n_in), dtype=np.uint8)
        position = {w: k for k, w in enumerate(ids)}
        for j, m in enumerate(maps):
            for w, v in acvm_amd.decompress_witness(m).items():
                vals[j, position[w]] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
                mask[j, position[w]] = 1
        host.set_initial_witness_masked(vals.tobytes(), mask.tobytes())
        return 0
    four_steps()
    one = sorted(wall_ms(lambda: host.set_initial_witness_maps_wire(maps) or 0) for _ in range(3))[1]
    four = sorted(wall_ms(four_steps) for _ in range(3))[1]
    print(f"  host form, {n} instances: set_initial_witness_maps_wire {one:8.2f} ms, the four-step host route (Python loop included) {four:8.2f} ms: {four / one:.1f} x", flush=True)
    for x in list(d_wire.values()) + list(d_len.values()) + [d_be, d_mask, first, second, host]:
        x.free()


circ, ids = synth.arithmetic_circuit(args.gates, seed=0xAC1D0002)
measure(f"metric circuit, {args.gates} gates", circ, ids, synth.witness_batch(B, seed=0xAC1D0002))
circ, ids = synth.hash_circuit()
measure("config 3, byte inputs", circ, ids, synth.byte_batch(B, len(ids)))
