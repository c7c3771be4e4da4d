"""The node's foreign-call handler against a hand-written per-tile loop: the relevel circuit of tools/t_foreign_calls.py (two oracle calls per instance, a
40-gate tail) at 2^16 instances in tiles, one drive = every tile solved, answered twice and exported (results, kept witnesses, digests). Three forms
alternate in one process:
  device  acvm_node_solve with a device-space handler: 'invert' hands the node's own input column back as its answer (an echo: no kernel, no copy),
          'double' two columns of zeros that live on the device;
  host    the same node with a host-space handler: the node copies the inputs down, the handler echoes the bytes, the node uploads them;
  loop    one plain Batch of a tile's size driven by hand through the device calls (acvm_batch_foreign_call_inputs_device,
          acvm_batch_resolve_foreign_calls_device_rows) with the same answers, tile after tile, with results, digests and the kept witnesses read back.
All three must give the same digests. Printed per form: witnesses/s (median and range), the handler's share of the wall clock and the bytes the round
trips moved.
    python tools/t_node_foreign.py [--log2-n 16] [--log2-tile 14] [--rounds 5] [--tail 40]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd.acir import P, Brillig, Circuit, Expression as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-n", type=int, default=16)
ap.add_argument("--log2-tile", type=int, default=14)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tail", type=int, default=40)
args = ap.parse_args()
N, TILE = 1 << args.log2_n, 1 << min(args.log2_tile, args.log2_n)
W = E.from_witness
MONT, WM = acvm_amd.ENC_MONT256_LE, acvm_amd.LAYOUT_WITNESS_MAJOR


def circuit(n_tail):
    ops = [Brillig(inputs=[W(1)], outputs=[3], bytecode=[("ForeignCall", "invert", [("Register", 0)], [("Register", 0)]), ("Stop",)]),
           E([(1, 3, 1)], [(P - 1, 4)], 0),
           Brillig(inputs=[E([], [(1, 2), (1, 4)], 0)], outputs=[5, 6],
                   bytecode=[("ForeignCall", "double", [("Register", 0), ("Register", 1)], [("Register", 0)]), ("Stop",)])]
    nw = 6
    for i in range(n_tail):
        ops.append(E([(1, nw, nw - 1)], [(1, 5), (P - 1, nw + 1)], 0))
        nw += 1
    return Circuit(nw, ops), [1, 2], nw


circ, ids, n_witnesses = circuit(args.tail)
gc = acvm_amd.Circuit(circ.to_bytes())
keep = [5, 6, n_witnesses]
values = np.frombuffer(b"".join((3 + j).to_bytes(32, "big") + (1000 + 7 * j).to_bytes(32, "big") for j in range(N)), dtype=np.uint8)
d_zeros = acvm_amd.DeviceBuffer(data=bytes(2 * TILE * 32))
d_cols = acvm_amd.DeviceBuffer(data=bytes(TILE * 32))
zeros = bytes(2 * TILE * 32)


def device_handler(r):
    if r.function == "invert":
        return dict(shape=[None], values=r.values, encoding=MONT, layout=WM)
    return dict(shape=[None, None], values=d_zeros.ptr, encoding=MONT, layout=WM)


def host_handler(r):
    if r.function == "invert":
        return dict(shape=[None], values=r.values_bytes(), encoding=MONT, layout=WM)
    return dict(shape=[None, None], values=zeros[:2 * r.n_rows * 32], encoding=MONT, layout=WM)


node = acvm_amd.Node(gc, ids, keep=keep, devices=[0], tile=TILE)
batch = acvm_amd.Batch(gc, TILE, ids)
handler_ms, moved = {}, {}


def drive_node(form):
    node.set_foreign_call_handler(device_handler if form == "device" else host_handler, space=acvm_amd.SPACE_DEVICE if form == "device" else acvm_amd.SPACE_HOST,
                                  in_encoding=MONT, in_layout=WM)
    t0 = time.perf_counter()
    not_solved, _, _, _, dig = node.solve(values, N)
    ms = (time.perf_counter() - t0) * 1e3
    assert not_solved == 0
    st = node.foreign_stats(0)
    handler_ms[form], moved[form] = st["handler_ms"], (st["h2d_bytes"], st["d2h_bytes"])
    return ms, dig.tobytes()


def drive_loop():
    t0 = time.perf_counter()
    s0 = batch.foreign_call_stats()
    digests = []
    for first in range(0, N, TILE):
        batch.set_initial_witness(values[first * 64:(first + TILE) * 64])
        while batch.solve():
            for s in batch.foreign_call_sites():
                rows = s["n_waiting"]
                longest = batch.foreign_call_inputs_device(s["opcode_index"], s["brillig_index"], n_rows=rows)
                batch.foreign_call_inputs_device(s["opcode_index"], s["brillig_index"], n_rows=rows, d_values=d_cols.ptr, encoding=MONT, layout=WM, n_columns=longest)
                k, src = (1, d_cols.ptr) if s["function"] == "invert" else (2, d_zeros.ptr)
                batch.resolve_foreign_calls_device_rows(s["opcode_index"], s["brillig_index"], [None] * k, src, n_rows=rows, encoding=MONT, layout=WM)
        batch.results()
        batch.extract(keep)
        digests.append(batch.digest().tobytes())
    ms = (time.perf_counter() - t0) * 1e3
    s1 = batch.foreign_call_stats()
    handler_ms["loop"], moved["loop"] = 0.0, (s1["h2d_bytes"] - s0["h2d_bytes"], s1["d2h_bytes"] - s0["d2h_bytes"])
    return ms, b"".join(digests)


forms = {"device": lambda: drive_node("device"), "host": lambda: drive_node("host"), "loop": drive_loop}
warm = {f: forms[f]()[1] for f in forms}  # warm-up: allocations, first launches; and the forms agree
assert len(set(warm.values())) == 1, "the forms disagree"
wall = {f: [] for f in forms}
for _ in range(args.rounds):
    for f in forms:
        wall[f].append(forms[f]()[0])
print(f"relevel circuit, {args.tail}-gate tail, {N} instances in tiles of {TILE}, two calls per instance, {args.rounds} drives per form, library {acvm_amd.LIB_PATH}")
for f in forms:
    xs = sorted(wall[f])
    rate = lambda ms: N * n_witnesses / (ms * 1e-3)  # noqa: E731
    med = xs[len(xs) // 2]
    print(f"  {f:6s}: wall ms median {med:9.3f} (min {xs[0]:9.3f} - max {xs[-1]:9.3f}) | witnesses/s median {rate(med):.3e} ({rate(xs[-1]):.3e} - {rate(xs[0]):.3e})"
          f" | handler {handler_ms[f]:8.3f} ms of the last drive ({100 * handler_ms[f] / wall[f][-1]:.1f} %) | {moved[f][0]} B host-to-device, {moved[f][1]} B device-to-host")
loop = sorted(wall["loop"])[len(wall["loop"]) // 2]
for f in ("device", "host"):
    med = sorted(wall[f])[len(wall[f]) // 2]
    print(f"  node form, {f} space, against the hand-written loop: {100 * (med - loop) / loop:+.1f} % wall clock")
node.free()
batch.free()
