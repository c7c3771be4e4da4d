"""The device-resident witness import (acvm_batch_import_device) on two shapes: the metric's tile (2^17 instances x 16 inputs of random
256-bit strings) and config 3's (2^16 instances x 64 byte inputs with byte planes: synth.hash_circuit(n_msg=32)). Wall time of the synchronous
call for each encoding x layout, the bytes it moves (source read + rows written + plane and event words, from the shapes), against the streaming
ceiling of acvm_debug_stream_rate and against acvm_batch_set_initial_witness_device on the same big-endian instance-major buffer, which the
plain descriptor must equal (it is the same launch). A call is a launch and a stream synchronisation: tens of microseconds of the wall time
are not the kernel's. For kernel times run under `rocprofv3 --kernel-trace` and read the launches of import_* in the order this tool prints.
The masked leg (acvm_batch_import_device_masked): the import with a mask of all ones against the unmasked import of the same buffer, both
layouts, on both shapes -- the difference is the mask pass and the read-back of its three words -- and, with --solve-gates N, the solve of the
metric's tile (N gates) in which one instance in 1 000 lacks an input against the same tile with none.
    python tools/t_import_device.py [--log2-tile 17] [--log2-hash-tile 16] [--rounds 21] [--solve-gates 0]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd import synth  # noqa: E402
from acvm_amd.acir import P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-tile", type=int, default=17)
ap.add_argument("--log2-hash-tile", type=int, default=16)
ap.add_argument("--rounds", type=int, default=21)
ap.add_argument("--solve-gates", type=int, default=0, help="gates of the circuit of the masked solve leg (0: no such leg; 10000: the metric's)")
args = ap.parse_args()
ENC = {"be32": acvm_amd.ENC_BE32, "le32": acvm_amd.ENC_LE32, "mont256": acvm_amd.ENC_MONT256_LE}
LAY = {"instance-major": acvm_amd.LAYOUT_INSTANCE_MAJOR, "witness-major": acvm_amd.LAYOUT_WITNESS_MAJOR}


def timed(fn, rounds):
    fn()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return sorted(out)


def byte_elements(encoding):
    """[256][32]: the byte b as an element of the encoding"""
    tab = np.zeros((256, 32), dtype=np.uint8)
    for b in range(256):
        v = (b << 256) % P if encoding == acvm_amd.ENC_MONT256_LE else b
        tab[b] = np.frombuffer(v.to_bytes(32, "big" if encoding == acvm_amd.ENC_BE32 else "little"), dtype=np.uint8)
    return tab


def shape(name, circ, ids, B, bytes_only):
    gc = acvm_amd.Circuit(circ.to_bytes())
    batch = acvm_amd.Batch(gc, B, ids)
    n_in, planes = len(ids), batch.stats()["n_byte_planes"]
    moved = B * n_in * 64 + B * planes * 4 + B * 4
    print(f"{name}: {B} instances x {n_in} inputs, {planes} byte planes; {B * n_in * 32 / 1e6:.1f} MB in, {moved / 1e6:.1f} MB moved per import", flush=True)
    rng = np.random.default_rng(0x1A90D7)
    digits = rng.integers(0, 256, (B, n_in), dtype=np.uint8)

    def source(encoding, layout):
        # every 256-bit string is a valid element of every encoding: random strings need no conversion; bytes go through a table
        el = byte_elements(encoding)[digits] if bytes_only else rng.integers(0, 256, (B, n_in, 32), dtype=np.uint8)
        if layout == acvm_amd.LAYOUT_WITNESS_MAJOR:
            el = np.ascontiguousarray(el.transpose(1, 0, 2))
        return acvm_amd.DeviceBuffer(el.tobytes())

    def line(what, us):
        med = us[len(us) // 2]
        print(f"  {what:34s} wall us median {med:9.1f} min {us[0]:9.1f} max {us[-1]:9.1f} | {moved / med / 1e3:7.0f} GB/s = {moved / med / 1e3 / ceiling:.2f} of the ceiling",
              flush=True)
        return med

    plain = source(acvm_amd.ENC_BE32, acvm_amd.LAYOUT_INSTANCE_MAJOR)
    old = line("set_initial_witness_device", timed(lambda: batch.set_initial_witness_device(plain.ptr), args.rounds))
    for lname, layout in LAY.items():
        for ename, enc in ENC.items():
            buf = plain if (lname, ename) == ("instance-major", "be32") else source(enc, layout)
            med = line(f"{lname} {ename}" + (" (= the old launch)" if buf is plain else ""), timed(lambda: batch.import_device(buf.ptr, encoding=enc, layout=layout), args.rounds))
            print(f"  {'':34s} {med / old:.2f} x set_initial_witness_device", flush=True)
            if buf is not plain:
                buf.free()
    # a scattered column list, the case the instance-major kernel pays for (kernels_import.hip import_device_im_kernel)
    perm = [(5 * k + 3) % n_in for k in range(n_in)] if n_in % 5 else [(3 * k + 1) % n_in for k in range(n_in)]
    for lname, layout in LAY.items():
        buf = source(acvm_amd.ENC_LE32, layout)
        line(f"{lname} le32, columns permuted", timed(lambda: batch.import_device(buf.ptr, encoding=acvm_amd.ENC_LE32, layout=layout, columns=perm), args.rounds))
        buf.free()
    # the masked import with a mask of all ones against the unmasked import of the same buffer, interleaved
    for lname, layout in LAY.items():
        buf, ones = source(acvm_amd.ENC_MONT256_LE, layout), acvm_amd.DeviceBuffer(bytes([1]) * (B * n_in))
        un, ma = [], []
        for _ in range(3):
            un += timed(lambda: batch.import_device(buf.ptr, encoding=acvm_amd.ENC_MONT256_LE, layout=layout), args.rounds)
            ma += timed(lambda: batch.import_device(buf.ptr, encoding=acvm_amd.ENC_MONT256_LE, layout=layout, d_assigned=ones.ptr), args.rounds)
        assert batch.import_missing() == 0
        u, m = line(f"{lname} mont256", sorted(un)), line(f"{lname} mont256, mask of ones", sorted(ma))
        print(f"  {'':34s} the mask pass and its read-back: {m - u:.1f} us = {(m - u) / u:.2f} of the unmasked import", flush=True)
        buf.free()
        ones.free()
    plain.free()
    batch.free()


def masked_solve(gates, B):
    """the solve of a tile in which one instance in 1 000 lacks an input (it takes the exact path from opcode 0) against the same tile with none"""
    circ, ids = synth.arithmetic_circuit(gates, seed=0xAC1D0002)
    batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
    n_in = len(ids)
    values = np.frombuffer(synth.witness_batch(B, seed=0xAC1D0002, edge_cases=False), dtype=np.uint8)
    mask = np.ones((B, n_in), dtype=np.uint8)
    mask[500::1000, 3] = 0
    buf, ones, some = acvm_amd.DeviceBuffer(values.tobytes()), acvm_amd.DeviceBuffer(bytes([1]) * (B * n_in)), acvm_amd.DeviceBuffer(mask.tobytes())
    print(f"masked solve: {gates} gates, {B} instances, {int((mask == 0).sum())} of them lack one input", flush=True)

    def solve(d_mask):
        batch.import_device(buf.ptr, d_assigned=d_mask.ptr)
        t0 = time.perf_counter()
        batch.solve()
        return (time.perf_counter() - t0) * 1e3, batch.stats()
    for d_mask in (ones, some):
        solve(d_mask)
    for r in range(args.rounds if args.rounds < 5 else 5):
        for name, d_mask in (("none absent", ones), ("1 in 1 000", some)):
            wall, st = solve(d_mask)
            print(f"  round {r} {name:12s} wall ms {wall:8.2f} device ms {st['solve_device_ms']:8.2f} exact path ms {st['slow_path_ms']:7.2f} "
                  f"exact lanes {st['n_slow_instances']:4d} missing {batch.import_missing()}", flush=True)
    for x in (buf, ones, some, batch):
        x.free()


ceiling = max(acvm_amd.stream_rate(1 << 30) for _ in range(3))
print(f"streaming ceiling (acvm_debug_stream_rate, 3 x 1 GiB): {ceiling:.0f} GB/s", flush=True)
circ, ids = synth.arithmetic_circuit(100, seed=0xAC1D0002)
shape("metric tile", circ, ids, 1 << args.log2_tile, False)
if args.log2_hash_tile:  # (0: the metric's tile alone, e.g. under a kernel trace whose statistics should be of one shape)
    circ, ids = synth.hash_circuit(n_msg=32)
    shape("config 3", circ, ids, 1 << args.log2_hash_tile, True)
if args.solve_gates:
    masked_solve(args.solve_gates, 1 << args.log2_tile)
