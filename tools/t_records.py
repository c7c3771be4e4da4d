"""The record import (acvm_batch_import_device_records, acvm_node_solve_records) measured, one process, three sections:

 1. import timing on config 3's tile (2^16 instances of synth.hash_circuit(n_msg=32): 64 byte inputs with byte planes): dense 64-byte records
    against ACVM_ENC_U8 instance-major -- the same bytes in, the same rows out, through import_narrow_im_kernel -- run A-B-A-B in pairs, and
    against ACVM_ENC_BE32 instance-major;
 2. a mixed 108-byte record { msg: [u8; 64], root: Field, idx: u32, flags: [bool; 8] } on a 74-input read-back circuit, against the same values
    as ACVM_ENC_BE32;
 3. end to end: config 3's circuit through acvm_node_solve (32-byte rows from host memory) and acvm_node_solve_records (64-byte records) in
    turn: instances/s, the host-to-device bytes of the inputs (instances x row size: what the upload thread copies), and whether results and
    kept witnesses agree (checked on a separate, smaller call that asks for them).

 4. the masked record import (acvm_batch_import_device_records_masked) in alternating legs, 2^16 and 2^17 instances of config 3's 64 byte inputs
    and of a 64 x Field record, each with the mask bytes beside their elements ({valid, value} pairs) and gathered at the record's head (for
    the Field record that is the far form): (i) the unmasked record import of the same buffer, (ii) masked with nothing absent, (iii) with one
    instance in 1 000 absent and with everyone absent, (iv) what a caller did before: (i) plus the mask pass of acvm_batch_import_device_masked
    over a column mask of the same bits -- the mask pass is not callable alone, so its time is the masked column import minus the unmasked
    column import of the same values. The legs are timed twice: rotated (a leg then pays for what its predecessor left on the stream) and each
    on its own, back to back. `--only-masked` runs this section alone.

Wall time of the synchronous call: a launch and a stream synchronisation, tens of microseconds of which are not the kernel's. For kernel times
run under `rocprofv3 --kernel-trace --stats` and read import_records_kernel / import_narrow_im_kernel / import_witness_kernel.
    python tools/t_records.py [--log2-tile 16] [--rounds 21] [--pairs 3] [--log2-total 20] [--e2e-rounds 3]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd import synth  # noqa: E402
from acvm_amd.acir import Circuit, Expression as E, P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-tile", type=int, default=16)
ap.add_argument("--rounds", type=int, default=21, help="timed calls per run")
ap.add_argument("--pairs", type=int, default=3, help="A-B pairs of section 1")
ap.add_argument("--log2-total", type=int, default=20, help="instances of the end-to-end section (0: skip it)")
ap.add_argument("--e2e-rounds", type=int, default=3)
ap.add_argument("--only-masked", action="store_true", help="section 4 alone")
ap.add_argument("--masked-rounds", type=int, default=15, help="rotations of section 4's legs")
args = ap.parse_args()
U8, U32, BE32, IM = acvm_amd.ENC_U8, acvm_amd.ENC_U32, acvm_amd.ENC_BE32, acvm_amd.LAYOUT_INSTANCE_MAJOR


def timed(fn, rounds):
    fn()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return sorted(out)


def line(what, us, moved):
    med = us[len(us) // 2]
    print(f"  {what:44s} wall us median {med:8.1f} min {us[0]:8.1f} max {us[-1]:8.1f} | {moved / med / 1e3:6.0f} GB/s", flush=True)
    return med


def be32_rows(values):
    """[B][n] integers below 2^64 -> [B][n][32] big-endian bytes"""
    out = np.zeros(values.shape + (32,), dtype=np.uint8)
    out[..., 24:] = values.astype(">u8")[..., None].view(np.uint8).reshape(values.shape + (8,))
    return out


# ---- 4. the masked record import (defined here, run last -- or alone)
def masked_section():
    L = acvm_amd.lib()
    rng = np.random.default_rng(0x4EC04D6)
    ceiling = acvm_amd.stream_rate()
    print(f"4. masked record import; streaming ceiling of this device {ceiling:.0f} GB/s; wall us of the synchronous call, median (min) of "
          f"{args.masked_rounds} rotations of the legs, then of {args.masked_rounds} calls of each leg back to back", flush=True)
    n = 64
    hash_circ, hash_ids = synth.hash_circuit(n_msg=32)
    circuits = {"bytes": (acvm_amd.Circuit(hash_circ.to_bytes()), hash_ids, U8, 1),
                "fields": (acvm_amd.Circuit(Circuit(2 * n, [E([], [(3, k), (P - 1, n + k)], 1) for k in range(1, n + 1)]).to_bytes()), list(range(1, n + 1)), BE32, 32)}
    for log2 in (16, 17):
        B = 1 << log2
        for shape, (gc4, ids4, enc, size) in circuits.items():
            assert len(ids4) == n
            batch4 = acvm_amd.Batch(gc4, B, ids4)
            planes4 = batch4.stats()["n_byte_planes"]
            vals = rng.integers(0, 256, (B, n, size), dtype=np.uint8)
            if size == 32:
                vals[:, :, 0] &= 0x1F  # (below p)
            held = {"none": np.ones((B, n), dtype=np.uint8), "1 in 1000": np.ones((B, n), dtype=np.uint8), "everyone": np.ones((B, n), dtype=np.uint8)}
            j = np.arange(B)
            held["1 in 1000"][j[::1000], j[::1000] % n] = 0
            held["everyone"][j, j % n] = 0
            written = B * n * 32 + B * planes4 * 4 + B * 4
            d_cols, d_mask = acvm_amd.DeviceBuffer(vals.tobytes()), {k: acvm_amd.DeviceBuffer(h.tobytes()) for k, h in held.items()}
            cdesc = acvm_amd.ImportDesc(encoding=enc, layout=IM)
            for where in ("beside", "head"):
                pitch = n * (size + 1)
                if where == "beside":
                    fl = [(k, enc, k * (size + 1) + 1, k * (size + 1)) for k in range(n)]
                else:
                    fl = [(k, enc, n + k * size, k) for k in range(n)]
                far = sum(max(f[2] + size, f[3] + 1) - min(f[2], f[3]) > 256 for f in fl) if pitch > 256 else 0
                bufs = {}
                for k, h in held.items():
                    rec = np.zeros((B, pitch), dtype=np.uint8)
                    for f in fl:
                        rec[:, f[2]:f[2] + size] = vals[:, f[0]]
                        rec[:, f[3]] = h[:, f[0]]
                    bufs[k] = acvm_amd.DeviceBuffer(rec.tobytes())
                    del rec
                udesc4, _k1 = acvm_amd.record_desc(pitch, [f[:3] for f in fl])
                mdesc4, _k2 = acvm_amd.record_masked_desc(pitch, fl)
                legs = {
                    "(i) unmasked record import": lambda: L.acvm_batch_import_device_records(batch4._h, udesc4, bufs["none"].ptr),
                    "(ii) masked, nothing absent": lambda: L.acvm_batch_import_device_records_masked(batch4._h, mdesc4, bufs["none"].ptr),
                    "(iii) masked, 1 in 1000 absent": lambda: L.acvm_batch_import_device_records_masked(batch4._h, mdesc4, bufs["1 in 1000"].ptr),
                    "(iii) masked, everyone absent": lambda: L.acvm_batch_import_device_records_masked(batch4._h, mdesc4, bufs["everyone"].ptr),
                    "column import, no mask": lambda: L.acvm_batch_import_device(batch4._h, cdesc, d_cols.ptr),
                    "column import + mask pass, nothing absent": lambda: L.acvm_batch_import_device_masked(batch4._h, cdesc, d_cols.ptr, d_mask["none"].ptr),
                    "column import + mask pass, everyone absent": lambda: L.acvm_batch_import_device_masked(batch4._h, cdesc, d_cols.ptr, d_mask["everyone"].ptr),
                }
                times = {k: [] for k in legs}
                for fn in legs.values():
                    assert fn() == 0
                for _ in range(args.masked_rounds):
                    for k, fn in legs.items():
                        t0 = time.perf_counter()
                        fn()
                        times[k].append((time.perf_counter() - t0) * 1e6)
                med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
                # ... and each leg on its own, back to back as sections 1 and 2 time theirs: what a rotation adds to a leg is its predecessor's
                alone = {k: timed(fn, args.masked_rounds) for k, fn in legs.items()}
                print(f"  2^{log2} x {shape}, mask bytes {where} ({far} of {n} far), pitch {pitch}: {B * pitch / 1e6:.1f} MB read, {written / 1e6:.1f} MB written", flush=True)
                for k, v in times.items():
                    moved = written + (B * pitch if k.startswith("(") else B * n * size + (B * n if "mask pass" in k else 0))
                    solo = alone[k][len(alone[k]) // 2]
                    print(f"    {k:44s} {med[k]:8.1f} ({min(v):8.1f}) us | {moved / med[k] / 1e3:6.0f} GB/s, {moved / med[k] / 1e3 / ceiling:5.2f} of the ceiling"
                          f" | back to back {solo:8.1f} ({alone[k][0]:8.1f}) us, {moved / solo / 1e3 / ceiling:5.2f}", flush=True)
                for tag in ("nothing", "everyone"):
                    pass_us = med[f"column import + mask pass, {tag} absent"] - med["column import, no mask"]
                    print(f"    (iv) record import + the mask pass, {tag} absent: {med['(i) unmasked record import']:.1f} + {pass_us:.1f} = "
                          f"{med['(i) unmasked record import'] + pass_us:.1f} us", flush=True)
                for x in bufs.values():
                    x.free()
            for x in [d_cols, batch4] + list(d_mask.values()):
                x.free()


if args.only_masked:
    masked_section()
    sys.exit(0)

# ---- 1. dense byte records on config 3's tile
B = 1 << args.log2_tile
circ, ids = synth.hash_circuit(n_msg=32)
gc = acvm_amd.Circuit(circ.to_bytes())
n_in = len(ids)
batch = acvm_amd.Batch(gc, B, ids)
planes = batch.stats()["n_byte_planes"]
rng = np.random.default_rng(0x4EC04D5)
digits = rng.integers(0, 256, (B, n_in), dtype=np.uint8)
d_bytes = acvm_amd.DeviceBuffer(digits.tobytes())
d_be32 = acvm_amd.DeviceBuffer(be32_rows(digits.astype(np.uint64)).tobytes())
rows_out = B * n_in * 32 + B * planes * 4 + B * 4
fields = [(k, U8, k) for k in range(n_in)]
print(f"1. config 3's tile: {B} instances x {n_in} byte inputs, {planes} byte planes; {rows_out / 1e6:.1f} MB of rows, plane and event words written per import", flush=True)
# (the descriptors are built once and the C entry points called directly: 64 ctypes structures per call would be most of a call's time)
L = acvm_amd.lib()
rdesc, _rkeep = acvm_amd.record_desc(n_in, fields)
udesc, bdesc = acvm_amd.ImportDesc(encoding=U8, layout=IM), acvm_amd.ImportDesc(encoding=BE32, layout=IM)
rec, u8 = [], []
for pair in range(args.pairs):
    rec.append(line(f"pair {pair} A: 64-byte records", timed(lambda: L.acvm_batch_import_device_records(batch._h, rdesc, d_bytes.ptr), args.rounds), rows_out + B * n_in))
    u8.append(line(f"pair {pair} B: ENC_U8 instance-major", timed(lambda: L.acvm_batch_import_device(batch._h, udesc, d_bytes.ptr), args.rounds), rows_out + B * n_in))
print(f"  records: medians {min(rec):.1f} .. {max(rec):.1f} us; ENC_U8: medians {min(u8):.1f} .. {max(u8):.1f} us; "
      f"records {'inside' if min(u8) <= sorted(rec)[len(rec) // 2] <= max(u8) else 'OUTSIDE'} the spread of the ENC_U8 runs", flush=True)
line("ENC_BE32 instance-major (32-byte elements)", timed(lambda: L.acvm_batch_import_device(batch._h, bdesc, d_be32.ptr), args.rounds), rows_out + B * n_in * 32)
for x in (d_bytes, d_be32, batch):
    x.free()

# ---- 2. the mixed 108-byte record
dt = np.dtype([("msg", np.uint8, 64), ("root", "V32"), ("idx", "<u4"), ("flags", np.bool_, 8)])
pitch, mfields = acvm_amd.record_fields_from_dtype(dt, {"msg": range(64), "root": 64, "idx": 65, "flags": range(66, 74)})
n_m = 74
mc = acvm_amd.Circuit(Circuit(2 * n_m, [E([], [(3, k), (P - 1, n_m + k)], 1) for k in range(1, n_m + 1)]).to_bytes())
mb = acvm_amd.Batch(mc, B, list(range(1, n_m + 1)))
records = np.zeros(B, dtype=dt)
records["msg"] = rng.integers(0, 256, (B, 64), dtype=np.uint8)
roots = rng.integers(0, 256, (B, 32), dtype=np.uint8)
roots[:, 0] &= 0x1F  # (below p: the BE32 leg holds the same value)
records["root"] = roots.view("V32").reshape(B)
records["idx"] = rng.integers(0, 1 << 32, B, dtype=np.uint64).astype("<u4")
records["flags"] = rng.integers(0, 2, (B, 8)).astype(np.bool_)
values = np.zeros((B, n_m, 32), dtype=np.uint8)
values[:, :64] = be32_rows(records["msg"].astype(np.uint64))
values[:, 64] = roots
values[:, 65] = be32_rows(records["idx"].astype(np.uint64))
values[:, 66:] = be32_rows(records["flags"].astype(np.uint64))
d_rec, d_val = acvm_amd.DeviceBuffer(records.tobytes()), acvm_amd.DeviceBuffer(values.tobytes())
moved = B * n_m * 32 + B * 4
print(f"2. mixed record: {B} instances x {pitch} bytes, {n_m} inputs (64 x u8, 1 x 32 bytes, 1 x u32, 8 x bool), no byte planes", flush=True)
mdesc, _mkeep = acvm_amd.record_desc(pitch, mfields)
line("108-byte records", timed(lambda: L.acvm_batch_import_device_records(mb._h, mdesc, d_rec.ptr), args.rounds), moved + B * pitch)
mb.solve()
a = mb.extract(list(range(1, 2 * n_m + 1)), n=4096)
line("ENC_BE32 instance-major, the same values", timed(lambda: L.acvm_batch_import_device(mb._h, bdesc, d_val.ptr), args.rounds), moved + B * n_m * 32)
mb.solve()
print(f"  the two imports leave the same witnesses (first 4096 instances): {bool(np.array_equal(a, mb.extract(list(range(1, 2 * n_m + 1)), n=4096)))}", flush=True)
for x in (d_rec, d_val, mb):
    x.free()

# ---- 3. end to end from host memory
if args.log2_total:
    N = 1 << args.log2_total
    keep = list(range(n_in + 33, n_in + 65))  # the Keccak digest bytes
    node = acvm_amd.Node(gc, ids, keep=keep, devices=[0], tile=B)
    host_bytes = rng.integers(0, 256, (N, n_in), dtype=np.uint8)
    host_be32 = be32_rows(host_bytes.astype(np.uint64))
    print(f"3. end to end: {N} instances of config 3's circuit, tiles of {B}, one device; inputs from pageable host memory, no outputs asked for", flush=True)
    for r in range(args.e2e_rounds):
        for name, row, call in (("acvm_node_solve, 32-byte rows", n_in * 32, lambda: node.solve(host_be32, N, results=False, kept=False, digests=False)),
                                ("acvm_node_solve_records, 64-byte records", n_in, lambda: node.solve_records(host_bytes, N, n_in, fields, results=False, kept=False, digests=False))):
            t0 = time.perf_counter()
            not_solved = call()[0]
            dt_s = time.perf_counter() - t0
            st = node.stats()
            print(f"  round {r} {name:42s} {N / dt_s / 1e6:8.2f} M instances/s  wall ms {dt_s * 1e3:8.1f}  H2D {N * row / 1e6:8.1f} MB ({N * row / dt_s / 1e9:5.1f} GB/s)  "
                  f"device ms {sum(st['solve_device_ms']):7.1f} h2d wait ms {sum(st['h2d_wait_ms']):7.1f}  not solved {not_solved}", flush=True)
    n_check = min(N, 2 * B + 100)
    a, b = node.solve(host_be32[:n_check], n_check), node.solve_records(host_bytes[:n_check], n_check, n_in, fields)
    same = a[0] == b[0] and [r.as_tuple() for r in a[1]] == [r.as_tuple() for r in b[1]] and all(np.array_equal(a[k], b[k]) for k in (2, 3, 4))
    print(f"  results, kept witnesses, assigned bytes and digests of the first {n_check} instances agree: {bool(same)}", flush=True)
    node.free()

masked_section()
