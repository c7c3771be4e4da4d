"""The record export (acvm_batch_export_device_records) measured, one process: on config 3's tile (2^16 instances of
synth.hash_circuit(n_msg=32)) the 32 Keccak digest bytes plus one Field leave as

 1. records { digest: [u8; 32], root: Field } of 64 bytes: 32 ACVM_ENC_U8 fields and one ACVM_ENC_BE32 field, one launch;
 2. the same 33 witnesses through acvm_batch_export_device instance-major as ACVM_ENC_U8 (one byte per element: the Field truncated);
 3. the same 33 witnesses as ACVM_ENC_BE32 (32 bytes per element), the form a consumer of rows had to take before.

Run A-B-C in turns. All three load the same 33 rows of 32 bytes per instance; what differs is what they write. Wall time of the synchronous
call: a launch and a stream synchronisation, tens of microseconds of which are not the kernel's. For kernel times run under
`rocprofv3 --kernel-trace --stats` and read export_records_kernel / export_narrow_im_kernel / export_device_im_kernel.
    python tools/t_records_out.py [--log2-tile 16] [--rounds 21] [--turns 3]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-tile", type=int, default=16)
ap.add_argument("--rounds", type=int, default=21, help="timed calls per run")
ap.add_argument("--turns", type=int, default=3, help="A-B-C turns")
args = ap.parse_args()
U8, BE32, IM = acvm_amd.ENC_U8, acvm_amd.ENC_BE32, acvm_amd.LAYOUT_INSTANCE_MAJOR


def timed(fn, rounds):
    fn()
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        rc = fn()
        out.append((time.perf_counter() - t0) * 1e6)
        assert rc == 0, acvm_amd.lib().acvm_last_error()
    return sorted(out)


def line(what, us, moved):
    med = us[len(us) // 2]
    print(f"  {what:52s} wall us median {med:8.1f} min {us[0]:8.1f} max {us[-1]:8.1f} | {moved / med / 1e3:6.0f} GB/s", flush=True)
    return med


B = 1 << args.log2_tile
circ, ids = synth.hash_circuit(n_msg=32)
gc = acvm_amd.Circuit(circ.to_bytes())
n_in = len(ids)
digest = list(range(n_in + 33, n_in + 65))  # the Keccak digest bytes
root = ids[0]
ws = digest + [root]
batch = acvm_amd.Batch(gc, B, ids)
rng = np.random.default_rng(0x4EC04D6)
values = np.zeros((B, n_in, 32), dtype=np.uint8)
values[:, :, 31] = rng.integers(0, 256, (B, n_in), dtype=np.uint8)
batch.set_initial_witness(values.tobytes())
assert batch.solve() == 0
loaded = B * len(ws) * 32
print(f"config 3's tile: {B} instances, {len(ws)} witnesses each (32 digest bytes, one Field): {loaded / 1e6:.1f} MB of rows loaded per export", flush=True)

pitch = 64
fields = [(w, U8, k) for k, w in enumerate(digest)] + [(root, BE32, 32)]
d_rec = acvm_amd.DeviceBuffer(size=B * pitch)
d_u8 = acvm_amd.DeviceBuffer(size=B * len(ws))
d_be = acvm_amd.DeviceBuffer(size=B * len(ws) * 32)
L = acvm_amd.lib()
# (the descriptors are built once and the C entry points called directly: 33 ctypes structures per call would be most of a call's time)
rdesc, _rkeep = acvm_amd.record_out_desc(pitch, fields, 0, B)
warr = (acvm_amd.C.c_uint32 * len(ws))(*ws)
udesc = acvm_amd.ExportDesc(encoding=U8, layout=IM, first=0, n=B, witnesses=warr, n_witnesses=len(ws), stride=0)
bdesc = acvm_amd.ExportDesc(encoding=BE32, layout=IM, first=0, n=B, witnesses=warr, n_witnesses=len(ws), stride=0)
rec, u8, be = [], [], []
for turn in range(args.turns):
    rec.append(line(f"turn {turn} A: 64-byte records (32 x u8 + BE32)", timed(lambda: L.acvm_batch_export_device_records(batch._h, rdesc, None, d_rec.ptr), args.rounds), loaded + B * pitch))
    u8.append(line(f"turn {turn} B: ENC_U8 instance-major, 33 bytes per instance", timed(lambda: L.acvm_batch_export_device(batch._h, udesc, d_u8.ptr, None), args.rounds), loaded + B * len(ws)))
    be.append(line(f"turn {turn} C: ENC_BE32 instance-major, 1056 bytes per instance", timed(lambda: L.acvm_batch_export_device(batch._h, bdesc, d_be.ptr, None), args.rounds), loaded + B * len(ws) * 32))
med = lambda x: sorted(x)[len(x) // 2]
print(f"  medians of the turns: records {med(rec):.1f} us, ENC_U8 {med(u8):.1f} us, ENC_BE32 {med(be):.1f} us; records / ENC_U8 = {med(rec) / med(u8):.2f}, "
      f"records / ENC_BE32 = {med(rec) / med(be):.2f}", flush=True)
# the three forms hold the same bytes
r = np.frombuffer(d_rec.download(), dtype=np.uint8).reshape(B, pitch)
u = np.frombuffer(d_u8.download(), dtype=np.uint8).reshape(B, len(ws))
b = np.frombuffer(d_be.download(), dtype=np.uint8).reshape(B, len(ws), 32)
print(f"  digest bytes agree (records, ENC_U8, ENC_BE32): {bool(np.array_equal(r[:, :32], u[:, :32]) and np.array_equal(r[:, :32], b[:, :32, 31]))}; "
      f"the Field agrees (records, ENC_BE32): {bool(np.array_equal(r[:, 32:], b[:, 32]))}", flush=True)
for x in (d_rec, d_u8, d_be, batch):
    x.free()
