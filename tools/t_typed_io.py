"""The narrow encodings of the device I/O on config 3's shape (2^16 instances x 64 byte inputs with byte planes: synth.hash_circuit(n_msg=32)),
after tools/t_import_device.py: wall time of the synchronous call, the bytes it moves (source read + rows written + plane and event words for an
import; rows read + elements and mask bytes written for an export), against the streaming ceiling of acvm_debug_stream_rate.
  import: the 64 byte inputs as ACVM_ENC_U8 witness-major and instance-major against ACVM_ENC_BE32 witness-major (and the plain descriptor)
  export: the 64 digest witnesses as ACVM_ENC_U8 against ACVM_ENC_BE32, both layouts, with the mask
A call is a launch and a stream synchronisation: for kernel times run the tool under `rocprofv3 --kernel-trace --stats` in a run of its own
(every line uses a kernel of its own: import_witness_kernel, import_device_wm_kernel, import_narrow_wm_kernel, import_narrow_im_kernel,
export_device_direct_kernel, export_device_im_kernel, export_narrow_direct_kernel, export_narrow_im_kernel). A library without the narrow
encodings (an older build through ACVM_AMD_LIB, tools/gpu_ab_lib.sh) runs the 32-byte lines only.
    python tools/t_typed_io.py [--log2-tile 16] [--rounds 21]"""
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
ap.add_argument("--rounds", type=int, default=21)
args = ap.parse_args()
IM, WM = acvm_amd.LAYOUT_INSTANCE_MAJOR, acvm_amd.LAYOUT_WITNESS_MAJOR
BE32, U8 = acvm_amd.ENC_BE32, acvm_amd.ENC_U8
narrow = hasattr(acvm_amd.lib(), "acvm_batch_import_device_parts")


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
    print(f"  {what:38s} wall us median {med:9.1f} min {us[0]:9.1f} max {us[-1]:9.1f} | {moved / 1e6:7.1f} MB moved, {moved / med / 1e3:7.0f} GB/s = "
          f"{moved / med / 1e3 / ceiling:.2f} of the ceiling", flush=True)
    return med


ceiling = max(acvm_amd.stream_rate(1 << 30) for _ in range(3))
print(f"streaming ceiling (acvm_debug_stream_rate, 3 x 1 GiB): {ceiling:.0f} GB/s; narrow encodings: {'yes' if narrow else 'no (an older library)'}", flush=True)
circ, ids = synth.hash_circuit(n_msg=32)
B, n_in = 1 << args.log2_tile, len(ids)
batch = acvm_amd.Batch(acvm_amd.Circuit(circ.to_bytes()), B, ids)
planes = batch.stats()["n_byte_planes"]
written = B * n_in * 32 + B * planes * 4 + B * 4
print(f"config 3: {B} instances x {n_in} inputs, {planes} byte planes", flush=True)
digits = np.random.default_rng(0x1A90D7).integers(0, 256, (B, n_in), dtype=np.uint8)
be = np.zeros((B, n_in, 32), dtype=np.uint8)
be[:, :, 31] = digits
src = {("be32", IM): acvm_amd.DeviceBuffer(be.tobytes()), ("be32", WM): acvm_amd.DeviceBuffer(np.ascontiguousarray(be.transpose(1, 0, 2)).tobytes())}
if narrow:
    src[("u8", IM)] = acvm_amd.DeviceBuffer(digits.tobytes())
    src[("u8", WM)] = acvm_amd.DeviceBuffer(np.ascontiguousarray(digits.T).tobytes())
print("import", flush=True)
med = {}
for (ename, layout), buf in src.items():
    enc, size = (BE32, 32) if ename == "be32" else (U8, 1)
    what = f"{ename} {'witness-major' if layout == WM else 'instance-major'}" + (" (the plain launch)" if (ename, layout) == ("be32", IM) else "")
    med[(ename, layout)] = line(what, timed(lambda: batch.import_device(buf.ptr, encoding=enc, layout=layout), args.rounds), B * n_in * size + written)
if narrow:
    for layout in (WM, IM):
        print(f"  u8 {'witness-major' if layout == WM else 'instance-major'} / be32 witness-major: {med[('u8', layout)] / med[('be32', WM)]:.2f} by wall time, "
              f"{(B * n_in + written) / (B * n_in * 32 + written):.2f} by bytes", flush=True)
batch.import_device(src[("be32", IM)].ptr)
assert batch.solve() == 0
digests = list(range(n_in + 1, n_in + 65))
out, mask = acvm_amd.DeviceBuffer(size=B * 64 * 32), acvm_amd.DeviceBuffer(size=B * 64)
print("export of the 64 digest witnesses, with the mask", flush=True)
for ename, enc, size in (("be32", BE32, 32), ("u8", U8, 1)):
    if enc == U8 and not narrow:
        continue
    for layout in (WM, IM):
        what = f"{ename} {'witness-major' if layout == WM else 'instance-major'}"
        line(what, timed(lambda: batch.export_device(out.ptr, encoding=enc, layout=layout, witnesses=digests, d_assigned=mask.ptr), args.rounds), B * 64 * (32 + size + 1))
for x in list(src.values()) + [out, mask, batch]:
    x.free()
