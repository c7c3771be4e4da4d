"""The foreign-call round trip of a whole batch, per instance and on the device: the circuit of tests/test_gpu_foreign_relevel.py (two oracle calls per
instance, a 40-gate tail) at B = 2^16, one full drive = set_initial_witness, solve, answer everybody, solve, answer everybody, solve. The two forms
alternate in one process; a host clock around each drive, the bytes each form moved over PCIe for the round trip (acvm_debug_foreign_call_stats) and
the device times of the two batch-wide kernels (HIP events). The oracle is the same for both forms and costs nothing on either side, so that the
round trip itself is what is timed: an echo -- 'invert' answers its input, 'double' answers (its input, 0); the circuit constrains neither. On the
device that is no kernel at all: the Montgomery-256 witness-major column the inputs were written to is handed back as the first answer column, beside
a column of zeros. The per-instance form's answers are made by the host loop.
The form `rows` is the device form answered through acvm_batch_resolve_foreign_calls_device_rows with both of its device columns given (a length
column, read by the sizing launch, and a mask of ones, downloaded): what the per-row call costs on top of the one-shape call for the same answers.
    python tools/t_foreign_calls.py [--log2-b 16] [--rounds 5] [--tail 40] [--forms instance,device,rows]
With ACVM_AMD_LIB pointing at a build without the device form, --forms instance measures that build's per-instance form alone (A-B runs)."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd  # noqa: E402
from acvm_amd.acir import P, Brillig, Circuit, Expression as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-b", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tail", type=int, default=40)
ap.add_argument("--forms", default="instance,device")
args = ap.parse_args()
B = 1 << args.log2_b
W = E.from_witness


def circuit(n_tail):
    ops = [Brillig(inputs=[W(1)], outputs=[3], bytecode=[("ForeignCall", "invert", [("Register", 0)], [("Register", 0)]), ("Stop",)]),
           E([(1, 3, 1)], [(P - 1, 4)], 0),
           Brillig(inputs=[E([], [(1, 2), (1, 4)], 0)], outputs=[5, 6],
                   bytecode=[("ForeignCall", "double", [("Register", 0), ("Register", 1)], [("Register", 0)]), ("Stop",)])]
    nw = 6
    for i in range(n_tail):
        ops.append(E([(1, nw, nw - 1)], [(1, 5), (P - 1, nw + 1)], 0))
        nw += 1
    return Circuit(nw, ops), [1, 2]


circ, ids = circuit(args.tail)
gc = acvm_amd.Circuit(circ.to_bytes())
batch = None  # the handle of the form being driven: one handle per form, so that neither pays for what the other left in the result store
values = b"".join((3 + j).to_bytes(32, "big") + (1000 + 7 * j).to_bytes(32, "big") for j in range(B))
L = acvm_amd.lib()
has_stats = hasattr(L, "acvm_debug_foreign_call_stats")
N_OUT = {"invert": 1, "double": 2}


def fc_stats():
    return batch.foreign_call_stats() if has_stats else dict(h2d_bytes=0, d2h_bytes=0, inputs_kernel_ms=0.0, append_kernel_ms=0.0, store_bytes=0)


def answer_per_instance():
    """the caller's loop of acvm_js/src/execute.rs:109-113 over the batch, on the raw ABI (no Python object per value)"""
    info = acvm_amd.ForeignCallInfo()
    lens = (C.c_uint32 * 4)()
    vals = C.create_string_buffer(32 * 4)
    is_arr = bytes(2)
    one = (C.c_uint32 * 2)(1, 1)
    zero32 = bytes(32)
    n = 0
    for j in range(B):
        if L.acvm_batch_pending_foreign_call(batch._h, j, C.byref(info)) != 1:
            continue
        acvm_amd._check(L.acvm_batch_pending_foreign_call_inputs(batch._h, j, lens, vals))
        k = N_OUT[info.function.decode()]
        acvm_amd._check(L.acvm_batch_resolve_foreign_call(batch._h, j, k, is_arr, one, vals.raw[:32] + zero32 * (k - 1)))
        n += 1
    return n


kernel_ms = {"inputs": [], "append": []}


d_cols = acvm_amd.DeviceBuffer(data=bytes(2 * B * 32))  # two witness-major columns of Montgomery-256 elements; the second stays zero


d_row_lens = acvm_amd.DeviceBuffer(data=bytes(2 * B * 4))
d_answered = acvm_amd.DeviceBuffer(data=bytes([1]) * B)


def answer_on_device(per_row=False):
    n = 0
    for s in batch.foreign_call_sites():
        rows = s["n_waiting"]
        longest = batch.foreign_call_inputs_device(s["opcode_index"], s["brillig_index"], n_rows=rows)
        assert longest == 1
        batch.foreign_call_inputs_device(s["opcode_index"], s["brillig_index"], n_rows=rows, d_values=d_cols.ptr, encoding=acvm_amd.ENC_MONT256_LE,
                                         layout=acvm_amd.LAYOUT_WITNESS_MAJOR, n_columns=longest, stride=B)
        kernel_ms["inputs"].append(fc_stats()["inputs_kernel_ms"])
        k = N_OUT[s["function"]]
        # the echo oracle costs no kernel: the column the inputs were written to IS the first answer column, the zero column the second
        if per_row:
            batch.resolve_foreign_calls_device_rows(s["opcode_index"], s["brillig_index"], [None] * k, d_cols.ptr, n_rows=rows, encoding=acvm_amd.ENC_MONT256_LE,
                                                    layout=acvm_amd.LAYOUT_WITNESS_MAJOR, n_columns=k, stride=B, d_lens=d_row_lens.ptr, d_answered=d_answered.ptr)
        else:
            batch.resolve_foreign_calls_device(s["opcode_index"], s["brillig_index"], [None] * k, d_cols.ptr, n_rows=rows, encoding=acvm_amd.ENC_MONT256_LE,
                                               layout=acvm_amd.LAYOUT_WITNESS_MAJOR, n_columns=k, stride=B)
        kernel_ms["append"].append(fc_stats()["append_kernel_ms"])
        n += rows
    return n


def drive(form):
    global batch
    batch, answer = handles[form], forms[form]
    batch.set_initial_witness(values)
    t0 = time.perf_counter()
    s0 = fc_stats()
    rounds = 0
    while batch.solve():
        assert answer() > 0
        rounds += 1
    ms = (time.perf_counter() - t0) * 1e3
    s1 = fc_stats()
    assert rounds == 2
    return ms, s1["h2d_bytes"] - s0["h2d_bytes"], s1["d2h_bytes"] - s0["d2h_bytes"]


def stats(xs):
    xs = sorted(xs)
    return f"median {xs[len(xs) // 2]:10.3f} (min {xs[0]:10.3f} - max {xs[-1]:10.3f})"


forms = {"instance": answer_per_instance, "device": answer_on_device, "rows": lambda: answer_on_device(per_row=True)}
todo = [f for f in args.forms.split(",") if f]
handles = {f: acvm_amd.Batch(gc, B, ids) for f in todo}
maps = {}
for f in todo:  # warm-up: allocations, the first launches; and the two forms give the same witness maps
    drive(f)
    maps[f] = batch.digest().tobytes()
assert len(set(maps.values())) == 1, "the two forms disagree"
wall = {f: [] for f in todo}
moved = {}
for _ in range(args.rounds):
    for f in todo:
        ms, up, down = drive(f)
        wall[f].append(ms)
        moved[f] = (up, down)
print(f"relevel circuit, {args.tail}-gate tail, B = {B}, two calls per instance, {args.rounds} drives per form, library {acvm_amd.LIB_PATH}")
for f in todo:
    up, down = moved[f]
    print(f"  {f:8s} form: wall ms {stats(wall[f])} | per drive {up} B host-to-device, {down} B device-to-host" + ("" if has_stats else " (this build does not count)"))
if "device" in todo or "rows" in todo:
    print(f"  fc_inputs_kernel ms {stats(kernel_ms['inputs'])} | fc_append_kernel ms {stats(kernel_ms['append'])} (HIP events, one site of {B} rows per launch)")
d_cols.free()
for h in handles.values():
    h.free()
