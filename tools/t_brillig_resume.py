"""What a long Brillig program costs on the exact path with a restart per raised limit and with brillig_resume = 1 (csrc/brillig_resume.hpp): the
counting loop of tests/test_gpu_brillig_limits.py -- 4 n + 6 steps -- at 2^20, 2^22 and 2^24 steps, ONE instance, in one process.

    python tools/t_brillig_resume.py [log2 list = 20,22,24] [slice_log2 = 20] [base_log2 = 16]
Both modes lose a first pass of 2^base_log2 steps in the class scratch. restart: brillig_resume = 0 with brillig_steps_max_log2 raised to the
program's length -- 16-fold passes, each from the program's start; resume: slices of 2^slice_log2 steps, each continuing the one before.
Prints one JSON line: per length and mode the wall time of the solve, the retry passes, and under resume the steps executed in compact passes and
the lanes continued -- hence steps per second of one exact lane.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acvm_amd
from acvm_amd.acir import Brillig, Circuit, Expression as E
from acvm_amd.synth import values_from_rows

logs = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "20,22,24").split(",")]
slice_log2 = int(sys.argv[2]) if len(sys.argv) > 2 else 20
base_log2 = int(sys.argv[3]) if len(sys.argv) > 3 else 16

bc = [("Const", 1, 0), ("Const", 2, 1),
      ("BinaryFieldOp", 3, "Equals", 1, 0), ("JumpIf", 3, 6),
      ("BinaryFieldOp", 1, "Add", 1, 2), ("Jump", 2),
      ("Mov", 0, 1), ("Stop",)]
data = Circuit(2, [Brillig(inputs=[E.from_witness(1)], outputs=[2], bytecode=bc)]).to_bytes()
out = {"device": acvm_amd.device_arch(), "slice_log2": slice_log2, "base_log2": base_log2, "runs": []}
for lg in logs:
    n = ((1 << lg) - 6) // 4
    steps = 4 * n + 6
    for mode, keys in (("restart", dict(brillig_resume=0, brillig_steps_log2=base_log2, brillig_steps_max_log2=max(lg, base_log2))),
                       ("resume", dict(brillig_resume=1, brillig_steps_log2=base_log2, brillig_steps_max_log2=slice_log2, brillig_steps_total_log2=40))):
        with acvm_amd.tuning(**keys):
            batch = acvm_amd.Batch(acvm_amd.Circuit(data), 1, [1])
            batch.set_initial_witness(values_from_rows([[n]]))
            batch.set_force_slow_path(True)
            t0 = time.perf_counter()
            not_solved = batch.solve()
            dt = time.perf_counter() - t0
            asg, vals = batch.witness_map()
            ok = not_solved == 0 and int.from_bytes(vals[0, 2].tobytes(), "big") == n
            st = batch.brillig_resume_stats()
            out["runs"].append(dict(log2=lg, steps=steps, mode=mode, ok=ok, seconds=round(dt, 4), passes=batch.stats()["n_brillig_retries"],
                                    steps_executed=st["steps_executed"], lanes_continued=st["lanes_continued"],
                                    steps_per_second=round(steps / dt)))
            batch.free()
print(json.dumps(out))
