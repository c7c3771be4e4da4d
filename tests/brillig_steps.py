"""How many VM steps a Brillig opcode runs: tests/brillig_ref.py's VM with a counter around process_opcode (one call = one instruction the reference's
VM::process_opcode executes, brillig_vm/src/lib.rs:154-307). The step budgets of tests/test_gpu_brillig_resume.py are set against these counts."""
import brillig_ref
from acvm_amd.acir import Brillig, Expression


def padded_loop(pad):
    """counting_loop of tests/test_gpu_brillig_limits.py with `pad` more Const instructions behind the loop: 4 n + 6 + pad steps on input n"""
    bc = [("Const", 1, 0), ("Const", 2, 1),
          ("BinaryFieldOp", 3, "Equals", 1, 0), ("JumpIf", 3, 6),
          ("BinaryFieldOp", 1, "Add", 1, 2), ("Jump", 2)] + [("Const", 4, 7)] * pad + [("Mov", 0, 1), ("Stop",)]
    return Brillig(inputs=[Expression.from_witness(1)], outputs=[2], bytecode=bc)


def loop_of(steps):
    """(pad, n): padded_loop(pad) on input n runs exactly `steps` steps"""
    pad = (steps - 6) % 4
    return pad, (steps - 6 - pad) // 4


def count_steps(brillig, wm, extra_results=()):
    """(outcome, steps) of brillig_ref.run(brillig, dict(wm), extra_results)"""
    steps = [0]

    plain = brillig_ref.VM

    class CountingVM(plain):
        def process_opcode(self):
            steps[0] += 1
            return plain.process_opcode(self)

    brillig_ref.VM = CountingVM
    try:
        outcome = brillig_ref.run(brillig, dict(wm), extra_results)
    finally:
        brillig_ref.VM = plain
    return outcome, steps[0]
