"""The Arithmetic level program executed on the HOST: tools/gate_host_test.hip runs the planner's gate records through the same record
evaluation as arith_level_kernel (acvm_amd/csrc/gate_eval.hpp is __host__ __device__) with every stored row raised to the worst
representative the planner's bound allows (relaxed rows: any representative below 2^256), checks each value against that bound, and
writes the canonical witness maps, which are compared here with the CPU oracle's (ArithmeticSolver, acvm/src/pwg/arithmetic.rs:27-127).
No GPU is needed: hipcc builds the host side only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import arith_cases as ac
from acvm_amd import synth
from acvm_amd.acir import P, Circuit, Expression as E
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acvm_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = str(tmp_path_factory.mktemp("gate_host") / "gate_host_test")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-x", "hip", os.path.join(ROOT, "tools", "gate_host_test.hip"),
                    os.path.join(CSRC, "plan.cpp"), os.path.join(CSRC, "circuit.cpp"), os.path.join(CSRC, "tuning.cpp"), "-lz", "-o", out],
                   check=True, timeout=900)
    return out


def run(exe, tmp_path, circ, ids, values, B, seed=1, tuning=None):
    data = circ.to_bytes()
    blob = struct.pack("<I", len(data)) + data + struct.pack("<I", len(ids)) + struct.pack(f"<{len(ids)}I", *ids) + struct.pack("<I", B) + bytes(values)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fin, "wb").write(blob)
    env = dict(os.environ)
    if tuning:
        env["ACVM_TUNING"] = tuning
    r = subprocess.run([exe, fin, fout, str(seed)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:] + r.stderr[-1000:]
    raw = np.fromfile(fout, dtype=np.uint8)
    nw, b = struct.unpack("<II", raw[:8].tobytes())
    rec = raw[8:].reshape(b, 4 + nw * 33)
    flagged = rec[:, :4].copy().view(np.uint32)[:, 0]
    body = rec[:, 4:].reshape(b, nw, 33)
    ores, oasg, ovals = ob.solve_batch(ob.Circuit(data), ids, values, B)
    n_cmp = 0
    for j in range(B):
        generic = ores[j].as_tuple()[0] == 0 and flagged[j] == 0xFFFFFFFF  # status Solved
        if flagged[j] != 0xFFFFFFFF:
            continue  # left the generic path (zero denominator / failing assert): the exact kernels own it on the device
        assert generic, (j, ores[j].as_tuple())
        produced = body[j, :, 0].astype(bool)
        assert np.array_equal(produced[: oasg.shape[1]], oasg[j].astype(bool)), j
        assert np.array_equal(body[j, produced, 1:], ovals[j][produced[: oasg.shape[1]]]), j
        n_cmp += 1
    assert n_cmp >= B // 2
    return r.stdout


def test_config2_mix(exe, tmp_path):
    circ, ids = synth.arithmetic_circuit(3000, seed=0xAC1D0002)
    out = run(exe, tmp_path, circ, ids, synth.witness_batch(6, seed=0xAC1D0002, edge_cases=False), 6)
    assert "raised by p" in out


def test_linear_chains_force_the_weak_reduction(exe, tmp_path):
    # every gate adds its predecessor with coefficient +-1: the bound grows by one or two p per gate until the planner asks for a reduction
    circ, ids = synth.arithmetic_circuit(600, seed=5, chain=True, mix=(10, 80, 10, 0))
    out = run(exe, tmp_path, circ, ids, synth.witness_batch(4, seed=5, edge_cases=False), 4)
    modes = [int(x) for x in out.split("asis/weak/canon ")[1].split(",")[0].split("/")]
    assert modes[1] > 20, out


def test_wide_gates_and_asserts(exe, tmp_path):
    # up to 200 + 200 terms per gate (the side sum's limb budget and the periodic reduction of the running sum), satisfied assert gates
    for seed, mt, n in ((0xAC1D0A11, 12, 120), (77, 40, 100), (123, 200, 30)):
        circ, ids = synth.wide_gate_circuit(n, seed=seed, max_terms=mt)
        run(exe, tmp_path, circ, ids, synth.witness_batch(3, seed=seed, edge_cases=False), 3, seed=seed)


def test_unit_coefficient_gates(exe, tmp_path):
    # sums and differences only (no multiplier at all), and products with coefficient -1
    n_in = 4
    ops, out = [], n_in
    for i in range(200):
        out += 1
        a, b, c = 1 + (7 * i) % (out - 1), 1 + (11 * i + 3) % (out - 1), 1 + (13 * i + 5) % (out - 1)
        if i % 3 == 0:
            ops.append(E([], [(1, a), (P - 1, b), (1, c), (P - 1, out)], i % 5))
        elif i % 3 == 1:
            ops.append(E([(P - 1, a, b)], [(P - 1, c), (1, out)], 0))
        else:
            ops.append(E([(1, a, b), (P - 1, b, c)], [(1, out)], 3))
    circ = Circuit(current_witness_index=out, opcodes=ops, private_parameters=list(range(1, n_in + 1)), return_values=[out])
    run(exe, tmp_path, circ, list(range(1, n_in + 1)), synth.witness_batch(4, n_in=n_in, seed=9, edge_cases=False), 4)


def test_without_relaxed_rows(exe, tmp_path):
    circ, ids = synth.arithmetic_circuit(800, seed=3)
    out = run(exe, tmp_path, circ, ids, synth.witness_batch(3, seed=3, edge_cases=False), 3, tuning="relax=0")
    modes = [int(x) for x in out.split("asis/weak/canon ")[1].split(",")[0].split("/")]
    assert modes[0] == 0 and modes[1] == 0


# list C of tests/arith_cases.py: forced outputs at the limb boundaries, sums that are k p, 0..20 and 254..300 unit terms of each kind, 255 general terms, 31..65
# multiplied terms (16, 17, 32 and 33 reductions), the grid of record shapes, the large bounds under subtraction and in front of the inverse. The tool runs
# plans of gates alone that cover their circuit, so the RANGE readers are left out (they assign nothing: the rows and the maps stay what they are; an output
# they pinned may now be stored relaxed, which is one more plan to bound) and the two circuits whose plan ends at a gate of 256 general terms do not run here.
LIST_C = [c for c in ac.lists()["C"] if ac.expected_truncation(c) == ac.NOT_TRUNCATED]


@pytest.mark.parametrize("tuning", [None, "scale=0"], ids=["default", "scale=0"])
@pytest.mark.parametrize("case", LIST_C, ids=lambda c: c.name)
def test_list_c_of_the_arithmetic_edge_cases(exe, tmp_path, case, tuning):
    gates = [op for op in case.circuit.opcodes if isinstance(op, E)]
    circ = Circuit(current_witness_index=case.circuit.current_witness_index, opcodes=gates)
    run(exe, tmp_path, circ, case.ids, synth.values_from_rows(case.rows), len(case.rows), tuning=tuning)
