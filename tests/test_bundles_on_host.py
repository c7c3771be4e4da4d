"""Bundles on the host (acvm_amd/csrc/gate_record.hpp "bundles"; tuning keys share, max_bundle): the planner's last pass groups the wave programs of a
gate launch that read the same operand row, and the gate kernel loads that row once per bundle. Here, without a GPU: the promises of that pass
(plan.cpp check_bundles) recomputed in Python from the decoded records over the circuit corpus, the two tuning keys, the injected violation, what the
pass finds on the headline circuit -- and gate_eval on the HOST with a shared operand: tools/gate_host_test.hip walks the bundles as arith_level_body
does (the row fetched once per bundle, every operand word that names it served from that copy) and its witness maps are compared with Python
integers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import acvm_amd
import bundle_cases as bc
from acvm_amd import synth
from acvm_amd.acir import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acvm_amd", "csrc")
DEFAULT_CAP = 8


def _plan(gc, ids, cap=None, **kw):
    mode = {"plan_validate": 1}
    if cap is not None:
        mode["max_bundle"] = cap
    with acvm_amd.tuning(**mode):
        return gc.gate_records(ids, **kw), gc.bundle_plan(ids, **kw)


def test_default_tuning():
    assert acvm_amd.tuning_get("share") == 1 and acvm_amd.tuning_get("max_bundle") == DEFAULT_CAP


def test_the_bundle_plan_keeps_its_promises_over_the_corpus():
    import circuit_corpus as cc
    n, n_shared = 0, 0
    for name, data, ids in cc.corpus():
        gc = acvm_amd.Circuit(data)
        if ids is None:
            ids = gc.witness_set("circuit_arguments")
        keep = gc.witness_set("return_values")
        for kw in ({}, {"reuse_slots": True, "keep": keep}, {"fold_digest": True}):
            try:
                records, plan = _plan(gc, ids, **kw)
            except acvm_amd.AcvmError as e:
                assert "slot reuse needs" in str(e), (name, kw, str(e))  # (the planner's only refusal on the corpus: tests/test_plan_host.py)
                continue
            assert plan["n_findings"] == 0, (name, kw)  # the hazard checker's partition check of the same table
            n_shared += bc.check_bundle_plan(records, plan, DEFAULT_CAP)[0]
            n += 1
    assert n >= 60 and n_shared >= 500


def test_share_0_gives_singletons_in_the_programs_order():
    circ, ids = synth.arithmetic_circuit(2000, seed=0xAC1D0002)
    gc = acvm_amd.Circuit(circ.to_bytes())
    with acvm_amd.tuning(share=0, plan_validate=1):
        plan = gc.bundle_plan(ids)
        n_programs = len(bc.programs_of(gc.gate_records(ids)))
    assert plan["n_shared_bundles"] == 0 and plan["n_shared_loads_saved"] == 0 and plan["n_bundles"] == n_programs
    # one program per bundle, no row, and the dispatch order the programs had (longest first inside a level: plan.cpp order_and_dependencies)
    assert [(b, r) for launch in plan["launches"] for b, r in launch] == [([q], None) for q in range(n_programs)]
    with acvm_amd.tuning(max_bundle=1):  # (below two programs per bundle there is nothing to share either)
        assert gc.bundle_plan(ids)["n_shared_bundles"] == 0


@pytest.mark.parametrize("cap", [2, 4, 8])
def test_max_bundle_is_respected(cap):
    circ, ids = synth.arithmetic_circuit(2000, seed=0xAC1D0002)
    gc = acvm_amd.Circuit(circ.to_bytes())
    for kw in ({}, {"reuse_slots": True, "keep": gc.witness_set("return_values")}):
        records, plan = _plan(gc, ids, cap=cap, **kw)
        n_shared, _ = bc.check_bundle_plan(records, plan, cap)
        assert n_shared > 50
        assert max(len(b) for launch in plan["launches"] for b, _ in launch) == cap  # (the early witnesses have readers enough to fill one)


def test_the_injected_violation_is_reported():
    circ, ids = synth.arithmetic_circuit(400, seed=3, mix=(30, 30, 20, 20))
    gc = acvm_amd.Circuit(circ.to_bytes())
    with acvm_amd.tuning(plan_validate=104):  # a wave program named twice
        with pytest.raises(acvm_amd.AcvmError, match="plan invariant violated after pass bundle_shared_rows"):
            gc.plan_stats(ids)
    with acvm_amd.tuning(plan_validate=1):
        assert gc.plan_stats(ids)["n_opcodes"] == 400
    # the same mutation of a copy of the finished plan: the hazard checker's partition check (schedule_check.cpp) sees a program run twice and one never
    assert gc.bundle_plan(ids)["n_findings"] == 0
    assert gc.bundle_plan(ids, mutation=1)["n_findings"] >= 2


def test_the_headline_circuit_saves_two_thousand_row_loads():
    circ, ids = synth.arithmetic_circuit(10000, seed=0xAC1D0002)
    gc = acvm_amd.Circuit(circ.to_bytes())
    records, plan = _plan(gc, ids)
    _, saved = bc.check_bundle_plan(records, plan, DEFAULT_CAP)
    assert saved >= 2000, saved  # of the ~17 000 rows an instance loads (operand rows and the inverses of the SOLVE_DYN records)
    # none of it touches what the fingerprint hashes or the traffic model: tests/test_plan_host.py pins both


def test_hot_inputs_bundle_nearly_every_program():
    circ, ids = synth.arithmetic_circuit(200, hot_inputs=True)
    gc = acvm_amd.Circuit(circ.to_bytes())
    records, plan = _plan(gc, ids)
    bc.check_bundle_plan(records, plan, DEFAULT_CAP)
    alone = sum(1 for launch in plan["launches"] for _, row in launch if row is None)
    # every operand is one of the 16 inputs: the greedy pass stops only when no row has two readers left, so at most one program per input stays alone
    assert alone <= 16 and plan["n_bundles"] - alone >= (len(bc.programs_of(records)) - 16) // DEFAULT_CAP


# ---------------------------------------------------------------------------------------------------------------- gate_eval on the host
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = str(tmp_path_factory.mktemp("gate_host_bundles") / "gate_host_test")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-x", "hip", os.path.join(ROOT, "tools", "gate_host_test.hip"),
                    os.path.join(CSRC, "plan.cpp"), os.path.join(CSRC, "circuit.cpp"), os.path.join(CSRC, "tuning.cpp"), "-lz", "-o", out],
                   check=True, timeout=900)
    return out


def _run_tool(exe, tmp_path, circ, ids, values, B, tuning=None):
    """-> (stdout, flagged [B], produced [B][nw] bool, canonical values [B][nw] as Python integers)"""
    data = circ.to_bytes()
    blob = struct.pack("<I", len(data)) + data + struct.pack("<I", len(ids)) + struct.pack(f"<{len(ids)}I", *ids) + struct.pack("<I", B) + bytes(values)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fin, "wb").write(blob)
    env = dict(os.environ)
    if tuning:
        env["ACVM_TUNING"] = tuning
    r = subprocess.run([exe, fin, fout, "1"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:] + r.stderr[-1000:]
    raw = np.fromfile(fout, dtype=np.uint8)
    nw, b = struct.unpack("<II", raw[:8].tobytes())
    rec = raw[8:].reshape(b, 4 + nw * 33)
    flagged = rec[:, :4].copy().view(np.uint32)[:, 0]
    body = rec[:, 4:].reshape(b, nw, 33)
    vals = [[int.from_bytes(body[j, w, 1:].tobytes(), "big") for w in range(nw)] for j in range(b)]
    return r.stdout, flagged, body[:, :, 0].astype(bool), vals


@pytest.mark.parametrize("tuning", [None, "max_bundle=2", "max_bundle=4", "scale=0", "share=0"])
def test_gate_eval_on_the_host_with_a_shared_operand(exe, tmp_path, tuning):
    """the shared row as the first factor of a product, as the second, as both, in a linear term, in a tail that also reads the forwarded value, in a
    SOLVE_DYN record's numerator and in an ASSERT: every place is reached by the plan, served from the bundle's copy, and the values are the integers'"""
    circ, ids = bc.shared_positions_circuit()
    mode = dict(kv.split("=") for kv in tuning.split(",")) if tuning else {}
    gc = acvm_amd.Circuit(circ.to_bytes())
    with acvm_amd.tuning(**{k: int(v) for k, v in mode.items()}):
        records, plan = gc.gate_records(ids), gc.bundle_plan(ids)
    if mode.get("share") != "0":
        assert bc.shared_operand_places(records, plan) == {"product_first", "product_second", "square", "linear", "beside_local", "solve_dyn", "assert"}
    B = 8
    rows = [[(0x9E3779B97F4A7C15 * (j * bc.N_IN + k + 1)) ** 5 % P for k in range(bc.N_IN)] for j in range(B)]
    rows[1] = [P - 1, 1, P - 1, 0]  # the edges of the field in the shared row and beside it
    rows[2] = [0, 5, 7, P - 1]      # the shared row is zero
    rows[3][1] = 0                  # a zero denominator: the instance leaves the generic path at the inversion
    out, flagged, produced, vals = _run_tool(exe, tmp_path, circ, ids, synth.values_from_rows(rows), B, tuning=tuning)
    served = int(out.split("operands served from them ")[1].split()[0])
    assert served == B * (plan["n_shared_loads_saved"] + plan["n_shared_bundles"])  # every operand word that names a bundle's row, in every instance
    assert (served == 0) == (mode.get("share") == "0")
    for j in range(B):
        want = bc.shared_positions_values(circ, rows[j])
        if want is None:
            assert flagged[j] != 0xFFFFFFFF and j == 3
            continue
        assert flagged[j] == 0xFFFFFFFF, j
        assert [w for w in range(len(produced[j])) if produced[j][w]] == sorted(want), j
        for w, v in want.items():
            assert vals[j][w] == v, (j, w)


def test_gate_eval_on_the_host_over_bundled_plans_against_the_oracle(exe, tmp_path):
    """whole plans with hundreds of bundles through the same walk: hot inputs (nearly every program bundled) and the config-2 mix, stored rows raised
    to the worst representative their bound allows -- the shared copy of a relaxed row included"""
    from test_gate_eval_on_host import run
    for circ, ids, seed in ((*synth.arithmetic_circuit(300, hot_inputs=True), 2), (*synth.arithmetic_circuit(1500, seed=0xAC1D0002), 3)):
        out = run(exe, tmp_path, circ, ids, synth.witness_batch(5, seed=seed, edge_cases=False), 5)
        assert int(out.split("operands served from them ")[1].split()[0]) > 5 * 100
