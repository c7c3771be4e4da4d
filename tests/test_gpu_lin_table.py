"""Linear tables on the device (tuning key lin_table; acvm_amd/csrc/gate_record.hpp "linear tables"): whole solves against the oracle, bit for bit,
with the tables (1) and without (0), the canonical witness maps of the two settings byte-equal, at batch sizes around the wave and the block --
circuits of linear gates only, of SOLVE_DYN gates only (with a planted zero denominator, which takes the exact path; at the default tuning the
planner's scale turns every numerator's coefficient into 1, so no record of it qualifies -- the same circuit runs once more with scale = 0, where 231 of
its 300 numerators carry a table), the inversion-heavy mix,
linear chains (fused tails with tables behind hosts with and without), wide gates (odd and even counts of coefficient terms, records with products
that keep the old form), unit coefficients only (no table anywhere), and the config-5 shape with recycled rows; inputs with the edge cases 0, p - 1
and unreduced 256-bit values. And fr29_lin_add itself through acvm_debug_lin_add over the case list of tests/lin_table_ref.py against Python
integers. The same routine on the host, 10^5 cases: tests/test_lin_table_on_host.py."""
import numpy as np
import pytest

import lin_table_ref as ref

pytestmark = pytest.mark.gpu

SIZES = (1, 64, 65, 130, 300)


def unit_coefficient_circuit():
    """sums and differences only, and products with coefficient +-1 (the circuit of tests/test_gate_eval_on_host.py): no general coefficient at all"""
    from acvm_amd.acir import P, Circuit, Expression as E
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
    return Circuit(current_witness_index=out, opcodes=ops, private_parameters=list(range(1, n_in + 1)), return_values=[out]), list(range(1, n_in + 1))


def build(name):
    """(circuit, ids, n_in, seed, planted zero: the input witness to clear in the last instance or None, handle options, tuning)"""
    from acvm_amd import synth
    if name == "linear":
        return synth.arithmetic_circuit(300, mix=(0, 100, 0, 0)) + (16, 1, None, {}, {})
    if name in ("solve_dyn", "solve_dyn_unscaled"):
        circ, ids = synth.arithmetic_circuit(300, mix=(0, 0, 0, 100))
        partner = next(t[1] for i, e in enumerate(circ.opcodes) for t in e.mul_terms if t[2] == 16 + 1 + i and t[1] <= 16)
        return circ, ids, 16, 2, partner, {}, {"scale": 0} if name == "solve_dyn_unscaled" else {}
    if name == "inversion_heavy":
        return synth.arithmetic_circuit(300, mix=(20, 20, 20, 40)) + (16, 3, None, {}, {})
    if name == "chains":
        return synth.arithmetic_circuit(600, seed=5, chain=True, mix=(10, 80, 10, 0)) + (16, 5, None, {}, {})
    if name == "wide":
        return synth.wide_gate_circuit(120, max_terms=12) + (16, 6, None, {}, {})
    if name == "unit":
        return unit_coefficient_circuit() + (4, 9, None, {}, {})
    if name == "mixed_reuse":
        return synth.mixed_circuit(900, seed=0xAC1D0711) + (16, 7, None, {"reuse_slots": True}, {})
    raise KeyError(name)


CIRCUITS = ("linear", "solve_dyn", "solve_dyn_unscaled", "inversion_heavy", "chains", "wide", "unit", "mixed_reuse")


@pytest.mark.parametrize("name", CIRCUITS)
def test_whole_solves_with_and_without_tables(oracle, name):
    import acvm_amd
    from acvm_amd import synth
    circ, ids, n_in, seed, planted, opts, mode = build(name)
    data = circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    if opts.get("reuse_slots"):
        opts = dict(opts, keep=gc.witness_set("return_values"))
    # what the plan holds: tables where the shapes say so, none where no record qualifies or the key is off
    with acvm_amd.tuning(**mode):
        info = gc.lin_plan(ids, **{k: v for k, v in opts.items() if k in ("reuse_slots", "keep")})
    assert info["ok"], info["report"]
    if name in ("unit", "solve_dyn"):
        assert info["n_lin_terms"] == 0 and info["n_programs_with_tables"] == 0
    else:
        assert 0 < info["n_lin_records"] <= info["n_lin_terms"]
    if name in ("linear", "solve_dyn_unscaled"):
        assert info["n_lin_records"] >= 200
    if name == "chains":  # tails behind their hosts, records with and without tables inside the programs
        assert info["n_gate_records"] > info["n_wave_programs"] >= info["n_programs_with_tables"] > 0 and info["n_lin_records"] < info["n_gate_records"]
    if name == "wide":  # records with products keep the old form
        assert info["n_lin_records"] < info["n_gate_records"]
    for B in SIZES:
        values = bytearray(synth.witness_batch(B, n_in=n_in, seed=seed, edge_cases=True))
        if planted is not None:
            off = ((B - 1) * n_in + planted - 1) * 32
            values[off:off + 32] = bytes(32)
        values = bytes(values)
        ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values, B)
        solved = [j for j in range(B) if ores[j].as_tuple()[0] == 0]
        maps = []
        for lin_table in (0, 1):
            with acvm_amd.tuning(lin_table=lin_table, **mode):
                batch = acvm_amd.Batch(gc, B, ids, **opts)
                batch.set_initial_witness(values)
                batch.solve()
                gres = batch.results()
                if opts.get("reuse_slots"):  # recycled rows: the map leaves as its digest (folded into the solve) and the kept witnesses
                    # (an instance that failed has no kept witness to hand out)
                    dig, kept = batch.digest(), [batch.extract(opts["keep"], j, 1) for j in solved]
                else:
                    gasg, gvals = batch.witness_map()
                st = batch.stats()
                batch.free()
            for j in range(B):
                assert gres[j].as_tuple() == ores[j].as_tuple(), (name, B, lin_table, j, gres[j].as_tuple(), ores[j].as_tuple())
            if opts.get("reuse_slots"):
                assert solved or B == 1
                for j in solved:
                    assert bytes(dig[j]) == oracle.witness_map_digest(oasg[j], ovals[j]), (name, B, lin_table, j)
                maps.append((np.asarray(dig).tobytes(), b"".join(np.asarray(k).tobytes() for k in kept)))
            else:
                nw = min(oasg.shape[1], gasg.shape[1])
                assert np.array_equal(oasg[:, :nw], gasg[:, :nw]), (name, B, lin_table, "assigned sets differ")
                assert np.array_equal(ovals[:, :nw], gvals[:, :nw]), (name, B, lin_table, "witness values differ")
                maps.append((gasg.tobytes(), gvals.tobytes()))
            if planted is not None:
                assert st["n_slow_instances"] >= 1  # the planted zero denominator left the generic path
        assert maps[0] == maps[1], (name, B, "the canonical witness maps with and without tables differ")


def test_lin_add_on_the_device_against_integers():
    import acvm_amd
    n_terms, coef_w, row_w, hs, coefs, rows = ref.cases(1 << 12)
    tables, out = acvm_amd.debug_lin_add(n_terms, coef_w, row_w, hs)
    ref.check_tables(n_terms, coefs, tables)
    ref.check_results(n_terms, coefs, rows, hs, out)


def test_lin_add_partial_last_wave():
    # 64 + 5 items: the last wave has 59 lanes predicated off
    import acvm_amd
    n_terms, coef_w, row_w, hs, coefs, rows = ref.cases(69, seed=4)
    tables, out = acvm_amd.debug_lin_add(n_terms, coef_w, row_w, hs)
    ref.check_results(n_terms, coefs, rows, hs, out)
