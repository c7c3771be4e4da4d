"""Bundles on the device (tuning keys share, max_bundle; acvm_amd/csrc/gate_record.hpp "bundles"): whole solves in which the gate kernel runs several
wave programs per wave and serves their common operand row from the copy it fetched once. Every case: results, assigned sets and witness maps
bit for bit against the oracle AND against the same circuit solved with share = 0, at 1, 65 and 257 instances (a partial wave, a second wave, a
partial block of 256). The plans are looked at first (tests/bundle_cases.py), so that each case is known to reach what it is there for."""
import numpy as np
import pytest

import bundle_cases as bc

pytestmark = pytest.mark.gpu

SIZES = (1, 65, 257)


def three_gates_circuit():
    """one level of three gates that share w1 as the first factor, the second factor and both"""
    from acvm_amd.acir import P, Circuit, Expression as E
    ops = [E([(1, 1, 2)], [(P - 1, 5)], 3), E([(1, 3, 1)], [(P - 1, 6)], 0), E([(1, 1, 1)], [(P - 1, 7)], 1)]
    return Circuit(current_witness_index=7, opcodes=ops, private_parameters=[1, 2, 3, 4], return_values=[5, 6, 7]), [1, 2, 3, 4]


def failing_assert_circuit():
    """w4 = w1 w2 is asserted beside gates that share w1 with the assertion (one level); the inputs make it hold except where the test breaks w4"""
    from acvm_amd.acir import P, Circuit, Expression as E
    ops = [
        E([(1, 1, 3)], [(P - 1, 5)], 0),          # w5 = w1 w3
        E([(1, 1, 2)], [(P - 1, 4)], 0),          # assert w1 w2 - w4 = 0
        E([], [(3, 1), (1, 3), (P - 1, 6)], 0),   # w6 = 3 w1 + w3
        E([(1, 1, 1)], [(P - 1, 7)], 0),          # w7 = w1^2
        E([(1, 5, 6)], [(1, 7), (P - 1, 8)], 0),  # w8 = w5 w6 + w7
    ]
    return Circuit(current_witness_index=8, opcodes=ops, private_parameters=[1, 2, 3, 4], return_values=[8]), [1, 2, 3, 4]


def build(name):
    """(circuit, ids, n_in, handle options, tuning, edit(rows of input integers) or None, places the plan must reach)"""
    from acvm_amd import synth
    from acvm_amd.acir import P
    if name in ("hot_inputs", "hot_inputs_cap2", "hot_inputs_cap8", "hot_inputs_reuse"):
        mode = {"hot_inputs_cap2": {"max_bundle": 2}, "hot_inputs_cap8": {"max_bundle": 8}}.get(name, {})
        return synth.arithmetic_circuit(300, hot_inputs=True) + (16, {"reuse_slots": True} if name == "hot_inputs_reuse" else {}, mode, None, set())
    if name == "three_gates":
        return three_gates_circuit() + (4, {}, {}, None, {"product_first", "product_second", "square"})
    if name in ("positions", "positions_cap2", "positions_cap8"):
        # the tail that reads the shared row beside the forwarded value, the SOLVE_DYN members, and in the last instance a zero denominator
        def zero_denominator(rows):
            rows[-1][1] = 0
        mode = {"positions_cap2": {"max_bundle": 2}, "positions_cap8": {"max_bundle": 8}}.get(name, {})
        return bc.shared_positions_circuit() + (4, {}, mode, zero_denominator, {"product_first", "product_second", "square", "linear", "beside_local", "solve_dyn", "assert"})
    if name == "failing_assert":
        def satisfy_but_one(rows):
            for r in rows:
                r[3] = r[0] * r[1] % P
            rows[len(rows) // 2][3] = (rows[len(rows) // 2][3] + 1) % P
        return failing_assert_circuit() + (4, {}, {}, satisfy_but_one, {"assert"})
    if name == "mixed_light":
        return synth.mixed_circuit(290, seed=0xAC1D0711, heavy=False, blocks=4, cells=16) + (16, {}, {}, None, set())
    raise KeyError(name)


CASES = ("hot_inputs", "hot_inputs_cap2", "hot_inputs_cap8", "hot_inputs_reuse", "three_gates", "positions", "positions_cap2", "positions_cap8", "failing_assert",
         "mixed_light")


@pytest.mark.parametrize("name", CASES)
def test_whole_solves_with_and_without_bundles(oracle, name):
    import acvm_amd
    from acvm_amd import synth
    from acvm_amd.acir import P
    circ, ids, n_in, opts, mode, edit, places = build(name)
    assert len(circ.opcodes) <= 300
    data = circ.to_bytes()
    gc = acvm_amd.Circuit(data)
    if opts.get("reuse_slots"):
        opts = dict(opts, keep=gc.witness_set("return_values"))
    with acvm_amd.tuning(**mode):
        records, plan = gc.gate_records(ids, **opts), gc.bundle_plan(ids, **opts)
    cap = mode.get("max_bundle", acvm_amd.tuning_get("max_bundle"))
    n_shared, _ = bc.check_bundle_plan(records, plan, cap)
    assert n_shared >= 1 and plan["n_findings"] == 0
    assert places <= bc.shared_operand_places(records, plan)
    if name.startswith("hot_inputs"):
        assert max(len(b) for launch in plan["launches"] for b, _ in launch) == cap
    if name == "mixed_light":  # gates and light records in one launch: kernels_ops.hip arith_light_level_kernel
        assert gc.plan_stats(ids)["n_other_records"] > 0
    for B in SIZES:
        values = synth.witness_batch(B, n_in=n_in, seed=11, edge_cases=True)
        if edit is not None:
            rows = [[int.from_bytes(values[(j * n_in + k) * 32:(j * n_in + k + 1) * 32], "big") % P for k in range(n_in)] for j in range(B)]
            edit(rows)
            values = synth.values_from_rows(rows)
        ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(data), ids, values, B)
        solved = [j for j in range(B) if ores[j].as_tuple()[0] == 0]
        if name == "failing_assert":
            assert [j for j in range(B) if j not in solved] == [B // 2]
        maps, slow = [], []
        for share in (0, 1):
            with acvm_amd.tuning(share=share, **mode):
                batch = acvm_amd.Batch(gc, B, ids, **opts)
                batch.set_initial_witness(values)
                batch.solve()
                gres = batch.results()
                if opts.get("reuse_slots"):  # recycled rows: the map leaves as its digest (folded into the solve) and the kept witnesses
                    dig, kept = batch.digest(), [batch.extract(opts["keep"], j, 1) for j in solved]
                else:
                    gasg, gvals = batch.witness_map()
                slow.append(batch.stats()["n_slow_instances"])
                batch.free()
            for j in range(B):
                assert gres[j].as_tuple() == ores[j].as_tuple(), (name, B, share, j, gres[j].as_tuple(), ores[j].as_tuple())
            if opts.get("reuse_slots"):
                for j in solved:
                    assert bytes(dig[j]) == oracle.witness_map_digest(oasg[j], ovals[j]), (name, B, share, j)
                maps.append((np.asarray(dig).tobytes(), b"".join(np.asarray(k).tobytes() for k in kept)))
            else:
                nw = min(oasg.shape[1], gasg.shape[1])
                assert np.array_equal(oasg[:, :nw], gasg[:, :nw]), (name, B, share, "assigned sets differ")
                assert np.array_equal(ovals[:, :nw], gvals[:, :nw]), (name, B, share, "witness values differ")
                maps.append((gasg.tobytes(), gvals.tobytes()))
        assert maps[0] == maps[1], (name, B, "the witness maps with and without bundles differ")
        assert slow[0] == slow[1], (name, B, "the same instances leave the generic path either way")  # (the event words: one flag per failing instance)
        if name in ("positions", "failing_assert"):
            assert slow[1] >= 1
