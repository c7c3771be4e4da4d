"""Circuits and checks shared by the bundle tests (tests/test_bundles_on_host.py, tests/test_gpu_bundles.py): hand-written levels whose gates share an
operand row in every position a record has, and the promises of the planner's bundle pass recomputed from the decoded records
(acvm_amd.Circuit.gate_records, .bundle_plan; acvm_amd/csrc/gate_record.hpp "bundles")."""
from acvm_amd.acir import P, Circuit, Expression as E

LOCAL = 0xFFFFFFFF
N_IN = 4


def shared_positions_circuit():
    """One level of gates that all read w1: as the first factor of a product, as the second, as both (a square), in a linear term with a coefficient
    and with +-1, in a host whose fused tail reads w1 again beside the forwarded value, in the numerator of a gate whose unknown is multiplied by a
    known witness (SOLVE_DYN; w2 is the denominator: an instance with w2 = 0 leaves the generic path), and in an ASSERT gate (w1 w2 - w2 w1 = 0:
    holds for every input). Returns (Circuit, ids)."""
    ops = [
        E([(1, 1, 2)], [(P - 1, 5)], 3),                    # w5 = w1 w2 + 3
        E([(1, 3, 1)], [(P - 1, 6)], 0),                    # w6 = w3 w1
        E([(1, 1, 1)], [(P - 1, 7)], 1),                    # w7 = w1^2 + 1
        E([(7, 1, 4)], [(5, 3), (P - 1, 8)], 0),            # w8 = 7 w1 w4 + 5 w3
        E([(9, 4, 1)], [(P - 1, 9)], 2),                    # w9 = 9 w4 w1 + 2
        E([], [(5, 1), (1, 2), (P - 1, 10)], 0),            # w10 = 5 w1 + w2
        E([], [(1, 1), (P - 1, 3), (P - 1, 11)], 4),        # w11 = w1 - w3 + 4
        E([], [(P - 1, 1), (1, 4), (P - 1, 12)], 0),        # w12 = w4 - w1
        E([(1, 1, 3)], [(1, 4), (P - 1, 13)], 0),           # w13 = w1 w3 + w4          (a host ...
        E([(1, 13, 1)], [(P - 1, 14)], 7),                  # w14 = w13 w1 + 7          ... and its tail: the forwarded value times the shared row)
        E([(3, 13, 14)], [(2, 1), (P - 1, 15)], 0),         # w15 = 3 w13 w14 + 2 w1
        E([(1, 2, 16)], [(1, 1), (6, 3)], 0),               # w2 w16 + w1 + 6 w3 = 0: w16 = -(w1 + 6 w3) / w2
        E([(1, 2, 17), (1, 1, 1)], [(1, 4)], 0),            # w2 w17 + w1^2 + w4 = 0
        E([(1, 1, 2), (P - 1, 2, 1)], [], 0),               # assert w1 w2 - w2 w1 = 0
        E([(1, 5, 6)], [(1, 7), (P - 1, 18)], 0),           # a second level that reads the first
        E([(1, 16, 17)], [(1, 15), (P - 1, 19)], 0),
    ]
    circ = Circuit(current_witness_index=19, opcodes=ops, private_parameters=list(range(1, N_IN + 1)), return_values=[18, 19])
    return circ, list(range(1, N_IN + 1))


def shared_positions_values(circ, inputs):
    """the witness map of shared_positions_circuit for one instance in Python integers: {witness: value}, or None where w2 = 0"""
    w = {i + 1: v % P for i, v in enumerate(inputs)}
    if w[2] == 0:
        return None
    inv2 = pow(w[2], P - 2, P)
    w[5] = (w[1] * w[2] + 3) % P
    w[6] = w[3] * w[1] % P
    w[7] = (w[1] * w[1] + 1) % P
    w[8] = (7 * w[1] * w[4] + 5 * w[3]) % P
    w[9] = (9 * w[4] * w[1] + 2) % P
    w[10] = (5 * w[1] + w[2]) % P
    w[11] = (w[1] - w[3] + 4) % P
    w[12] = (w[4] - w[1]) % P
    w[13] = (w[1] * w[3] + w[4]) % P
    w[14] = (w[13] * w[1] + 7) % P
    w[15] = (3 * w[13] * w[14] + 2 * w[1]) % P
    w[16] = -(w[1] + 6 * w[3]) * inv2 % P
    w[17] = -(w[1] * w[1] + w[4]) * inv2 % P
    w[18] = (w[5] * w[6] + w[7]) % P
    w[19] = (w[16] * w[17] + w[15]) % P
    return w


def programs_of(records):
    """gate records (Circuit.gate_records) -> per wave program: {"records": [...], "reads": rows its records name as operands (not the forwarded value),
    "writes": rows its records store}"""
    progs = {}
    for r in records:
        p = progs.setdefault(r["program"], {"records": [], "reads": set(), "writes": set()})
        p["records"].append(r)
        p["reads"].update(x for x in r["operands"] if x != LOCAL)
        if r["kind"] != "ASSERT":
            p["writes"].add(r["out"])
    return progs


def check_bundle_plan(records, plan, cap):
    """The promises of plan.cpp check_bundles, recomputed: the bundles of the launches name every wave program exactly once, launch by launch a
    contiguous range of the level-major list; a bundle with a shared row has at least two programs that read the row as an operand; no record of
    such a bundle writes the row; a bundle without a row is one program; no bundle has more than `cap`. Returns (bundles with a row, row loads
    per instance they save)."""
    progs = programs_of(records)
    nxt, n_shared, saved = 0, 0, 0
    for launch in plan["launches"]:
        members = sorted(q for bundle, _ in launch for q in bundle)
        assert members == list(range(nxt, nxt + len(members))), "a launch's bundles are not a partition of its wave programs"
        nxt += len(members)
        for bundle, row in launch:
            assert 1 <= len(bundle) <= max(cap, 1)
            if row is None:
                assert len(bundle) == 1
                continue
            assert sum(row in progs[q]["reads"] for q in bundle) >= 2, (bundle, row)
            assert all(row not in progs[q]["writes"] for q in bundle), (bundle, row)
            n_shared += 1
            saved += sum(r["operands"].count(row) for q in bundle for r in progs[q]["records"]) - 1
    assert nxt == len(progs)
    assert plan["n_shared_bundles"] == n_shared and plan["n_shared_loads_saved"] == saved
    return n_shared, saved


def shared_operand_places(records, plan):
    """where the bundles' shared rows stand in the records that name them: a set of "product_first", "product_second", "square", "linear",
    "beside_local" (a record behind the head of its wave program that names the row and the forwarded value), "solve_dyn", "assert" """
    progs = programs_of(records)
    places = set()
    for launch in plan["launches"]:
        for bundle, row in launch:
            if row is None:
                continue
            for q in bundle:
                for r in progs[q]["records"]:
                    ops = r["operands"]
                    if row not in ops:
                        continue
                    n_pairs = r["np_mac"]
                    pairs = [(ops[2 * i], ops[2 * i + 1]) for i in range(n_pairs)]
                    at = 2 * n_pairs + r["nl_mac"]
                    linear = ops[2 * n_pairs:at]
                    pairs += [(ops[at + 2 * i], ops[at + 2 * i + 1]) for i in range(r["np_pos"] + r["np_neg"])]
                    linear += ops[at + 2 * (r["np_pos"] + r["np_neg"]):]
                    for a, b in pairs:
                        if a == row and b == row:
                            places.add("square")
                        elif a == row:
                            places.add("product_first")
                        elif b == row:
                            places.add("product_second")
                    if row in linear:
                        places.add("linear")
                    if r["position"] > 0 and LOCAL in ops:
                        places.add("beside_local")
                    if r["kind"] == "SOLVE_DYN":
                        places.add("solve_dyn")
                    if r["kind"] == "ASSERT":
                        places.add("assert")
    return places
