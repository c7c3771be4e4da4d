"""One handle driven through the call sequences the ABI documents (include/acvm_amd.h: stepping, acvm_batch_reset, acvm_batch_set_instances,
acvm_batch_solve_then_import, the exact-only mode) and then solved: whatever ran on the handle before, the final solve must leave exactly what a
FRESH handle given the same inputs leaves, and what the CPU oracle computes -- results and messages, the number of instances on the exact path,
the whole witness map, the return witnesses, one device export and (where the handle folds it) the digest.

The circuit is the one of test_gpu_parity.test_projective_witnesses_hand_over: scaled columns (exported through 1 / scale unless the instance took
the exact path), every 5th instance failing a constraint in mid-circuit and one instance whose scaled denominator vanishes. Both kinds of lane are
present on every compared solve (0 < n_slow_instances < B), so that an event word that is stale in either direction shows: a failing instance
reported Solved, or a scaled column leaving the device without 1 / scale. (The import leaves the event words ready for the level solve behind it,
which then skips its reset launch: batch.hpp events_fresh. Sequences 1, 2, 3 and 6 are the ones in which something else wrote those words in
between.)"""
import functools

import numpy as np
import pytest

import acvm_amd
from acvm_amd.acir import BlackBoxFuncCall as BB, Circuit, Expression as E, FunctionInput as FI, P

pytestmark = pytest.mark.gpu
IDS = [1, 2, 9]
RET = [10]
N_OPCODES = 9


@functools.lru_cache(maxsize=None)
def _circuit_bytes():
    ops = [
        E([(5, 1, 2)], [(P - 1, 3)], 11),                  # w3 = 5 w1 w2 + 11                (scaled)
        E([(7, 3, 1)], [(3, 2), (P - 9, 4)], 0),           # 9 w4 = 7 w3 w1 + 3 w2            (scaled, reads a scaled witness)
        E([(2, 4, 5)], [(13, 3)], 1),                      # 2 w4 w5 + 13 w3 + 1 = 0          (inversion gate, scaled denominator)
        E([], [(1, 5), (P - 1, 6)], 0),                    # w6 = w5                          (read by RANGE below: pinned)
        BB("RANGE", {"input": FI(6, 254)}),
        E([(3, 5, 6)], [(P - 1, 7)], 0),                   # w7 = 3 w5 w6
        E([(1, 7, 7)], [(P - 4, 8)], 5),                   # 4 w8 = w7^2 + 5
        E([], [(6, 8), (P - 6, 9)], 0),                    # constraint on scaled witnesses: fails unless w9 == w8
        E([(11, 8, 3)], [(P - 1, 10)], 0),                 # after the failing opcode: the return witness
    ]
    assert len(ops) == N_OPCODES
    return Circuit(10, ops, private_parameters=list(IDS), return_values=list(RET)).to_bytes()


_CASES = {}


def _case(oracle, B, clean=False, seed=7):
    """(values, oracle results, oracle assigned, oracle values) of B instances, computed once per shape and shared (read only). Not clean: every 5th
    instance fails opcode 7, instance 6 has a vanishing denominator at opcode 2; clean: every instance is Solved on the generic path."""
    key = (B, clean, seed)
    if key not in _CASES:
        oc = oracle.Circuit(_circuit_bytes())
        rng = np.random.default_rng(seed + B)
        rows = [[int.from_bytes(rng.bytes(31), "big") for _ in range(2)] for _ in range(B)]
        rows[3] = [0, 5]
        rows[4] = [1, 0]
        if not clean:
            rows[6] = [1, (-77 * pow(38, -1, P)) % P]
        probe = b"".join(b"".join(v.to_bytes(32, "big") for v in r + [0]) for r in rows)
        _, _, pvals = oracle.solve_batch(oc, IDS, probe, B)
        w8 = [int.from_bytes(bytes(pvals[j, 8]), "big") for j in range(B)]
        values = b"".join(b"".join(v.to_bytes(32, "big") for v in rows[j] + [w8[j] if (clean or j % 5) else (w8[j] + 1) % P]) for j in range(B))
        ores, oasg, ovals = oracle.solve_batch(oc, IDS, values, B)
        ovals[oasg == 0] = 0
        n_fail = sum(1 for r in ores if r.status != 0)
        assert n_fail == (0 if clean else len(range(0, B, 5)) + 1)
        _CASES[key] = (values, ores, oasg, ovals)
    return _CASES[key]


def _runs(flags):
    """maximal runs [first, first + n) of set flags"""
    out, j = [], 0
    while j < len(flags):
        if flags[j]:
            k = j
            while k < len(flags) and flags[k]:
                k += 1
            out.append((j, k - j))
            j = k
        else:
            j += 1
    return out


def _state(batch, solved, whole_map=True, digest=False, keep=()):
    """everything a caller can read of a solved handle"""
    B = batch.B
    res = batch.results()
    st = {"results": [r.as_tuple() for r in res], "messages": [r.message for r in res], "n_slow": batch.stats()["n_slow_instances"]}
    st["extract"] = [(first, batch.extract(RET, first, n).tobytes()) for first, n in _runs(solved)]
    if whole_map:
        asg, vals = batch.witness_map()
        st["assigned"], st["values"] = asg, vals
        d = acvm_amd.DeviceBuffer(size=B * batch.nw * 32)
        try:
            batch.export_device(d.ptr, encoding=acvm_amd.ENC_BE32, layout=acvm_amd.LAYOUT_INSTANCE_MAJOR)
            st["export"] = d.download()
        finally:
            d.free()
    else:
        st["kept"] = [tuple(x.tobytes() for x in batch.witness(w)) for w in keep]
    if digest:
        st["digest"] = batch.digest()
    return st


def _assert_final(oracle, batch, B, clean=False, both_kinds=True, **opts):
    """the handle (just solved, inputs = _case(B, clean)) against a fresh handle of the same options and against the oracle"""
    values, ores, oasg, ovals = _case(oracle, B, clean)
    solved = [r.status == 0 for r in ores]
    whole_map = not opts.get("reuse_slots")
    digest = bool(opts.get("fold_digest") or opts.get("reuse_slots"))
    keep = opts.get("keep", ())
    got = _state(batch, solved, whole_map, digest, keep)
    fresh = acvm_amd.Batch(batch.circuit, B, IDS, **opts)
    fresh.set_initial_witness(values)
    fresh.solve()
    want = _state(fresh, solved, whole_map, digest, keep)
    fresh.free()
    # the oracle first: it says which of the two handles is wrong, should they differ
    for name, st in (("fresh handle", want), ("handle under test", got)):
        bad = [j for j in range(B) if st["results"][j] != ores[j].as_tuple() or st["messages"][j] != ores[j].message]
        assert not bad, f"{name}: result of instance {bad[0]} is {st['results'][bad[0]]}, the oracle's {ores[bad[0]].as_tuple()} ({len(bad)} differ)"
        if both_kinds:
            assert 0 < st["n_slow"] < B, f"{name}: {st['n_slow']} of {B} instances on the exact path"
            assert st["n_slow"] >= sum(1 for s in solved if not s)
        else:
            assert st["n_slow"] == 0
        for first, raw in st["extract"]:
            n = len(raw) // (32 * len(RET))
            assert raw == ovals[first:first + n][:, RET].tobytes(), f"{name}: return witnesses of instances [{first}, {first + n})"
        if whole_map:
            nw = min(oasg.shape[1], st["assigned"].shape[1])
            assert np.array_equal(st["assigned"][:, :nw], oasg[:, :nw]), f"{name}: assigned sets differ"
            bad = np.argwhere((st["values"][:, :nw] != ovals[:, :nw]).any(axis=2))
            assert bad.size == 0, f"{name}: witness {bad[0][1]} of instance {bad[0][0]} differs from the oracle's ({len(bad)} differ)"
            exp = np.frombuffer(st["export"], dtype=np.uint8).reshape(B, -1, 32)
            assert np.array_equal(exp[:, :nw], ovals[:, :nw]) and not exp[:, nw:].any(), f"{name}: device export differs"
        else:
            for w, (vals, asg) in zip(keep, st["kept"]):
                a = np.frombuffer(asg, dtype=np.uint8).astype(bool)
                v = np.frombuffer(vals, dtype=np.uint8).reshape(B, 32)
                assert np.array_equal(a, oasg[:, w].astype(bool)) and np.array_equal(v[a], ovals[:, w][a]), f"{name}: kept witness {w}"
        if digest:
            bad = [j for j in range(B) if bytes(st["digest"][j]) != oracle.witness_map_digest(oasg[j], ovals[j])]
            assert not bad, f"{name}: digest of instance {bad[0]} ({len(bad)} differ)"
    # and bit for bit against each other
    assert got["results"] == want["results"] and got["messages"] == want["messages"]
    assert got["n_slow"] == want["n_slow"]
    assert got["extract"] == want["extract"]
    if whole_map:
        assert np.array_equal(got["assigned"], want["assigned"]) and np.array_equal(got["values"], want["values"])
        assert got["export"] == want["export"]
    else:
        assert got["kept"] == want["kept"]
    if digest:
        assert np.array_equal(got["digest"], want["digest"])


def _handle(B, **opts):
    gc = acvm_amd.Circuit(_circuit_bytes())
    batch = acvm_amd.Batch(gc, B, IDS, **opts)
    if not opts:
        assert batch.stats()["n_scaled_witnesses"] >= 4
    return batch


@pytest.mark.parametrize("B", [70, 130])
@pytest.mark.parametrize("k", [1, 5, N_OPCODES])
def test_steps_then_reset_then_solve(oracle, B, k):
    """sequence 1: import -> solve_opcode x k -> reset -> solve. The steps run every instance on the exact kernels; reset goes "back to the state
    right after set_initial_witness", so the solve is a level solve of the same inputs."""
    values = _case(oracle, B)[0]
    batch = _handle(B)
    batch.set_initial_witness(values)
    for _ in range(k):
        batch.solve_opcode()
    batch.reset()
    batch.solve()
    _assert_final(oracle, batch, B)
    batch.free()


@pytest.mark.parametrize("B", [70, 130])
def test_steps_finished_by_solve_then_reset_then_solve(oracle, B):
    """sequence 2: import -> solve_opcode x 3 -> solve (the stepping path runs the rest) -> reset -> solve"""
    values = _case(oracle, B)[0]
    batch = _handle(B)
    batch.set_initial_witness(values)
    for _ in range(3):
        batch.solve_opcode()
    n_fail = len(range(0, B, 5)) + 1
    assert batch.solve() == n_fail
    assert batch.stats()["n_slow_instances"] == B  # (every instance was an exact lane)
    batch.reset()
    assert batch.solve() == n_fail
    _assert_final(oracle, batch, B)
    batch.free()


@pytest.mark.parametrize("B", [70, 130])
def test_step_reset_then_pipelined_solve_holds_the_import_back(oracle, B):
    """sequence 3: import -> solve_opcode -> reset -> solve(then_import=next) -> set_initial_witness_device(next) -> solve, next = clean inputs.
    The first solve has failing instances: it returns their count and holds the import of `next` back (the exact path needs this tile's rows), so
    its whole state can still be read and is compared here, both kinds of lane present; set_initial_witness_device then performs the import, and
    the solve of the clean inputs (nobody on the exact path, by construction of `next`) is compared as well."""
    values = _case(oracle, B)[0]
    nxt = acvm_amd.DeviceBuffer(_case(oracle, B, clean=True)[0])
    batch = _handle(B)
    batch.set_initial_witness(values)
    batch.solve_opcode()
    batch.reset()
    n_fail = len(range(0, B, 5)) + 1
    assert batch.solve(then_import=nxt.ptr) == n_fail and batch.stats()["n_slow_instances"] >= n_fail
    _assert_final(oracle, batch, B)
    batch.set_initial_witness_device(nxt.ptr)
    assert batch.solve() == 0
    _assert_final(oracle, batch, B, clean=True, both_kinds=False)
    batch.free()
    nxt.free()


@pytest.mark.parametrize("B", [70, 130])
def test_exact_only_solve_then_reset_then_level_solve(oracle, B):
    """sequence 4: import -> set_force_slow_path(True) -> solve -> reset -> set_force_slow_path(False) -> solve, no second import"""
    values = _case(oracle, B)[0]
    batch = _handle(B)
    batch.set_initial_witness(values)
    batch.set_force_slow_path(True)
    batch.solve()
    assert batch.stats()["n_slow_instances"] == B
    batch.reset()
    batch.set_force_slow_path(False)
    batch.solve()
    _assert_final(oracle, batch, B)
    batch.free()


def test_live_count_changes_between_a_step_and_the_solves(oracle):
    """sequence 5, one handle of capacity 300: set_instances(300) -> import -> solve_opcode -> set_instances(70) -> import -> solve ->
    set_instances(300) -> import -> solve. The solve of 70 runs over event words of which [70, 300) still hold what the step left there."""
    batch = _handle(300)
    batch.set_instances(300)
    batch.set_initial_witness(_case(oracle, 300)[0])
    batch.solve_opcode()
    batch.set_instances(70)
    batch.set_initial_witness(_case(oracle, 70)[0])
    batch.solve()
    _assert_final(oracle, batch, 70)
    batch.set_instances(300)
    batch.set_initial_witness(_case(oracle, 300)[0])
    batch.solve()
    _assert_final(oracle, batch, 300)
    batch.free()


@pytest.mark.parametrize("B", [70, 130])
def test_steps_reset_solve_with_a_folded_digest(oracle, B):
    """sequence 6, fold_digest: import -> solve_opcode x 5 -> reset -> solve; the digest summed during the solve takes the exact lanes' part from
    their own table, which it finds through the same event words"""
    values = _case(oracle, B)[0]
    batch = _handle(B, fold_digest=True)
    batch.set_initial_witness(values)
    for _ in range(5):
        batch.solve_opcode()
    batch.reset()
    batch.solve()
    _assert_final(oracle, batch, B, fold_digest=True)
    batch.free()


@pytest.mark.parametrize("B", [70, 130])
def test_reset_solve_with_recycled_rows(oracle, B):
    """sequence 6, reuse_slots: a handle that recycles rows has no table to step in -- acvm_batch_solve_opcode refuses (asserted) and leaves the
    handle as the import left it; reset -> solve must then give what a fresh handle gives"""
    values = _case(oracle, B)[0]
    opts = dict(reuse_slots=True, keep=tuple(RET + [3]))
    try:
        batch = _handle(B, **opts)
    except acvm_amd.AcvmError as e:
        pytest.skip(f"planner refuses this mode for the circuit: {e}")
    batch.set_initial_witness(values)
    with pytest.raises(acvm_amd.AcvmError, match="stepping needs the full witness table"):
        batch.solve_opcode()
    batch.reset()
    batch.solve()
    _assert_final(oracle, batch, B, **opts)
    batch.free()
