"""Every host read of a solved handle against the CPU oracle and against the other reads: they share one staging function, one view of the table
being read and one assigned set (batch_export.cpp read_witnesses, batch_internal.hpp level_table / side_table, assigned_view.hpp). Circuit and
cases are those of test_gpu_handle_sequences: scaled columns, every 5th instance failing opcode 7 (it lacks witness 10), instance 6 failing opcode
2 (it lacks 5 .. 8 and 10), so that exact lanes and level lanes sit on both sides of a 64-lane boundary and 5, 6 are a run of two exact lanes."""
import re

import numpy as np
import pytest

import acvm_amd
from acvm_amd.acir import P
from test_gpu_handle_sequences import IDS, RET, _case, _circuit_bytes, _handle, _runs

pytestmark = pytest.mark.gpu
SIZES = [70, 130]
NOT_FOUND = "Failed to extract witness %d from witness map. Witness not found. (instance %d)"
GONE = "the initial witnesses of this solve are gone: acvm_batch_solve_then_import put the next tile's inputs into the table behind the solve"


def _solved(B, values, **opts):
    batch = _handle(B, **opts)
    batch.set_initial_witness(values)
    batch.solve()
    return batch


def _has(oasg, j, w):
    return w < oasg.shape[1] and bool(oasg[j, w])


def _refusal(oasg, first, n, listed):
    """the text of the extraction's refusal by the oracle's assigned sets: the lowest instance that lacks a listed witness, then its first in list order"""
    for j in range(first, first + n):
        for w in listed:
            if not _has(oasg, j, w):
                return NOT_FOUND % (w, j)
    return None


def _extract_runs(batch, oasg, ovals, B, listed):
    """extract over every maximal run of instances that have all listed witnesses, against the oracle; returns the runs"""
    runs = _runs([all(_has(oasg, j, w) for w in listed) for j in range(B)])
    for first, n in runs:
        assert np.array_equal(batch.extract(listed, first, n), ovals[first:first + n][:, listed]), (listed, first, n)
    return runs


@pytest.mark.parametrize("B", SIZES)
def test_reads_of_a_plain_handle_agree_with_the_oracle_and_each_other(oracle, B):
    values, ores, oasg, ovals = _case(oracle, B)
    batch = _solved(B, values)
    nw = batch.nw
    assert nw <= oasg.shape[1] and 0 < batch.stats()["n_slow_instances"] < B
    asg, vals = batch.witness_map()
    assert np.array_equal(asg, oasg[:, :nw]) and np.array_equal(vals, ovals[:, :nw])
    for w in range(nw + 1):  # (one beyond the last: zeros, unassigned)
        v, a = batch.witness(w)
        assert np.array_equal(a, asg[:, w] if w < nw else np.zeros(B, np.uint8)) and np.array_equal(v, vals[:, w] if w < nw else np.zeros((B, 32), np.uint8)), w
    # a range that starts inside the run of exact lanes 5, 6 and ends on the exact lane 10; the run itself; one lane
    assert all(ores[j].status != 0 for j in (5, 6, 10))
    for first, n in ((6, 5), (5, 2), (6, 1), (0, B), (B - 1, 1)):
        a, v = batch.witness_map(first, n)
        assert np.array_equal(a, asg[first:first + n]) and np.array_equal(v, vals[first:first + n]), (first, n)
    runs = _extract_runs(batch, oasg, ovals, B, RET)
    assert len(runs) > 2
    runs = _extract_runs(batch, oasg, ovals, B, [3, 1, 3, 9])  # (every instance has these: one run with the exact lanes in it, a repeated witness)
    assert runs == [(0, B)]
    d = acvm_amd.DeviceBuffer(size=B * nw * 32)
    try:
        batch.export_device(d.ptr, encoding=acvm_amd.ENC_BE32, layout=acvm_amd.LAYOUT_INSTANCE_MAJOR)
        assert np.array_equal(np.frombuffer(d.download(), dtype=np.uint8).reshape(B, nw, 32), vals)
    finally:
        d.free()
    batch.free()


@pytest.mark.parametrize("B", SIZES)
def test_extract_names_the_lowest_instance_and_its_first_missing_witness(oracle, B):
    values, ores, oasg, ovals = _case(oracle, B)
    batch = _solved(B, values)
    # (i) witness 0 is produced by nothing: missing for everybody, level lanes and exact lanes alike
    assert not oasg[:, 0].any()
    # (ii) [5, 10] over [5, 8): instance 5 lacks 10 only, instance 6 lacks 5 as well -- a scan by witness would name 5 and instance 6
    assert oasg[5, 5] and not oasg[5, 10] and not oasg[6, 5] and not oasg[6, 10]
    cases = [([1, 0, 10], 0, B), ([10, 0], 1, 3), ([0], 6, 1), ([5, 10], 5, 3), ([10, 5], 5, 3), ([5, 10], 6, 2), ([5, 10], 1, B - 1), ([8, 3, 10, 5], 1, 9)]
    for listed, first, n in cases:
        want = _refusal(oasg, first, n, listed)
        assert want is not None
        with pytest.raises(acvm_amd.AcvmError, match=re.escape(want)):
            batch.extract(listed, first, n)
    assert _refusal(oasg, 5, 3, [5, 10]) == NOT_FOUND % (10, 5)
    assert _refusal(oasg, 1, B - 1, [5, 10]) == NOT_FOUND % (10, 5)
    with pytest.raises(acvm_amd.AcvmError, match=re.escape(NOT_FOUND % (batch.nw, 3))):  # (beyond the map: named before anything is looked up)
        batch.extract([0, batch.nw], 3, 2)
    batch.free()


@pytest.mark.parametrize("B", SIZES)
def test_reads_with_recycled_rows(oracle, B):
    """reuse_slots: kept and initial witnesses come from the level table through the row map, those of the exact lanes from the side table"""
    values, ores, oasg, ovals = _case(oracle, B)
    keep = (RET[0], 3)
    batch = _solved(B, values, reuse_slots=True, keep=keep)
    assert 0 < batch.stats()["n_slow_instances"] < B
    for w in list(keep) + IDS:
        v, a = batch.witness(w)
        assert np.array_equal(a, oasg[:, w]) and np.array_equal(v, ovals[:, w]), w
    assert len(_extract_runs(batch, oasg, ovals, B, RET)) > 2
    assert _extract_runs(batch, oasg, ovals, B, [3, 9, 1, 2, 3]) == [(0, B)]
    assert np.array_equal(batch.extract([3, 2], 5, 2), ovals[5:7][:, [3, 2]])  # (exact lanes only)
    with pytest.raises(acvm_amd.AcvmError, match=re.escape(NOT_FOUND % (10, 5))):
        batch.extract([3, 10], 5, 3)
    text = re.escape("witness 4 was not kept: the batch recycles witness rows (ACVM_BATCH_REUSE_SLOTS); only the initial witnesses and keep_ids can be read back")
    with pytest.raises(acvm_amd.AcvmError, match=text):
        batch.witness(4)
    with pytest.raises(acvm_amd.AcvmError, match=text):
        batch.extract([3, 4], 1, 3)
    with pytest.raises(acvm_amd.AcvmError, match="full maps are not kept; read the kept witnesses and the digest"):
        batch.witness_map()
    batch.free()


@pytest.mark.parametrize("B", SIZES)
def test_reads_behind_solve_then_import(oracle, B):
    values, ores, oasg, ovals = _case(oracle, B, clean=True)
    nxt = acvm_amd.DeviceBuffer(values)
    batch = _handle(B)
    batch.set_initial_witness(values)
    assert batch.solve(then_import=nxt.ptr) == 0  # nobody left the generic path: the import ran behind the solve
    for read in (lambda: batch.witness(IDS[0]), batch.witness_map, lambda: batch.witness_map(3, 2), lambda: batch.extract([RET[0], IDS[2]])):
        with pytest.raises(acvm_amd.AcvmError, match=re.escape(GONE)):
            read()
    for w in (RET[0], 3, 5):
        v, a = batch.witness(w)
        assert a.all() and np.array_equal(v, ovals[:, w]), w
    assert np.array_equal(batch.extract([RET[0], 4]), ovals[:, [RET[0], 4]])
    batch.free()
    nxt.free()


def _check_node(oracle, node, values, B, keep, ores, oasg, ovals):
    """one Node solve: results, messages, digests, kept values and kept-assigned flags of every instance against the oracle"""
    not_solved, res, kept, asg, dig = node.solve(values, B)
    assert not_solved == sum(1 for r in ores if r.status != 0)
    for j in range(B):
        assert res[j].as_tuple() == ores[j].as_tuple() and res[j].message == ores[j].message, j
        assert bytes(dig[j]) == oracle.witness_map_digest(oasg[j], ovals[j]), j
    for k, w in enumerate(keep):
        want_a = oasg[:, w] if w < oasg.shape[1] else np.zeros(B, np.uint8)
        want_v = ovals[:, w] if w < ovals.shape[1] else np.zeros((B, 32), np.uint8)
        assert np.array_equal(asg[:, k], want_a) and np.array_equal(kept[:, k], want_v), w
    return asg


KEEP = [RET[0], 3, 8, IDS[0], 0, 1 << 20]  # (10: missing for every failing instance; 8: for instance 6; 0 and 2^20: for everybody)


@pytest.mark.parametrize("devices,B", [([0, 0], 130), ([0], 70)])
def test_node_outcome_of_asynchronous_exact_jobs(oracle, devices, B):
    """tiles of 64 with a few failing instances each: every tile's exact job runs beside the next tile, so the exact lanes' kept witnesses, flags
    and digests arrive with the job's outcome (side_table_outcome; the last tile's through batch_finish_pending). The level lanes' kept witnesses
    take the node driver's overlapped export here (batch_enqueue_kept), their results and digests batch_export_tile."""
    values, ores, oasg, ovals = _case(oracle, B)
    node = acvm_amd.Node(acvm_amd.Circuit(_circuit_bytes()), IDS, keep=KEEP, devices=devices, tile=64)
    asg = _check_node(oracle, node, values, B, KEEP, ores, oasg, ovals)
    st = node.stats()
    assert all(st["async_exact"]) and sum(st["exact_instances"]) >= sum(1 for r in ores if r.status != 0)
    assert not asg[6, 2] and asg[5, 2] and not asg[5, 0]
    node.free()


_MOSTLY_FAILING = {}


def _mostly_failing_case(oracle, B):
    """the clean case with the constraint of opcode 7 broken for three instances of four (j % 4 != 3): they lack witness 10, the others are level lanes"""
    if B not in _MOSTLY_FAILING:
        raw = np.frombuffer(_case(oracle, B, clean=True)[0], dtype=np.uint8).reshape(B, len(IDS), 32).copy()
        for j in range(B):
            if j % 4 != 3:
                raw[j, 2] = np.frombuffer(((int.from_bytes(raw[j, 2].tobytes(), "big") + 1) % P).to_bytes(32, "big"), dtype=np.uint8)
        values = raw.tobytes()
        ores, oasg, ovals = oracle.solve_batch(oracle.Circuit(_circuit_bytes()), IDS, values, B)
        ovals[oasg == 0] = 0
        assert [r.status != 0 for r in ores] == [j % 4 != 3 for j in range(B)]
        _MOSTLY_FAILING[B] = (values, ores, oasg, ovals)
    return _MOSTLY_FAILING[B]


@pytest.mark.parametrize("reuse_slots", [False, True])
def test_node_tile_whose_exact_path_stays_synchronous(oracle, reuse_slots):
    """B = 192 in tiles of 128, three instances of four failing. The first tile flags 96 instances: 8 x 96 > max(128, 512), so its exact path
    stays synchronous (batch_schedule.cpp go_async) and batch_export_tile delivers the kept witnesses of level lanes and exact lanes alike --
    the exact lanes' values from their own columns, or from the side table when rows are recycled (reuse_patch_exact), their flags from the
    bitmap. The second tile (64 live instances, 48 flagged) goes asynchronous behind it: its outcome is collected by batch_finish_pending."""
    B = 192
    values, ores, oasg, ovals = _mostly_failing_case(oracle, B)
    node = acvm_amd.Node(acvm_amd.Circuit(_circuit_bytes()), IDS, keep=KEEP, devices=[0], tile=128, reuse_slots=reuse_slots)
    for _ in range(2):  # (the second solve starts behind a tile that ended asynchronous)
        asg = _check_node(oracle, node, values, B, KEEP, ores, oasg, ovals)
    assert sum(node.stats()["exact_instances"]) >= 144
    assert asg[3, 0] and not asg[2, 0] and asg[2, 2] and not asg[:, 4].any()  # (10 for level lanes only, 8 for all, 0 for nobody)
    node.free()
