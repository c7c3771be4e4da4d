"""The precomputed coefficient x row reduction on the HOST: tools/lin_table_host_test.hip runs the planner's table builder (lin_table.hpp, fed the
inline words plan.cpp writes into a record) and fr29_lin_add<1 / 2> (fr_device.hpp is __host__ __device__) over the case list of
tests/lin_table_ref.py -- rows 0, 1, p - 1, p, 2^256 - 1 and random 256-bit patterns, coefficients 1, 2, p - 1 and random, h zero, all limbs 2^32 - 1
and random -- and every table word and every result is compared with Python integers here: the residue, the routine's bound p (1 + 2^-25) + h, the
normalised limbs, and the column accumulator, which the tool follows in 128 bits (it must stay within the routine's documented
(9 N + 2) 2^58 + carry, far from 64 bits). The checker's side: a swapped table or a shifted offset is a finding that names the record. No GPU is
needed: hipcc builds the host side only. The same cases on the device: tests/test_gpu_lin_table.py."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import lin_table_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITEMS = 100_032  # 1 563 groups of 64


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = str(tmp_path_factory.mktemp("lin_table") / "lin_table_host_test")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-O2", "-std=c++17", "-x", "hip", os.path.join(ROOT, "tools", "lin_table_host_test.hip"), "-o", out],
                   check=True, timeout=900)
    return out


@pytest.fixture(scope="module")
def run(exe, tmp_path_factory):
    d = tmp_path_factory.mktemp("lin_table_run")
    n_terms, coef_w, row_w, hs, coefs, rows = ref.cases(N_ITEMS)
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", N_ITEMS))
        for a in (n_terms, coef_w, row_w, hs):
            f.write(np.ascontiguousarray(a, dtype="<u4").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    raw = open(fout, "rb").read()
    G = len(n_terms)
    tables = np.frombuffer(raw, dtype="<u4", count=G * 162).reshape(G, 2, 81)
    out = np.frombuffer(raw, dtype="<u4", count=N_ITEMS * 9, offset=G * 162 * 4).reshape(N_ITEMS, 9)
    max1, max2, disagree = struct.unpack_from("<QQI", raw, (G * 162 + N_ITEMS * 9) * 4)
    return n_terms, coefs, rows, hs, tables, out, (max1, max2), disagree


def test_case_list_covers_the_extremes():
    n_terms, coef_w, row_w, hs, coefs, rows = ref.cases(64 * 8)
    for n in (1, 2):
        for t in range(n):
            assert {c[t] for g, c in enumerate(coefs) if n_terms[g] == n} >= set(ref.COEF_SPECIALS)
    for t in (0, 1):
        for kind in (0, 0xFFFFFFFF):
            assert {rows[j][t] for j in range(len(rows)) if (hs[j] == kind).all()} >= set(ref.ROW_SPECIALS)
    assert any((hs[j] != 0).any() and (hs[j] != 0xFFFFFFFF).any() for j in range(len(rows)))


def test_planner_tables_against_integers(run):
    n_terms, coefs, rows, hs, tables, out, acc, disagree = run
    ref.check_tables(n_terms, coefs, tables)
    assert int(tables.max()) < 1 << 29


def test_lin_add_against_integers(run):
    n_terms, coefs, rows, hs, tables, out, acc, disagree = run
    assert len(rows) >= 10 ** 5
    worst = ref.check_results(n_terms, coefs, rows, hs, out)
    print("largest (result - h) / p: %.9f" % worst)


def test_accumulator_never_wraps(run):
    n_terms, coefs, rows, hs, tables, out, acc, disagree = run
    assert disagree == 0  # the 128-bit scan and the routine's 64-bit one hand out the same limbs
    for n, m in ((1, acc[0]), (2, acc[1])):
        print("N = %d: largest column accumulator %.4f x 2^58" % (n, m / 2 ** 58))
        assert 0 < m < (9 * n + 2) * 2 ** 58 + 2 ** 36 < 2 ** 64


def test_checker_names_the_record_of_a_swapped_table_or_a_shifted_offset():
    import acvm_amd
    from acvm_amd import synth
    circ, ids = synth.arithmetic_circuit(300, mix=(0, 100, 0, 0))
    c = acvm_amd.Circuit(circ.to_bytes())
    good = c.lin_plan(ids)
    assert good["ok"] and good["n_lin_terms"] >= good["n_lin_records"] > 100, good
    for mutation in (1, 2):
        bad = c.lin_plan(ids, mutation=mutation)
        assert not bad["ok"] and bad["n_findings"] >= 1
        assert "LINEAR TABLES: gate of opcode " in bad["report"], bad["report"]
    with acvm_amd.tuning(lin_table=0):
        off = c.lin_plan(ids)
        assert off["ok"] and off["n_lin_terms"] == 0 and off["n_programs_with_tables"] == 0
