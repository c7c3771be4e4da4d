"""The gzip import's per-row reader without a device: acvm_amd/csrc/wire_inflate.hpp compiled for the host with the host side under
AddressSanitizer and UndefinedBehaviorSanitizer (tools/wire_inflate_host_test.hip: every row's input, output and tables in heap blocks of
exactly their sizes). Bytes, length, class, block and CRC of every case row and of a seeded sweep of 20 000 mutations and truncations are
tests/wire_inflate_ref.py's; then the argument checks that need no GPU and the Python view."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

import wire_inflate_cases as cases
import wire_inflate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acvm_amd", "csrc")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wire_inflate") / "wire_inflate_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "wire_inflate_host_test.hip"), os.path.join(CSRC, "wire_inflate_plan.cpp"),
                           os.path.join(CSRC, "wire_in_plan.cpp"), os.path.join(CSRC, "wire_plan.cpp"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _ask(tool, rows_and_caps):
    got = []
    for line in tool(["inflate %d %s" % (cap, row.hex() or "-") for row, cap in rows_and_caps]):
        cls, block, length, crc, out = line.split()
        got.append((int(cls), int(block), int(length), int(crc), b"" if out == "-" else bytes.fromhex(out)))
    return got


def _want(row, cap):
    m = cases.judged(row, cap)
    return m.cls, m.block, len(m.out), m.crc, m.out


def test_the_arithmetic_of_the_symbol_tables(tool):
    tok = [int(x) for x in tool(["codes"])[0].split()]
    assert tok[0:58:2] == list(ref.LENGTH_BASE) and tok[1:58:2] == list(ref.LENGTH_EXTRA)
    assert tok[58:118:2] == list(ref.DIST_BASE) and tok[59:118:2] == list(ref.DIST_EXTRA)
    assert tok[118:] == list(ref.CLC_ORDER)


def test_every_case_row(tool):
    asked = [(c.row, cases.CAP if c.cap is None else c.cap) for c in cases.everything()]
    # a cap of exactly the output, one below it and zero for the small accepted rows: the bound is met at the last byte, one before it, at once
    for c in cases.list_a() + cases.list_b():
        n = len(cases.judged(c.row, cases.CAP).out)
        if n <= 3100:
            asked += [(c.row, n), (c.row, max(n - 1, 0)), (c.row, 0)]
    got = _ask(tool, asked)
    classes = set()
    for (row, cap), g in zip(asked, got):
        assert g == _want(row, cap), (row[:24].hex(), cap, g[:4])
        classes.add(g[0])
    assert classes == set(range(0, 11))


def test_a_seeded_sweep_of_mutations_and_truncations(tool):
    rows = cases.mutations(20000)
    assert len(rows) >= 20000
    got = _ask(tool, [(r, 3048) for r in rows])
    seen = {}
    for row, g in zip(rows, got):
        assert g == _want(row, 3048), (row.hex(), g[:4])
        seen[g[0]] = seen.get(g[0], 0) + 1
    assert seen.get(0, 0) > 100 and len(seen) >= 9, seen  # the sweep reaches most classes, and some mutations are harmless


def test_the_finding_key_orders_instance_class_block(tool):
    triples = [(0, 1, 0), (0, 7, 0), (0, 7, 817), (0, 10, 1), (1, 1, 0), (64, 5, 8), (64, 6, 0), (65, 2, 3), ((1 << 27) - 1, 10, (1 << 32) - 1)]
    keys = []
    for t, got in zip(triples, tool(["key %d %d %d" % t for t in triples])):
        key, j, cls, block = (int(x) for x in got.split())
        assert (j, cls, block) == t and 0 < key < 1 << 64
        keys.append(key)
    assert keys == sorted(keys, reverse=True)  # atomicMax keeps the smallest triple


def test_argument_checks_without_a_device():
    import acvm_amd
    L = acvm_amd.lib()
    for name in ("acvm_batch_import_device_wire_gzip", "acvm_batch_set_initial_witness_maps_gzip", "acvm_debug_inflate_rows"):
        assert name in acvm_amd.ABI_SYMBOLS
    desc = acvm_amd.WireInDesc(container=acvm_amd.WIRE_GZIP_DEFLATE, pitch=64)
    assert L.acvm_batch_import_device_wire_gzip(None, C.byref(desc), 16, None) == -1 and b"null batch" in L.acvm_last_error()
    lengths = (C.c_uint64 * 1)(8)
    assert L.acvm_batch_set_initial_witness_maps_gzip(None, bytes(8), 8, lengths) == -1 and b"null batch" in L.acvm_last_error()
    out, words = (C.c_uint8 * 8)(), (C.c_uint64 * 4)()
    assert L.acvm_debug_inflate_rows(None, 8, None, 1, 8, out, words, words, None) == -1 and b"null argument" in L.acvm_last_error()
    assert L.acvm_debug_inflate_rows(bytes(8), 8, None, 1, 6, out, words, words, None) == -1 and b"multiple of 4" in L.acvm_last_error()
    assert L.acvm_debug_inflate_rows(None, 0, None, 0, 0, None, None, None, None) == 0  # no rows: nothing to do, no device asked for
    assert L.acvm_abi_version() == 6


def test_python_view():
    import acvm_amd
    assert list(inspect.signature(acvm_amd.Batch.import_device_wire_gzip).parameters)[1:] == ["d_ptr", "pitch", "d_lengths"]
    assert list(inspect.signature(acvm_amd.Batch.set_initial_witness_maps_gzip).parameters)[1:] == ["maps"]
    assert list(inspect.signature(acvm_amd.debug_inflate_rows).parameters) == ["rows", "out_cap", "fill", "pitch", "lengths"]
