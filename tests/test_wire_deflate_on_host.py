"""The deflating wire-format kernel's per-entry code without a device: acvm_amd/csrc/wire_deflate.hpp compiled for the host
(tools/wire_deflate_host_test.hip) over the plan's code table. The parse, the bit cost and the emitted bits of every entry of the case rows
(tests/wire_deflate_cases.py) are judged by tests/wire_deflate_ref.py; then the argument checks that need no GPU and the Python view."""
import ctypes as C
import os
import subprocess

import pytest

import wire_deflate_cases as cases
import wire_deflate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wire_deflate") / "wire_deflate_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "wire_deflate_host_test.hip"),
                           os.path.join(ROOT, "acvm_amd", "csrc", "wire_plan.cpp"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _entries():
    """(entry, predecessor or None) of every case row, each pair once"""
    seen, out = set(), []
    for m in cases.rows() + cases.keyed_rows() + cases.count_rows():
        body = ref.body(m)
        prev = None
        for at in range(8, len(body), ref.ENTRY):
            cur = body[at:at + ref.ENTRY]
            if (cur, prev) not in seen:
                seen.add((cur, prev))
                out.append((cur, prev))
            prev = cur
    return out


OFFSETS = list(range(32)) + [95, 3111]  # every place in a dword, and behind a window's earlier entries


def _hex(entry):
    return entry.hex() if entry is not None else "-"


def test_constants(tool):
    container, entry_max, min_match, window = (int(x) for x in tool(["const"])[0].split())
    assert (container, entry_max, min_match, window) == (ref.GZIP_DEFLATE, 12 * 10 + 64 * 5, 3, cases.window())
    ns = [0, 1, 9, 1000, 1 << 27]
    assert [int(x) for x in tool(["bound %d %d" % (ref.HEADER_BITS, n) for n in ns])] == [ref.bound(ref.GZIP_DEFLATE, n) for n in ns]


def test_token_lists_and_bit_costs_of_the_case_rows(tool):
    entries = _entries()
    assert len(entries) > 1500 and any(p is None for _, p in entries)
    for (cur, prev), line in zip(entries, tool(["parse %s %s" % (_hex(cur), _hex(prev)) for cur, prev in entries])):
        got = [int(x) for x in line.split()]
        want = ref.MODEL.parse(cur, prev)
        assert got[0] == ref.MODEL.entry_cost(cur, prev) <= 440 and got[1] == len(want) <= 76
        pairs = list(zip(got[2::2], got[3::2]))
        assert pairs == [(0, t[1]) if t[0] == "lit" else (t[1], t[2]) for t in want], (cur, prev)


def test_emission_at_every_bit_offset(tool):
    entries = _entries()
    picked = entries[::37] + [e for e in entries if ref.MODEL.entry_cost(*e) < 40][:8] + [max(entries, key=lambda e: ref.MODEL.entry_cost(*e))]
    commands = ["emit %d %s %s" % (offset, _hex(cur), _hex(prev)) for cur, prev in picked for offset in OFFSETS]
    lines = iter(tool(commands))
    for cur, prev in picked:
        b = ref.Bits()
        for t in ref.MODEL.parse(cur, prev):
            ref.MODEL.token_bits(b, t)
        for offset in OFFSETS:
            end, data = next(lines).split()
            assert int(end) == offset + b.n
            assert int.from_bytes(bytes.fromhex(data), "little") == b.acc << offset, (cur, prev, offset)


def test_argument_checks_without_a_device_and_the_python_view():
    """Without a handle every call answers "null batch" before it looks at the container, so "an unknown container is refused as today" cannot be
    asked of acvm_batch_wire_bound or the Python view here: tests/test_wire_deflate_plan_on_host.py asks it of wire_plan() (containers 2, 3, 9),
    tests/test_gpu_wire_deflate.py of Batch.wire_bound, witness_maps_wire_device and witness_maps_wire on a handle."""
    import inspect
    import acvm_amd
    L = acvm_amd.lib()
    assert (acvm_amd.WIRE_BINCODE, acvm_amd.WIRE_GZIP_STORED, acvm_amd.WIRE_GZIP_DEFLATE) == (0, 1, 8)
    desc, _keep = acvm_amd.wire_desc(acvm_amd.WIRE_GZIP_DEFLATE, 0, 4)
    assert L.acvm_batch_wire_bound(None, C.byref(desc)) < 0 and b"null batch" in L.acvm_last_error()
    assert L.acvm_batch_witness_maps_wire_device(None, C.byref(desc), None, 16, None) == -1 and b"null batch" in L.acvm_last_error()
    assert L.acvm_batch_witness_maps_wire(None, C.byref(desc), None, None) == -1
    header = open(os.path.join(ROOT, "include", "acvm_amd.h")).read()
    assert "ACVM_WIRE_GZIP_DEFLATE = 8" in header
    for method in (acvm_amd.Batch.wire_bound, acvm_amd.Batch.witness_maps_wire_device, acvm_amd.Batch.witness_maps_wire):
        assert "WIRE_GZIP_DEFLATE" in inspect.getdoc(method)
