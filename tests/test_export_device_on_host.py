"""The device-resident witness export without a device: the per-element encoding and the tile index maps of
acvm_amd/csrc/export_encode.hpp compiled for the host (tools/export_device_host_test.hip) and judged by Python integers; the
argument checks of acvm_batch_export_device that need no GPU; the Python view."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BE32, LE32, MONT256_LE = 0, 1, 2
INSTANCE_MAJOR, WITNESS_MAJOR = 0, 1


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("export_device") / "export_device_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tools", "export_device_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        return out.stdout.split("\n")[:-1]
    return run


def _expected(x, encoding):
    if encoding == BE32:
        return x.to_bytes(32, "big")
    if encoding == LE32:
        return x.to_bytes(32, "little")
    return ((x << 256) % P).to_bytes(32, "little")


def test_encode_against_python_integers(tool):
    """Three encodings x {row stored as is, scaled row}: the row holds x * 2^261 * scale mod p, possibly as a non-canonical representative
    x * 2^261 * scale + k p < 2^256 (relaxed rows); the factor is 1 or 2^256 mod p for a plain row, 1 / scale or 2^256 / scale for a scaled one."""
    rng = random.Random(0xE4901)
    values = [0, 1, P - 1, 1 << 253, 5, (1 << 128) - 1] + [rng.randrange(P) for _ in range(200)]
    plain = [int(h, 16) for h in tool(["factor %d" % e for e in (BE32, LE32, MONT256_LE)])]
    assert plain == [1, 1, (1 << 256) % P]
    commands, want = [], []
    for n, x in enumerate(values):
        for scaled in (False, True):
            scale = rng.randrange(1, P) if scaled else 1
            stored = x * (1 << 261) * scale % P
            reps = [stored] + [stored + k * P for k in range(1, 6) if stored + k * P < (1 << 256)]  # 2^256 / p > 5: up to five more
            rows = reps if n < 6 else [reps[0], rng.choice(reps)]
            for encoding in (BE32, LE32, MONT256_LE):
                factor = plain[encoding] * pow(scale, -1, P) % P
                for row in rows:
                    commands.append("enc %d 1 %064x %064x" % (encoding, row, factor))
                    want.append(_expected(x, encoding))
    # unassigned: 32 zero bytes in every encoding, whatever the row holds
    for encoding in (BE32, LE32, MONT256_LE):
        commands.append("enc %d 0 %064x %064x" % (encoding, rng.randrange(1 << 256), plain[encoding]))
        want.append(bytes(32))
    got = tool(commands)
    assert len(got) == len(want)
    for c, g, w in zip(commands, got, want):
        assert bytes.fromhex(g) == w, c


@pytest.mark.parametrize("layout,n,n_sel,T,stride", [
    (INSTANCE_MAJOR, 64, 16, 16, 16), (INSTANCE_MAJOR, 130, 37, 16, 37), (INSTANCE_MAJOR, 130, 37, 16, 41), (INSTANCE_MAJOR, 1, 4, 16, 4),
    (INSTANCE_MAJOR, 63, 15, 16, 20), (INSTANCE_MAJOR, 65, 17, 16, 17), (INSTANCE_MAJOR, 200, 33, 8, 40), (INSTANCE_MAJOR, 70, 9, 4, 9),
    (INSTANCE_MAJOR, 129, 50, 32, 64), (WITNESS_MAJOR, 130, 37, 0, 130), (WITNESS_MAJOR, 300, 5, 0, 333), (WITNESS_MAJOR, 1, 3, 0, 1),
    (INSTANCE_MAJOR, 300, 1, 0, 1), (INSTANCE_MAJOR, 70, 3, 0, 5), (INSTANCE_MAJOR, 1, 1, 0, 1)])
def test_tile_maps_write_every_unit_once(tool, layout, n, n_sel, T, stride):
    """Every 16-byte unit and every mask byte of the described elements is written exactly once, nothing else is: no unit of the padding
    between rows, no unit beyond n_witnesses of a row, for shapes with tails in both dimensions. T = 0: the direct kernel (witness-major, and
    instance-major lists shorter than the tiled kernel's four waves), else the tiled kernel with T positions per tile."""
    lines = tool(["tile %d %d %d %d %d" % (layout, n, n_sel, T, stride)])
    assert lines[-1] == "end" and not [l for l in lines if l.startswith("bad")]
    units = sorted(int(l[2:]) for l in lines if l.startswith("u "))
    masks = sorted(int(l[2:]) for l in lines if l.startswith("m "))
    at = (lambda i, k: k * stride + i) if layout == WITNESS_MAJOR else (lambda i, k: i * stride + k)
    elements = sorted(at(i, k) for i in range(n) for k in range(n_sel))
    assert masks == elements
    assert units == sorted(2 * e + h for e in elements for h in (0, 1))


def test_argument_checks_without_a_device():
    import acvm_amd
    L = acvm_amd.lib()
    assert "acvm_batch_export_device" in acvm_amd.ABI_SYMBOLS and "acvm_device_download" in acvm_amd.ABI_SYMBOLS
    E_INVALID = -1
    good = acvm_amd.ExportDesc(encoding=acvm_amd.ENC_LE32, layout=acvm_amd.LAYOUT_WITNESS_MAJOR, first=0, n=1, stride=0)
    assert L.acvm_batch_export_device(None, C.byref(good), 16, None) == E_INVALID
    assert L.acvm_batch_export_device(None, None, 16, None) == E_INVALID
    bad = acvm_amd.ExportDesc(encoding=3, layout=0, first=0, n=1, stride=0)
    assert L.acvm_batch_export_device(None, C.byref(bad), 16, None) == E_INVALID
    assert b"encoding" in L.acvm_last_error()
    bad = acvm_amd.ExportDesc(encoding=0, layout=2, first=0, n=1, stride=0)
    assert L.acvm_batch_export_device(None, C.byref(bad), 16, None) == E_INVALID
    assert b"layout" in L.acvm_last_error()
    buf = C.create_string_buffer(8)
    assert L.acvm_device_download(buf, None, 8) == E_INVALID
    assert L.acvm_device_download(None, None, 0) == 0


def test_python_view():
    import acvm_amd
    assert (acvm_amd.ENC_BE32, acvm_amd.ENC_LE32, acvm_amd.ENC_MONT256_LE) == (0, 1, 2)
    assert (acvm_amd.LAYOUT_INSTANCE_MAJOR, acvm_amd.LAYOUT_WITNESS_MAJOR) == (0, 1)
    assert callable(acvm_amd.Batch.export_device) and callable(acvm_amd.DeviceBuffer.download)
    # acvm_export_desc_t as the C compiler lays it out: 4 x u32, a pointer, a u32 (+ padding), a u64
    assert C.sizeof(acvm_amd.ExportDesc) == 40 and acvm_amd.ExportDesc.stride.offset == 32 and acvm_amd.ExportDesc.witnesses.offset == 16
