"""The device-resident witness import without a device: the per-element decoding of acvm_amd/csrc/import_decode.hpp compiled for the host
(tools/import_device_host_test.hip) and judged by Python integers, on the reduction-edge values of tests/test_gpu_import.py and on seeded
random 256-bit strings, in all three encodings; the argument checks of acvm_batch_import_device that need no GPU; the Python view."""
import ctypes as C
import importlib.util
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BE32, LE32, MONT256_LE = 0, 1, 2
INSTANCE_MAJOR, WITNESS_MAJOR = 0, 1
N_RANDOM = 2000


def _edge_values():
    """tests/test_gpu_import.py::_edge_values, from that file"""
    spec = importlib.util.spec_from_file_location("_gpu_import_for_edges", os.path.join(ROOT, "tests", "test_gpu_import.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._edge_values()


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("import_device") / "import_device_host_test")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
                           os.path.join(ROOT, "tools", "import_device_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-400:]
        return out.stdout.split("\n")[:-1]
    return run


def _strings():
    """the 256-bit strings every encoding is given: each is read as the encoding reads it (every string is a valid element)"""
    edge = _edge_values()
    assert len(edge) == 72
    rng = random.Random(0x1A90D7)
    return edge + [rng.getrandbits(256) for _ in range(N_RANDOM)]


def _value(s, encoding):
    """the field element the 32 bytes of the integer s (written most significant first) mean in the encoding"""
    b = s.to_bytes(32, "big")
    if encoding == BE32:
        return int.from_bytes(b, "big") % P
    if encoding == LE32:
        return int.from_bytes(b, "little") % P
    return int.from_bytes(b, "little") * pow(1 << 256, -1, P) % P


def test_constants(tool):
    r266, r522, two5 = (int(h, 16) for h in tool(["const"])[0].split())
    assert (r266, r522, two5) == (pow(2, 266, P), pow(2, 522, P), 32)


@pytest.mark.parametrize("command", ["dec", "pieces"])
def test_decode_against_python_integers(tool, command):
    """canonical value, row and byte-plane word of every string in every encoding. The row is the fully reduced x * 2^261 mod p: the bound
    fr_device.hpp documents for what anything but an Arithmetic gate reads, which initial witnesses are (hash inputs, RANGE operands)."""
    strings = _strings()
    commands, want = [], []
    for encoding in (BE32, LE32, MONT256_LE):
        for s in strings:
            commands.append("%s %d %064x" % (command, encoding, s))
            want.append(_value(s, encoding))
    got = tool(commands)
    assert len(got) == len(want)
    n_bytes = 0
    for c, g, x in zip(commands, got, want):
        canonical, row, plane = (int(h, 16) for h in g.split())
        assert canonical < P and canonical == x, c
        assert row < P and row == x * (1 << 261) % P, c
        assert plane == (x & 0x1FFFFFFF) | (int(x < 256) << 31), c
        n_bytes += x < 256
    assert n_bytes >= 19  # (k p + 0, 1, 2 for six k and 255, read big-endian; the other encodings' bytes: the two tests below)


def test_montgomery_256_edges(tool):
    """what an exporting prover writes (x * 2^256 mod p for x at the byte and plane-word boundaries) and the same residues as unreduced
    representatives m + k p < 2^256 (m >= p is not an error): the value is m * 2^-256 mod p either way"""
    xs = [0, 1, 255, 256, 257, (1 << 29) - 1, 1 << 29, (1 << 29) + 7, (1 << 253) + 7, P - 1, P - 256]
    commands, want = [], []
    for x in xs:
        m = (x << 256) % P
        for k in range(6):
            if m + k * P < (1 << 256):
                commands.append("dec %d %s" % (MONT256_LE, (m + k * P).to_bytes(32, "little").hex()))
                want.append(x)
    for g, x, c in zip(tool(commands), want, commands):
        canonical, row, plane = (int(h, 16) for h in g.split())
        assert (canonical, row, plane) == (x, x * (1 << 261) % P, (x & 0x1FFFFFFF) | (int(x < 256) << 31)), c


def test_export_then_import_reproduces_the_value(tool):
    """the inverse of what export_encode writes: the bytes each encoding exports for x decode to x"""
    rng = random.Random(0xE4901)
    for x in [0, 1, 255, P - 1] + [rng.randrange(P) for _ in range(50)]:
        exported = {BE32: x.to_bytes(32, "big"), LE32: x.to_bytes(32, "little"), MONT256_LE: ((x << 256) % P).to_bytes(32, "little")}
        got = tool(["dec %d %s" % (e, exported[e].hex()) for e in (BE32, LE32, MONT256_LE)])
        assert [int(g.split()[0], 16) for g in got] == [x, x, x]


def test_element_addressing(tool):
    """element (instance i, column c) of the caller's buffer lies where the export puts element (i, k = c)"""
    cases = [(INSTANCE_MAJOR, 7, 5, 3), (INSTANCE_MAJOR, 9, 129, 8), (WITNESS_MAJOR, 130, 129, 8), (WITNESS_MAJOR, 192, 0, 41), (WITNESS_MAJOR, 1 << 33, 5, 9)]
    got = tool(["at %d %d %d %d" % c for c in cases])
    assert [int(g) for g in got] == [c * s + i if layout == WITNESS_MAJOR else i * s + c for layout, s, i, c in cases]


def test_argument_checks_without_a_device():
    import acvm_amd
    L = acvm_amd.lib()
    for name in ("acvm_batch_import_device", "acvm_batch_solve_then_import_ex"):
        assert name in acvm_amd.ABI_SYMBOLS
    E_INVALID = -1
    good = acvm_amd.ImportDesc(encoding=acvm_amd.ENC_LE32, layout=acvm_amd.LAYOUT_WITNESS_MAJOR, n_columns=0, stride=0)
    assert L.acvm_batch_import_device(None, C.byref(good), 16) == E_INVALID
    assert L.acvm_batch_import_device(None, None, 16) == E_INVALID
    assert L.acvm_batch_solve_then_import_ex(None, C.byref(good), 16) == E_INVALID
    bad = acvm_amd.ImportDesc(encoding=3, layout=0, n_columns=0, stride=0)
    assert L.acvm_batch_import_device(None, C.byref(bad), 16) == E_INVALID
    assert b"encoding" in L.acvm_last_error()
    bad = acvm_amd.ImportDesc(encoding=0, layout=2, n_columns=0, stride=0)
    assert L.acvm_batch_import_device(None, C.byref(bad), 16) == E_INVALID
    assert b"layout" in L.acvm_last_error()


def test_python_view():
    import acvm_amd
    import inspect
    assert callable(acvm_amd.Batch.import_device)
    sig = inspect.signature(acvm_amd.Batch.import_device)
    assert list(sig.parameters)[1:] == ["d_ptr", "encoding", "layout", "columns", "n_columns", "stride"]
    assert sig.parameters["encoding"].default == acvm_amd.ENC_BE32 and sig.parameters["layout"].default == acvm_amd.LAYOUT_INSTANCE_MAJOR
    assert "then_import_desc" in inspect.signature(acvm_amd.Batch.solve).parameters
    # acvm_import_desc_t as the C compiler lays it out: 2 x u32, a pointer, a u32 (+ padding), a u64
    assert C.sizeof(acvm_amd.ImportDesc) == 32 and acvm_amd.ImportDesc.columns.offset == 8 and acvm_amd.ImportDesc.stride.offset == 24
