"""The host-only decisions of the packed wire export (acvm_amd/csrc/wire_pack_plan.cpp) without a device and without a handle: the module is
compiled as plain C++ (tools/wire_pack_plan_host_test.cpp) -- once as it is, once with AddressSanitizer and UndefinedBehaviorSanitizer as
`make asan` builds it, a stand-alone program either way. Every refusal, the chunk rule, the arena carve and what n_fit and total mean at a
capacity. The refusals are those tests/test_gpu_wire_packed.py asserts on the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, OFFSETS = 1 << 20, 1 << 21
BINCODE, GZIP, DEFLATE = 0, 1, 8
CHUNK_BYTES = 64 << 20


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    sources = [os.path.join(ROOT, "tools", "wire_pack_plan_host_test.cpp")] + [os.path.join(ROOT, "acvm_amd", "csrc", f) for f in ("wire_pack_plan.cpp", "wire_plan.cpp")]
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("wire_pack_plan") / "wire_pack_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sources + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "wire_pack_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/wire_pack_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith(("live", "nolive", "circuit")) for c in commands)
        return lines
    return run


def pack(container=GZIP, first=0, n=65, pitch=0, ptr=PTR, capacity=1 << 30, offsets=OFFSETS, lst=0, device=1, witnesses=None):
    listed = "-" if witnesses is None else "%d" % len(witnesses) + "".join(" %d" % w for w in witnesses)
    return "pack %d %d %d %d %d %d %d %d %d %s" % (container, first, n, pitch, ptr, capacity, offsets, lst, device, listed)


def test_every_refusal(tool):
    asked = [
        ("pack null", "null argument"),
        (pack(pitch=16), "a packed export has no pitch"),
        (pack(pitch=1 << 20), "a packed export has no pitch"),
        (pack(offsets=0), "null offsets"),
        (pack(ptr=0), "null buffer with a capacity"),
        (pack(ptr=PTR + 8), "not aligned to 16 bytes"),
        (pack(container=2), "unknown container 2"),
        (pack(witnesses=[3, 3]), "not strictly ascending"),
        (pack(first=40, n=61), "beyond the 100 live instances"),
        (pack(first=1, lst=1), "first must be 0 for a list export"),
    ]
    got = tool(["live 100", "circuit 10"] + [a for a, _ in asked] + ["nolive", pack()])
    for (command, text), line in zip(asked + [(pack(), "null batch")], got):
        assert line.startswith("err -1 ") and text in line, (command, line)


def test_what_passes(tool):
    asked = [pack(container=c) for c in (BINCODE, GZIP, DEFLATE)] + [
        pack(ptr=0, capacity=0),              # the sizing call
        pack(ptr=PTR + 8, device=0),          # the host form's buffer needs no alignment
        pack(n=0, ptr=0, capacity=0),
        pack(n=500, lst=1),                   # a list may be longer than the batch
        pack(first=35, n=65),
        pack(witnesses=[1, 4, 9]),
    ]
    got = tool(["live 100", "circuit 10"] + asked)
    bounds = {BINCODE: 8 + 76 * 10, GZIP: 16 + 8 + 76 * 10 + 8}
    for command, line in zip(asked, got):
        assert line.startswith("ok "), (command, line)
    for c, line in zip((BINCODE, GZIP), got):
        n, pitch, bound = (int(t) for t in line.split()[1:])
        assert (n, pitch, bound) == (65, (bounds[c] + 15) // 16 * 16, (bounds[c] + 15) // 16 * 16)  # the slots are made at the bound
    assert got[8].split()[1:] == ["65", "272", "272"]  # 16 + 8 + 76 * 3 + 8 = 260


def test_the_chunk_rule(tool):
    cases = [(960, 65728), (1100, 65728), (959, 65728), (1, 16), (64, 1 << 30), (63, 1 << 30), (1 << 17, 760016), (1 << 22, 16), (5 << 22, 16), (200, CHUNK_BYTES // 64), (200, CHUNK_BYTES // 64 + 16)]
    got = [int(x) for x in tool(["chunk %d %d" % c for c in cases])]
    for (n, pitch), chunk in zip(cases, got):
        assert chunk == min(n, max(64, CHUNK_BYTES // pitch // 64 * 64)), (n, pitch)
        assert chunk == n or (chunk % 64 == 0 and (chunk == 64 or chunk * pitch <= CHUNK_BYTES))
    assert got[:2] == [960, 960]  # 1 021 slots of 65 728 bytes fit 64 MiB: 960 is the whole blocks of 64 among them
    assert got[4:7] == [64, 63, 64] and got[7:9] == [1 << 22, 1 << 22] and got[9:] == [64, 64]


def test_the_arena_carve(tool):
    cases = [(0, 64, 272, 0), (1000, 64, 272, 1), (4096, 960, 65728, 1), (4096, 960, 65728, 0), (300, 1, 16, 1)]
    for (front, chunk, pitch, host), line in zip(cases, tool(["arena %d %d %d %d" % c for c in cases])):
        state, lengths, slots, packed, offsets, end = (int(t) for t in line.split())
        assert all(x % 256 == 0 for x in (state, lengths, slots, packed, offsets, end))
        assert state >= front and lengths >= state + 16 and slots >= lengths + chunk * 8 and packed >= slots + chunk * pitch
        if host:  # a second region as large as the slots, and the chunk's offsets
            assert offsets >= packed + chunk * pitch and end >= offsets + (chunk + 1) * 8
        else:
            assert end == packed == offsets
        assert end <= front + 16 + chunk * 8 + chunk * pitch * (2 if host else 1) + (chunk + 1) * 8 + 6 * 256  # the chunk and the tables, never n * pitch


def test_n_fit_and_total_at_a_capacity(tool):
    lens = [63, 8, 84, 160, 63, 0, 760]
    offsets = [0]
    for n in lens:
        offsets.append(offsets[-1] + n)
    asked = []
    for k in (1, 4, len(lens)):
        asked += [offsets[k] - 1, offsets[k], offsets[k] + 1]
    asked += [0, 1 << 63]
    got = tool(["fit %d %d" % (cap, len(lens)) + "".join(" %d" % o for o in offsets) for cap in asked] + ["fit 0 0 0", "fit 5 2 0 0 0"])
    for cap, line in zip(asked, got):
        n_fit, total = (int(t) for t in line.split())
        assert total == offsets[-1]
        assert n_fit == max(k for k in range(len(lens) + 1) if offsets[k] <= cap and all(o <= cap for o in offsets[:k + 1])), cap
    want = {offsets[1] - 1: 0, offsets[1]: 1, offsets[1] + 1: 1, offsets[4] - 1: 3, offsets[4]: 4, offsets[4] + 1: 4, offsets[7] - 1: 6, offsets[7]: 7, offsets[7] + 1: 7}
    for cap, line in zip(asked[:9], got):
        assert int(line.split()[0]) == want[cap]
    assert got[-2] == "0 0" and got[-1] == "2 0"
