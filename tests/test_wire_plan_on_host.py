"""The checks, the generic instance's entries and ranks, the bound, the framing offsets and the CRC power table of the batch-wide wire format
(acvm_amd/csrc/wire_plan.cpp) without a device and without a handle: the module is compiled as plain C++ (tools/wire_plan_host_test.cpp) -- once
as it is, once with AddressSanitizer and UndefinedBehaviorSanitizer as `make asan` builds it, a stand-alone program either way -- and its
answers are judged by tests/wire_ref.py and zlib. The refusals are those tests/test_gpu_wire.py asserts on the device."""
import os
import random
import subprocess
import zlib

import pytest

import wire_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 1 << 20
BINCODE, GZIP = 0, 1


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    sources = [os.path.join(ROOT, "tools", "wire_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "wire_plan.cpp")]
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("wire_plan") / "wire_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sources + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "wire_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/wire_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith(("live", "nolive", "circuit")) for c in commands)
        return lines
    return run


def wire_command(container=GZIP, first=0, n=65, pitch=0, ptr=PTR, lst=0, device=1, witnesses=None):
    listed = "-" if witnesses is None else "%d" % len(witnesses) + "".join(" %d" % w for w in witnesses)
    return "wire %d %d %d %d %d %d %d %s" % (container, first, n, pitch, ptr, lst, device, listed)


def circuit_command(n_witnesses, unproduced=()):
    return "circuit %d %d" % (n_witnesses, len(unproduced)) + "".join(" %d" % w for w in unproduced)


def parse(line):
    """("err", text) or a dict"""
    if line.startswith("err "):
        code, text = line[4:].split(" ", 1)
        assert code == "-1"
        return ("err", text)
    tok = [int(t) for t in line.split()[1:]]
    keys = ("container", "first", "n", "pitch", "bound", "whole", "n_positions", "n_windows", "x64")
    out = dict(zip(keys, tok))
    at = len(keys)
    n_entries = tok[at]
    out["entries"] = tok[at + 1:at + 1 + n_entries]
    at += 1 + n_entries
    out["rank"] = tok[at:at + out["n_positions"] + 1]
    at += out["n_positions"] + 1
    out["mask"] = tok[at + 1:at + 1 + tok[at]]
    at += 1 + tok[at]
    out["pow"] = tok[at + 1:at + 1 + tok[at]]
    assert at + 1 + tok[at] == len(tok)
    return out


def _raw(data):
    return zlib.crc32(data) ^ zlib.crc32(bytes(len(data)))


def _mul(a, b):
    """a * b mod P, reflected: bit 31 is x^0"""
    p = 0
    for k in range(31, -1, -1):
        if (a >> k) & 1:
            p ^= b
        b = (b >> 1) ^ (0xEDB88320 if b & 1 else 0)
    return p


def _x_pow_bytes(m):
    """x^(8 m) mod P by square and multiply from x^8 = 0x00800000"""
    r, sq = 0x80000000, 0x00800000
    while m:
        if m & 1:
            r = _mul(r, sq)
        sq = _mul(sq, sq)
        m >>= 1
    return r


def test_the_models_powers_are_zlibs():
    """what the power table is judged by is itself judged by zlib: c * x^(8 m) is c advanced over m zero bytes"""
    rng = random.Random(0x31BE1000)
    for m in (0, 1, 8, 76, 76 * 863, 100000):
        d = bytes(rng.randrange(256) for _ in range(76))
        assert _mul(_x_pow_bytes(m), _raw(d)) == _raw(d + bytes(m))


# ---- the refusals, one by one
@pytest.mark.parametrize("case", [
    ("an unknown container", dict(container=2), "unknown container 2"),
    ("a list that repeats a witness", dict(witnesses=[1, 4, 4, 9]), "the witness list is not strictly ascending: entry 2 (witness 4) follows witness 4"),
    ("a list that descends", dict(witnesses=[1, 9, 4]), "not strictly ascending: entry 2 (witness 4) follows witness 9"),
    ("a pitch below the bound", dict(pitch=wire_ref.bound(GZIP, 40) - 16), "pitch %d is below the bound %d" % (wire_ref.bound(GZIP, 40) - 16, wire_ref.bound(GZIP, 40))),
    ("a pitch below the bound of a list", dict(pitch=16, witnesses=[1, 2]), "pitch 16 is below the bound %d" % wire_ref.bound(GZIP, 2)),
    ("a pitch that is no multiple of 16", dict(pitch=wire_ref.bound(GZIP, 40) + 8), "is not a multiple of 16"),
    ("a misaligned buffer", dict(ptr=PTR + 8), "the buffer is not aligned to 16 bytes"),
    ("a range beyond the live instances", dict(first=60, n=6), "instances [60, 66) are beyond the 65 live instances"),
    ("first beyond the live instances", dict(first=66, n=0), "are beyond the 65 live instances"),
    ("first + n wraps 2^32", dict(first=2, n=(1 << 32) - 1), "are beyond the 65 live instances"),
    ("first != 0 with a list", dict(first=1, n=3, lst=1), "first must be 0 for a list export"),
    ("a null buffer while n > 0", dict(ptr=0), "null buffer"),
    ("n * pitch beyond any buffer", dict(pitch=((1 << 57) // 65 + 16) // 16 * 16), "is beyond any device buffer"),
], ids=lambda c: c[0])
def test_refusal(tool, case):
    _, args, text = case
    answer = parse(tool(["live 65", circuit_command(40), wire_command(**args)])[0])
    assert answer[0] == "err" and text in answer[1], answer


def test_refusals_of_the_arguments_themselves(tool):
    lines = tool(["live 65", circuit_command(40), "wire null", "nolive", wire_command()])
    assert lines == ["err -1 null argument", "err -1 null batch"]


def test_what_is_accepted(tool):
    bound = wire_ref.bound(GZIP, 40)
    cases = [
        dict(),
        dict(container=BINCODE),
        dict(pitch=bound), dict(pitch=bound + 48),
        dict(first=60, n=5), dict(first=65, n=0),
        dict(first=0, n=1000, lst=1),                 # a list is as long as it likes
        dict(n=0, ptr=0),                             # nothing to write: a null buffer is fine
        dict(ptr=PTR + 3, device=0),                  # the host form's buffer needs no alignment
        dict(witnesses=[]), dict(witnesses=[0]), dict(witnesses=[3, 39, 40, 1 << 31, (1 << 32) - 1]),  # a witness beyond the circuit is unassigned
    ]
    for c, line in zip(cases, tool(["live 65", circuit_command(40)] + [wire_command(**c) for c in cases])):
        a = parse(line)
        assert isinstance(a, dict), (c, a)
        n_positions = 40 if c.get("witnesses") is None else len(c["witnesses"])
        want_bound = wire_ref.bound(c.get("container", GZIP), n_positions)
        assert (a["container"], a["first"], a["n"], a["bound"], a["pitch"]) == (c.get("container", GZIP), c.get("first", 0), c.get("n", 65), want_bound, c.get("pitch", 0) or want_bound)
        assert a["whole"] == (c.get("witnesses") is None) and a["n_positions"] == n_positions


def _check_plan(a, n_witnesses, unproduced, witnesses, window):
    positions = list(range(n_witnesses)) if witnesses is None else witnesses
    produced = [w < n_witnesses and w not in unproduced for w in positions]
    assert a["entries"] == [w for w, p in zip(positions, produced) if p]
    assert a["rank"] == [sum(produced[:k]) for k in range(len(positions) + 1)]
    assert a["n_windows"] == (len(positions) + window - 1) // window
    want_mask = [0] * ((n_witnesses + 31) // 32)
    for w in positions:
        if w < n_witnesses:
            want_mask[w >> 5] |= 1 << (w & 31)
    assert a["mask"] == want_mask
    if a["container"] == GZIP:
        assert a["x64"] == _x_pow_bytes(8)
        assert len(a["pow"]) == len(positions) + 1
        for k in sorted({0, min(1, len(positions)), min(2, len(positions)), len(positions) // 2, len(positions)}):
            assert a["pow"][k] == _x_pow_bytes(76 * k), k
    else:
        assert a["pow"] == []


def test_entries_ranks_mask_and_powers(tool):
    window = int(tool(["window"])[0])
    rng = random.Random(0x31BE1001)
    cases = [(40, [], None), (40, [0, 7, 39], None), (1, [], None), (0, [], None), (33, [32], None), (64, list(range(64)), None),
             (40, [0, 7, 39], [0, 3, 6, 7, 9, 38, 39, 40, 41, 5000]),       # a list with holes, unproduced witnesses and witnesses beyond the circuit
             (40, [], [39]), (40, [5], [5]), (2000, rng.sample(range(2000), 300), None),
             (2000, rng.sample(range(2000), 300), sorted(rng.sample(range(2100), 700)))]
    for container in (BINCODE, GZIP):
        commands = ["live 65"]
        for nw, un, ws in cases:
            commands += [circuit_command(nw, un), wire_command(container=container, witnesses=ws)]
        for (nw, un, ws), line in zip(cases, tool(commands)):
            a = parse(line)
            assert isinstance(a, dict), a
            _check_plan(a, nw, set(un), ws, window)


def test_bound_lengths_and_offsets_against_the_model(tool):
    ns = [0, 1, 2, 861, 862, 863, 864, 1724, 1725, 1726, 5000, 10017, 1 << 26]
    ks = [0, 7, 8, 65531, 65532, 65533, 131063, 131064, 3 * 65532 - 1, 3 * 65532, 1 << 33]
    commands = ["%s %d %d" % (what, c, n) for what in ("length", "bound") for c in (BINCODE, GZIP) for n in ns] + ["offset %d %d" % (c, k) for c in (BINCODE, GZIP) for k in ks]
    for cmd, got in zip(commands, tool(commands)):
        what, c, v = cmd.split()
        want = {"length": wire_ref.length, "bound": wire_ref.bound, "offset": wire_ref.body_offset}[what](int(c), int(v))
        assert int(got) == want, cmd
    # the lengths are those of the bytes the model builds, and the boundaries fall where the framing says: 862 entries fill one block but 12 bytes
    for n in (0, 1, 862, 863, 1724, 1725):
        m = {w: w for w in range(n)}
        for c in (BINCODE, GZIP):
            assert len(wire_ref.encode(m, c)) == wire_ref.length(c, n)
    assert [wire_ref.n_blocks(8 + 76 * n) for n in (862, 863, 1724, 1725)] == [1, 2, 2, 3]
    # every body byte lies where the offset says
    body = wire_ref.body({w: w * w for w in range(1725)})
    member = wire_ref.member(body)
    for k in [0, 8, 100] + [b * 65532 + d for b in (1, 2) for d in (-1, 0, 1)] + [len(body) - 1]:
        assert member[wire_ref.body_offset(GZIP, k)] == body[k]
