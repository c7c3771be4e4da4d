"""The checks, the key table, the CRC power table and the host form's judgement of a row of the batch-wide wire import
(acvm_amd/csrc/wire_in_plan.cpp) without a device and without a handle: the module is compiled as plain C++ (tools/wire_in_plan_host_test.cpp) --
once as it is, once with AddressSanitizer and UndefinedBehaviorSanitizer as `make asan` builds it, a stand-alone program either way -- and its
answers are judged by tests/wire_ref.py, tests/wire_in_cases.py and zlib. The refusals are those tests/test_gpu_wire_in.py asserts on the device."""
import os
import random
import subprocess
import zlib

import pytest

import wire_in_cases as wc
import wire_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 1 << 20
BINCODE, GZIP = 0, 1
IDS = [2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 17, 18]
VALUES = [(0x1234567890 << (8 * k)) + k for k in range(len(IDS))]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    sources = [os.path.join(ROOT, "tools", "wire_in_plan_host_test.cpp")] + [os.path.join(ROOT, "acvm_amd", "csrc", f) for f in ("wire_in_plan.cpp", "wire_plan.cpp")]
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("wire_in_plan") / "wire_in_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sources + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "wire_in_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/wire_in_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith(("live", "nolive", "ids")) for c in commands)
        return lines
    return run


def ids_command(ids):
    return "ids %d" % len(ids) + "".join(" %d" % w for w in ids)


def plan_command(container=GZIP, pitch=1024, ptr=PTR, device=1):
    return "plan %d %d %d %d" % (container, pitch, ptr, device)


def test_the_powers_model_is_the_export_plans(tool):
    """the reader's power table is the writer's function: entry k advances a raw CRC over k entries of 76 zero bytes"""
    rng = random.Random(0x31BE4000)
    raw = lambda d: zlib.crc32(d) ^ zlib.crc32(bytes(len(d)))
    line = tool(["live 4", ids_command(list(range(1, 41))), plan_command()])[0].split()
    pows = [int(x) for x in line[7 + 80 + 1:]]
    assert int(line[7 + 80]) == 41 == len(pows) and pows[0] == 0x80000000
    mul = _mul
    for k in (1, 2, 20, 40):
        d = bytes(rng.randrange(256) for _ in range(76))
        assert mul(pows[k], raw(d)) == raw(d + bytes(76 * k)), k
    assert mul(int(line[6]), raw(b"abcd")) == raw(b"abcd" + bytes(8))  # x^64


def _mul(a, b):
    """a * b mod P, reflected: bit 31 is x^0"""
    p = 0
    for k in range(31, -1, -1):
        if (a >> k) & 1:
            p ^= b
        b = (b >> 1) ^ (0xEDB88320 if b & 1 else 0)
    return p


# ---- the refusals, one by one
@pytest.mark.parametrize("case", [
    ("an unknown container", dict(container=2), "unknown container 2"),
    ("pitch 0", dict(pitch=0), "pitch 0"),
    ("pitch 8", dict(pitch=8), "pitch 8 is not a multiple of 16"),
    ("a pitch that is no multiple of 16", dict(pitch=1032), "is not a multiple of 16"),
    ("a misaligned buffer", dict(ptr=PTR + 8), "the buffer is not aligned to 16 bytes"),
    ("a null buffer while B > 0", dict(ptr=0), "null buffer"),
    ("B * pitch beyond any buffer", dict(pitch=((1 << 57) // 65 + 16) // 16 * 16), "is beyond any device buffer"),
], ids=lambda c: c[0])
def test_refusal(tool, case):
    _, args, text = case
    line = tool(["live 65", ids_command(IDS), plan_command(**args)])[0]
    assert line.startswith("err -1 ") and text in line, line


def test_refusals_of_the_arguments_themselves(tool):
    lines = tool(["live 65", ids_command(IDS), "plan null", "nolive", plan_command()])
    assert lines == ["err -1 null argument", "err -1 null batch"]
    assert tool(["live 0", ids_command([]), plan_command(ptr=0)])[0].startswith("ok ")  # nothing to read: a null buffer is fine


def test_what_is_accepted_and_the_key_table(tool):
    rng = random.Random(0x31BE4001)
    for ids in ([], [7], IDS, list(reversed(IDS)), rng.sample(range(1, 5000), 870), [(1 << 32) - 1, 0]):
        for container in (BINCODE, GZIP):
            for kw in (dict(), dict(pitch=16), dict(ptr=PTR + 3, device=0, pitch=77), dict(pitch=0, device=0)):
                tok = tool(["live 130", ids_command(ids), plan_command(container=container, **kw)])[0].split()
                assert tok[0] == "ok", tok[:8]
                n = len(ids)
                got_container, pitch, n_initial, n_windows, rank_bits = (int(x) for x in tok[1:6])
                assert (got_container, pitch, n_initial, n_windows) == (container, kw.get("pitch", 1024), n, (n + 7) // 8)
                assert (1 << rank_bits) >= max(n, 1) and (rank_bits == 0 or (1 << (rank_bits - 1)) < n)
                keys, positions = [int(x) for x in tok[7:7 + n]], [int(x) for x in tok[7 + n:7 + 2 * n]]
                assert keys == sorted(ids) and [ids[p] for p in positions] == keys
                assert int(tok[7 + 2 * n]) == (n + 1 if container == GZIP else 0) and len(tok) == 8 + 2 * n + int(tok[7 + 2 * n])


def _hex(b):
    return b.hex() if b else "-"


def test_the_canonical_shape(tool):
    rng = random.Random(0x31BE4002)
    good = [wc.good_row(m, BINCODE, case, seed=3) for case in ("lower", "upper", "mixed")
            for m in ({}, dict(zip(IDS, VALUES)), {IDS[0]: 0}, {w: rng.randrange(1 << 256) for w in IDS[1::3]})]
    bad = [b.row for b in wc.bad_rows(IDS, VALUES, BINCODE, 8)]
    full = wc.good_row(dict(zip(IDS, VALUES)), BINCODE)
    bad += [b"", full[:7], full[:-1], full + b"\x00", full[:8 + 76 * 3], wc.good_row({1: 5}, BINCODE), wire_ref.member(full)]
    lines = tool([ids_command(IDS)] + ["canonical " + _hex(r) for r in good + bad])
    assert lines == ["1"] * len(good) + ["0"] * len(bad)
    for r in good:  # what the host form calls canonical is what the device form finds nothing in
        assert wc.findings(wc.slots([r], wire_ref.bound(BINCODE, len(IDS))), BINCODE, IDS) == []


def test_a_map_from_the_reader_becomes_a_canonical_body(tool):
    value = lambda v: v.to_bytes(32, "big").hex()
    cases = [
        ([], {}),
        ([(IDS[3], 7)], {IDS[3]: 7}),
        ([(IDS[5], 1), (IDS[0], 2), (IDS[5], 3), (IDS[11], wc.P - 1)], {IDS[0]: 2, IDS[5]: 3, IDS[11]: wc.P - 1}),  # unordered, repeated: last one wins
        (list(zip(reversed(IDS), VALUES)), dict(zip(reversed(IDS), VALUES))),
    ]
    commands = [ids_command(IDS)] + ["ofmap %d" % len(m) + "".join(" %d %s" % (w, value(v)) for w, v in m) for m, _ in cases]
    for (_, want), got in zip(cases, tool(commands)):
        assert got == "ok " + wire_ref.body(want).hex()
    lines = tool([ids_command(IDS), "ofmap 2 %d %s %d %s" % (IDS[0], value(1), 4, value(2)), "ofmap 1 %d %s" % ((1 << 32) - 1, value(0))])
    assert lines == ["err -1 witness 4 is not an initial witness of this handle", "err -1 witness 4294967295 is not an initial witness of this handle"]
    assert [int(x) for x in tool(["stagepitch 0", "stagepitch 1", "stagepitch 12", "stagepitch 870"])] == [wire_ref.bound(BINCODE, n) for n in (0, 1, 12, 870)]
