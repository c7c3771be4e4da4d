"""The deflating container's part of the wire plan (acvm_amd/csrc/wire_plan.cpp) without a device: tools/wire_deflate_plan_host_test.cpp compiled
as plain C++ -- once as it is, once with AddressSanitizer and UndefinedBehaviorSanitizer as `make asan` builds it, a stand-alone program either
way -- and judged by tests/wire_deflate_ref.py: the code tables, the constant header, the bound, the device's table, the completeness of the
literal/length code, the match-versus-literals inequality, and wire_plan()'s word on containers 0, 1, 2 and 8."""
import os
import subprocess

import pytest

import wire_deflate_ref as ref
import wire_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    sources = [os.path.join(ROOT, "tools", "wire_deflate_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "wire_plan.cpp")]
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("wire_deflate_plan") / "wire_deflate_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sources + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "wire_deflate_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/wire_deflate_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _ints(line):
    return [int(x) for x in line.split()]


def test_code_tables_are_the_models(tool):
    lit, match, lengths, kraft = (_ints(x) for x in tool(["lit", "match", "lengths", "kraft"]))
    assert kraft == [1 << 15]  # the literal/length code is complete: zlib rejects a block whose code is not
    assert lengths == ref.litlen_lengths()
    want = ref.MODEL.litlen
    assert len(lit) == 2 * 257
    for s in range(257):
        code, n = want[s]
        assert (lit[2 * s], lit[2 * s + 1]) == (ref.reverse(code, n), n), s
    assert len(match) == 2 * 74
    for k, n in enumerate(range(3, 77)):
        s, eb, extra = ref.length_symbol(n)
        code, bits = want[s]
        assert bits == 7 and (match[2 * k], match[2 * k + 1]) == (ref.reverse(code, 7) | extra << 7, 7 + eb), n


def test_header_words_and_device_table(tool):
    header, table = (_ints(x) for x in tool(["header", "table"]))
    acc, n = ref.MODEL.header()
    assert header[0] == n == ref.HEADER_BITS and len(header) - 1 == (n + 31) // 32
    assert sum(w << (32 * k) for k, w in enumerate(header[1:])) == acc
    prefix_bits, words = table[0], table[1:]
    assert prefix_bits == 88 + n and len(words) == 346
    lit = _ints(tool(["lit"])[0])
    assert words[:257] == [lit[2 * s] | lit[2 * s + 1] << 16 for s in range(257)]
    assert words[257:260] == [0, 0, 0] and words[257 + 76] >> 16 == 7 + 4
    prefix = sum(w << (32 * k) for k, w in enumerate(words[334:]))
    assert prefix == int.from_bytes(ref.HEADER, "little") | acc << 88
    # the prefix is how every member starts
    member = ref.encode({3: 5})
    assert int.from_bytes(member[:48], "little") & ((1 << prefix_bits) - 1) == prefix


def test_match_never_costs_more_than_its_literals(tool):
    rows = _ints(tool(["inequality"])[0])
    seen = set()
    for n, distance, bits, literal_bits in zip(*[iter(rows)] * 4):
        b = ref.Bits()
        ref.MODEL.token_bits(b, ("match", n, distance))
        assert bits == b.n <= literal_bits == 5 * n and bits <= 17
        seen.add((n, distance))
    assert seen == {(n, d) for n in range(3, 77) for d in (1, 76)}  # exhaustively: every length times both distances


def test_bound(tool):
    ns = [0, 1, 2, 7, 8, 9, 100, 863, 10017, 1 << 27]
    for n, got in zip(ns, tool(["bound 8 %d" % n for n in ns])):
        assert int(got) == ref.bound(ref.GZIP_DEFLATE, n) and int(got) % 16 == 0
    assert (1 << 27) * 440 > 1 << 32  # why the bit position within a row is 64-bit
    for c in (0, 1):
        for n, got in zip(ns, tool(["bound %d %d" % (c, n) for n in ns])):
            assert int(got) == wire_ref.bound(c, n)  # containers 0 and 1 as before


def test_wire_plan_on_every_container(tool):
    nw = 100
    got = tool(["plan %d %d - 0" % (c, nw) for c in (0, 1, 2, 8, 3, 9)])
    assert got[0].split() == ["ok", "0", str(wire_ref.bound(0, nw)), str(wire_ref.bound(0, nw)), "100", "13", "0", "0", "0"]
    assert got[1].split() == ["ok", "1", str(wire_ref.bound(1, nw)), str(wire_ref.bound(1, nw)), "100", "13", "101", "0", "0"]
    assert got[2] == "err -1 unknown container 2" and got[4] == "err -1 unknown container 3" and got[5] == "err -1 unknown container 9"
    bound = ref.bound(ref.GZIP_DEFLATE, nw)
    assert got[3].split() == ["ok", "8", str(bound), str(bound), "100", "13", "101", "346", str(88 + ref.HEADER_BITS)]
    listed = ref.bound(ref.GZIP_DEFLATE, 5)
    lines = tool(["plan 8 %d 5 0" % nw, "plan 8 %d 5 %d" % (nw, listed - 16), "plan 8 %d 5 %d" % (nw, listed + 8), "plan 8 %d 5 %d" % (nw, listed + 48)])
    assert lines[0].split()[2:6] == [str(listed), str(listed), "5", "1"]
    assert lines[1] == "err -1 pitch %d is below the bound %d (acvm_batch_wire_bound)" % (listed - 16, listed)
    assert "not a multiple of 16" in lines[2] and lines[3].split()[2:4] == [str(listed + 48), str(listed)]
