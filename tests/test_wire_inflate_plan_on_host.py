"""The checks, the arena layout and the fixed-code tables of the gzip import (acvm_amd/csrc/wire_inflate_plan.cpp) without a device and without a
handle: the module is compiled as plain C++ (tools/wire_inflate_plan_host_test.cpp) -- once as it is, once with AddressSanitizer and
UndefinedBehaviorSanitizer as `make asan` builds it, a stand-alone program either way. The refusals are those tests/test_gpu_wire_inflate.py
asserts on the device; the fixed code is judged by RFC 1951 3.2.6 as tests/wire_inflate_ref.py restates it."""
import os
import subprocess

import pytest

import wire_inflate_ref as ref
import wire_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 1 << 20
DEFLATE = 8
LCNT, DCNT, LSYM, DSYM, HALFWORDS = 0, 16, 48, 336, 368


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    sources = [os.path.join(ROOT, "tools", "wire_inflate_plan_host_test.cpp")] + [os.path.join(ROOT, "acvm_amd", "csrc", f)
                                                                                 for f in ("wire_inflate_plan.cpp", "wire_in_plan.cpp", "wire_plan.cpp")]
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("wire_inflate_plan") / "wire_inflate_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + sources + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "wire_inflate_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/wire_inflate_plan_host_test"], capture_output=True, text=True)
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


def plan_command(container=DEFLATE, pitch=1024, ptr=PTR, device=1, host_row=0):
    return "plan %d %d %d %d %d" % (container, pitch, ptr, device, host_row)


def test_the_refusals_one_by_one(tool):
    ids = ids_command([1, 2, 3])
    for commands, message in ((["nolive", ids, plan_command()], "null batch"), (["live 4", ids, "plan null"], "null argument"),
                              (["live 4", ids, plan_command(container=0)], "container 0 is not ACVM_WIRE_GZIP_DEFLATE"),
                              (["live 4", ids, plan_command(container=1)], "container 1 is not ACVM_WIRE_GZIP_DEFLATE"),
                              (["live 4", ids, plan_command(container=9)], "container 9 is not ACVM_WIRE_GZIP_DEFLATE"),
                              (["live 4", ids, plan_command(pitch=0)], "pitch 0 is not a multiple of 16 above 0"),
                              (["live 4", ids, plan_command(pitch=1000)], "pitch 1000 is not a multiple of 16"),
                              (["live 4", ids, plan_command(pitch=1 << 60)], "is beyond any device buffer"),
                              (["live 4", ids, plan_command(ptr=0)], "null buffer"), (["live 4", ids, plan_command(ptr=PTR + 8)], "the buffer is not aligned to 16 bytes"),
                              (["live 4", ids, plan_command(ptr=0, device=0, pitch=77)], "null buffer"),
                              (["live %d" % ((1 << 27) + 1), ids, plan_command(pitch=16)], "more instances than a finding can name")):
        assert tool(commands) == ["err -1 " + message] or message in tool(commands)[0], message
    # the order: the container before the pitch before the buffer
    assert "container 0" in tool(["live 4", ids, plan_command(container=0, pitch=8, ptr=0)])[0]
    assert "pitch 8 " in tool(["live 4", ids, plan_command(pitch=8, ptr=0)])[0]
    # what the host form does not ask for: a pitch of any kind, any alignment; nothing to read needs no buffer
    assert tool(["live 4", ids, plan_command(pitch=77, ptr=PTR + 3, device=0, host_row=70)])[0].startswith("ok 80 ")
    assert tool(["live 0", ids, plan_command(ptr=0)])[0].startswith("ok ")
    assert tool(["live %d" % (1 << 27), ids, plan_command(pitch=16)])[0].startswith("ok ")


@pytest.mark.parametrize("B,n_initial,device,host_row", [(1, 0, 1, 0), (4, 3, 1, 0), (65, 40, 1, 0), (130, 440, 1, 0), (4, 3, 0, 0), (65, 40, 0, 1), (65, 40, 0, 16), (130, 440, 0, 17001)])
def test_the_arena_layout(tool, B, n_initial, device, host_row):
    ids = list(range(5, 5 + 2 * n_initial, 2))
    line = tool(["live %d" % B, ids_command(ids), plan_command(pitch=1024, device=device, host_row=host_row)])[0].split()
    assert line[0] == "ok"
    pitch, out_pitch, out_cap, at_scratch, at_lengths, at_findings, at_tables, at_fixed, at_result, at_rows, at_row_lengths, front, body_container, body_pitch, body_n, n_keys = (int(x) for x in line[1:])
    assert out_cap == 8 + 76 * n_initial and out_pitch == wire_ref.bound(wire_ref.BINCODE, n_initial) and out_cap <= out_pitch < out_cap + 16 and out_pitch % 16 == 0
    assert pitch == (1024 if device else max((host_row + 15) // 16 * 16, 16))
    # the parts in order, each at a multiple of 256, none overlapping the next
    sizes = [B * out_pitch, B * 8, B * 8, B * 900, HALFWORDS * 2, 16, 0 if device else B * pitch, 0 if device else B * 8]
    starts = [at_scratch, at_lengths, at_findings, at_tables, at_fixed, at_result, at_rows, at_row_lengths, front]
    assert starts[0] == 0
    for k, size in enumerate(sizes):
        assert starts[k] % 256 == 0 and starts[k] + size <= starts[k + 1] < starts[k] + size + 256, (k, starts)
    # stage 2: the BINCODE body import over the scratch
    assert (body_container, body_pitch, body_n, n_keys) == (wire_ref.BINCODE, out_pitch, n_initial, n_initial)


def test_the_fixed_code_tables_against_the_rfc(tool):
    t = [int(x) for x in tool(["fixed"])[0].split()]
    assert len(t) == HALFWORDS
    for cnt, sym, lengths in ((LCNT, LSYM, ref.FIXED_LIT_LENGTHS), (DCNT, DSYM, ref.FIXED_DIST_LENGTHS)):
        left, _, counts, symbols = ref.canonical(lengths)
        assert left == 0
        assert t[cnt + 1:cnt + 16] == counts[1:] and t[sym:sym + len(symbols)] == symbols
    assert len(ref.FIXED_LIT_LENGTHS) == 288 and len(ref.FIXED_DIST_LENGTHS) == 32 and LSYM + 288 == DSYM and DSYM + 32 == HALFWORDS
    # RFC 1951 3.2.6 itself: 0 .. 143 have 8 bits from 00110000, 144 .. 255 9 bits from 110010000, 256 .. 279 7 bits from 0, 280 .. 287 8 bits from 11000000
    import wire_inflate_cases as cases
    codes = cases.codes_of(ref.FIXED_LIT_LENGTHS)
    assert codes[0] == (0b00110000, 8) and codes[143] == (0b10111111, 8) and codes[144] == (0b110010000, 9) and codes[255] == (0b111111111, 9)
    assert codes[256] == (0, 7) and codes[279] == (0b0010111, 7) and codes[280] == (0b11000000, 8) and codes[287] == (0b11000111, 8)
