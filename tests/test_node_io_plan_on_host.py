"""The checks and the tile views of acvm_node_solve_device (acvm_amd/csrc/node_io_plan.cpp) without a device and without a node: the module is
compiled as plain C++ (tools/node_io_plan_host_test.cpp), once as it is and once through `make asan`, and its answers -- the checked lanes, a
tile's pointers and strides, or the refusal with its code and text -- are judged by the Python restatement below. The refusals are those
tests/test_gpu_node_device.py asserts on a real node, with the same texts."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BE32, LE32, MONT, U8, U16, U32, U64, U128 = 0, 1, 2, 16, 17, 18, 19, 20
ENCODINGS = (BE32, LE32, MONT, U8, U16, U32, U64, U128)
IM, WM, BC = 0, 1, 16
PTR = 1 << 30  # a device address aligned to everything
SOURCES = [os.path.join(ROOT, "tools", "node_io_plan_host_test.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "node_io_plan.cpp"), os.path.join(ROOT, "acvm_amd", "csrc", "import_plan.cpp")]


def size_of(encoding):
    return 1 << (encoding - U8) if U8 <= encoding <= U128 else 32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    """the tool compiled as it is, and the second binary of `make asan` (AddressSanitizer + UndefinedBehaviorSanitizer): a stand-alone program on
    the CPU, given the same command streams -- a report ends it with a non-zero status"""
    if request.param == "plain":
        exe = str(tmp_path_factory.mktemp("node_io_plan") / "node_io_plan_host_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall"] + SOURCES + ["-o", exe])
    else:
        exe = os.path.join(ROOT, "tools", "asan", "node_io_plan_host_test")
        r = subprocess.run(["make", "-C", ROOT, "tools/asan/node_io_plan_host_test"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == sum(not c.startswith("shape") for c in commands)
        return lines
    return run


def fmt(lst):
    return "null" if lst is None else "e" if not len(lst) else ",".join(str(x) for x in lst)


def lane(n, values=PTR, encoding=BE32, layout=IM, n_columns=0, stride=0, columns=None, kept=2 * PTR, mask=3 * PTR, kept_encoding=BE32, kept_layout=IM, kept_stride=0,
         status=4 * PTR, err=5 * PTR, opcode=6 * PTR, digests=7 * PTR):
    return dict(n=n, values=values, encoding=encoding, layout=layout, n_columns=n_columns, stride=stride, columns=columns, kept=kept, mask=mask, kept_encoding=kept_encoding,
                kept_layout=kept_layout, kept_stride=kept_stride, status=status, err=err, opcode=opcode, digests=digests)


def check_command(lanes, n_expected=None):
    return "check %d %d " % (len(lanes) if n_expected is None else n_expected, len(lanes)) + " ".join(
        "%d %d %d %d %d %d %s %d %d %d %d %d %d %d %d %d" % (l["n"], l["values"], l["encoding"], l["layout"], l["n_columns"], l["stride"], fmt(l["columns"]), l["kept"], l["mask"],
                                                            l["kept_encoding"], l["kept_layout"], l["kept_stride"], l["status"], l["err"], l["opcode"], l["digests"]) for l in lanes)


def refusal(line):
    assert line.startswith("err "), line
    code, text = line[4:].split(" ", 1)
    assert int(code) == -1, line  # ACVM_E_INVALID
    return text


def parse_check(line):
    tok = line.split()
    assert tok[0] == "ok", line
    return [tuple(int(x) for x in tok[2 + 7 * q:9 + 7 * q]) for q in range(int(tok[1]))]  # in stride, in size, kept, mask, kept stride, kept size, tiles


# ---- 1. every refusal, with its code and text
def test_refusals_name_the_lane(tool):
    n_in, n_keep, tile = 5, 3, 64
    good = lane(150)
    cases = [
        (lane(1 << 32), "n 4294967296 is not below 2^32"),
        (lane((1 << 40) + 7), "n 1099511627783 is not below 2^32"),
        (lane(150, values=0), "input: null values"),
        (lane(150, stride=n_in - 1), "input: stride 4 is below the dense stride 5 of the layout"),
        (lane(150, layout=WM, stride=149), "input: stride 149 is below the dense stride 150 of the layout"),  # (against the LANE's n, not the tile)
        (lane(150, layout=WM, stride=tile), "input: stride 64 is below the dense stride 150 of the layout"),
        (lane(150, columns=[0, 1, 2, 3, 7], n_columns=7), "input: column 7 of initial witness 4 is not below n_columns 7"),
        (lane(150, columns=[0, 1, 2, 3, 4], n_columns=7, stride=6), "input: stride 6 is below the dense stride 7 of the layout"),
        (lane(150, encoding=3), "input: unknown encoding 3"),
        (lane(150, encoding=21), "input: unknown encoding 21"),
        (lane(150, layout=2), "input: unknown layout 2"),
        (lane(150, layout=BC), "input: unknown layout 16"),
        (lane(150, encoding=LE32, values=PTR + 8), "input: d_values must be 16-byte aligned"),
        (lane(150, encoding=U32, layout=WM, values=PTR + 2), "input: d_values must be aligned to the element size, 4 bytes"),
        (lane(150, stride=(1 << 57) + 1), "input: stride %d is beyond any device buffer" % ((1 << 57) + 1)),
        (lane(150, kept_encoding=15), "kept: unknown encoding 15"),
        (lane(150, kept_layout=BC), "kept: unknown layout 16"),
        (lane(150, kept_encoding=MONT, kept=2 * PTR + 8), "kept: d_values must be 16-byte aligned"),
        (lane(150, kept_encoding=U64, kept=2 * PTR + 4), "kept: d_values must be aligned to the element size, 8 bytes"),
        (lane(150, kept_stride=n_keep - 1), "kept: stride 2 is below the dense stride 3 of the layout"),
        (lane(150, kept_layout=WM, kept_stride=149), "kept: stride 149 is below the dense stride 150 of the layout"),
        (lane(150, kept_layout=WM, kept_stride=(1 << 57) // 3 + 1), "kept: stride %d is beyond any device buffer" % ((1 << 57) // 3 + 1)),
        (lane(150, kept_stride=(1 << 57) // 150 + 1), "kept: stride %d is beyond any device buffer" % ((1 << 57) // 150 + 1)),
        (lane(150, kept=0), "kept: d_kept_assigned without d_kept"),
    ]
    commands = ["shape %d %d %d" % (n_in, n_keep, tile)]
    for bad, _ in cases:
        commands += [check_command([bad]), check_command([good, good, bad])]
    lines = tool(commands)
    for q, (_, text) in enumerate(cases):
        assert refusal(lines[2 * q]) == "lane 0: " + text
        assert refusal(lines[2 * q + 1]) == "lane 2: " + text
    # the first refused lane wins; the number of lanes is judged first, then the array
    lines = tool(commands[:1] + [check_command([good, cases[3][0], cases[0][0]]), check_command([good, good], n_expected=3), check_command([], n_expected=1),
                                 "check 2 null 2", check_command([cases[0][0]], n_expected=2)])
    assert [refusal(l) for l in lines] == ["lane 1: " + cases[3][1], "n_lanes 2 is not the node's number of handles, 3", "n_lanes 0 is not the node's number of handles, 1",
                                           "null argument", "n_lanes 1 is not the node's number of handles, 2"]


def test_what_is_not_refused(tool):
    n_in, n_keep, tile = 5, 3, 64
    nothing = dict(values=0, kept=0, mask=0, status=0, err=0, opcode=0, digests=0)
    lines = tool(["shape %d %d %d" % (n_in, n_keep, tile),
                  check_command([lane(0, **nothing), lane(0, encoding=99, layout=7, kept_encoding=99, kept_stride=1, values=3, kept=5)]),  # an idle lane: nothing of it is read
                  check_command([lane(150, **dict(nothing, values=PTR + 1))]),                    # every output NULL; the plain input shape reads any pointer
                  check_command([lane(150, mask=0, kept_encoding=U8, kept=2 * PTR + 1)]),         # kept without a mask; U8 takes any pointer
                  check_command([lane((1 << 32) - 1, layout=WM, kept_layout=WM)]),                # the largest lane
                  check_command([lane(150, kept_stride=(1 << 57) // 150), lane(150, kept_layout=WM, kept_stride=(1 << 57) // 3)]),
                  "shape 0 0 64",
                  check_command([lane(150, values=0, kept=0, mask=5)])])                          # no initial witnesses, nothing kept: neither buffer is looked at
    got = [parse_check(l) for l in lines]
    assert [g[6] for g in got[0]] == [0, 0]
    assert got[1][0] == (n_in, 32, 0, 0, 0, 32, 3)
    assert got[2][0][2:6] == (2 * PTR + 1, 0, n_keep, 1)
    assert got[3][0] == ((1 << 32) - 1, 32, 2 * PTR, 3 * PTR, (1 << 32) - 1, 32, 1 << 26)
    assert got[5][0][2:4] == (0, 0) and got[5][0][6] == 3


# ---- 2. the address rule: the tile's view of element (i', c) is the lane's element (k * tile + i', c)
def address(base, layout, stride, i, c, size):
    """include/acvm_amd.h: element (i, c) at (i * stride + c) * size instance-major, (c * stride + i) * size witness-major"""
    return base + ((c * stride + i) if layout == WM else (i * stride + c)) * size


def test_random_tiles_address_the_lanes_elements(tool):
    rng = random.Random(0x90DE10)
    commands, cases = [], []
    for _ in range(120):
        n_in, n_keep, tile = rng.randrange(1, 7), rng.randrange(1, 6), rng.choice((1, 3, 64, 100, 512))
        n = rng.choice((1, 3, tile - 1 or 1, tile, tile + 1, 2 * tile, 3 * tile + rng.randrange(tile), rng.randrange(1, 5000)))
        e_in, l_in, e_k, l_k = rng.choice(ENCODINGS), rng.choice((IM, WM)), rng.choice(ENCODINGS), rng.choice((IM, WM))
        has = rng.random() < 0.5
        n_columns = n_in + rng.randrange(4) if has else 0
        cols = [rng.randrange(n_columns) for _ in range(n_in)] if has else None
        dense_in = n if l_in == WM else (n_columns if has else n_in)
        dense_k = n if l_k == WM else n_keep
        s_in, s_k = rng.choice((0, dense_in, dense_in + rng.randrange(1, 9))), rng.choice((0, dense_k, dense_k + rng.randrange(1, 9)))
        ln = lane(n, values=PTR + 64 * rng.randrange(4), encoding=e_in, layout=l_in, n_columns=n_columns, stride=s_in, columns=cols, kept=2 * PTR + 64 * rng.randrange(4),
                  mask=3 * PTR + rng.randrange(7), kept_encoding=e_k, kept_layout=l_k, kept_stride=s_k, status=4 * PTR + rng.randrange(7), err=5 * PTR + rng.randrange(7),
                  opcode=6 * PTR + 4 * rng.randrange(7), digests=7 * PTR + rng.randrange(7))
        n_tiles = (n + tile - 1) // tile
        ks = sorted({0, n_tiles - 1, rng.randrange(n_tiles)})
        commands += ["shape %d %d %d" % (n_in, n_keep, tile), check_command([lane(0), ln])] + ["tile 1 %d" % k for k in ks] + ["tile 1 %d" % n_tiles]
        cases.append((n_in, n_keep, tile, ln, s_in or dense_in, s_k or dense_k, n_tiles, ks, cols))
    lines = iter(tool(commands))
    for n_in, n_keep, tile, ln, s_in, s_k, n_tiles, ks, cols in cases:
        checked = parse_check(next(lines))[1]
        assert checked == (s_in, size_of(ln["encoding"]), ln["kept"], ln["mask"], s_k, size_of(ln["kept_encoding"]), n_tiles)
        for k in ks:
            tok = next(lines).split()
            assert tok[0] == "ok"
            first, m, values, t_s_in, kept, mask, t_s_k, status, err, opcode, digests = (int(x) for x in tok[1:])
            assert first == k * tile and m == min(tile, ln["n"] - first) and m >= 1
            columns = cols if cols is not None else list(range(n_in))
            for i in {0, m - 1, rng.randrange(m)}:
                for c in columns:
                    assert address(values, ln["layout"], t_s_in, i, c, size_of(ln["encoding"])) == address(ln["values"], ln["layout"], s_in, first + i, c, size_of(ln["encoding"]))
                for c in range(n_keep):
                    assert address(kept, ln["kept_layout"], t_s_k, i, c, size_of(ln["kept_encoding"])) == address(ln["kept"], ln["kept_layout"], s_k, first + i, c, size_of(ln["kept_encoding"]))
                    assert address(mask, ln["kept_layout"], t_s_k, i, c, 1) == address(ln["mask"], ln["kept_layout"], s_k, first + i, c, 1)
                assert status + i == ln["status"] + first + i and err + i == ln["err"] + first + i
                assert opcode + 4 * i == ln["opcode"] + 4 * (first + i) and digests + 32 * i == ln["digests"] + 32 * (first + i)
            # the tile's strides pass the batch's own checks for m live instances: at least the dense stride of the tile
            assert t_s_in >= (m if ln["layout"] == WM else 1) and t_s_k >= (m if ln["kept_layout"] == WM else n_keep)
        assert refusal(next(lines)) == "tile %d is not below the lane's %d tiles" % (n_tiles, n_tiles)


def test_null_outputs_stay_null_in_every_tile(tool):
    lines = tool(["shape 2 2 64", check_command([lane(200, kept=0, mask=0, status=0, err=0, opcode=0, digests=0)]), "tile 0 0", "tile 0 3"])
    for line in lines[1:]:
        tok = [int(x) for x in line.split()[1:]]
        assert tok[4:6] == [0, 0] and tok[7:] == [0, 0, 0, 0] and tok[2] != 0


# ---- 3. offsets are 64-bit and overflow is refused
def test_overflowing_offsets_are_refused(tool):
    cases = [(IM, 3, 64, 7, 32), (WM, 3, 64, 7, 32), (IM, (1 << 26) - 1, 64, 1 << 20, 32), (IM, 1 << 32, 1 << 32, 1, 1), (WM, 1 << 32, 1 << 32, 1, 1), (IM, 1 << 20, 1 << 20, 1 << 24, 1),
             (IM, 1 << 20, 1 << 20, (1 << 24) - 1, 1), (WM, 1 << 31, 1 << 31, 1 << 63, 4), (WM, 1 << 31, 1 << 31, 1 << 63, 3), (IM, 0, 1 << 63, 1 << 63, 1 << 63)]
    lines = tool(["offset %d %d %d %d %d" % c for c in cases])
    for (layout, k, tile, stride, size), line in zip(cases, lines):
        want = k * tile * (1 if layout == WM else stride) * size
        assert line == ("ok %d" % want if want < 1 << 64 else "overflow"), (layout, k, tile, stride, size)
    assert [l.split()[0] for l in lines] == ["ok", "ok", "ok", "overflow", "overflow", "overflow", "ok", "overflow", "ok", "ok"]
    # a base pointer near the top of the address space: the tile's address itself must fit
    top = (1 << 64) - 4096
    lines = tool(["shape 1 1 64", check_command([lane(200, kept_encoding=U8, kept=top, mask=0)]), "tile 0 0", "tile 0 3", check_command([lane(200, digests=top)]), "tile 0 1", "tile 0 2"])
    assert lines[1].startswith("ok ") and lines[2].startswith("ok ") and lines[4].startswith("ok ")
    assert refusal(lines[5]) == "tile 2: a buffer's offset does not fit 64 bits"
