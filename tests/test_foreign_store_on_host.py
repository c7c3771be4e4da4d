"""The appending side of the foreign-call result store without a device: acvm_amd/csrc/foreign_store.hpp compiled for the host
(tools/foreign_store_host_test.hip runs what a lane of fc_append_kernel runs) against the layout batch_exact.cpp upload_fc_tables writes for the same
results, restated here: descriptor words [n_results, (n_values, (is_array, n) x n_values) x n_results] of instance j at desc[w * Bp + j], values as
rows x * 2^261 mod p in the order of the descriptor."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BE32, LE32, MONT, U8, U64 = 0, 1, 2, 16, 19


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def tool(request, tmp_path_factory):
    """the stand-alone host program, as it is and with the host code under AddressSanitizer + UndefinedBehaviorSanitizer: the tables and the caller's
    buffer are heap arrays of exactly the stated size, so a store or a load past an edge ends the program with a report"""
    exe = str(tmp_path_factory.mktemp("foreign_store") / "foreign_store_host_test")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17"] + flags + [os.path.join(ROOT, "tools", "foreign_store_host_test.hip"), "-o", exe])

    def run(commands):
        out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-400:] + out.stderr[-2000:]
        return out.stdout.split("\n")[:-1]
    return run


def fmt(lst):
    return "e" if not len(lst) else ",".join(str(int(x)) for x in lst)


def element(x, encoding):
    """the bytes of one element of the caller's buffer whose 256-bit string is x (any x < 2^256), and the field value the store must hold for it"""
    if encoding == BE32:
        return x.to_bytes(32, "big"), x % P
    if encoding == LE32:
        return x.to_bytes(32, "little"), x % P
    if encoding == MONT:
        return x.to_bytes(32, "little"), x * pow(1 << 256, -1, P) % P
    size = 1 << (encoding - U8)
    x %= 1 << (8 * size)
    return x.to_bytes(size, "little"), x


def append_command(j, encoding, shape, xs):
    """shape: None for a single value, else the array's length; xs: one integer per value"""
    els = [element(x, encoding) for x in xs]
    cmd = "append %d %d %s %s %s" % (j, encoding, fmt([0 if s is None else 1 for s in shape]), fmt([5 if s is None else s for s in shape]),
                                     ",".join(b.hex() for b, _ in els) or "e")
    return cmd, [v for _, v in els]


class Column:
    """what upload_fc_tables writes for the results of one instance"""

    def __init__(self):
        self.results = []

    def words(self):
        out = [len(self.results)]
        for shape, _ in self.results:
            out.append(len(shape))
            for s in shape:
                out += [0, 1] if s is None else [1, s]
        return out

    def values(self):
        return [v for _, vals in self.results for v in vals]


def random_shape(rng):
    return tuple(rng.choice((None, None, 0, 1, 2, 3)) for _ in range(rng.randrange(0, 4)))


@pytest.mark.parametrize("Bp", [1, 64, 65])
def test_appends_build_the_layout_of_the_host_store(tool, Bp):
    rng = random.Random(0x5707E + Bp)
    desc_words, vals_cap = 48, 24
    columns = {j: Column() for j in sorted({0, Bp - 1, rng.randrange(Bp), rng.randrange(Bp)})}
    commands, checks = ["new %d %d %d" % (Bp, desc_words, vals_cap)], []
    for k in range(5):
        for j, col in columns.items():
            if rng.random() < 0.25:
                continue  # columns grow at different rates: the walk is per instance
            shape = random_shape(rng)
            n = sum(1 if s is None else s for s in shape)
            if len(col.words()) + 1 + 2 * len(shape) > desc_words or len(col.values()) + n > vals_cap:
                continue
            enc = rng.choice((BE32, LE32, MONT, U8, U64))
            xs = [rng.choice((rng.randrange(1 << 256), P, P + 1, (1 << 256) - 1, 0, rng.randrange(300))) for _ in range(n)]
            cmd, vals = append_command(j, enc, shape, xs)
            commands.append(cmd)
            checks.append("ok %d %d %d" % (len(col.words()), len(col.values()), len(col.results)))  # the walk positions equal the Python ones
            col.results.append((shape, vals))
    for j, col in columns.items():
        commands += ["walk %d" % j, "column %d" % j, "values %d %d" % (j, vals_cap)]
    # a column nobody appended to stays empty
    untouched = next((j for j in range(Bp) if j not in columns), None)
    if untouched is not None:
        commands += ["walk %d" % untouched, "column %d" % untouched]
    lines = tool(commands)
    assert lines[:len(checks)] == checks
    at = len(checks)
    assert any(len(c.results) >= 2 for c in columns.values())
    for j, col in columns.items():
        assert lines[at] == "%d %d %d" % (len(col.words()), len(col.values()), len(col.results))
        assert [int(x) for x in lines[at + 1].split()] == col.words() + [0] * (desc_words - len(col.words())), j
        got = [int(x, 16) for x in lines[at + 2].split()]
        want = [v * (1 << 261) % P for v in col.values()]
        assert got == want + [0] * (vals_cap - len(want)), j
        at += 3
    if untouched is not None:
        assert lines[at] == "1 0 0" and [int(x) for x in lines[at + 1].split()] == [0] * desc_words


def test_an_append_at_the_capacity_edge_is_refused_not_written(tool):
    # 8 descriptor words, 3 values: [count] + (1 + 2) + (1 + 2) fills 7 words and 2 values
    commands = ["new 65 8 3"]
    commands.append(append_command(64, BE32, (None,), [7])[0])
    commands.append(append_command(64, BE32, (None,), [8])[0])
    commands += ["column 64", "values 64 3"]
    before = len(commands)
    commands.append(append_command(64, BE32, (None,), [9])[0])             # 3 more words: past the descriptor
    commands.append(append_command(64, BE32, (), [])[0])                   # 1 more word: fits exactly
    commands.append(append_command(64, BE32, (), [])[0])                   # and the next does not
    commands += ["column 64", "values 64 3", "walk 64"]
    commands += ["new 65 16 3", append_command(3, LE32, (2,), [1, 2])[0], append_command(3, LE32, (2,), [3, 4])[0],  # 4 values into 3: refused
                 append_command(3, LE32, (1,), [5])[0], append_command(3, LE32, (None,), [6])[0], "column 3", "values 3 3", "column 2", "column 4"]
    lines = tool(commands)
    assert lines[:2] == ["ok 1 0 0", "ok 4 1 1"]
    assert lines[2] == "2 1 0 1 1 0 1 0"
    full = lines[3]
    assert lines[before - 1:before + 2] == ["refused 7 2 2", "ok 7 2 2", "refused 8 2 3"]
    assert lines[before + 2] == "3 1 0 1 1 0 1 0" and lines[before + 3] == full and lines[before + 4] == "8 2 3"
    rest = lines[before + 5:]
    assert rest[:4] == ["ok 1 0 0", "refused 4 2 1", "ok 4 2 1", "refused 7 3 2"]
    assert [int(x) for x in rest[4].split()] == [2, 1, 1, 2, 1, 1, 1] + [0] * 9
    assert [int(x, 16) for x in rest[5].split()] == [v * (1 << 261) % P for v in (1, 2, 5)]
    assert [int(x) for x in rest[6].split()] == [0] * 16 and [int(x) for x in rest[7].split()] == [0] * 16  # the neighbours' columns are untouched
