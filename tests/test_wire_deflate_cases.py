"""What tests/wire_deflate_cases.py covers, asserted with the model (tests/wire_deflate_ref.py): every match length with each distance that can
produce it, every length-code base and the length below it, ties, distance 1 inside a value, the edge values, the keys that move the
distance-76 run, the entry counts around the kernel's window, and every alignment a member can end at."""
import functools

import wire_deflate_cases as cases
import wire_deflate_ref as ref


@functools.lru_cache(maxsize=None)
def parsed():
    """per row: (the map, the body, its tokens)"""
    out = []
    for m in cases.rows() + cases.keyed_rows() + cases.count_rows():
        body = ref.body(m)
        out.append((m, body, ref.MODEL.tokens(body)))
    return out


def _matches(rows):
    return {t[1:] for _, _, tokens in rows for t in tokens if t[0] == "match"}


def test_every_match_length_with_each_distance_that_can_produce_it():
    n_case = cases.N_ROWS
    device_rows = parsed()[:n_case]  # the rows tests/test_gpu_wire_deflate.py runs as instances
    got = _matches(device_rows)
    # distance 76: a run cannot start at byte 0 and reach the end (two keys differ), so 75 is the longest; distance 1: a value has 64 digits
    assert {n for n, d in got if d == 76} >= set(range(3, 76)) and (76, 76) not in got
    assert {n for n, d in got if d == 1} >= set(range(3, 64))
    for base in ref.LENGTH_BASES:
        for n in (base - 1, base):
            if n >= 3:
                assert (n, 76) in got and (n > 63 or (n, 1) in got), n


def test_ties_runs_inside_a_value_and_edge_values():
    ties = far_inside = near_inside = 0
    for m, body, _ in parsed():
        prev = None
        for at in range(8, len(body), ref.ENTRY):
            cur, p = body[at:at + ref.ENTRY], 0
            for t in ref.MODEL.parse(cur, prev):
                if t[0] == "match":
                    l1 = 0
                    while p and p + l1 < ref.ENTRY and cur[p + l1] == cur[p + l1 - 1]:
                        l1 += 1
                    ties += t[2] == 76 and l1 == t[1]
                    far_inside += t[2] == 76 and p > 12
                    near_inside += t[2] == 1 and p > 12
                p += t[1] if t[0] == "match" else 1
            prev = cur
    assert ties >= 5 and far_inside >= 60 and near_inside >= 60
    values = {v for m, _, _ in parsed() for v in m.values()}
    assert {0, 1, cases.P - 1, int("0" + "a" * 63, 16), int("0" + "f" * 63, 16), int("12" * 32, 16), int("0a" * 32, 16)} <= values


def test_keys_move_the_start_of_the_distance_76_run():
    starts = set()
    for m in cases.keyed_rows():
        body = ref.body(m)
        prev = None
        for at in range(8, len(body), ref.ENTRY):
            cur, p = body[at:at + ref.ENTRY], 0
            for t in ref.MODEL.parse(cur, prev):
                if t[0] == "match" and t[2] == 76 and p < 12:
                    starts.add(p)
                p += t[1] if t[0] == "match" else 1
            prev = cur
    assert starts >= {0, 1, 2, 4}, starts  # w + 2^24 (three equal key bytes), w + 1, w + 256 and a carry, w + 2^16 / 2^24 behind the key


def test_entry_counts_and_alignments():
    w = cases.window()
    counts = [len(m) for m in cases.count_rows()]
    assert counts == [0, 1, w - 1, w, w + 1, 2 * w + 1, 600]
    lengths, bits, trailers = set(), set(), set()
    for m, body, _ in parsed():
        member = ref.member(body)
        n_bits = ref.MODEL.block(body)[1]
        lengths.add(len(member) % 4)
        bits.add(n_bits % 8)
        trailers.add((len(member) - 8) % 4)
    assert lengths == {0, 1, 2, 3} and trailers == {0, 1, 2, 3} and bits == set(range(8))  # (0: an end-of-block that ends exactly on a byte)
