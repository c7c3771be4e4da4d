"""tests/wire_in_cases.py pinned without a device: its good rows decode, through acvm_amd.decompress_witness, to the maps they were built from;
each of its malformed rows is rejected by decompress_witness or -- the shapes WitnessMap::try_from reads and the device form refuses by a
documented rule -- is read by it with another meaning than the device form would give; and the Python restatement of the device's judgement
(findings) names for every row the class and rank the case declares. This is how the lists tests/test_gpu_wire_in.py plants are shown to bite."""
import random

import pytest

import acvm_amd
import wire_in_cases as wc
import wire_ref
from wire_in_cases import BINCODE, GZIP_STORED, P

WINDOW = 8
IDS = [2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 17, 18]
VALUES = [(0x1234567890 << (8 * k)) + k for k in range(len(IDS))]
CONTAINERS = (BINCODE, GZIP_STORED)


@pytest.mark.parametrize("container", CONTAINERS)
@pytest.mark.parametrize("case", ["lower", "upper", "mixed"])
def test_good_rows_decode_to_their_maps(container, case):
    rng = random.Random(0x31BE3001)
    maps = [dict(zip(IDS, VALUES)), {}, {IDS[0]: 0}, {IDS[-1]: P - 1}, {w: rng.randrange(1 << 256) for w in IDS[::2]}, {IDS[3]: (1 << 256) - 1, IDS[7]: P}]
    for m in maps:
        row = wc.good_row(m, container, case, seed=len(m))
        assert acvm_amd.decompress_witness(wc.gz(row)) == wc.decoded(m)
        assert len(row) == wire_ref.length(container, len(m))
        for pitch in (wire_ref.bound(container, len(IDS)), wire_ref.bound(container, len(IDS)) + 48):
            slot = wc.slots([row], pitch)
            assert wc.findings(slot, container, IDS) == [] and wc.findings(slot, container, IDS, len(row)) == []
            assert wc.findings(slot, container, IDS, len(row) + 1) == [(wc.COUNT, 0)]
            assert wc.findings(wc.slots([row], pitch, rng=rng), container, IDS) == []  # nothing behind the length is read
    if case != "lower":
        assert wc.good_row(maps[0], container, case) != wc.good_row(maps[0], container)


@pytest.mark.parametrize("container", CONTAINERS)
def test_malformed_rows_bite(container):
    bad = wc.bad_rows(IDS, VALUES, container, WINDOW)
    assert {b.cls for b in bad} == set(range(1, 8 if container == GZIP_STORED else 6))
    want = dict(zip(IDS, VALUES))
    pitch = wire_ref.bound(container, len(IDS))
    for b in bad:
        assert len(b.row) <= pitch, b
        assert wc.findings(wc.slots([b.row], pitch), container, IDS) == [(b.cls, b.rank)], b
        if b.host == "rejected":
            with pytest.raises(acvm_amd.AcvmError):
                acvm_amd.decompress_witness(wc.gz(b.row))
        else:  # the reference reads it, and the device form's documented rule is what refuses it
            got = acvm_amd.decompress_witness(wc.gz(b.row))
            if b.cls == wc.HEX:      # 64 characters with the prefix: 31 bytes in the reference, a shape the device form does not read
                assert b"0x" in b.row and got == want, b
            elif b.cls == wc.KEY:    # a key the handle does not have
                assert set(got) - set(IDS), b
            else:                    # unordered or repeated keys: serde sorts them, the last one wins, and a witness goes missing
                assert b.cls == wc.ORDER and (got != want or len(got) < len(IDS)), b
