"""The BN254-Fr field library (acvm_amd/csrc/fr_device.hpp, the byte helpers of ops_common.hpp) run ON THE DEVICE against Python integers, through
the acvm_debug_fr probe: the cases of tests/fr_ref.py -- the edges of every routine's contract, long runs of ones and zeros, a few thousand
random values -- one lane per item, raw limbs in, raw limbs out, every word compared with the reference's exact integer. The same cases run
through the host compiler in tests/test_fr_probe_on_host.py; here the column scans are the asm blocks of fr_blocks.inc and the multiply-adds the
device's own, and both the block form and the C form of a scan are compared with Python, not with each other. The second factors of the
scalar-register forms are one value per launch (a kernel argument): a few dozen launches each."""
import pytest

import fr_ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(fr_ref.WHATS))
def test_routine_on_device(name):
    import acvm_amd
    what = fr_ref.WHATS[name][0]
    launches = fr_ref.sections(name)
    assert (len(launches) >= 24) == (name in fr_ref.UNIFORM)
    for k, (u, items) in enumerate(launches):
        assert len(items) <= 40000
        fr_ref.compare(name, acvm_amd.debug_fr(what, items, u), k)
    print(f"{name}: {fr_ref.n_cases(name)} cases in {len(launches)} launch(es)")


def test_both_inversions_agree_with_each_other_and_with_python():
    """0, 1, p - 1, 2^k and p - 2^k for every k, their inverses, 2 000 random values: fr_inv == fr_inv_eea == pow(a, -1, p) in Montgomery form"""
    import acvm_amd
    (_, items), = fr_ref.sections("fr_inv")
    assert fr_ref.sections("fr_inv_eea") == fr_ref.sections("fr_inv") and len(items) >= 3000
    a, b = acvm_amd.debug_fr(fr_ref.WHATS["fr_inv"][0], items), acvm_amd.debug_fr(fr_ref.WHATS["fr_inv_eea"][0], items)
    assert (a == b).all()
    for w, got in list(zip(items, a))[::7] + list(zip(items, a))[:8]:
        x, v = fr_ref.s_value(w), fr_ref.s_value(got)
        assert v < fr_ref.P and (v * x - fr_ref.R2) % fr_ref.P == 0 if x else v == 0, hex(x)
