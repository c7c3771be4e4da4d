"""Pins oracle/hashes.c. SHA-256: the reference's own vector (brillig_vm/src/black_box.rs:203-208).
Keccak-256 / BLAKE2s: the reference holds no fixed vector -> externally pinned: standard KATs and
Python hashlib."""
import ctypes as C
import hashlib
import random

from keccak_ref import keccak256 as _keccak256_py


def h(oracle, name, data):
    out = C.create_string_buffer(32)
    getattr(oracle.lib(), "oracle_" + name)(data, len(data), out)
    return out.raw


def test_sha256_reference_vector(oracle):
    assert h(oracle, "sha256", b"hello world").hex() == "b94d27b9934d3e08a52e52d7da7dabfac484efe37a5380ee9088f7ace2efcde9"


def test_sha256_blake2s_against_hashlib(oracle):
    rng = random.Random(5)
    for n in [0, 1, 31, 32, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 200, 1000]:
        data = bytes(rng.randrange(256) for _ in range(n))
        assert h(oracle, "sha256", data) == hashlib.sha256(data).digest()
        assert h(oracle, "blake2s", data) == hashlib.blake2s(data).digest()


def test_keccak256_known_answers(oracle):
    # original Keccak padding (0x01), not SHA3 (0x06)
    assert h(oracle, "keccak256", b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert h(oracle, "keccak256", b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    # SURVEY Appendix A.2 intermediate: keccak256(u64_be(1) || 0^24) -> gen[0] seed
    assert h(oracle, "keccak256", (1).to_bytes(8, "big") + bytes(24)).hex() == \
        "9fa0f24a436c57f2e4a6265cefa754ab96755741c6f4a8180f9b49dd4e77d101"
    # rate boundary (136) cases: cross-check the permutation against hashlib's sha3 state via a Python keccak
    for n in [135, 136, 137, 272]:
        data = bytes(range(256)) * 2
        assert h(oracle, "keccak256", data[:n]) == _keccak256_py(data[:n])

