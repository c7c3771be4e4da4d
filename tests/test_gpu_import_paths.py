"""Every import entry point reaches the kernels through one checked plan, one list buffer and one launcher (acvm_amd/csrc/batch_import.cpp): a
descriptor and the one part that says the same leave the same table, and the three users of the list buffer -- an import behind a solve, an
import from parts, an import by descriptor -- take turns on one handle without reading each other's lists. Judged by the CPU oracle."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import acvm_amd
from acvm_amd import synth
from acvm_amd.acir import P

pytestmark = pytest.mark.gpu
BE32, LE32, MONT, U8, U64 = acvm_amd.ENC_BE32, acvm_amd.ENC_LE32, acvm_amd.ENC_MONT256_LE, acvm_amd.ENC_U8, acvm_amd.ENC_U64
IM, WM = acvm_amd.LAYOUT_INSTANCE_MAJOR, acvm_amd.LAYOUT_WITNESS_MAJOR
N_IN, N_COLUMNS = 5, 7  # one full group of four inputs and a partial one for the instance-major kernels
COLUMNS = [5, 0, 6, 2, 3]


def _typed_io_module():
    spec = importlib.util.spec_from_file_location("_gpu_typed_io_for_import_paths", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_typed_io.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_T = _typed_io_module()
_buffer, _whole_state, _assert_same_state, _oracle_state = _T._buffer, _T._whole_state, _T._assert_same_state, _T._oracle_state


@functools.lru_cache(maxsize=None)
def _circuit():
    circ, ids = synth.arithmetic_circuit(40, n_in=N_IN, seed=0xAC1D0720)
    assert len(ids) == N_IN
    return circ.to_bytes(), ids


@functools.lru_cache(maxsize=None)
def _columns_of_values(B, bits, seed, edges=True):
    """[B][N_COLUMNS] integers below 2^bits (below p for bits = 254); edges: instance 0 of a batch of several holds the edges of the width (its zero
    fails an inversion: that instance takes the exact path)"""
    rng = np.random.default_rng(seed)
    top = P if bits == 254 else 1 << bits
    vals = [[int.from_bytes(rng.bytes(32), "big") % top for _ in range(N_COLUMNS)] for _ in range(B)]
    if edges and B > 1:
        vals[0] = [0, 1, top - 1, 255 % top, 256 % top, top - 2, 2][:N_COLUMNS]
    return vals


def _rows(vals, columns=COLUMNS):
    return [[row[c] for c in columns] for row in vals]


@functools.lru_cache(maxsize=None)
def _oracle_of(B, bits, seed, columns=tuple(COLUMNS), edges=True):
    from oracle import binding
    data, ids = _circuit()
    return _oracle_state(binding, data, ids, _rows(_columns_of_values(B, bits, seed, edges), columns))


# ---- 1. a descriptor and its one-part twin leave the same table
@pytest.mark.parametrize("B", [1, 65])  # one lane; one wave plus one lane
def test_descriptor_and_its_one_part_twin_leave_the_same_table(oracle, B):
    data, ids = _circuit()
    gc = acvm_amd.Circuit(data)
    by_desc, by_parts = acvm_amd.Batch(gc, B, ids), acvm_amd.Batch(gc, B, ids)
    for encoding, bits in ((BE32, 254), (LE32, 254), (MONT, 254), (U8, 8), (U64, 64)):
        vals = _columns_of_values(B, bits, 0xAC1D0721)
        want = _oracle_of(B, bits, 0xAC1D0721)
        for layout in (IM, WM):
            what = f"encoding {encoding} layout {layout} B {B}"
            buf = acvm_amd.DeviceBuffer(_buffer(vals, encoding, layout))
            by_desc.import_device(buf.ptr, encoding=encoding, layout=layout, columns=COLUMNS, n_columns=N_COLUMNS)
            by_desc.solve()
            got_desc = _whole_state(by_desc)
            by_parts.import_device_parts([dict(d_ptr=buf.ptr, encoding=encoding, layout=layout, positions=range(N_IN), columns=COLUMNS, n_columns=N_COLUMNS)])
            by_parts.solve()
            got_parts = _whole_state(by_parts)
            buf.free()
            assert got_desc[0] == got_parts[0] and np.array_equal(got_desc[1], got_parts[1]) and np.array_equal(got_desc[2], got_parts[2]), what
            _assert_same_state(got_desc, want, what + ": against the oracle")
    by_desc.free()
    by_parts.free()


# ---- 2. one list buffer, three users, on one handle
@pytest.mark.parametrize("parts_first", [False, True])
def test_one_list_buffer_three_users_on_one_handle(oracle, parts_first):
    B = 65
    data, ids = _circuit()
    gc = acvm_amd.Circuit(data)
    tiles = [_columns_of_values(B, 254, 0xAC1D0730 + t, edges=False) for t in range(3)]
    bufs = [acvm_amd.DeviceBuffer(_buffer(t, LE32, WM)) for t in tiles]
    desc = dict(encoding=LE32, layout=WM, columns=COLUMNS, n_columns=N_COLUMNS)
    other = [6, 1, 0, 4, 2]  # the parts read other columns, in another order of positions: other lists
    parts = lambda buf: [dict(d_ptr=buf.ptr, encoding=LE32, layout=WM, positions=[4, 0, 2], columns=[other[4], other[0], other[2]], n_columns=N_COLUMNS),
                         dict(d_ptr=buf.ptr, encoding=LE32, layout=WM, positions=[3, 1], columns=[other[3], other[1]], n_columns=N_COLUMNS)]
    want = _oracle_of(B, 254, 0xAC1D0731, edges=False)
    assert all(r[0] == 0 for r in _oracle_of(B, 254, 0xAC1D0730, edges=False)[0])  # (tile 0 solves clean: the import behind its solve runs)
    fresh = acvm_amd.Batch(gc, B, ids)
    fresh.import_device(bufs[1].ptr, **desc)
    fresh.solve()
    want_fresh = _whole_state(fresh)
    fresh.free()

    h = acvm_amd.Batch(gc, B, ids)
    if parts_first:
        h.import_device_parts([dict(d_ptr=bufs[0].ptr, encoding=LE32, layout=WM, positions=range(N_IN), columns=COLUMNS, n_columns=N_COLUMNS)])
    else:
        h.import_device(bufs[0].ptr, **desc)
    # 1. tile 1 by descriptor behind the solve of tile 0: its column list is in the list buffer, the import runs
    assert h.solve(then_import=bufs[1].ptr, then_import_desc=desc) == 0
    copies = h.import_list_copies()
    assert copies == (2 if parts_first else 1)
    # 2. tile 2 from parts: other lists in the same buffer; the import behind the solve no longer counts
    h.import_device_parts(parts(bufs[2]))
    assert h.import_list_copies() == copies + 1
    # 3. tile 1 by the descriptor of step 1, same pointer: it must import again, and upload its columns again
    h.import_device(bufs[1].ptr, **desc)
    assert h.import_list_copies() == copies + 2
    # 4.
    h.solve()
    got = _whole_state(h)
    _assert_same_state(got, want_fresh, "against a fresh handle")
    assert np.array_equal(got[2], want_fresh[2])
    _assert_same_state(got, want, "against the oracle")
    # (the parts of step 2 again: the buffer holds the descriptor's columns by now, so they travel once more; a second time they do not)
    h.import_device_parts(parts(bufs[2]))
    h.import_device_parts(parts(bufs[2]))
    assert h.import_list_copies() == copies + 3
    h.solve()
    _assert_same_state(_whole_state(h), _oracle_of(B, 254, 0xAC1D0732, tuple(other), edges=False), "the parts of tile 2 against the oracle")
    for x in bufs + [h]:
        x.free()
