"""CPU: the float64 / int64 statement of the stacked correlation (tdoa_amd.stacking) on a hand-worked case, and the
boundary of tdoa_num_stacks, tdoa_process_stacked and tdoa_group_process_stacked that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tdoa_num_stacks", "tdoa_process_stacked", "tdoa_group_process_stacked"]


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h")).read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go")).read()
    lib = capi.load()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
        assert ("C.%s(" % name) in go, name
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("num_stacks", "process_stacked"):
        assert hasattr(capi.Context, method)
    assert hasattr(capi.Group, "process_stacked")
    assert "func (g *gpuCorrelator) ProcessStacked(" in go and "func (g *Group) ProcessStacked(" in go
    # the definition is in the header in the words the tests hold the library to
    for phrase in ("q_w[l] = llrint(c_w[l] * 2^32)", "C[l]   = (double)Q[l] * 2^-32 / sqrt(n_w)", "not\n * defined behaviour"):
        assert phrase in hdr, phrase


def test_null_handles_are_invalid_without_a_device(capi):
    lib = capi.load()
    a, b = C.c_int(-5), C.c_int(-5)
    assert lib.tdoa_num_stacks(None, 0, C.byref(a), C.byref(b)) == 1 and (a.value, b.value) == (-5, -5)
    peaks = (capi.Peak * 16)()
    count = (C.c_int32 * 4)()
    for m, k, sep, gate in [(0, 1, 1, 0.0), (-1, 1, 1, 0.0), (0, 0, 1, 0.0), (0, 17, 1, 0.0), (0, 1, 0, 0.0), (0, 1, 1, -1.0)]:
        assert lib.tdoa_process_stacked(None, 0, 1, m, k, sep, gate, C.cast(peaks, C.c_void_p), count, None, None, None) == 1
        assert lib.tdoa_group_process_stacked(None, m, k, sep, gate, C.cast(peaks, C.c_void_p), count, None, None) == 1


def test_stack_ids():
    from tdoa_amd import stacking
    assert stacking.stack_ids(5, 2) == (3, [(0, [0, 1]), (1, [2, 3]), (2, [4]), (3, [5, 6]), (4, [7, 8]), (5, [9]),
                                            (6, [10, 11]), (7, [12, 13]), (8, [14])])
    assert stacking.stack_ids(4, 0) == (1, [(0, [0, 1, 2, 3]), (1, [4, 5, 6, 7]), (2, [8, 9, 10, 11])])
    assert stacking.stack_ids(4, 9) == stacking.stack_ids(4, 0)           # longer than a block: the block
    assert stacking.stack_ids(2, 1)[0] == 2 and [w for _, w in stacking.stack_ids(2, 1)[1]] == [[k] for k in range(6)]
    with pytest.raises(ValueError):
        stacking.stack_ids(4, -1)


def test_hand_worked_case():
    """3 windows per block x 1 pair x 5 lags, stacks of 2 (a full stack and a short one per block).  Block 0 by hand:
    window 0 holds 2^-33 and 3 * 2^-33 (ties at half a quantum: to even, 0 and 2), window 1 the exact 0.5 and -1.25,
    window 2 a value that is not a multiple of the quantum."""
    from tdoa_amd import stacking
    h = 2.0 ** -33
    s = np.zeros((9, 1, 5))
    s[0, 0] = [h, 3 * h, 1.0, -2.0, 0.25]
    s[1, 0] = [0.5, -1.25, 3.0, 2.0, 5 * h]
    s[2, 0] = [0.1, -0.3, 7.0, 1e-12, -3 * h]
    s[3:6] = -s[0:3]
    q, c, n_w = stacking.stack_surfaces(s, 3, 2)
    assert q.dtype == np.int64 and q.shape == (6, 1, 5) and list(n_w) == [2, 1] * 3
    one = 2 ** 32
    assert list(q[0, 0]) == [0 + one // 2, 2 - 5 * one // 4, 4 * one, 0, one // 4 + 2]      # 5 h -> 2.5 quanta -> 2
    assert list(q[1, 0]) == [int(np.rint(0.1 * one)), int(np.rint(-0.3 * one)), 7 * one, 0, -2]   # -3 h -> -1.5 -> -2
    assert np.array_equal(q[2:4], -q[0:2]) and not q[4:].any()
    assert np.array_equal(c[0, 0], q[0, 0].astype(np.float64) / one / np.sqrt(2.0))
    # a stack of one window is the llrint round trip of that window's surface, divided by 1
    assert np.array_equal(c[1, 0], np.rint(s[2, 0] * one) / one)
    assert c[1, 0, 2] == 7.0 and c[1, 0, 3] == 0.0 and abs(c[1, 0, 0] - 0.1) <= 2.0 ** -33
    # order does not matter: the windows of a stack in any order, and the stack split in two partial sums
    assert np.array_equal(stacking.to_fixed(s[[1, 0]]).sum(axis=0), q[0])
    assert np.array_equal(stacking.to_fixed(s[0]) + stacking.to_fixed(s[1]), q[0])
    # peak 1 of the full stack: lag 0 (index 2), its value the float64 C; the refinement stays within half a sample
    pk = stacking.stacked_peaks(c[0, 0], 3, 2, 1)
    assert pk[0] == (0, 4.0 / np.sqrt(2.0)) and pk[1][0] == 2      # (-1 is no local maximum, 1 holds 0)
    assert abs(stacking.refine(c[0, 0], 3, 0)) <= 0.5
    assert stacking.refine(c[0, 0], 3, -2) == -2.0 and stacking.refine(c[0, 0], 3, 2) == 2.0     # the edge: frac 0
    with pytest.raises(ValueError):
        stacking.stack_surfaces(s[:8], 3, 2)
