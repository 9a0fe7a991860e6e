"""CPU: the boundary of the correlation-surface and peak-selection calls (tdoa_process_lags, tdoa_process_peaks,
tdoa_fm_xcorr_peaks_u8, tdoa_debug_select_peaks) and the float64 statement of the selection rule (tdoa_amd.peaks) that the
GPU kernel is held to in tests/test_gpu_peaks.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["tdoa_process_lags", "tdoa_process_peaks", "tdoa_fm_xcorr_peaks_u8", "tdoa_debug_select_peaks"]


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h")).read()
    lib = capi.load()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.tdoa_abi_version() == 4                    # additions only


def test_null_context_and_bad_arguments_are_invalid(capi):
    """every check that needs no device: a NULL context, k outside 1..16, min_separation < 1, NULL outputs"""
    lib = capi.load()
    peaks = (capi.Peak * 16)()
    count = C.c_int32()
    buf = (C.c_float * 8)()
    iq = (C.c_uint8 * 16)()
    assert lib.tdoa_process_lags(None, 0, 1, buf, None) == 1
    assert lib.tdoa_process_lags(None, 0, 1, None, None) == 1
    for k, sep in [(8, 8), (0, 8), (17, 8), (8, 0), (1, -3)]:
        assert lib.tdoa_process_peaks(None, 0, 1, k, sep, C.cast(peaks, C.c_void_p), C.byref(count)) == 1
        assert lib.tdoa_fm_xcorr_peaks_u8(None, iq, 8, iq, 8, 4, k, sep, C.cast(peaks, C.c_void_p), C.byref(count)) == 1
        assert lib.tdoa_debug_select_peaks(None, buf, 8, -4, k, sep, C.cast(peaks, C.c_void_p), C.byref(count)) == 1
    assert lib.tdoa_process_peaks(None, 0, 1, 8, 8, None, None) == 1


def test_rule_plateau_edges_nan_zero_and_few_candidates():
    from tdoa_amd.peaks import select_peaks
    # plateau: both lags of a flat top are local maxima; the tie goes to the smaller |lag|, which then suppresses the other
    c = [0.0, 1.0, 3.0, 3.0, 1.0, 0.0, 2.0, 0.5]                       # lags -4 .. 3
    assert select_peaks(c, -4, 4, 1) == [(-1, 3.0), (2, 2.0)]
    assert select_peaks(c, -1, 4, 1) == [(1, 3.0), (5, 2.0)]          # lags -1 .. 6: the plateau at 1, 2 keeps 1
    assert select_peaks([1.0, 0.0, -1.0], -1, 4, 1) == [(1, -1.0), (-1, 1.0)]   # equal |c|, equal |lag|: positive first
    # a peak at either end of the range: the neighbour outside counts as smaller
    assert select_peaks([5.0, 1.0, 0.2, 1.0, 4.0], 10, 4, 1) == [(10, 5.0), (14, 4.0)]
    # NaN is never a peak, and its neighbours fail the comparison with it
    assert select_peaks([0.1, 2.0, np.nan, 1.0, 0.5, 0.7, 0.2], 0, 4, 1) == [(5, 0.7)]
    # all zero: nothing qualifies
    assert select_peaks(np.zeros(9), -4, 8, 1) == []
    # fewer candidates than k
    assert select_peaks([0.0, 1.0, 0.0, -2.0, 0.0], 0, 8, 1) == [(3, -2.0), (1, 1.0)]
    with pytest.raises(ValueError):
        select_peaks(c, 0, 17, 1)
    with pytest.raises(ValueError):
        select_peaks(c, 0, 4, 0)


def test_rule_separation_and_greedy_order():
    from tdoa_amd.peaks import select_peaks
    rng = np.random.default_rng(5)
    c = rng.standard_normal(4001)
    got = select_peaks(c, -2000, 16, 8)
    assert len(got) == 16
    mags = [abs(v) for _, v in got]
    assert mags == sorted(mags, reverse=True)
    lags = [l for l, _ in got]
    assert all(abs(a - b) > 8 for i, a in enumerate(lags) for b in lags[:i])
    assert got[0][0] == int(np.argmax(np.abs(c))) - 2000
    for lag, v in got:                                                 # each is a local maximum holding its own value
        i = lag + 2000
        assert c[i] == v and abs(v) >= abs(c[i - 1]) and abs(v) >= abs(c[i + 1])


def _rec(lag, corr):
    r = np.zeros((), dtype=np.dtype([("lag", np.int32), ("abs_corr", np.float32), ("corr", np.float64)]))
    r["lag"], r["corr"], r["abs_corr"] = lag, corr, np.float32(abs(corr))
    return r


def test_surface_max_and_the_record_check_on_hand_made_surfaces():
    """surface_max / record_is_surface_max (what the GPU tests hold every pair-window's record to): ties in the key's order, a
    negative winner, all zero, NaN, and every way a record can be wrong"""
    from tdoa_amd.peaks import record_is_surface_max, surface_max
    s = np.array([0.5, -3.0, 1.0, 0.0, 2.0, 3.0, -0.25], dtype=np.float32)         # lags -3 .. 3, ml = 4
    T, v = surface_max(s, -3)
    assert T == [2, -2] and v == np.float32(3.0)                                   # equal |lag|: the positive lag first
    assert record_is_surface_max(_rec(2, 3.0), s, 4) == [2, -2]
    for bad in [_rec(-2, -3.0), _rec(2, -3.0), _rec(1, 2.0), _rec(2, 3.0000002), _rec(0, 0.0), _rec(4, 3.0)]:
        with pytest.raises(AssertionError):
            record_is_surface_max(bad, s, 4)
    wrong_abs = _rec(2, 3.0)
    wrong_abs["abs_corr"] = 2.5
    with pytest.raises(AssertionError):
        record_is_surface_max(wrong_abs, s, 4)
    T, v = surface_max([1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0], 0)                    # smaller |lag| before the sign of the lag
    assert T == [0, 4, 6] and v == np.float32(1.0)
    n = np.array([0.5, 1.0, -7.0], dtype=np.float32)                               # a negative winner at the last lag
    assert surface_max(n, -1) == ([1], np.float32(-7.0))
    assert record_is_surface_max(_rec(1, -7.0), n, 2) == [1]
    with pytest.raises(AssertionError):
        record_is_surface_max(_rec(1, 7.0), n, 2)                                  # the sign belongs to the record
    # the double behind the record rounds to the surface's float: equal after rounding, not before
    third = np.array([0.0, np.float32(1.0 / 3.0), 0.0], dtype=np.float32)
    assert record_is_surface_max(_rec(0, float(third[1]) * (1 + 2.0 ** -30)), third, 2) == [0]
    z = np.array([0.0, -0.0, 0.0], dtype=np.float32)                               # all zero: only the zero record
    assert surface_max(z, -1)[0] == [0, 1, -1] and surface_max(z, -1)[1] == 0
    record_is_surface_max(_rec(0, 0.0), z, 2)
    for bad in [_rec(1, 0.0), _rec(0, 1e-30)]:
        with pytest.raises(AssertionError):
            record_is_surface_max(bad, z, 2)
    assert surface_max([np.nan, 2.0, np.nan], 5) == ([6], np.float32(2.0))         # NaN never counts
    assert surface_max([np.nan, np.nan], 0) == ([], np.float32(0.0)) and surface_max([], 0)[0] == []
