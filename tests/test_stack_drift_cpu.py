"""CPU: the numpy statement of drift-compensated stacking (tdoa_amd.stacking: shift, sheared_sum, drift_search,
drift_ppm; include/tdoa_mi355x.h, "drift-compensated stacking") on hand-computed values and on the noisy case the feature
exists for, and the boundary of tdoa_process_stacked_drift that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_point_declared_bound_and_exported(capi):
    name = "tdoa_process_stacked_drift"
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h")).read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go")).read()
    lib = capi.load()
    assert re.search(r"\bint %s\s*\(" % name, hdr)
    assert name in capi.SYMBOLS and hasattr(lib, name)
    assert ("C.%s(" % name) in go and "func (g *gpuCorrelator) ProcessStackedDrift(" in go
    assert lib.tdoa_abi_version() == 4                    # additions only
    assert hasattr(capi.Context, "process_stacked_drift")
    # the definition is in the header in the words the tests hold the library to, and the plain stack's premise is qualified
    for phrase in ("shift(h, j) = sgn(h) * ((2 |h| j + D) div (2 D))", "Q_h[L]      = sum over j of q_j[L + shift(h, j)]",
                   "The stations' clocks do not move within a block", "No rank / world and no group entry"):
        assert phrase in hdr, phrase


def test_null_handle_is_invalid_without_a_device(capi):
    lib = capi.load()
    peaks = (capi.Peak * 16)()
    count = (C.c_int32 * 4)()
    drift = (C.c_int32 * 4)()
    for m, k, sep, gate, H, D in [(0, 1, 1, 0.0, 0, 1), (0, 1, 1, 0.0, 4, 2), (-1, 1, 1, 0.0, 1, 1), (0, 0, 1, 0.0, 1, 1),
                                  (0, 1, 1, -1.0, 1, 1), (0, 1, 1, 0.0, -1, 1), (0, 1, 1, 0.0, 513, 1), (0, 1, 1, 0.0, 1, 0)]:
        assert lib.tdoa_process_stacked_drift(None, m, k, sep, gate, H, D, C.cast(peaks, C.c_void_p), count, None, None, None,
                                              drift, None) == 1


def test_shift_on_hand_computed_values():
    from tdoa_amd.stacking import shift
    # (h, j, D) -> nearest integer to h j / D, halves away from zero
    table = {(0, 5, 3): 0, (1, 0, 1): 0, (4, 5, 1): 20, (-4, 5, 1): -20,
             (1, 1, 2): 1, (-1, 1, 2): -1,               # +-0.5
             (3, 1, 2): 2, (-3, 1, 2): -2,               # +-1.5
             (1, 3, 2): 2, (-1, 3, 2): -2,               # +-1.5 again, by j
             (3, 2, 2): 3, (3, 3, 2): 5, (3, 11, 2): 17,  # 3, 4.5, 16.5
             (1, 1, 3): 0, (1, 2, 3): 1, (2, 2, 3): 1, (-2, 2, 3): -1,      # 0.33, 0.67, 1.33
             (-5, 3, 4): -4, (-5, 2, 4): -3, (-5, 1, 4): -1,                # -3.75, -2.5, -1.25
             (5, 7, 4): 9, (1, 7, 4): 2, (1, 5, 4): 1,                      # 8.75, 1.75, 1.25
             (512, 39, 1): 19968, (1, 1, 2 ** 31 - 1): 0}
    for (h, j, d), want in table.items():
        assert shift(h, j, d) == want, (h, j, d)
    for h in range(-9, 10):
        for j in range(0, 14):
            for d in (1, 2, 3, 4, 7, 32):
                assert shift(-h, j, d) == -shift(h, j, d)
                assert abs(shift(h, j, d) - h * j / d) <= 0.5
    # the delays of the noisy case below
    assert [7 + shift(3, w, 2) for w in range(12)] == [7, 9, 10, 12, 13, 15, 16, 18, 19, 21, 22, 24]
    with pytest.raises(ValueError):
        shift(1, 1, 0)


def test_sheared_sum_and_search_on_a_hand_worked_case():
    """3 windows x 7 lags (max_lag 4): a unit peak that walks one lag per window from lag -1"""
    from tdoa_amd import stacking
    one = 2 ** 32
    q = np.zeros((3, 7), dtype=np.int64)
    for j in range(3):
        q[j, 2 + j] = one                                  # lag -1 + j
    q[2, 0] = -5                                           # a term that leaves the range under h = -1: lag -3 - 2
    assert list(stacking.sheared_sum(q, 0, 1)) == [-5, 0, one, one, one, 0, 0]
    assert list(stacking.sheared_sum(q, 1, 1)) == [0, 0, 3 * one, 0, 0, 0, 0]
    assert list(stacking.sheared_sum(q, -1, 1)) == [0, 0, one - 5, 0, one, 0, one]
    assert list(stacking.sheared_sum(q, 1, 2)) == [0, 0, 2 * one, one, 0, 0, 0]        # shifts 0, 1 (a half), 1
    h, profile, qh = stacking.drift_search(q, 1, 1, 4)
    assert h == 1 and list(qh) == [0, 0, 3 * one, 0, 0, 0, 0]
    root = np.sqrt(3.0)
    # h = -1: one - 5 and one are the same float32: lag 1 of the tie (-1, 1, 3); h = 0: lag 0 of the tie (-1, 0, 1)
    assert [int(x) for x in profile["lag"]] == [1, 0, -1]
    assert profile["abs_corr"].tolist() == [np.float32(1 / root), np.float32(1 / root), np.float32(3 / root)]
    assert profile["corr"].tolist() == [float(np.float32(1 / root))] * 2 + [float(np.float32(3 / root))]
    # equal maxima: the smaller |h| wins, then the positive h; nothing but zeros: h* = 0 and zero records
    flat = np.zeros((2, 7), dtype=np.int64)
    flat[:, 3] = one
    h, profile, _ = stacking.drift_search(flat, 0, 1, 4)
    assert h == 0 and len(profile) == 1
    sym = np.zeros((2, 7), dtype=np.int64)
    sym[0, 3] = sym[1, 2] = sym[1, 4] = one                # h = +1 and h = -1 both reach 2, h = 0 reaches 1
    h, profile, _ = stacking.drift_search(sym, 1, 1, 4)
    assert h == 1 and profile["abs_corr"][0] == profile["abs_corr"][2] > profile["abs_corr"][1]
    h, profile, qh = stacking.drift_search(np.zeros((3, 7), dtype=np.int64), 2, 2, 4)
    assert h == 0 and not qh.any() and profile.tobytes() == bytes(profile.nbytes)
    with pytest.raises(ValueError):
        stacking.drift_search(q, 2, 1, 4)                  # shift(2, 2) = 4 > max_lag - 1
    assert stacking.drift_ppm(3, 2, 8192) == pytest.approx(183.10546875)
    assert stacking.drift_ppm(-1, 32, 2_000_000) == pytest.approx(-0.015625)


def test_the_search_finds_the_delay_the_plain_stack_misses(oracle):
    """12 windows of 8192 samples at noise 0.7 (simulate_delayed_fm, modulation index 1, content seed 100 + w, noise seeds
    1000 + w / 2000 + w), window w delayed by 7 + shift(3, w, 2) = 7, 9, 10, 12, ..., 24: a slope of 3/2 lag per window.
    Measured with the float64 pipeline: 11 of 12 single-window argmaxes are wrong, the plain stack peaks at lag -61 (|C| 3.20,
    1.10 x its second peak), the stack along h = 3 of H = 8, D = 2 at lag 7 with |C| 5.08, 1.95 x its second peak and
    1.49 x the best of the 16 other slopes."""
    from tdoa_amd import stacking
    wl, wpb, ml, d0, H, D = 8192, 12, 64, 7, 8, 2
    delays = [d0 + stacking.shift(3, w, D) for w in range(wpb)]
    q, missed = [], 0
    for w in range(wpb):
        a = oracle.simulate_delayed_fm(wl, 0, 100 + w, 1000 + w, 1.0, 0.7)
        b = oracle.simulate_delayed_fm(wl, delays[w], 100 + w, 2000 + w, 1.0, 0.7)
        cw = oracle.b_xcorr_all_lags(oracle.b_preprocess(a)[0], oracle.b_preprocess(b)[0], ml)
        missed += int(oracle.b_pick_peak(cw, ml)[0] != delays[w])
        q.append(stacking.to_fixed(cw))
    q = np.array(q)
    plain = stacking.stacked_peaks(stacking.from_fixed(q.sum(axis=0), wpb), ml, 2, 2)
    h, profile, qh = stacking.drift_search(q, H, D, ml)
    assert np.array_equal(stacking.sheared_sum(q, 0, D), q.sum(axis=0))
    pk = stacking.stacked_peaks(stacking.from_fixed(qh, wpb), ml, 2, 2)
    others = np.delete(profile["abs_corr"], h + H).max()
    ratio, over = abs(pk[0][1]) / abs(pk[1][1]), float(profile[h + H]["abs_corr"]) / float(others)
    print("%d of %d windows miss; plain stack lag %d |C| %.3f ratio %.3f; h* %d lag %d |C| %.3f ratio %.3f, %.3f x the best other slope"
          % (missed, wpb, plain[0][0], abs(plain[0][1]), abs(plain[0][1]) / abs(plain[1][1]), h, pk[0][0], abs(pk[0][1]), ratio, over))
    assert missed >= 9
    assert plain[0][0] != d0
    assert h == 3 and pk[0][0] == d0 and int(profile[h + H]["lag"]) == d0
    assert np.float32(abs(pk[0][1])) == profile[h + H]["abs_corr"]
    assert ratio >= 1.5
    assert over >= 1.25
