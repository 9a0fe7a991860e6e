"""CPU: the numpy statement of delay tracks (tdoa_amd.tracking; include/tdoa_mi355x.h, "delay tracks") on hand-worked
cases, against an enumeration of every track, and on the noisy case the feature exists for; and the boundary of
tdoa_process_track that needs no device."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 2 ** 32


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_point_declared_bound_and_exported(capi):
    name = "tdoa_process_track"
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    assert re.search(r"\bint %s\s*\(" % name, hdr)
    assert name in capi.SYMBOLS and hasattr(lib, name)
    assert ("C.%s(" % name) in go and "func (g *gpuCorrelator) ProcessTrack(" in go
    assert lib.tdoa_abi_version() == 4                    # additions only
    assert hasattr(capi.Context, "process_track")
    # the definition is in the header in the words the tests hold the library to
    for phrase in ("T_{n_w-1}[l] = σ q_{n_w-1}[l]",
                   "T_j[l]       = σ q_j[l] + max over |δ| <= J, l+δ inside the range, of T_{j+1}[l+δ]",
                   "D_j[l]       = the δ of that maximum; equal maxima: the smaller |δ|, then the positive δ",
                   "L_0          = the l with the largest T_0[l]; equal maxima: the smaller |l|, then the positive l",
                   "L_{j+1}      = L_j + D_j[L_j]",
                   "There is no rank / world and no group entry: a track crosses every window of its stack"):
        assert phrase in hdr, phrase
    # the profiling names are appended: the existing scopes keep their numbers
    names = [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))]
    assert names[:6] == ["k_fm_demod", "k_fwd_col", "k_fwd_row", "k_inv_row_pair", "k_inv_col_peak", "k_decode_peaks"]
    assert names[6:] == ["k_track_step", "k_track_finish"]


def test_null_handle_is_invalid_without_a_device(capi):
    lib = capi.load()
    score = (capi.Peak * 4)()
    lags = (C.c_int32 * 64)()
    for m, J in [(0, 1), (0, 0), (2, 64), (-1, 1), (0, -1), (0, 65), (5000, 1)]:
        assert lib.tdoa_process_track(None, m, J, C.cast(score, C.c_void_p), lags, None, None, None) == 1
    assert lib.tdoa_process_track(None, 0, 1, None, None, None, None, None) == 1


def _all_tracks(q, J):
    """every track of q [m][n] with steps of at most J, by enumeration: {first index: [(sum, path)]}"""
    m, n = q.shape
    out = {}
    for start in range(n):
        paths = [(start,)]
        for _ in range(m - 1):
            paths = [p + (p[-1] + d,) for p in paths for d in range(-J, J + 1) if 0 <= p[-1] + d < n]
        out[start] = [(sum(int(q[j, l]) for j, l in enumerate(p)), p) for p in paths]
    return out


def test_a_peak_that_walks_one_lag_per_window():
    """3 windows x 7 lags (max_lag 4), a unit peak at the lags -1, 0, -1"""
    from tdoa_amd import tracking
    q = np.zeros((3, 7), dtype=np.int64)
    q[0, 2] = q[1, 3] = q[2, 2] = ONE
    score, lags, values, total = tracking.track(q, 1, 4)
    assert score == 3 * ONE and list(lags) == [-1, 0, -1] and list(values) == [ONE] * 3
    # worked by hand: T_2 = q_2; T_1 = (0, 1, 1, 2, 0, 0, 0); T_0 = (1, 1, 3, 2, 2, 0, 0)
    assert list(total) == [ONE, ONE, 3 * ONE, 2 * ONE, 2 * ONE, 0, 0]
    # J = 0: the plain stack
    score0, lags0, values0, total0 = tracking.track(q, 0, 4)
    assert list(total0) == list(q.sum(axis=0)) == [0, 0, 2 * ONE, ONE, 0, 0, 0]
    assert score0 == 2 * ONE and list(lags0) == [-1, -1, -1] and list(values0) == [ONE, 0, ONE]
    # negative polarity: the same lags, the score and every sum change sign
    nscore, nlags, nvalues, ntotal = tracking.track(-q, 1, 4)
    assert nscore == -score and list(nlags) == list(lags) and list(nvalues) == [-ONE] * 3 and list(ntotal) == list(-total)
    rec = tracking.score_record(nscore, nlags[0], 3)
    assert int(rec["lag"]) == -1 and float(rec["corr"]) == -3.0 / np.sqrt(3.0) and rec["abs_corr"] == np.float32(3.0 / np.sqrt(3.0))


def test_no_steps_is_the_plain_stack():
    from tdoa_amd import stacking, tracking
    rng = np.random.default_rng(11)
    for m, ml in ((1, 4), (5, 9), (16, 33)):
        q = rng.integers(-3 * ONE, 3 * ONE, size=(m, 2 * ml - 1), dtype=np.int64)
        score, lags, values, total = tracking.track(q, 0, ml)
        assert np.array_equal(total, q.sum(axis=0))
        c = stacking.from_fixed(total, m)
        (lag, corr), = stacking.stacked_peaks(c, ml, 1, 1)
        rec = tracking.score_record(score, lags[0], m)
        assert (int(rec["lag"]), float(rec["corr"])) == (lag, corr) and rec["abs_corr"] == np.float32(abs(corr))
        assert (lags == lag).all() and np.array_equal(values, q[:, lag + ml - 1])
        assert tracking.surface(total, m).tobytes() == c.astype(np.float32).tobytes()


def test_the_range_clamps_a_track_and_the_tie_rules():
    from tdoa_amd import tracking
    # a peak that walks out of the range: ..., 2, 3, then it would be 4 -- the last window's best inside the range is taken
    q = np.zeros((3, 7), dtype=np.int64)
    q[0, 5] = q[1, 6] = ONE
    q[2, 6] = ONE // 2
    q[2, 0] = ONE                                          # larger, but out of reach
    score, lags, _, total = tracking.track(q, 1, 4)
    assert list(lags) == [2, 3, 3] and score == 2 * ONE + ONE // 2
    assert total[6] == ONE + ONE // 2                      # T_0 at the edge: steps 0 and -1 only
    # an all-zero middle window keeps the step 0
    q = np.zeros((3, 7), dtype=np.int64)
    q[0, 3] = q[2, 3] = ONE
    assert list(tracking.track(q, 1, 4)[1]) == [0, 0, 0]
    assert list(tracking.track(q, 3, 4)[1]) == [0, 0, 0]
    # equal maxima at +d and -d: the positive step; at |d| = 1 and |d| = 2: the smaller
    q = np.zeros((2, 7), dtype=np.int64)
    q[0, 3] = q[1, 2] = q[1, 4] = ONE
    assert list(tracking.track(q, 1, 4)[1]) == [0, 1]
    q[1, 2] = 0
    q[1, 1] = ONE
    assert list(tracking.track(q, 2, 4)[1]) == [0, 1]
    q[1, 4] = 0
    q[1, 5] = q[1, 2] = ONE
    q[1, 1] = 0
    assert list(tracking.track(q, 2, 4)[1]) == [0, -1]
    # equal L_0 candidates: the smaller |l|, then the positive l
    q = np.zeros((1, 7), dtype=np.int64)
    q[0, 2] = q[0, 4] = ONE
    assert list(tracking.track(q, 1, 4)[1]) == [1]
    q[0, 4] = 0
    q[0, 5] = ONE
    assert list(tracking.track(q, 1, 4)[1]) == [-1]
    # equal maxima of the two polarities: +1
    q = np.zeros((1, 7), dtype=np.int64)
    q[0, 1] = -ONE
    q[0, 5] = ONE
    score, lags, _, total = tracking.track(q, 0, 4)
    assert score == ONE and list(lags) == [2] and np.array_equal(total, q[0])
    # nothing but zeros: the zero record, zero lags and values
    score, lags, values, total = tracking.track(np.zeros((4, 7), dtype=np.int64), 2, 4)
    assert score == 0 and not lags.any() and not values.any() and not total.any()
    assert tracking.score_record(score, 0, 4).tobytes() == bytes(tracking.score_record(0, 0, 1).nbytes)
    with pytest.raises(ValueError):
        tracking.track(np.zeros((2, 6), dtype=np.int64), 1, 4)
    with pytest.raises(ValueError):
        tracking.track(np.zeros((2, 7), dtype=np.int64), -1, 4)


def test_against_every_track_enumerated():
    """small random stacks (few distinct values, so equal maxima are common): total and the score against the
    enumeration of all tracks, the returned track is one of them, carries the score and obeys the tie rules"""
    from tdoa_amd import tracking
    rng = np.random.default_rng(5)
    for m, ml, J in itertools.product((1, 2, 4), (2, 4), (0, 1, 2, 5)):
        n = 2 * ml - 1
        q = rng.integers(-2, 3, size=(m, n), dtype=np.int64)
        score, lags, values, total = tracking.track(q, J, ml)
        tracks = _all_tracks(q, J)
        top = {s: max(v for v, _ in tracks[s]) for s in tracks}
        low = {s: min(v for v, _ in tracks[s]) for s in tracks}
        sigma = 1 if max(top.values()) >= -min(low.values()) else -1
        want_total = [top[s] if sigma > 0 else low[s] for s in range(n)]
        assert list(total) == want_total, (m, ml, J)
        want = max(top.values()) if sigma > 0 else min(low.values())
        assert score == want
        if want == 0:
            assert not lags.any() and not values.any()
            continue
        idx = [int(l) + ml - 1 for l in lags]
        assert all(abs(a - b) <= J for a, b in zip(idx, idx[1:]))
        assert sum(int(q[j, l]) for j, l in enumerate(idx)) == score
        assert list(values) == [int(q[j, l]) for j, l in enumerate(idx)]
        # L_0 among the starts that reach the score: the smaller |l|, then the positive l
        starts = [s - (ml - 1) for s in range(n) if want_total[s] == want]
        assert int(lags[0]) == min(starts, key=lambda l: (abs(l), l < 0))
        # every step: among the steps that keep the best remaining sum, the smaller |d|, then the positive d
        best_tail = {}
        for s in tracks:
            for v, p in tracks[s]:
                for j in range(m):
                    tail = sigma * sum(int(q[k, p[k]]) for k in range(j, m))
                    best_tail[(j, p[j])] = max(best_tail.get((j, p[j]), tail), tail)
        for j in range(m - 1):
            ok = [d for d in range(-J, J + 1) if 0 <= idx[j] + d < n and
                  sigma * int(q[j, idx[j]]) + best_tail[(j + 1, idx[j] + d)] == best_tail[(j, idx[j])]]
            assert idx[j + 1] - idx[j] == min(ok, key=lambda d: (abs(d), d < 0)), (m, ml, J, j)


def test_more_steps_never_lower_the_score_and_cover_the_slope_search():
    from tdoa_amd import stacking, tracking
    rng = np.random.default_rng(23)
    m, ml = 6, 20
    for trial in range(4):
        q = rng.integers(-ONE, ONE, size=(m, 2 * ml - 1), dtype=np.int64)
        tops = [abs(tracking.track(q, J, ml)[0]) for J in (0, 1, 2, 3, 8, 64)]
        assert tops == sorted(tops)
        for H, D in ((3, 1), (3, 2), (2, 4)):
            h, profile, qh = stacking.drift_search(q, H, D, ml)
            L = int(profile[h + H]["lag"])
            path = [L + stacking.shift(h, j, D) for j in range(m)]
            if all(-ml < l < ml for l in path):
                J = -(-H // D)
                assert abs(tracking.track(q, J, ml)[0]) >= abs(int(qh[L + ml - 1])), (trial, H, D)


def test_the_track_follows_a_delay_no_line_fits(oracle):
    """16 windows of 8192 samples at noise 0.7 (simulate_delayed_fm, modulation index 1, content seed 100 + w, noise seeds
    1000 + w / 2000 + w), the delay rising from 7 to 12 and falling to 3.  Measured with the float64 pipeline: 15 of 16
    single-window argmaxes are wrong, the plain stack peaks at lag 58 (|C| 2.41), the slope search (H 3, D 1) picks -1 at
    lag 18 (|C| 3.86); the J = 1 track starts at 7, is exact on 15 windows and one lag off on the other, |C| 7.38: 3.06 x
    the plain stack and 1.32 x the best J = 1 track of a pair with nothing in common (station 1 with the content seeds
    500 + w and no delay: |C| 5.59, the noise floor of the statistic)."""
    from tdoa_amd import stacking, tracking
    wl, ml = 8192, 64
    delays = [7, 8, 9, 10, 11, 12, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3]
    wpb = len(delays)
    q, qn, missed = [], [], 0
    for w in range(wpb):
        a = oracle.b_preprocess(oracle.simulate_delayed_fm(wl, 0, 100 + w, 1000 + w, 1.0, 0.7))[0]
        b = oracle.b_preprocess(oracle.simulate_delayed_fm(wl, delays[w], 100 + w, 2000 + w, 1.0, 0.7))[0]
        other = oracle.b_preprocess(oracle.simulate_delayed_fm(wl, 0, 500 + w, 2000 + w, 1.0, 0.7))[0]
        cw = oracle.b_xcorr_all_lags(a, b, ml)
        missed += int(oracle.b_pick_peak(cw, ml)[0] != delays[w])
        q.append(stacking.to_fixed(cw))
        qn.append(stacking.to_fixed(oracle.b_xcorr_all_lags(a, other, ml)))
    q, qn = np.array(q), np.array(qn)
    plain = stacking.stacked_peaks(stacking.from_fixed(q.sum(axis=0), wpb), ml, 1, 1)[0]
    h, profile, _ = stacking.drift_search(q, 3, 1, ml)
    score, lags, values, total = tracking.track(q, 1, ml)
    noise = tracking.track(qn, 1, ml)[0]
    c = abs(float(stacking.from_fixed(np.int64(score), wpb)))
    cn = abs(float(stacking.from_fixed(np.int64(noise), wpb)))
    off = np.abs(lags - np.array(delays))
    print("%d of %d windows miss; plain stack lag %d |C| %.3f; slope %d lag %d |C| %.3f; track %s |C| %.3f (%.2f x plain), "
          "%d exact; unrelated pair %.3f (%.2f x)" % (missed, wpb, plain[0], abs(plain[1]), h, int(profile[h + 3]["lag"]),
                                                      float(profile[h + 3]["abs_corr"]), list(lags), c, c / abs(plain[1]),
                                                      int((off == 0).sum()), cn, c / cn))
    assert missed >= 13
    assert plain[0] != 7 and int(profile[h + 3]["lag"]) != 7
    assert int(lags[0]) == 7 and off.max() <= 1 and int((off == 0).sum()) >= 13
    assert c >= 2.5 * abs(plain[1])
    assert c >= 1.2 * cn
    assert np.array_equal(values, q[np.arange(wpb), lags + ml - 1]) and int(values.sum()) == score
