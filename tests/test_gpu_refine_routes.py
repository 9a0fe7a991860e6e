"""GPU: the sub-sample refinement on every route the decimated inverse can take at the reference's 20 000 lags, against the
float64 oracle (ob_refine_peak) on poisoned workspace.

The refinement is the only mode-B output that reads the inverse's intermediate array again after the peak is picked
(launch_refine: three neighbours out of V' -- or V on the full inverse).  Which kernels wrote that array depends on the route
plan_fm_batch chose, so every case here
- starts on a fresh context; one warm-up call of the same shape (other data, or another gate) sizes the workspace, since
  tdoa_debug_poison_workspace only reaches what is allocated;
- fills the float workspaces with NaN (Context.poison_workspace) right before the call under test: a value the route reads
  but did not write shows up as NaN instead of an earlier call's bytes;
- asserts the route it is named for (Context.last_route);
- holds lag, corr, the neighbours y, frac, delay and plausible against the oracle with test_gpu_fine's tolerances.
Batched cases then poison once more and call process_fine again: the replayed step graph gives the same records."""
import numpy as np
import pytest

from test_gpu_fine import _check

pytestmark = pytest.mark.gpu

ML = 20000
GATE = 200.0          # samples: the batched stations' delay differences (< 400) fall on either side of it
PLANS = {1_100_000: (4096, 256), 2_200_001: (4096, 512)}


def _pair(oracle, wl, peak):
    """two captures whose correlation peaks at +19 999, -19 999 (the neighbour outside the searched range), 0, or a
    negative-correlation peak (I and Q of the second swapped: the phase runs backwards); returns (a, b, expected lag)"""
    if peak == "neg":
        a = oracle.simulate_delayed_fm(wl, 0, 77, 1)
        b = oracle.simulate_delayed_fm(wl, 9, 77, 2)
        binv = b.copy()
        binv[0::2], binv[1::2] = b[1::2], b[0::2]
        return a, binv, 9
    d = int(peak)
    return oracle.simulate_delayed_fm(wl, max(0, -d), 4242, 1), oracle.simulate_delayed_fm(wl, max(0, d), 4242, 2), d


def _pair_vs_oracle(oracle, c, a, b, want_lag, gate=120.0):
    c.fm_xcorr_fine(b, a, ML, gate)                    # warm-up on other data: the workspace at this call's size
    c.poison_workspace()
    (lag, corr), fine = c.fm_xcorr_fine(a, b, ML, gate)
    route = c.last_route()
    ta, _ = oracle.b_preprocess(a)
    tb, _ = oracle.b_preprocess(b)
    olag, ocorr, _ = oracle.b_xcorr_peak_fft(ta, tb, ML)
    assert lag == olag == want_lag
    assert abs(corr - ocorr) <= 1e-5 * abs(ocorr)
    if want_lag == 9:
        assert corr < 0 and fine["y"][1] > 0              # y is sign-normalised
    _check(fine, oracle.b_refine_peak(ta, tb, lag, gate), lag)
    return route


@pytest.mark.parametrize("wl", sorted(PLANS))
@pytest.mark.parametrize("peak", ["19999", "-19999", "0", "neg"])
@pytest.mark.parametrize("fused_always", [False, True])
def test_single_pair_decimated_tiles(oracle, wl, peak, fused_always):
    """one pair: the decimated inverse, tile pair step, small plan as two kernels -- also under small_fused_always, because a
    batch that refines reads V', which the fused small plan never writes"""
    import tdoa_amd
    a, b, want = _pair(oracle, wl, peak)
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        c.debug_flags(small_fused_always=fused_always)
        r = _pair_vs_oracle(oracle, c, a, b, want)
        assert tuple(c.plan_info()[1:]) == PLANS[wl]
    assert (r["inverse"], r["pair_step"], r["small_fused"], r["pruned"]) == ("decimated", "tiles", False, True)


@pytest.mark.parametrize("wl", sorted(PLANS))
@pytest.mark.parametrize("peak", ["19999", "-19999", "0", "neg"])
def test_single_pair_full_inverse(oracle, wl, peak):
    """TDOA_DEBUG_NO_DECIMATE at 20 000 lags: the full inverse with the pruned column pass; neighbours out of V"""
    import tdoa_amd
    a, b, want = _pair(oracle, wl, peak)
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        c.debug_flags(no_decimate=True)
        r = _pair_vs_oracle(oracle, c, a, b, want)
    assert (r["inverse"], r["pruned"]) == ("full", True)


def _captures(oracle, n_stations, wl, wpb, seed):
    """n_stations captures of three blocks of wpb windows each; station delays below 400 samples"""
    rng = np.random.default_rng(seed)
    delays = [int(x) for x in rng.integers(0, 400, size=n_stations)]
    caps = [np.concatenate([oracle.simulate_delayed_fm(wpb * wl, d, 500 + k, 100 * (s + 1) + k) for k in range(3)])
            for s, d in enumerate(delays)]
    return caps, delays


def _run_batch(c, caps, **flags):
    """upload, warm up (another gate: the step graph is captured again for the call under test), poison, process_fine;
    then poison again and replay"""
    for s, cap in enumerate(caps):
        c.capture_upload(s, cap)
    c.debug_flags(**flags)
    c.process_fine(GATE / 2)
    c.poison_workspace()
    peaks, fine = c.process_fine(GATE)
    route = c.last_route()
    assert np.isfinite(fine["y"]).all() and np.isfinite(fine["frac"]).all(), "the refinement read workspace it did not write"
    c.poison_workspace()
    peaks2, fine2 = c.process_fine(GATE)
    assert c.last_route() == route
    assert np.array_equal(peaks2, peaks) and np.array_equal(fine2, fine)
    return peaks, fine, route


def _units_vs_oracle(oracle, caps, delays, wl, wpb, peaks, fine, units):
    n = len(caps)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    pre = {}

    def station_window(s, wid):
        if (s, wid) not in pre:
            off = (wid // wpb) * (wpb * wl) + (wid % wpb) * wl
            pre[(s, wid)] = oracle.b_preprocess(caps[s][2 * off:2 * (off + wl)])[0]
        return pre[(s, wid)]

    for wid, p in units:
        i, j = pairs[p]
        t, s = station_window(i, wid), station_window(j, wid)
        olag, ocorr, _ = oracle.b_xcorr_peak_fft(t, s, ML)
        g = peaks[wid, p]
        lag = int(g["lag"])
        assert lag == olag == delays[j] - delays[i], (wid, (i, j), lag, olag)
        assert abs(float(g["corr"]) - ocorr) <= 1e-5 * abs(ocorr), (wid, (i, j))
        _check(fine[wid, p], oracle.b_refine_peak(t, s, lag, GATE), lag)


@pytest.mark.parametrize("wl", sorted(PLANS))
@pytest.mark.parametrize("once", [True, False])
def test_batch_staged_walk(oracle, wl, once):
    """3 stations x 3 windows: the LDS-staged column walk next to a loader wave; single-look K1 on and off"""
    import tdoa_amd
    caps, delays = _captures(oracle, 3, wl, 1, 11)
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        peaks, fine, r = _run_batch(c, caps, no_k1_once=not once)
        assert c.last_k1(0)[1] == once
    assert (r["inverse"], r["pair_step"], r["stg_folded"], r["once"], r["small_fused"]) == ("decimated", "staged", False, once, False)
    assert peaks.shape == (3, 3)
    _units_vs_oracle(oracle, caps, delays, wl, 1, peaks, fine, [(w, p) for w in range(3) for p in range(3)])


@pytest.mark.parametrize("wl", sorted(PLANS))
@pytest.mark.parametrize("n_stations,flags,step", [
    (2, {}, "tiles"),                                                   # one pair, two stations: the library picks the tile form
    (5, {"dec_cols_always": True, "no_dec_staged": True}, "columns"),   # one pair-window per wave from memory
])
def test_batch_tiles_and_per_pair_walk(oracle, wl, n_stations, flags, step):
    import tdoa_amd
    caps, delays = _captures(oracle, n_stations, wl, 1, 20 + n_stations)
    n_pairs = n_stations * (n_stations - 1) // 2
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        peaks, fine, r = _run_batch(c, caps, **flags)
    assert (r["inverse"], r["pair_step"], r["small_fused"]) == ("decimated", step, False)
    _units_vs_oracle(oracle, caps, delays, wl, 1, peaks, fine, [(w, p) for w in range(3) for p in range(n_pairs)])


def test_library_default_at_a_thousand_pair_windows(oracle, capsys):
    """16 stations x 9 windows of 1 100 000 samples: 1 080 pair-windows in one launch, where process() takes the fused small
    plan.  process_fine takes the two kernels: its peaks are process()'s bit for bit, its records those of a context that
    never fuses (TDOA_DEBUG_NO_SMALL_FUSED), and a seeded sample of 64 pair-windows matches the oracle."""
    import tdoa_amd
    wl, wpb, n = 1_100_000, 3, 16
    caps, delays = _captures(oracle, n, wl, wpb, 16)
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        for s, cap in enumerate(caps):
            c.capture_upload(s, cap)
        base = c.process()
        r0 = c.last_route()
        peaks, fine, r = _run_batch(c, caps)
    assert base.shape == (9, 120)
    assert (r0["inverse"], r0["pair_step"], r0["stg_folded"], r0["small_fused"]) == ("decimated", "staged", True, True)
    assert (r["inverse"], r["pair_step"], r["stg_folded"], r["small_fused"]) == ("decimated", "staged", True, False)
    assert np.array_equal(peaks, base)
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        peaks_two, fine_two, r_two = _run_batch(c, caps, no_small_fused=True)
    assert r_two == r
    assert np.array_equal(peaks_two, peaks) and np.array_equal(fine_two, fine)
    rng = np.random.default_rng(1080)
    units = [(int(u) // 120, int(u) % 120) for u in rng.choice(9 * 120, size=64, replace=False)]
    _units_vs_oracle(oracle, caps, delays, wl, wpb, peaks, fine, units)
    with capsys.disabled():
        print("\n  16 stations x 9 windows: route %r; 64 of 1080 pair-windows vs ob_refine_peak" % (r,))
