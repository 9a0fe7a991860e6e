"""GPU: tdoa_params' optional K1 steps -- k1_smooth = W (the prebuilt reference binary's applyLowPassFilter(W) on its
discriminator output) and k1_gate (its power gate: windows of mean power <= 0.01 carry envelope codes) -- at the geometry
the binary runs them at, at the edges of their kernels, and under TDOA_LAGS_GO, against the f64 oracle.

Either option keeps K1's codes in memory, so fused and single-look K1 are off (plan_fm_batch) and the decimated inverse runs
on its own chain: k_fm_demod<true> -> k_k1_power -> k_k1_envelope -> k_k1_smooth into codes_lp, the code-reading forward
column pass (k_fwd_col256_c16 on the 4096 x 256 plan, k_fwd_colx_c16 on 4096 x 512), the row pass, the staged column walk
(loader-wave and folded forms) and the small plan (fused, or two kernels).

1. Batches at max_lag 20 000 with (k1_smooth, k1_gate) in (10, 0), (0, 1), (10, 1), each on poisoned workspace, the route
   asserted.  Some stations are AM captures (mean power ~0.003-0.007: the envelope class under the gate), the others delayed
   FM, and one station switches class between blocks -- so windows pair an envelope row with a discriminator row, and a
   launch group holds windows of different class mixes.  Every sampled (window, pair) is held against ob_preprocess_gate +
   b_xcorr_peak_fft on the bytes read back from the device (lag identical, corr within 1e-5), two per batch against the
   independent float64 pipeline, and where both stations carry the common message (same class under the gate; both FM
   without it) the lag is the geometry's.
2. The option kernels' edges bit for bit (Context.fm_preprocess against ob_preprocess_smooth / ob_preprocess_gate): widths
   2 .. 2001, windows shorter than the half-window, tails at k_k1_smooth's 2048-sample chunks, the gate at equality.
3. TDOA_LAGS_GO: K1 and its statistics over the whole window (processor.go's preprocessSignal), the transforms over the
   template's first B corr_block codes."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import float_pipeline as fp
from test_gpu_fine import _check
from test_k1_options_cpu import WIDTHS, edge_lengths, threshold_capture

pytestmark = pytest.mark.gpu

ML = 20000
OPTIONS = [(10, 0), (0, 1), (10, 1)]
FINE_GATE = 4.0               # samples: case (a)'s pair (1, 2) lies 3 samples apart, its others further
# f64 FFT correlations of the sampled units run side by side (numpy's FFT releases the GIL); a few hundred MB each
THREADS = max(1, min(8, int(os.environ.get("OMP_NUM_THREADS", "8"))))

# case: (stations, window length, windows per block, delays, {station: blocks where it is an AM capture})
_RNG_B, _RNG_D = np.random.default_rng(80), np.random.default_rng(160)
CASES = {
    "a": (3, 2_000_000, 1, [0, 150, 153], {0: (0, 1, 2), 2: (1,)}),
    "b": (8, 1_100_000, 1, [int(x) for x in _RNG_B.integers(0, 400, size=8)], {0: (0, 1, 2), 5: (0, 1, 2), 7: (1,)}),
    "c": (4, 2_200_001, 1, [0, -123, 64, 1500], {1: (0, 1, 2), 3: (2,)}),
    "d": (16, 1_100_000, 3, [int(x) for x in _RNG_D.integers(0, 400, size=16)], {3: (0, 1, 2), 11: (0, 1, 2), 14: (1,)}),
}
_BASE = 400                   # every station's delay is _BASE + delay: inside am_capture's range [0, 2048]

_cached = {}


def _captures(oracle, case):
    """three blocks per station: fp.am_capture (one message per block, amplitude 0.05 .. 0.08) where the case says so,
    oracle.simulate_delayed_fm (one content per block) elsewhere.  Kept for the next option of the same case."""
    if case not in _cached:
        _cached.clear()
        n_st, wl, wpb, delays, am = CASES[case]
        blk = wl * wpb
        caps = []
        for s, d in enumerate(delays):
            caps.append(np.concatenate([
                fp.am_capture(blk, _BASE + d, 0.05 + 0.01 * (s % 4), 60 + k, s) if k in am.get(s, ())
                else oracle.simulate_delayed_fm(blk, _BASE + d, 900 + k, 100 * (s + 1) + k) for k in range(3)]))
        _cached[case] = caps
    return _cached[case]


def _is_am(case, s, wid):
    return (wid // CASES[case][2]) in CASES[case][4].get(s, ())


def _carries(case, gate, i, j, wid):
    """both stations carry the block's common message: the same class under the gate; without it only the FM stations do
    (an AM capture's discriminator output is its own phase walk)"""
    a, b = _is_am(case, i, wid), _is_am(case, j, wid)
    return a == b if gate else not (a or b)


def _run(c, caps, **kw):
    """one step on other data of the same shape (the captures one station on: every buffer of the step written with other
    values -- the poison reaches the float workspaces only, not the code rows, statistics or power sums), poison, then the
    step under test on `caps`"""
    for s, cap in enumerate(caps[1:] + caps[:1]):
        c.capture_upload(s, cap)
    c.process(**kw)
    for s, cap in enumerate(caps):
        c.capture_upload(s, cap)
    c.poison_workspace()
    return c.process(**kw)


def _sample_units(pairs, n_windows, groups, n_units, seed, kinds):
    """every unit when n_units is None; else a seeded sample of n_units that holds a unit of every staged-walk group, the first
    and the last window, and a unit of every class mix (kinds: unit -> key)"""
    all_units = [(w, p) for w in range(n_windows) for p in range(len(pairs))]
    if n_units is None:
        return all_units
    rng = np.random.default_rng(seed)
    units = {(0, int(rng.integers(len(pairs)))), (n_windows - 1, int(rng.integers(len(pairs))))}
    for _, members in groups:
        units.add((int(rng.integers(n_windows)), int(rng.choice(members))))
    by_kind = {}
    for u in all_units:
        by_kind.setdefault(kinds(u), []).append(u)
    for k in sorted(by_kind):
        units.add(by_kind[k][int(rng.integers(len(by_kind[k])))])
    while len(units) < n_units:
        units.add(all_units[int(rng.integers(len(all_units)))])
    return sorted(units)


def _check_units(oracle, c, case, smooth, gate, peaks, units, tag, capsys):
    n_st, wl, wpb, delays, _ = CASES[case]
    pairs = [(i, j) for i in range(n_st) for j in range(i + 1, n_st)]
    raw, pre = {}, {}
    for wid, p in units:
        for s in pairs[p]:
            if (s, wid) not in pre:
                raw[(s, wid)] = c.capture_download(s, (wid // wpb) * wpb * wl + (wid % wpb) * wl, wl)
                code, _, cls = oracle.b_preprocess_gate(raw[(s, wid)], window=smooth, gate=gate)
                assert cls == int(bool(gate) and _is_am(case, s, wid)), (tag, s, wid)       # the capture is where it should be
                pre[(s, wid)] = code
    # two units against the float64 pipeline: one whose stations carry the message in FM, one in AM where the gate makes
    # that an envelope pair
    fm_units = [u for u in units if _carries(case, gate, *pairs[u[1]], u[0]) and not _is_am(case, pairs[u[1]][0], u[0])]
    am_units = [u for u in units if _carries(case, gate, *pairs[u[1]], u[0]) and _is_am(case, pairs[u[1]][0], u[0])]
    float_units = [fm_units[0], am_units[0] if gate and am_units else fm_units[-1]]

    def unit(u):
        wid, p = u
        i, j = pairs[p]
        return oracle.b_xcorr_peak_fft(pre[(i, wid)], pre[(j, wid)], ML)[:2]

    def float_unit(u):
        wid, p = u
        i, j = pairs[p]
        return fp.xcorr_peak_u8(raw[(i, wid)], raw[(j, wid)], ML, smooth=smooth, gate=bool(gate))[:2]

    with ThreadPoolExecutor(THREADS) as ex:
        want = list(ex.map(unit, units))
        fwant = list(ex.map(float_unit, float_units))
    worst, n_geo = 0.0, 0
    for (wid, p), (olag, ocorr) in zip(units, want):
        i, j = pairs[p]
        g = peaks[wid, p]
        assert int(g["lag"]) == olag, (tag, wid, (i, j), int(g["lag"]), olag)
        dev = abs(float(g["corr"]) - ocorr) / abs(ocorr)
        worst = max(worst, dev)
        assert dev < 1e-5, (tag, wid, (i, j), dev)
        if _carries(case, gate, i, j, wid):
            assert olag == delays[j] - delays[i], (tag, wid, (i, j), olag)
            n_geo += 1
    rows = []
    for (wid, p), (flag, fcorr) in zip(float_units, fwant):
        g = peaks[wid, p]
        fdev = abs(float(g["corr"]) - fcorr) / abs(fcorr)
        assert int(g["lag"]) == flag and fdev < 1e-5, (tag, wid, pairs[p], fdev)
        rows.append((wid, pairs[p][0], pairs[p][1], flag, fcorr, fdev))
    with capsys.disabled():
        print("\n  %s: %d of %d pair-windows vs ob_* (f64 FFT), %d at the geometry's lag: lag identical, worst |dcorr|/|corr| %.2e"
              % (tag, len(units), peaks.size, n_geo, worst))
        for r in rows:
            print("    window %d pair %d-%d lag %6d corr %12.5f  vs float64 pipeline %.2e" % r)
    return pre


ROUTE = dict(inverse="decimated", pair_step="staged", col_pass="c256", row_pass="unpack_blocks", fused_k1=False, once=False,
             small_fused=False, stg_folded=False)
EXPECT = {
    "a": (ROUTE, None),
    "b": (ROUTE, 24),
    "c": (dict(ROUTE, col_pass="colx"), None),
    "d": (dict(ROUTE, stg_folded=True, small_fused=True), 48),
}


@pytest.mark.parametrize("case,smooth,gate", [(case, s, g) for case in "abcd" for s, g in OPTIONS])
def test_decimated_batch_with_the_options(oracle, case, smooth, gate, capsys):
    """(a) 3 stations x 3 windows of 2 000 000 (cfg2's shape, 4096 x 256), also through process_fine; (b) 8 stations x 3 windows
    of 1 100 000 (two loader-wave groups); (c) 4 stations x 3 windows of 2 200 001 (4096 x 512: k_fwd_colx_c16); (d) 16
    stations x 9 windows of 1 100 000 (1080 pair-windows in one launch: the folded walk and the fused small plan).  (a) and (d)
    give the same bytes with two windows per launch group and split over two ranks."""
    import tdoa_amd
    from tdoa_amd import sharding
    n_st, wl, wpb, delays, _ = CASES[case]
    caps = _captures(oracle, case)
    n_pairs, n_windows = n_st * (n_st - 1) // 2, 3 * wpb
    kw = dict(max_lag=ML, window_len=wl, k1_smooth=smooth, k1_gate=gate)
    route_want, n_units = EXPECT[case]
    with tdoa_amd.Context(**kw) as c:
        peaks = _run(c, caps)
        route = c.last_route()
        assert not c.last_k1(0)[1]                                   # no single-look K1: the options need the codes
        assert tuple(c.plan_info())[1:] == ((4096, 512) if case == "c" else (4096, 256))
        assert {k: route[k] for k in route_want} == route_want, route
        assert peaks.shape == (n_windows, n_pairs)
        if case in "ad":
            parts = [_run(c, caps, rank=r, world=2) for r in range(2)]
            merged = sharding.merge_sharded(np.stack([sharding.peaks_as_bytes(p) for p in parts]), n_windows, n_pairs)
            assert np.array_equal(merged, peaks)
        if case == "a":
            # (e) the refinement: the two-kernel small plan (a batch that refines reads V'), the same peaks as process()
            # (the warm-up with another gate captures the step graph again for the call under test)
            c.process_fine(FINE_GATE / 2)
            c.poison_workspace()
            fpeaks, fine = c.process_fine(FINE_GATE)
            assert c.last_route() == route
            assert np.array_equal(fpeaks, peaks)
        pairs = [(i, j) for i in range(n_st) for j in range(i + 1, n_st)]
        groups = tdoa_amd.capi.staged_groups(n_st, 16 if route["stg_folded"] else 15)
        if case == "b":
            assert len(groups) == 2
        kinds = lambda u: (_is_am(case, pairs[u[1]][0], u[0]), _is_am(case, pairs[u[1]][1], u[0]))     # noqa: E731
        units = _sample_units(pairs, n_windows, groups, n_units, 1000 + ord(case), kinds)
        tag = "(%s) %d stations x %d windows of %d, k1_smooth %d k1_gate %d" % (case, n_st, n_windows, wl, smooth, gate)
        pre = _check_units(oracle, c, case, smooth, gate, peaks, units, tag, capsys)
    if case in "ad":
        with tdoa_amd.Context(windows_per_batch=2, **kw) as c:
            grouped = _run(c, caps)
        assert np.array_equal(grouped, peaks)
    if case == "a":
        for wid, p in units:
            i, j = pairs[p]
            lag = int(peaks[wid, p]["lag"])
            _check(fine[wid, p], oracle.b_refine_peak(pre[(i, wid)], pre[(j, wid)], lag, FINE_GATE), lag)
        assert fine["plausible"].any() and not fine["plausible"].all()


# ---- 2. the option kernels' edges, bit for bit ----------------------------------------------------------------------------

def _same(c, x, want, ost):
    got, st = c.fm_preprocess(x)
    assert (st.s1, st.s2_lo, st.s2_hi) == (ost.s1, ost.s2_lo, ost.s2_hi)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return got


@pytest.mark.parametrize("window", WIDTHS)
def test_smoothing_edges_bit_for_bit(oracle, window):
    """k_k1_smooth at width W (half-window W // 2) on windows of 1, 2, 7 samples, h - 1, h, h + 1, around its 2048-sample
    chunks; W = 2001 also on 2 000 000 samples.  With the gate on as well: an AM window (envelope class, not smoothed) and an
    FM window (smoothed) of every length"""
    import tdoa_amd
    n_long = 2_000_000 if window == 2001 else 16385
    fm = oracle.simulate_delayed_fm(n_long, 0, 9, 1)
    am = fp.am_capture(16385, 0, 0.07, 3, 1)
    lengths = edge_lengths(window)
    with tdoa_amd.Context(max_lag=100, window_len=16385, k1_smooth=window) as c:
        for n in sorted(set(lengths + [n_long]), reverse=True):       # longest first: stale rows beyond every window
            _same(c, fm[:2 * n], *oracle.b_preprocess_smooth(fm[:2 * n], window))
    with tdoa_amd.Context(max_lag=100, window_len=16385, k1_smooth=window, k1_gate=1) as c:
        for n in lengths[::-1]:
            for x in (fm[:2 * n], am[:2 * n]):
                _same(c, x, *oracle.b_preprocess_gate(x, window=window, gate=1)[:2])
        assert oracle.b_preprocess_gate(am, window=window)[2] == 1 and oracle.b_preprocess_gate(fm[:2 * 16385])[2] == 0


def test_gate_at_its_threshold_bit_for_bit(oracle):
    """a capture with 100 M == 65025 n exactly (the envelope class) and one with M + 8 (the discriminator class), n a multiple
    of 32 from one block to 2 000 000 samples, through k_k1_power's exact sums and k1_envelope_class; without and with
    k1_smooth = 10 (which an envelope window skips)"""
    import tdoa_amd
    with tdoa_amd.Context(max_lag=100, window_len=2048, k1_gate=1) as c, \
            tdoa_amd.Context(max_lag=100, window_len=2048, k1_gate=1, k1_smooth=10) as cs:
        for n in (32, 2048, 16416, 2_000_000):
            for above, cls in ((False, 1), (True, 0)):
                x = threshold_capture(n, above=above, seed=n)
                assert oracle.b_envelope_class(oracle.b_power_sum(x), n) == cls
                for ctx, w in ((c, 0), (cs, 10)):
                    want, ost, ocls = oracle.b_preprocess_gate(x, window=w, gate=1)
                    assert ocls == cls
                    got = _same(ctx, x, want, ost)
                    # the GPU took the branch of its class: the discriminator chain's output iff class 0
                    disc = oracle.b_preprocess_smooth(x, w)[0]
                    assert np.array_equal(got.view(np.uint32), disc.view(np.uint32)) == (cls == 0), (n, above, w)


# ---- 3. TDOA_LAGS_GO --------------------------------------------------------------------------------------------------------

GO_ML, GO_CB = 2000, 100_000


def _go_inputs(oracle, smooth, gate):
    """(template, signal, delay): a template of 299 999 samples whose first B = 2 blocks of 100 000 (corr_len 200 000) are
    what the transforms see, and whose tail makes K1 over the whole window differ from K1 over the cut -- with k1_smooth,
    FM of three times the modulation index (other statistics); with k1_gate, a head of mean power 0.012 (discriminator
    class on its own) and a faint tail that brings the whole window to 0.008 (envelope class)"""
    nt, ns, delay = 299_999, 301_500, 777
    if gate:
        t = np.concatenate([fp.am_capture(200_000, 0, 0.105, 41, 1), fp.am_capture(nt - 200_000, 0, 0.02, 42, 1)])
        s = fp.am_capture(ns, delay, 0.07, 41, 2)
    else:
        t = np.concatenate([oracle.simulate_delayed_fm(200_000, 0, 31, 1),
                            oracle.simulate_delayed_fm(nt - 200_000, 0, 32, 3, mod_index=3.0)])
        s = oracle.simulate_delayed_fm(ns, delay, 31, 2)
    return t, s, delay


@pytest.mark.parametrize("smooth,gate", [(10, 0), (0, 1)])
def test_go_lag_set_with_the_options(oracle, smooth, gate, capsys):
    """processor.go runs preprocessSignal on the whole template, then cuts it to its first B corr_block samples.  Expected:
    ob_preprocess_gate over the whole template (smoothed, or gated, and normalised with the whole window's statistics), cut to
    corr_len; the whole signal; ob_xcorr_all_lags over lags [0, eff), first strict maximum.  The library's sw_stats layout
    (K1 over the whole window, transforms over the first corr_len codes of the same row) must give exactly that, in either
    argument order; K1 over the cut alone would not (asserted on the oracle: another lag under the gate, another corr with
    the smoother).  Then tdoa_process at lag 0 on three stations, one of them AM, on the same layout."""
    import tdoa_amd
    t, s, delay = _go_inputs(oracle, smooth, gate)
    nt, ns = t.size // 2, s.size // 2
    corr_len, eff = 200_000, min(GO_ML, ns - nt)
    full, _, cls_t = oracle.b_preprocess_gate(t, window=smooth, gate=gate)
    sig, _, cls_s = oracle.b_preprocess_gate(s, window=smooth, gate=gate)
    assert cls_t == cls_s == gate
    want = oracle.b_xcorr_all_lags(full[:corr_len], sig, GO_ML)[GO_ML - 1:GO_ML - 1 + eff]
    idx = int(np.argmax(np.abs(want)))                                     # the first strict maximum
    assert idx == delay
    cut = oracle.b_xcorr_all_lags(oracle.b_preprocess_gate(t[:2 * corr_len], window=smooth, gate=gate)[0], sig, GO_ML)
    cut = cut[GO_ML - 1:GO_ML - 1 + eff]
    assert int(np.argmax(np.abs(cut))) != delay if gate else abs(cut[delay] - want[delay]) > 0.1 * abs(want[delay])
    kw = dict(max_lag=GO_ML, window_len=ns, corr_block=GO_CB, lag_mode=tdoa_amd.capi.LAGS_GO, k1_smooth=smooth, k1_gate=gate)
    with tdoa_amd.Context(**kw) as c:
        c.fm_xcorr(s[::-1].copy(), t[::-1].copy(), GO_ML)           # other data of the same lengths first
        c.poison_workspace()
        for a, b in ((t, s), (s, t)):
            lag, corr = c.fm_xcorr(a, b, GO_ML)
            lags = c.fm_xcorr_lags(a, b, GO_ML)
            assert not c.last_k1(0)[1]
            assert lag == idx and abs(corr - want[idx]) <= 1e-5 * abs(want[idx]), (lag, corr, want[idx])
            got = lags[GO_ML - 1:GO_ML - 1 + eff]
            lag_err = np.abs(got - want).max() / np.abs(want).max()
            assert lag_err <= 1e-5
            assert not lags[:GO_ML - 1].any() and not lags[GO_ML - 1 + eff:].any()
    # tdoa_process: every window has one length, so lag 0 only over the first corr_len samples of each window
    blk = wl = 70_000
    n_cut = (wl - 1) // 1000 * 1000
    caps = [np.concatenate([oracle.simulate_delayed_fm(blk, 100, 310 + k, 10 * st + k) for k in range(3)]) for st in range(2)]
    caps.append(np.concatenate([fp.am_capture(blk, 100, 0.06, 70 + k, 2) for k in range(3)]))
    with tdoa_amd.Context(max_lag=ML, window_len=wl, lag_mode=tdoa_amd.capi.LAGS_GO, k1_smooth=smooth, k1_gate=gate) as c:
        peaks = _run(c, caps)
    assert peaks.shape == (3, 3) and not peaks["lag"].any()
    worst = 0.0
    for wid in range(3):
        pre = [oracle.b_preprocess_gate(cp[2 * wid * wl:2 * (wid + 1) * wl], window=smooth, gate=gate) for cp in caps]
        assert [p[2] for p in pre] == [0, 0, gate]
        for p, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
            gc = float(np.dot(pre[i][0][:n_cut].astype(np.float64), pre[j][0][:n_cut].astype(np.float64))) / np.sqrt(n_cut)
            err = abs(float(peaks[wid, p]["corr"]) - gc)
            worst = max(worst, err / np.sqrt(n_cut))
            # pairs with the AM station are noise at lag 0: bound of full scale there, as test_gpu_anchors' lag-0 checks
            assert err <= 1e-5 * abs(gc) + 1e-6 * np.sqrt(n_cut), (wid, p, peaks[wid, p], gc)
    with capsys.disabled():
        print("\n  TDOA_LAGS_GO, k1_smooth %d k1_gate %d: template %d (first %d), signal %d, %d lags: index %d, lag array within "
              "%.2e of its peak; tdoa_process lag 0 within %.2e of full scale" % (smooth, gate, nt, corr_len, ns, eff, lag, lag_err, worst))
