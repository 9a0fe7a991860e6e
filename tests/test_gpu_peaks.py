"""GPU: per-pair-window correlation surfaces (tdoa_process_lags) and the K strongest separate peaks (tdoa_process_peaks,
tdoa_fm_xcorr_peaks_u8, tdoa_debug_select_peaks) on every route the step can take.

Each route case starts on a fresh context and asserts the route it is named for (Context.last_route), then holds:
- process_peaks(k = 1) to process() byte for byte, and peak 1 of process_peaks(k = 8) likewise;
- the surfaces to fm_xcorr_lags of the same two windows (1e-6 of the peak) and to the float64 oracle (2e-6 of the peak);
- the surfaces after poison_workspace, and from the replayed step graph, to the same bytes, without NaN;
- the selected peaks to the float64 rule (tdoa_amd.peaks) applied to the oracle's surfaces."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, SEP = 8, 8


def _captures(oracle, n_stations, wl, wpb, seed, max_delay=400):
    rng = np.random.default_rng(seed)
    delays = [int(x) for x in rng.integers(0, max_delay, size=n_stations)]
    caps = [np.concatenate([oracle.simulate_delayed_fm(wpb * wl, d, 500 + k, 100 * (s + 1) + k) for k in range(3)])
            for s, d in enumerate(delays)]
    return caps, delays


def _window(cap, wid, wl, wpb):
    off = (wid // wpb) * (wpb * wl) + (wid % wpb) * wl
    return cap[2 * off:2 * (off + wl)]


def _same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _record_is_surface_max(rec, s, ml):
    """no tolerance: float32(rec.corr) is s[rec.lag + ml - 1], sign included, rec.abs_corr its magnitude, that magnitude is
    max |s|, rec.lag the first lag in the key's order that holds it; max |s| = 0: the zero record (tdoa_amd.peaks)"""
    from tdoa_amd.peaks import record_is_surface_max
    return record_is_surface_max(rec, s, ml)


def _check_rule(got, cnt, want_surface, ml):
    """the kernel's records against the rule on the oracle's float64 surface: lags equal while the oracle's order is
    unambiguous (consecutive candidates more than 1e-5 apart, relative), magnitudes within 2e-6 of the peak"""
    from tdoa_amd.peaks import select_peaks
    want = select_peaks(want_surface, -(ml - 1), K, SEP)
    peak = abs(want[0][1])
    assert cnt == len(want)
    for r, (lag, v) in enumerate(want):
        assert abs(float(got[r]["corr"]) - v) <= 2e-6 * peak or int(got[r]["lag"]) != lag, (r, lag)
        if int(got[r]["lag"]) != lag:
            nxt = abs(want[r + 1][1]) if r + 1 < len(want) else 0.0
            assert abs(abs(v) - nxt) <= 1e-5 * abs(v), ("lag differs where the order is clear", r, lag, int(got[r]["lag"]))
            break
    assert np.all(got[cnt:]["lag"] == 0) and np.all(got[cnt:]["corr"] == 0.0)


def _route_case(oracle, c, caps, wl, wpb, ml, check_units=2, **flags):
    for s, cap in enumerate(caps):
        c.capture_upload(s, cap)
    c.debug_flags(**flags)
    base = c.process()
    route = c.last_route()
    one, cnt1 = c.process_peaks(1, SEP)
    assert _same_bytes(np.ascontiguousarray(one[..., 0]), base), "k = 1 is not tdoa_process"
    assert np.all(cnt1 == (base["abs_corr"] > 0))
    pk, cnt = c.process_peaks(K, SEP)
    assert c.last_route() == route
    assert _same_bytes(np.ascontiguousarray(pk[..., 0]), base)
    info = c.graph_info()
    assert info["memsets"] == 0 and info["roots"] == 1
    pk_again, cnt_again = c.process_peaks(K, SEP)                       # replayed graph
    assert _same_bytes(pk_again, pk) and np.array_equal(cnt_again, cnt)
    c.poison_workspace()
    lags = c.process_lags()
    assert np.isfinite(lags).all()
    c.poison_workspace()
    assert _same_bytes(c.process_lags(), lags)                          # replayed on poisoned workspace
    c.poison_workspace()
    pk_p, _ = c.process_peaks(K, SEP)
    assert _same_bytes(pk_p, pk)
    # at every pair-window's peak lag the surface holds the peak's value
    w, p = base.shape
    idx = base["lag"].astype(np.int64) + ml - 1
    at = np.take_along_axis(lags, idx[..., None], axis=2)[..., 0]
    assert np.allclose(at, base["corr"], rtol=1e-6, atol=0)
    # ... and, with no tolerance, every record is its own surface's maximum (the key's order decides ties)
    for wid in range(w):
        for q in range(p):
            _record_is_surface_max(base[wid, q], lags[wid, q], ml)
            _record_is_surface_max(pk[wid, q, 0], lags[wid, q], ml)
    n = len(caps)
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    rng = np.random.default_rng(len(caps) * 1000 + wl)
    units = [(int(u) // p, int(u) % p) for u in rng.choice(w * p, size=min(check_units, w * p), replace=False)]
    pair_lags = []
    for wid, q in units:
        i, j = pairs[q]
        a, b = _window(caps[i], wid, wl, wpb), _window(caps[j], wid, wl, wpb)
        ta, _ = oracle.b_preprocess(a)
        tb, _ = oracle.b_preprocess(b)
        _, _, want = oracle.b_xcorr_peak_fft(ta, tb, ml)
        peak = np.abs(want).max()
        assert np.abs(lags[wid, q] - want).max() <= 2e-6 * peak, (wid, q)
        _check_rule(pk[wid, q], int(cnt[wid, q]), want, ml)
        pair_lags.append((wid, q, a, b))
    for wid, q, a, b in pair_lags:                                      # (the pair calls change the context's graph)
        pl = c.fm_xcorr_lags(a, b, ml)
        assert np.abs(lags[wid, q] - pl).max() <= 1e-6 * np.abs(pl).max(), (wid, q)
    return route, base, lags, pk


@pytest.mark.parametrize("form", ["segments", "short_lag", "full"])
def test_short_ranges(oracle, form):
    """300 lags on 70 000-sample windows: the segment form, the short-lag inverse, the general pruned form"""
    import tdoa_amd
    ml, wl = 300, 70_000
    caps, _ = _captures(oracle, 3, wl, 2, 3, max_delay=200)
    flags = {"segments": {}, "short_lag": {"no_segment_form": True}, "full": {"no_segment_form": True, "no_short_lag": True}}[form]
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        r, *_ = _route_case(oracle, c, caps, wl, 2, ml, **flags)
    assert r["inverse"] == form


@pytest.mark.parametrize("once", [True, False])
def test_decimated_tiles_single_look_and_sharding(oracle, once):
    """2 stations at the reference's 20 000 lags: the decimated inverse with the tile pair step; single-look K1 on and off;
    rank / world sharding zero-fills the other rank's windows and gives this rank's windows the same bytes"""
    import tdoa_amd
    ml, wl = 20000, 1_100_000
    caps, _ = _captures(oracle, 2, wl, 1, 7)
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        r, base, lags, pk = _route_case(oracle, c, caps, wl, 1, ml, no_k1_once=not once)
        assert c.last_k1(0)[1] == once
        for rank in range(2):
            lr = c.process_lags(rank=rank, world=2)
            pr, cr = c.process_peaks(K, SEP, rank=rank, world=2)
            mine = np.arange(lr.shape[0]) % 2 == rank
            assert _same_bytes(lr[mine], lags[mine]) and not lr[~mine].any()
            assert _same_bytes(pr[mine], pk[mine]) and not pr[~mine]["lag"].any() and not cr[~mine].any()
    assert (r["inverse"], r["pair_step"], r["once"]) == ("decimated", "tiles", once)


def test_decimated_columns(oracle):
    import tdoa_amd
    ml, wl = 20000, 1_100_000
    caps, _ = _captures(oracle, 5, wl, 1, 25)
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        r, *_ = _route_case(oracle, c, caps, wl, 1, ml, dec_cols_always=True, no_dec_staged=True)
    assert (r["inverse"], r["pair_step"], r["small_fused"]) == ("decimated", "columns", False)


def test_staged_walk_not_folded(oracle):
    import tdoa_amd
    ml, wl = 20000, 1_100_000
    caps, _ = _captures(oracle, 3, wl, 1, 11)
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        r, *_ = _route_case(oracle, c, caps, wl, 1, ml)
    assert (r["inverse"], r["pair_step"], r["stg_folded"]) == ("decimated", "staged", False)


def test_staged_folded_and_small_fused(oracle):
    """16 stations x 9 windows: 1 080 pair-windows in one launch -- the folded staged walk with the fused small plan; then
    the same captures through the two-kernel small plan"""
    import tdoa_amd
    ml, wl, wpb = 20000, 1_100_000, 3
    caps, _ = _captures(oracle, 16, wl, wpb, 16)
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        r, base, lags, pk = _route_case(oracle, c, caps, wl, wpb, ml)
        assert base.shape == (9, 120)
    assert (r["inverse"], r["pair_step"], r["stg_folded"], r["small_fused"]) == ("decimated", "staged", True, True)
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        r2, base2, lags2, pk2 = _route_case(oracle, c, caps, wl, wpb, ml, no_small_fused=True)
    assert (r2["pair_step"], r2["stg_folded"], r2["small_fused"]) == ("staged", True, False)
    assert np.array_equal(base2["lag"], base["lag"])
    assert np.abs(lags2 - lags).max() <= 1e-6 * np.abs(lags).max()


@pytest.mark.parametrize("pow2", [False, True])
def test_full_inverse_no_decimate(oracle, pow2):
    import tdoa_amd
    ml, wl = 20000, 1_100_000
    caps, _ = _captures(oracle, 3, wl, 1, 31)
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        r, *_ = _route_case(oracle, c, caps, wl, 1, ml, no_decimate=True, pow2_only=pow2)
    assert (r["inverse"], r["pruned"]) == ("full", True)


def test_two_paths(oracle):
    """one capture whose second station hears the emitter over path d1 for the first 60 % of the window and over d2 after
    that: the two strongest separate peaks are d1 then d2; a separation wider than |d1 - d2| leaves d2 out"""
    import tdoa_amd
    n, ml, d1, d2 = 1_100_000, 20000, 137, 177
    cut = int(0.6 * n)
    a = oracle.simulate_delayed_fm(n, 0, 4242, 1)
    b = np.concatenate([oracle.simulate_delayed_fm(n, d1, 4242, 2)[:2 * cut], oracle.simulate_delayed_fm(n, d2, 4242, 3)[2 * cut:]])
    with tdoa_amd.Context(max_lag=ml, window_len=n) as c:
        pk, cnt = c.fm_xcorr_peaks(a, b, ml, K, 8)
        assert cnt == K
        assert (int(pk[0]["lag"]), int(pk[1]["lag"])) == (d1, d2)
        assert pk[0]["abs_corr"] > pk[1]["abs_corr"] > 2 * pk[2]["abs_corr"]
        lag, corr = c.fm_xcorr(a, b, ml)
        assert lag == d1 and pk[0]["corr"] == corr
        wide, _ = c.fm_xcorr_peaks(a, b, ml, K, 50)
        assert int(wide[0]["lag"]) == d1 and d2 not in [int(x) for x in wide["lag"]]
        ta, _ = oracle.b_preprocess(a)
        tb, _ = oracle.b_preprocess(b)
        _, _, want = oracle.b_xcorr_peak_fft(ta, tb, ml)
        _check_rule(pk, cnt, want, ml)


def test_selection_rule_edges():
    """tdoa_debug_select_peaks against the float64 rule: a plateau, peaks at either end, NaN, all zero, fewer candidates
    than k, and random surfaces with every k and a few separations; then the key at its limits: the rank of a lag is 2 |lag|
    in 31 bits, so the entry point takes lags up to +-(2^30 - 1) (TDOA_ERR_INVALID beyond), ties between +L and -L there,
    -0.0 next to 0.0, a lone negative value at the last index, and +d against -d with opposite signs"""
    import tdoa_amd
    from tdoa_amd.peaks import select_peaks

    def run(c, s, lag_lo, k, sep):
        s = np.asarray(s, dtype=np.float32)
        got, cnt = c.debug_select_peaks(s, lag_lo, k, sep)
        want = select_peaks(s, lag_lo, k, sep)
        assert cnt == len(want), (list(s[:16]), lag_lo, k, sep)
        assert [(int(g["lag"]), float(g["corr"])) for g in got[:cnt]] == [(l, float(np.float32(v))) for l, v in want]
        assert np.all(got[cnt:]["lag"] == 0) and np.all(got[cnt:]["corr"] == 0.0)
        return got, cnt

    with tdoa_amd.Context() as c:
        got, cnt = run(c, [0.0, 1.0, 3.0, 3.0, 1.0, 0.0, 2.0, 0.5], -4, 4, 1)
        assert cnt == 2 and int(got[0]["lag"]) == -1
        run(c, [1.0, 0.0, -1.0], -1, 4, 1)
        got, cnt = run(c, [5.0, 1.0, 0.2, 1.0, 4.0], 10, 4, 1)
        assert [int(x) for x in got["lag"][:2]] == [10, 14]
        got, cnt = run(c, [0.1, 2.0, np.nan, 1.0, 0.5, 0.7, 0.2], 0, 4, 1)
        assert cnt == 1 and int(got[0]["lag"]) == 5
        got, cnt = run(c, np.zeros(9), -4, 8, 1)
        assert cnt == 0 and not got["lag"].any() and not got["abs_corr"].any()
        got, cnt = run(c, [0.0, 1.0, 0.0, -2.0, 0.0], 0, 8, 1)
        assert cnt == 2 and got[0]["corr"] == -2.0
        far = 2 ** 30 - 1                                               # the largest |lag| a key holds
        s = np.zeros(far - (far - 6) + 1)
        s[[0, 3, 6]] = [2.0, -5.0, 1.0]                                 # lags far - 6 .. far, the last one a candidate
        got, cnt = run(c, s, far - 6, 8, 1)
        assert [int(x) for x in got["lag"][:cnt]] == [far - 3, far - 6, far]
        got, cnt = run(c, s[::-1], -far, 8, 1)
        assert [int(x) for x in got["lag"][:cnt]] == [-far + 3, -far + 6, -far]
        got, cnt = run(c, [4.0, 1.0, 4.0], far - 2, 2, 1)               # a tie inside one sign: the smaller |lag|
        assert int(got[0]["lag"]) == far - 2
        got, cnt = run(c, [4.0, 1.0, 4.0], -far, 2, 1)
        assert int(got[0]["lag"]) == -far + 2
        n = 2 ** 30
        for lag_lo in (-far, n - 5):                                    # lag_lo = -(2^30 - 1) and lag_lo = 2^30 - n
            got, cnt = run(c, np.linspace(1.0, 2.0, 5), lag_lo, 4, 1)
            assert cnt == 1 and int(got[0]["lag"]) == lag_lo + 4
        # +L against -L: a surface that held both far ends would be 2^31 - 1 floats; the tie on one of 2^21 + 1 floats instead
        # (the far ends themselves: each sign on its own, above)
        L = 1 << 20
        s = np.zeros(2 * L + 1, dtype=np.float32)
        s[0], s[-1] = -3.0, 3.0
        got, cnt = run(c, s, -L, 2, 1)
        assert [(int(g["lag"]), float(g["corr"])) for g in got[:cnt]] == [(L, 3.0), (-L, -3.0)]
        s[0], s[-1] = 3.0, -3.0
        got, cnt = run(c, s, -L, 2, 1)
        assert [(int(g["lag"]), float(g["corr"])) for g in got[:cnt]] == [(L, -3.0), (-L, 3.0)]
        got, cnt = run(c, np.array([-0.0, 0.0, -0.0, 0.0], dtype=np.float32), -2, 8, 1)
        assert cnt == 0 and not got["lag"].any() and not got["corr"].any()
        got, cnt = run(c, [0.0, 0.0, 0.0, 0.0, -1.5], -2, 8, 1)          # the only value: negative, at the last index
        assert cnt == 1 and (int(got[0]["lag"]), float(got[0]["corr"]), float(got[0]["abs_corr"])) == (2, -1.5, 1.5)
        for neg_first in (True, False):                                  # equal magnitude at -d and +d, opposite signs
            v = 2.5 if neg_first else -2.5
            got, cnt = run(c, [0.0, -v, 0.0, 0.0, 0.0, 0.0, 0.0, v, 0.0], -4, 2, 1)
            assert cnt == 2 and (int(got[0]["lag"]), float(got[0]["corr"])) == (3, v)
            assert (int(got[1]["lag"]), float(got[1]["corr"])) == (-3, -v)
        for bad_lo, n_bad in [(-far - 1, 3), (far - 1, 3), (far + 1, 1), (-2 ** 31, 3), (2 ** 31 - 1, 1)]:
            with pytest.raises(tdoa_amd.TdoaError) as e:                # a lag the key cannot hold
                c.debug_select_peaks(np.ones(n_bad), bad_lo, 4, 1)
            assert e.value.status == 1
        got, cnt = run(c, [1.0, 2.0, 3.0], far - 2, 4, 1)               # ... and the last one it can
        assert cnt == 1 and int(got[0]["lag"]) == far
        rng = np.random.default_rng(9)
        for trial in range(24):
            n = int(rng.integers(1, 50000))
            s = rng.standard_normal(n).astype(np.float32)
            if trial % 3 == 0:
                s = np.round(s * 4) / 4                                 # many equal magnitudes: the tie rule decides
            run(c, s, -(n // 2), int(rng.integers(1, 17)), int(rng.integers(1, 40)))


def test_errors():
    import ctypes as C
    import tdoa_amd
    from oracle import pyoracle as o
    a = o.simulate_delayed_fm(70_000, 0, 1, 1)
    with tdoa_amd.Context(max_lag=300, window_len=70_000) as c:
        for k, sep in [(0, 8), (17, 8), (8, 0)]:
            with pytest.raises(tdoa_amd.TdoaError) as e:
                c.fm_xcorr_peaks(a, a, 300, k, sep)
            assert e.value.status == 1
            with pytest.raises(tdoa_amd.TdoaError) as e:
                c.debug_select_peaks(np.ones(5), 0, k, sep)
            assert e.value.status == 1
        for s in range(2):
            c.capture_upload(s, np.concatenate([a, a, a]))
        with pytest.raises(tdoa_amd.TdoaError) as e:
            c.process_peaks(0, 8)
        assert e.value.status == 1
        L = c._L
        assert L.tdoa_process_peaks(c._h, 0, 1, 8, 8, None, None) == 1
        assert L.tdoa_process_lags(c._h, 0, 1, None, None) == 1
        assert L.tdoa_fm_xcorr_peaks_u8(c._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), 70_000,
                                        a.ctypes.data_as(C.POINTER(C.c_uint8)), 70_000, 300, 8, 8, None, None) == 1
    with tdoa_amd.Context(max_lag=300, window_len=70_000, lag_mode=tdoa_amd.capi.LAGS_GO) as c:
        for s in range(2):
            c.capture_upload(s, np.concatenate([a, a, a]))
        for call in (lambda: c.process_peaks(8, 8), lambda: c.process_lags(), lambda: c.fm_xcorr_peaks(a, a, 300, 8, 8)):
            with pytest.raises(tdoa_amd.TdoaError) as e:
                call()
            assert e.value.status == 5
