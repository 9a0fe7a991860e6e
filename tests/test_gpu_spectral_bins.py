"""GPU: mode B against the float64 oracle one spectral bin at a time.

Every other mode-B test feeds the kernels broadband input, on which each of the Nc bins carries about 1 / Nc of a surface: an
error confined to one bin, or to the handful of bins a special case of a kernel touches, stays below every bound relative to
the peak (tests/test_spectral_inputs_cpu.py holds both halves of that statement in float64).  Here the inputs are tones and
combs of up to four tones (tests/spectral_inputs.py) placed on the bins the kernels treat specially, addressed as (k2, k1) of
the packed spectrum [k2][k1] of the plan the route runs:
  the ends k = 1, 2, Nc - 1 and N / 2 (the alternating codes: the bin-0 word's second component); the self-mirror bins Nc / 2
  and Nc / 2 +- 1; row 0 and its 4096 - k1 mirror at k1 = 1, 63, 64, 4095; row N2 / 2 at k1 = 0, 2047, 4095; the six outputs at
  either end of a column (k2 = 1, 15, 16, 95, 96, N2 - 96, N2 - 16, N2 - 1) inside a 64-column block (k1 = 30), at both block
  edges (k1 = 63, 64) and where a column has no neighbour on one side (k1 = 0, 4095).
Routes: on N = 2^21 (4096 x 256) one pair through the default route, without the single look, the pruned full inverse, the
per-pair column walk and the any-size kernels, and batches of three stations (merged staged walk with the fused small plan, with
the two-kernel small plan, unmerged) and four (six unmerged walks beside a loader wave); on N = 2^22 (4096 x 512) the default
pair route and the four-station batch; on N = 2^17 (4096 x 16) the default route and the any-size kernels at 20 000 lags and
the segment, short-lag and general forms at 300; one comb on 5 x 2^22 (4096 x 2560: unit_root_any).

Every case starts on a fresh context, asserts its route, and holds: every searched lag within 1e-5 of the oracle's peak (the
project's standing bound); a finite surface, and the same bytes from the replayed call on poisoned workspace; the returned
record to the exact rule of tdoa_amd.peaks.record_is_surface_max on the route's own surface; its |corr| within 1e-5 of the
oracle's largest |c|.  Nothing is asserted on the lag: on these inputs up to 1 310 lags lie within 1e-3 of the peak and
neighbouring cosine tops differ by less than float32 resolution.  Batches check two pair-windows per case against the oracle,
by a seeded draw; every pair-window gets the other checks.  The measured maxima are printed per case and, at the end, per
route and bin class."""
import functools

import numpy as np
import pytest

import spectral_inputs as si

pytestmark = pytest.mark.gpu

ML = 20000
WINDOW_STEP = 7                                   # window w of a batch carries its stations' delays + 7 w
_MAXIMA = {}                                      # (plan, route, class) -> (error, input)


@functools.lru_cache(maxsize=64)
def _window(plan, idx, delay):
    P = si.PLANS[plan]
    bins = si.ten_second_comb()[1] if plan == "5x2^22" else si.inputs(P["N2"])[idx][1]
    w = si.tone_iq(bins, P["L"], P["N"], delay)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _oracle(plan, idx, da, db):
    """one float64 surface over +-(ML - 1) per (input, plan, pair of delays); shorter ranges are its middle"""
    from oracle import pyoracle
    ta, tb = pyoracle.b_preprocess(_window(plan, idx, da))[0], pyoracle.b_preprocess(_window(plan, idx, db))[0]
    if plan == "5x2^22":
        # the same definition on 2^25 points instead of the next power of two above both windows (2^26): a circular
        # correlation of length n >= L + ML holds every lag |d| < ML of the linear one
        n = 1 << 25
        r = np.fft.irfft(np.conj(np.fft.rfft(ta.astype(np.float64), n)) * np.fft.rfft(tb.astype(np.float64), n), n)
        c = r[np.arange(-(ML - 1), ML) % n] / np.sqrt(float(ta.size))
    else:
        _, _, c = pyoracle.b_xcorr_peak_fft(ta, tb, ML)
    c = np.ascontiguousarray(c)
    c.setflags(write=False)
    return c


def _want(plan, idx, da, db, ml):
    c = _oracle(plan, idx, da, db)
    return c[ML - ml:ML + ml - 1]


def _same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _record_rule(rec, s, ml, raw=None):
    """tdoa_amd.peaks.record_is_surface_max, no tolerance.  Its last line holds the lag to the first of the tied maxima T of
    the float32 surface; rounding raw x scale to float32 can merge two different raw values into such a tie (its docstring),
    and on a tone the tops differ by an ulp or not at all.  A record on a later member of T is therefore held to everything
    else of the rule by hand and, where the call returns the surface unrounded (raw: the pair call's float64), to a raw value
    strictly above the first member's -- on equal raw values the key would have taken the first"""
    from tdoa_amd.peaks import record_is_surface_max, surface_max
    s32 = np.asarray(s, dtype=np.float32)
    T, top = surface_max(s32, -(ml - 1))
    lag = int(rec["lag"])
    if not T or lag == T[0] or lag not in T:
        return record_is_surface_max(rec, s32, ml)
    at = s32[lag + ml - 1]
    corr = np.float32(rec["corr"])
    assert corr == at and np.signbit(corr) == np.signbit(at), (lag, float(corr), float(at))
    assert np.float32(rec["abs_corr"]) == np.abs(at) == np.abs(top)
    if raw is not None:
        assert abs(raw[lag + ml - 1]) > abs(raw[T[0] + ml - 1]), ("the tie went to the wrong lag", lag, T)
    return T


def _note(capsys, plan, route, idx, err_s, err_c, extra=""):
    P = si.PLANS[plan]
    name, bins = si.ten_second_comb() if plan == "5x2^22" else si.inputs(P["N2"])[idx]
    classes = ("ten-second comb",) if plan == "5x2^22" else si.classes_of(P["N2"], bins)
    for cls in set(classes):
        key = (plan, route, cls)
        if err_s >= _MAXIMA.get(key, (-1.0, ""))[0]:
            _MAXIMA[key] = (err_s, name)
    with capsys.disabled():
        print("\n  spectral bins, N = %s, %s, %s: surface %.2e, corr %.2e of the oracle's peak%s" % (plan, route, name, err_s, err_c, extra))


def _print_table(capsys):
    """what the cases run so far have noted (the file's last test calls it)"""
    with capsys.disabled():
        print("\n  spectral bins: largest |gpu - oracle| of a searched lag, relative to the oracle's peak, per route and bin class")
        for (plan, route, cls), (err, name) in sorted(_MAXIMA.items()):
            print("    N = %-6s %-34s %-13s %.2e  (%s)" % (plan, route, cls, err, name))


@pytest.fixture(autouse=True)
def _no_route_env(monkeypatch):
    for name in ("TDOA_NO_STG_MERGE", "TDOA_STG_FOLDED_ALWAYS", "TDOA_NO_STG_FOLDED", "TDOA_DEC_STAGED_CW"):
        monkeypatch.delenv(name, raising=False)


def _pair_case(capsys, plan, idx, ml, route, route_want, flags, once=None):
    import tdoa_amd
    P = si.PLANS[plan]
    da, db = si.DELAYS[0], si.DELAYS[1]
    a, b = _window(plan, idx, da), _window(plan, idx, db)
    want = _want(plan, idx, da, db, ml)
    with tdoa_amd.Context(max_lag=ml, window_len=P["L"]) as c:
        c.debug_flags(**flags)
        s = c.fm_xcorr_lags(a, b, ml)
        got = dict(c.last_route(), plan=tuple(c.plan_info()))
        assert {k: got[k] for k in route_want} == route_want, got
        assert got["plan"] == (P["N"], si.N1, P["N2"]), got["plan"]
        if once is not None:
            assert c.last_k1(0)[1] == once
        lag, corr = c.fm_xcorr(a, b, ml)
        c.poison_workspace()
        again = c.fm_xcorr_lags(a, b, ml)
        c.poison_workspace()
        lag_again, corr_again = c.fm_xcorr(a, b, ml)
    peak = np.abs(want).max()
    err_s = float(np.abs(s - want).max() / peak) if np.isfinite(s).all() else np.inf
    err_c = abs(abs(corr) - peak) / peak
    _note(capsys, plan, route, idx, err_s, err_c)
    assert np.isfinite(s).all()
    assert _same_bytes(again, s) and (lag_again, corr_again) == (lag, corr)
    assert err_s <= 1e-5, (route, idx, err_s)
    _record_rule(dict(lag=lag, corr=corr, abs_corr=abs(corr)), s, ml, raw=s)
    assert err_c <= 1e-5, (route, idx, err_c)


def _batch_case(capsys, monkeypatch, plan, idx, n_stations, route, route_want, flags, env=None):
    import tdoa_amd
    P = si.PLANS[plan]
    if env:
        monkeypatch.setenv(env, "1")
    delay = lambda s, w: si.DELAYS[s] + WINDOW_STEP * w
    with tdoa_amd.Context(max_lag=ML, window_len=P["L"]) as c:
        for s in range(n_stations):
            c.capture_upload(s, np.concatenate([_window(plan, idx, delay(s, w)) for w in range(3)]))
        c.debug_flags(**flags)
        base = c.process()
        got = dict(c.last_route(), plan=tuple(c.plan_info()))
        assert {k: got[k] for k in route_want} == route_want, got
        assert got["plan"] == (P["N"], si.N1, P["N2"]), got["plan"]
        lags = c.process_lags()
        c.poison_workspace()
        lags_again = c.process_lags()
        c.poison_workspace()
        base_again = c.process()
    pairs = [(i, j) for i in range(n_stations) for j in range(i + 1, n_stations)]
    assert base.shape == (3, len(pairs)) and lags.shape == (3, len(pairs), 2 * ML - 1)
    rng = np.random.default_rng(1000 * n_stations + idx)
    units = [(int(u) // len(pairs), int(u) % len(pairs)) for u in rng.choice(3 * len(pairs), size=2, replace=False)]
    err_s = err_c = 0.0
    for w, q in units:
        i, j = pairs[q]
        want = _want(plan, idx, delay(i, w), delay(j, w), ML)
        peak = np.abs(want).max()
        err_s = max(err_s, float(np.abs(lags[w, q] - want).max() / peak) if np.isfinite(lags[w, q]).all() else np.inf)
        err_c = max(err_c, abs(abs(float(base[w, q]["corr"])) - peak) / peak)
    _note(capsys, plan, route, idx, err_s, err_c, "; pair-windows %s" % (units,))
    assert np.isfinite(lags).all()
    assert _same_bytes(lags_again, lags) and _same_bytes(base_again, base)
    assert err_s <= 1e-5, (route, idx, err_s)
    for w in range(3):
        for q in range(len(pairs)):
            _record_rule(base[w, q], lags[w, q], ML)
    assert err_c <= 1e-5, (route, idx, err_c)


def _cases(plan, routes):
    """(input, route) with the input outermost: its windows and oracle surfaces are made once and shared by the routes"""
    table = si.inputs(si.PLANS[plan]["N2"])
    return [pytest.param(idx, r, id="%s-%s" % (table[idx][0], r)) for idx in range(len(table)) for r in routes]


DEC = {"inverse": "decimated"}
PAIR_ROUTES = {
    "default": (dict(DEC, pair_step="tiles", once=True), {}, True),
    "no_k1_once": (dict(DEC, pair_step="tiles", once=False), {"no_k1_once": True}, False),
    "no_decimate": ({"inverse": "full", "pruned": True}, {"no_decimate": True}, None),
    "per_pair_walk": (dict(DEC, pair_step="columns"), {"dec_cols_always": True, "no_dec_staged": True}, None),
    "force_generic": ({"inverse": "full", "pruned": False, "col_pass": "generic"}, {"generic": True}, None),
}
STAGED = dict(DEC, pair_step="staged", stg_folded=False)
BATCH_ROUTES = {
    "3_stations_merged_fused": (3, dict(STAGED, stg_merged=True, small_fused=True), {"small_fused_always": True}, None),
    "3_stations_no_small_fused": (3, dict(STAGED, stg_merged=True, small_fused=False), {"no_small_fused": True}, None),
    "3_stations_no_stg_merge": (3, dict(STAGED, stg_merged=False), {}, "TDOA_NO_STG_MERGE"),
    "4_stations": (4, dict(STAGED, stg_merged=False), {}, None),
}
SHORT_ROUTES = {                                  # N = 2^17: (max_lag, route, flags)
    "default": (ML, {"inverse": "full"}, {}),
    "force_generic": (ML, {"inverse": "full", "pruned": False, "col_pass": "generic"}, {"generic": True}),
    "segments_300": (300, {"inverse": "segments"}, {}),
    "short_lag_300": (300, {"inverse": "short_lag"}, {"no_segment_form": True}),
    "full_300": (300, {"inverse": "full"}, {"no_segment_form": True, "no_short_lag": True}),
}


@pytest.mark.parametrize("idx,route", _cases("2^21", PAIR_ROUTES))
def test_pair_on_4096x256(oracle, capsys, idx, route):
    want, flags, once = PAIR_ROUTES[route]
    _pair_case(capsys, "2^21", idx, ML, route, want, flags, once)


@pytest.mark.parametrize("idx,route", _cases("2^21", BATCH_ROUTES))
def test_batch_on_4096x256(oracle, capsys, monkeypatch, idx, route):
    n, want, flags, env = BATCH_ROUTES[route]
    _batch_case(capsys, monkeypatch, "2^21", idx, n, route, want, flags, env)


@pytest.mark.parametrize("idx,route", _cases("2^22", ["default", "4_stations"]))
def test_on_4096x512(oracle, capsys, monkeypatch, idx, route):
    if route == "default":
        want, flags, once = PAIR_ROUTES[route]
        _pair_case(capsys, "2^22", idx, ML, route, want, flags, once)
    else:
        n, want, flags, env = BATCH_ROUTES[route]
        _batch_case(capsys, monkeypatch, "2^22", idx, n, route, dict(DEC, pair_step="staged"), flags, env)


@pytest.mark.parametrize("idx,route", _cases("2^17", SHORT_ROUTES))
def test_pair_on_4096x16(oracle, capsys, idx, route):
    """the short column kernels and the any-size kernels; the bin classes that exist with N2 = 16"""
    ml, want, flags = SHORT_ROUTES[route]
    _pair_case(capsys, "2^17", idx, ml, route, want, flags)


def test_pair_on_4096x2560(oracle, capsys):
    """twiddles with a denominator 5 x 2^k (unit_root_any), the column walk down 2560 rows: a comb of k = 1, a row-0 bin, a
    row-N2/2 bin and Nc - 1 on twenty million samples.  The one case here above a few seconds: its float64 reference is a
    correlation on 2^25 points.  The file's last test: it ends with the table of the maxima noted by all of them"""
    try:
        _pair_case(capsys, "5x2^22", 0, ML, "default", dict(DEC, pair_step="columns"), {})
    finally:
        _print_table(capsys)
