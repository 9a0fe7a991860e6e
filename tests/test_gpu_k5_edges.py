"""GPU: K5 (csrc/peak_key.hpp: lag filter, NaN rule, key maximum, surface dump, one atomicMax per workgroup) on every route of
tdoa_process, with the winners of one batch swept across the search range instead of sitting next to lag 0.

One capture set per search range, shared by the routes.  Every window carries its own station delays (0, x, y) on a common
base offset, so its pair lags are x, y, y - x for the pairs (0,1), (0,2), (1,2) -- known by construction, asserted for every
pair-window of every route.  Over the batch they contain, for a range of +-(ml - 1):
  0, +1, -1, +(ml - 1), -(ml - 1), and b - 1 and b with both signs for every boundary b inside the range at which a K5
  kernel hands its lags from one output, column, wave or workgroup to the next:
  - k_segments_reduce: lag index d + P, 256 per workgroup, 64 per wave -- b = 64, 128, 256 (ml = 300: P = 512);
  - k_fused_reduce<FK>: lags 2 m + q, m = 256 k + j: 512 per FK block, 128 per wave, the two sides meet at 0 / -1;
  - pruned_outputs / pruned_col_finish (k_inv_col_pruned, k_inv_col_pruned_any): output n2 holds the lags
    [2 N1 n2, 2 N1 (n2 + 1)) -- multiples of 8192 on the 4096-column plans, np outputs from 0 up and nn from -1 down --, a
    workgroup 256 of them, a thread four;
  - small_offer's d (k_small_col_peak, k_small_rows_col_peak): d = 2 (n2 4096 + n1), d and d + 1 offered together:
    outputs change at the multiples of 8192, k_small_col_peak's workgroups at those of 512, its waves at those of 128;
    k_small_rows_col_peak's thread t holds n1 = t + 512 k: wave (n1 mod 512) / 64, so waves 4 .. 7 hold the lags with
    d mod 1024 >= 512 (4095, 8191, 12 287, 16 383 and 19 999 are theirs; 127, 511 and 4096 are not);
  - k_inv_col_peak (generic kernels): tiles of C columns, 2 C lags, C a power of two <= 64;
  ml = 300: b = 64, 128, 192, 256 -- every wave and workgroup boundary of k_segments_reduce; ml = 20 000: every multiple
  of 4096 (so every output boundary), and of the 156 wave and 39 workgroup boundaries of k_small_col_peak the first of each
  (128, 512) as a sample: the others differ from them by the workgroup number alone.
Two windows have the true delay of pair (0,1) one lag OUTSIDE the range (+ml, -ml): the record must be the oracle's in-range
maximum, and a filter that let lag +-ml in would return a record larger than every element of the surface.  One window has
I and Q of station 1 swapped (negative correlation on its pairs), one has station 1 constant (bytes 128: zero records, count
0, a finite all-zero surface on its pairs; pair (0,2) untouched) -- with the single-look K1 on and off.

Every case starts on a fresh context, asserts the route it is named for, then holds for EVERY pair-window: the designed
lag; the record of tdoa_process and peak 1 of tdoa_process_peaks(8, 8) to the maximum of the tdoa_process_lags surface with
no tolerance (tdoa_amd.peaks.record_is_surface_max), that maximum unique; the same bytes on poisoned workspace from the
replayed graph; finite surfaces.  The pair-windows at +-(ml - 1), the outside-range, the negative and the constant windows
also go to the float64 oracle: surface within 2e-6 and corr within 1e-5 of the peak (for the outside-range windows the peak
over a range widened to hold the true delay: the kernel's rounding error follows the signal's energy, not the sidelobe).

All routes are reached with three stations except the tile pair step, which the library takes for a single pair: two
stations, once each pair of stations of the same captures, so that the three runs together hold every target.

TDOA_LAGS_GO has no surfaces and searches lag 0 alone on equal windows, so it gets a case of its own at the end: K1's
statistics run over the whole window there and the transforms over a shorter one."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, SEP = 8, 8
WL = {300: 70_000, 20000: 1_100_000}
BOUNDARIES = {300: (64, 128, 192, 256), 20000: (128, 512, 4096, 8192, 12288, 16384)}
PAIRS3 = [(0, 1), (0, 2), (1, 2)]


@functools.lru_cache(maxsize=None)
def _design(ml):
    """per window: (x, y, kind); kind: None, "out" (pair (0,1) one lag outside), "neg", "const" (both station 1)"""
    wins = []
    for b in BOUNDARIES[ml]:
        wins.append((-1, b - 1, None))                    # lags -1, b - 1, b
        wins.append((1, -(b - 1), None))                  # lags +1, -(b - 1), -b
    wins += [(0, ml - 1, "edge"), (0, -(ml - 1), "edge"), (ml, 5, "out"), (-ml, -5, "out"), (9, -7, "neg"), (3, 11, "const")]
    while len(wins) % 3:                                  # tdoa_process takes its windows from the thirds of a capture
        wins.append((2, -2, None))                        # lags +2, -2, -4
    return tuple(wins)


@functools.lru_cache(maxsize=None)
def _captures(ml):
    from oracle import pyoracle
    wl, caps = WL[ml], [[], [], []]
    for wid, (x, y, kind) in enumerate(_design(ml)):
        for s, d in enumerate((0, x, y)):
            w = pyoracle.simulate_delayed_fm(wl, ml + d, 3100 + wid, 100 * (s + 1) + wid)
            if s == 1 and kind == "neg":
                sw = w.copy()
                sw[0::2], sw[1::2] = w[1::2], w[0::2]
                w = sw
            if s == 1 and kind == "const":
                w = np.full(2 * wl, 128, dtype=np.uint8)
            caps[s].append(w)
    caps = tuple(np.concatenate(c) for c in caps)
    for c in caps:
        c.setflags(write=False)
    return caps


def _window(ml, s, wid):
    wl = WL[ml]
    return _captures(ml)[s][2 * wid * wl:2 * (wid + 1) * wl]


@functools.lru_cache(maxsize=None)
def _pre(ml, s, wid):
    from oracle import pyoracle
    return pyoracle.b_preprocess(_window(ml, s, wid))[0]


@functools.lru_cache(maxsize=None)
def _oracle(ml, wid, i, j):
    """(lag, corr, surface over +-(ml - 1), peak over +-(ml + 1)) of one pair-window in float64"""
    from oracle import pyoracle
    _, _, wide = pyoracle.b_xcorr_peak_fft(_pre(ml, i, wid), _pre(ml, j, wid), ml + 2)
    c = np.ascontiguousarray(wide[2:-2])
    lag, corr = pyoracle.b_pick_peak(c, ml)
    c.setflags(write=False)
    return lag, corr, c, float(np.abs(wide).max())


def _same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _case(capsys, ml, tag, route_want, stations=(0, 1, 2), record=(), **flags):
    import tdoa_amd
    from tdoa_amd.peaks import record_is_surface_max
    design, caps = _design(ml), _captures(ml)
    pairs = [(stations[a], stations[b]) for a in range(len(stations)) for b in range(a + 1, len(stations))]
    with tdoa_amd.Context(max_lag=ml, window_len=WL[ml]) as c:
        for k, s in enumerate(stations):
            c.capture_upload(k, caps[s])
        c.debug_flags(**flags)
        base = c.process()
        route = dict(c.last_route(), plan=tuple(c.plan_info()))
        assert {k: route[k] for k in route_want} == route_want, route
        assert base.shape == (len(design), len(pairs))
        lags = c.process_lags()
        pk, cnt = c.process_peaks(K, SEP)
        assert dict(c.last_route(), plan=tuple(c.plan_info())) == route
        c.poison_workspace()
        assert _same_bytes(c.process(), base)                                 # replayed, on poisoned workspace
        c.poison_workspace()
        assert _same_bytes(c.process_lags(), lags)
        c.poison_workspace()
        pk_p, cnt_p = c.process_peaks(K, SEP)
        assert _same_bytes(pk_p, pk) and np.array_equal(cnt_p, cnt)
    assert np.isfinite(lags).all()
    assert _same_bytes(np.ascontiguousarray(pk[..., 0]), base)
    worst_s = worst_c = 0.0
    for wid, (x, y, kind) in enumerate(design):
        delay = (0, x, y)
        for q, (i, j) in enumerate(pairs):
            rec, s = base[wid, q], lags[wid, q]
            where = (tag, wid, (i, j))
            dead = kind == "const" and 1 in (i, j)
            outside = kind == "out" and (i, j) == (0, 1)
            T = record_is_surface_max(rec, s, ml)
            record_is_surface_max(pk[wid, q, 0], s, ml)
            if dead:
                assert not s.any() and int(cnt[wid, q]) == 0 and not pk[wid, q]["lag"].any() and not pk[wid, q]["corr"].any(), where
                assert (int(rec["lag"]), float(rec["corr"]), float(rec["abs_corr"])) == (0, 0.0, 0.0), where
            else:
                assert len(T) == 1 and int(cnt[wid, q]) >= 1, where + (T,)
                if not outside:
                    assert int(rec["lag"]) == delay[j] - delay[i], where + (int(rec["lag"]),)
                    assert (float(rec["corr"]) < 0) == (kind == "neg" and 1 in (i, j)), where
            if kind is None:
                continue
            olag, ocorr, want, peak = _oracle(ml, wid, i, j)
            assert int(rec["lag"]) == olag, where + (int(rec["lag"]), olag)
            if outside:
                assert abs(ocorr) < 0.5 * peak                                  # (the design: a sidelobe, the peak is outside)
            err_s, err_c = float(np.abs(s - want).max()), abs(float(rec["corr"]) - ocorr)
            if peak > 0:
                worst_s, worst_c = max(worst_s, err_s / peak), max(worst_c, err_c / peak)
            assert err_s <= 2e-6 * peak, where + (err_s, peak)
            assert err_c <= 1e-5 * peak, where + (err_c, peak)
    with capsys.disabled():
        print("\n  k5 edges, %s: %d pair-windows exact; vs f64 oracle worst surface %.2e, corr %.2e of the peak%s"
              % (tag, base.size, worst_s, worst_c, "".join("; %s %s" % (k, route[k]) for k in record)))
    return route


@pytest.fixture(autouse=True)
def _no_route_env(monkeypatch):
    for name in ("TDOA_NO_STG_MERGE", "TDOA_STG_FOLDED_ALWAYS", "TDOA_NO_STG_FOLDED", "TDOA_DEC_STAGED_CW"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("quads", [True, False])
def test_segments(oracle, capsys, quads):
    """both segment kernels transform the constant station-window next to a live one in one complex frame: its zero has
    to come from k_segments_reduce (fm_stats_flat), not from the transform, which leaves 1e-7 of the neighbour's peak"""
    _case(capsys, 300, "segments, quads %s" % quads, {"inverse": "segments", "seg_quads": quads}, no_segment_quads=not quads)


def test_short_lag(oracle, capsys):
    _case(capsys, 300, "short_lag (k_fused_reduce)", {"inverse": "short_lag"}, no_segment_form=True)


def test_full_300(oracle, capsys):
    _case(capsys, 300, "full at 300 lags (pruned columns)", {"inverse": "full", "pruned": True}, no_segment_form=True,
          no_short_lag=True)


def test_generic_kernels(oracle, capsys):
    _case(capsys, 300, "generic kernels (k_inv_col_peak)", {"inverse": "full", "pruned": False, "col_pass": "generic"},
          generic=True)


@pytest.mark.parametrize("once", [True, False])
@pytest.mark.parametrize("stations", [(0, 1), (0, 2), (1, 2)])
def test_decimated_tiles(oracle, capsys, stations, once):
    """two stations: (0,1) has the lags -1, +1, 0 and the outside-range windows, (0,2) has +-(b - 1), +-(ml - 1) and
    +-5, (1,2) has +-b and +-(ml - 1) again; (0,1) and (1,2) have the negative and the constant window"""
    _case(capsys, 20000, "decimated tiles, stations %s, single-look %s" % (stations, once),
          {"inverse": "decimated", "pair_step": "tiles", "once": once}, stations=stations, no_k1_once=not once)


def test_decimated_columns(oracle, capsys):
    _case(capsys, 20000, "decimated columns", {"inverse": "decimated", "pair_step": "columns"}, dec_cols_always=True,
          no_dec_staged=True)


@pytest.mark.parametrize("once", [True, False])
def test_staged_walk_as_chosen(oracle, capsys, once):
    _case(capsys, 20000, "staged walk, single-look %s" % once,
          {"inverse": "decimated", "pair_step": "staged", "stg_folded": False, "once": once}, record=("stg_merged", "small_fused"),
          no_k1_once=not once)


def test_staged_walk_unmerged(oracle, capsys, monkeypatch):
    monkeypatch.setenv("TDOA_NO_STG_MERGE", "1")
    _case(capsys, 20000, "staged walk, TDOA_NO_STG_MERGE", {"inverse": "decimated", "pair_step": "staged", "stg_merged": False})


def test_staged_walk_folded(oracle, capsys, monkeypatch):
    monkeypatch.setenv("TDOA_STG_FOLDED_ALWAYS", "1")
    _case(capsys, 20000, "staged walk, folded", {"inverse": "decimated", "pair_step": "staged", "stg_folded": True},
          record=("stg_merged",))


@pytest.mark.parametrize("fused", [True, False])
def test_small_plan(oracle, capsys, fused):
    """k_small_rows_col_peak (eight waves) / k_inv_rows_plain_r8 + k_small_col_peak"""
    _case(capsys, 20000, "small plan %s" % ("fused" if fused else "as two kernels"), {"inverse": "decimated", "small_fused": fused},
          record=("pair_step",), small_fused_always=fused, no_small_fused=not fused)


@pytest.mark.parametrize("pow2", [False, True])
def test_full_inverse_20000(oracle, capsys, pow2):
    """pow2_only chooses between 2^25 and 5 x 2^22 points for ten-second windows and nothing else (choose_fft_size): at
    this size both cases take the 4096 x 256 plan, asserted, and differ in the switch alone -- the second one holds only
    that the switch changes nothing here.  The 5 x 2^22 plan's full inverse is tests/test_gpu_ten_second_plan.py's."""
    route = _case(capsys, 20000, "full inverse at 20 000 lags, pow2_only %s" % pow2, {"inverse": "full", "pruned": True},
                  record=("plan",), no_decimate=True, pow2_only=pow2)
    assert route["plan"] == (1 << 21, 4096, 256), route["plan"]


def _offset_fm(n, step, seed, noise_seed):
    """IQ bytes of a carrier `step` radians per sample off centre with a slow phase modulation of 2 rad (content `seed`) and
    a little noise: the discriminator output is step +- a few hundredths, its mean tens of its sigmas"""
    rng, nrng = np.random.default_rng(seed), np.random.default_rng(noise_seed)
    t = np.arange(n)
    ph = step * t + 2.0 * np.sin(2 * np.pi * np.cumsum(rng.uniform(0.001, 0.01, n)))
    iq = np.empty(2 * n)
    iq[0::2] = 127.5 + 100.0 * np.cos(ph) + nrng.normal(0.0, 0.5, n)
    iq[1::2] = 127.5 + 100.0 * np.sin(ph) + nrng.normal(0.0, 0.5, n)
    return np.clip(np.rint(iq), 0, 255).astype(np.uint8)


def test_go_mode_carrier_offset_and_constant_station(oracle, capsys):
    """TDOA_LAGS_GO, tdoa_process (the segment form): K1 and its statistics run over the whole 70 000-sample window, the
    transforms over its first 69 blocks of 1000.  Windows 0 and 2: every station on a carrier +-1.2 rad per sample off
    centre, the codes' mean more than 8.3 sigma from 0 -- where sums over 70 000 samples read against a length of 69 000
    look like no variance at all; the record must be timeDomainCorrelation's at lag 0, a large value (the stations share
    the modulation).  Window 1: station 1 constant, its pairs (0, 0.0), pair (0,2) live.  Tolerances as
    test_gpu_anchors.test_k5_go_lag_set_edge_cases: 1e-5 of the value plus 1e-6 of full scale sqrt(69 000)."""
    import tdoa_amd
    from oracle import pyoracle
    wl, ml = 70_000, 20000
    steps = (1.2, 1.2, -1.2)
    caps = []
    for s in range(3):
        w = [_offset_fm(wl, steps[wid], 50 + wid, 10 * s + wid) for wid in range(3)]
        if s == 1:
            w[1] = np.full(2 * wl, 128, dtype=np.uint8)
        caps.append(np.concatenate(w))
    for s in range(3):
        for wid in (0, 2):
            st = pyoracle.b_preprocess(caps[s][2 * wid * wl:2 * (wid + 1) * wl])[1]
            assert ((st.s2_hi << 64) | st.s2_lo) * 69_000 <= st.s1 * st.s1 and st.var > 0     # (the design)
    with tdoa_amd.Context(max_lag=ml, window_len=wl, lag_mode=tdoa_amd.capi.LAGS_GO) as c:
        for s in range(3):
            c.capture_upload(s, caps[s])
        peaks = c.process()
        assert c.last_route()["inverse"] == "segments", c.last_route()
        c.poison_workspace()
        assert _same_bytes(c.process(), peaks)
    assert peaks.shape == (3, 3) and not peaks["lag"].any()
    worst = 0.0
    for wid in range(3):
        pre = [pyoracle.b_preprocess(cp[2 * wid * wl:2 * (wid + 1) * wl])[0].astype(np.complex64) for cp in caps]
        for q, (i, j) in enumerate(PAIRS3):
            rec = peaks[wid, q]
            if wid == 1 and 1 in (i, j):
                assert (int(rec["lag"]), float(rec["corr"]), float(rec["abs_corr"])) == (0, 0.0, 0.0), (wid, (i, j), rec)
                continue
            gd, gc = pyoracle.time_domain_correlation(pre[i], pre[j], ml)
            assert gd == 0 and abs(gc) > 0.5 * np.sqrt(69000.0), (wid, (i, j), gc)      # (the design: a strong peak at lag 0)
            err = abs(float(rec["corr"]) - gc)
            worst = max(worst, err / abs(gc))
            assert err <= 1e-5 * abs(gc) + 1e-6 * np.sqrt(69000.0), (wid, (i, j), rec, gc)
    with capsys.disabled():
        print("\n  k5 edges, TDOA_LAGS_GO on an offset carrier: 6 live pair-windows at lag 0, worst corr error %.2e of the value" % worst)
