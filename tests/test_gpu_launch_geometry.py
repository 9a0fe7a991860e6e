"""GPU: how a batch is DEALT TO WORKGROUPS -- the choices plan_fm_batch (csrc/fm_route.inc) makes out of the card's CU count,
the station count and the batch size, which a test otherwise only ever meets as the card gives them:

  1. k_inv_row_pair4096 on the XCD-grouped 1-D grid (padded to rounds of 8 groups) against the plain 2-D grid, the full inverse
     and every short-lag instance (FK = 1, 2, 4, 8);
  2. k_pair_decimate16 on its XCD-grouped grid (route flag dec_gp, TDOA_XCD_PAIR_MB=0) against the plain one;
  3. the segment form at forced chunk counts (TDOA_SEG_CHUNKS), quads and one pair-window at a time;
  4. the staged walk's ring: rows per phase, ring depth, loader waves (TDOA_DEC_STAGED_ROWS / _BUFS / _LOADERS);
  5. the padding of a two-sweep plan's TZ rows (TDOA_ZPAD).

None of these choices is meant to change a result: a geometry that only moves work returns THE SAME BYTES as the geometry it
is compared with (a wrong remap drops or doubles a row of one pair-window: a wrong byte, or poison that survives), and the
geometry under test is held against the f64 oracle (oracle.b_xcorr_peak_fft: lag identical, corr within north_star's 1e-5).
The one exception is 3.: another chunk count adds a pair-window's frames in another order -- there the oracle comparison holds
for every count and the lags are the same.

Environment knobs are read once, when a context is made: every variant is a fresh context, made after monkeypatch.setenv and
closed before the next.  Every run asserts the route it means to take (last_route).  Signals: oracle.simulate_delayed_fm with
planted delays; that the ORACLE's peak is the planted lag is asserted on the CPU, when the oracle's table is made, before a GPU
run is compared with it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5      # north_star: correlation magnitudes within 1e-5 relative (tests/test_gpu_fm.py)
ML_DEC = 20000      # the reference's lag range: the decimated inverse
GEOMETRY_ENV = ("TDOA_XCD_PAIR_MB", "TDOA_SEG_CHUNKS", "TDOA_DEC_STAGED_ROWS", "TDOA_DEC_STAGED_BUFS", "TDOA_DEC_STAGED_LOADERS",
                "TDOA_ZPAD", "TDOA_NO_XCD_ROWS")


def _pairs(n_st):
    return [(i, j) for i in range(n_st) for j in range(i + 1, n_st)]


def _planted(delays):
    return np.array([delays[j] - delays[i] for i, j in _pairs(len(delays))])


def _same_bytes(a, b):
    """the records byte for byte (a NaN that both hold compares equal here and is caught by the oracle comparison)"""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                                        np.ascontiguousarray(b).view(np.uint8))


def _assert_lags_close(got, want, tol=REL_TOL):
    """(tests/test_gpu_fm.py's rule: the largest error of a lag, relative to the peak)"""
    peak = np.abs(want).max()
    assert peak > 0
    err = np.abs(got - want).max() / peak
    assert err < tol, "max lag error %.3g of peak" % err


def _no_geometry_env():
    return not any(v in os.environ for v in GEOMETRY_ENV)


class Shape:
    """a tdoa_process batch: three blocks of `blk` samples per station, windows of `wl`, station s delayed by delays[s]; and
    the oracle's table of it, filled window by window as the tests ask (CPU only)"""

    def __init__(self, oracle, delays, wl, blk, base, content):
        self.o, self.delays, self.wl, self.blk, self.n_st = oracle, list(delays), wl, blk, len(delays)
        self.pairs = _pairs(self.n_st)
        self.caps = [np.concatenate([oracle.simulate_delayed_fm(blk, base + d, content + k, 100 * (s + 1) + k) for k in range(3)])
                     for s, d in enumerate(self.delays)]
        self.wpb = blk // wl
        self.n_windows = 3 * self.wpb
        self._pre, self._peak, self._fine = {}, {}, {}

    def first(self, wid):
        return (wid // self.wpb) * self.blk + (wid % self.wpb) * self.wl

    def window_bytes(self, s, wid):
        return self.caps[s][2 * self.first(wid):2 * (self.first(wid) + self.wl)]

    def pre(self, wid):
        if wid not in self._pre:
            self._pre[wid] = [self.o.b_preprocess(self.window_bytes(s, wid))[0] for s in range(self.n_st)]
        return self._pre[wid]

    def peaks(self, wid, ml):
        """[(lag, corr)] of window wid's pairs from oracle.b_xcorr_peak_fft; the oracle's peak IS the planted lag (asserted here,
        for the reference alone, before any GPU result is compared)"""
        if (wid, ml) not in self._peak:
            pre, out = self.pre(wid), []
            for i, j in self.pairs:
                olag, ocorr, _ = self.o.b_xcorr_peak_fft(pre[i], pre[j], ml)
                assert olag == self.delays[j] - self.delays[i], ("oracle", wid, (i, j), olag)
                out.append((olag, ocorr))
            self._peak[(wid, ml)] = out
        return self._peak[(wid, ml)]

    def fracs(self, wid, ml, gate):
        if (wid, ml, gate) not in self._fine:
            pre = self.pre(wid)
            self._fine[(wid, ml, gate)] = [self.o.b_refine_peak(pre[i], pre[j], olag, gate)["frac"]
                                           for (i, j), (olag, _) in zip(self.pairs, self.peaks(wid, ml))]
        return self._fine[(wid, ml, gate)]

    def upload(self, c):
        for s, cap in enumerate(self.caps):
            c.capture_upload(s, cap)
        assert c.num_windows() == (self.wpb, self.n_windows) and c.num_pairs() == len(self.pairs)

    def check(self, c, peaks, wids, ml, tag):
        """windows `wids` of `peaks` against the oracle ON THE BYTES THE DEVICE HOLDS (capture_download: asserted to be the
        bytes the table was made from): lag identical, corr within REL_TOL; returns the worst relative deviation"""
        assert peaks.shape == (self.n_windows, len(self.pairs))
        worst = 0.0
        for wid in wids:
            for s in range(self.n_st):
                assert np.array_equal(c.capture_download(s, self.first(wid), self.wl), self.window_bytes(s, wid)), (tag, wid, s)
            for p, (olag, ocorr) in enumerate(self.peaks(wid, ml)):
                g = peaks[wid, p]
                assert int(g["lag"]) == olag, (tag, wid, self.pairs[p], int(g["lag"]), olag)
                dev = abs(float(g["corr"]) - ocorr) / abs(ocorr)
                assert dev < REL_TOL, (tag, wid, self.pairs[p], dev)
                worst = max(worst, dev)
        return worst


# ---- the captures: made once per module, never changed ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def shape_a(oracle):
    """4 stations (6 pairs: the fewest with more pairs than stations), window_len = 66 000 -> N = 2^17, the 4096 x 16 plan -- the
    smallest with 4096-point rows: make_plan gives rows of Nc / 16 points below Nc = 65 536, so there is no 4096 x 8 plan and a
    window of 40 000 samples (N = 2^16) runs the any-size kernels on 2048 x 16 --: RP = N2 / 2 - 1 = 7 row pairs; one window per
    block: 3 windows, 21 (window, row pair) groups in 24 slots"""
    return Shape(oracle, [0, 41, -17, 203], 66_000, 66_000, 100, 910)


@pytest.fixture(scope="module")
def shape_b(oracle):
    """5 stations (10 pairs), window_len = 70 000 -> N = 2^17, the 4096 x 16 plan: RP = 7; two windows per block: 6 windows,
    42 groups in 48 slots (launch groups of four windows: 28 in 32 and 14 in 16).  Every lag difference is below 299: inside
    the 300-lag range with its refinement neighbours"""
    return Shape(oracle, [0, 41, -17, 203, -90], 70_000, 140_000, 100, 640)


@pytest.fixture(scope="module")
def caps_256(oracle):
    """eight stations x three windows of 1 100 000 samples (4096 x 256 plan at 20 000 lags); the tests take the first 3, 5 or 8"""
    return Shape(oracle, [0, 41, -17, 203, -350, 19, 77, -5], 1_100_000, 1_100_000, 400, 900)


@pytest.fixture(scope="module")
def caps_512(oracle):
    """four stations x three windows of 2 200 001 samples (odd: the last element of a window holds one sample): 4096 x 512 plan"""
    return Shape(oracle, [0, -123, 64, 1999], 2_200_001, 2_200_001, 2100, 1900)


def _first_stations(shape, n_st):
    """the batch of the first n_st stations of `shape` (the same capture bytes, no new signal)"""
    if n_st == shape.n_st:
        return shape
    sub = Shape.__new__(Shape)
    sub.__dict__.update(shape.__dict__)
    sub.delays, sub.n_st, sub.pairs, sub.caps = shape.delays[:n_st], n_st, _pairs(n_st), shape.caps[:n_st]
    sub._pre, sub._peak, sub._fine = {}, {}, {}
    return sub


# ---- 1. k_inv_row_pair4096 on the XCD grid ------------------------------------------------------------------------------------

# (max_lag, no_short_lag) -> the route it must take: FK = 1, 2, 4, 8 and the full inverse (FK = 0)
ROW_PAIR_INSTANCES = [(300, False, ("short_lag", 1)), (1000, False, ("short_lag", 2)), (2000, False, ("short_lag", 4)),
                      (4000, False, ("short_lag", 8)), (300, True, ("full", 0))]
ROW_PAIR_SHAPES = [("a", 0, (4096, 16)), ("b", 0, (4096, 16)), ("b", 4, (4096, 16))]


def _row_pair_route(c, want, xcd):
    r = c.last_route()
    assert (r["inverse"], r["fk"]) == want and r["xcd_pairs"] == xcd, r


@pytest.mark.parametrize("ml,no_short_lag,want", ROW_PAIR_INSTANCES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("name,per_batch,plan", ROW_PAIR_SHAPES, ids=["A", "B", "B-groups-of-4"])
def test_row_pair_kernel_on_the_xcd_grid(shape_a, shape_b, name, per_batch, plan, ml, no_short_lag, want, capsys):
    """every instance of k_inv_row_pair4096<false, FK> on the 1-D grid that puts the pair-windows of one (window, row pair) group
    on one XCD -- the library's choice from four stations on -- with a last round of 8 groups that is padded (shape A: 21 groups
    in 24 slots, the workgroups of the last 3 return early; shape B: 42 in 48; in launch groups of four windows 28 in 32 and 14 in 16): the same bytes
    as the plain (N2 / 2 - 1, n_pw) grid (the per-row arithmetic is the same), on poisoned workspace, and the first and the last
    window against the oracle"""
    import tdoa_amd
    shape = shape_a if name == "a" else shape_b
    wids = (0, shape.n_windows - 1)
    for wid in wids:
        shape.peaks(wid, ml)                                          # the oracle alone: its peaks are the planted lags (CPU)
    assert _no_geometry_env()
    with tdoa_amd.Context(max_lag=ml, window_len=shape.wl, windows_per_batch=per_batch) as c:
        shape.upload(c)
        c.debug_flags(no_segment_form=True, no_short_lag=no_short_lag)
        warm = c.process()
        assert tuple(c.plan_info())[1:] == plan
        _row_pair_route(c, want, True)
        c.debug_flags(no_segment_form=True, no_short_lag=no_short_lag, no_xcd_rows=True)
        c.poison_workspace()
        plain = c.process()
        _row_pair_route(c, want, False)
        c.debug_flags(no_segment_form=True, no_short_lag=no_short_lag)
        c.poison_workspace()
        xcd = c.process()
        _row_pair_route(c, want, True)
        worst = shape.check(c, xcd, wids, ml, "xcd grid")
    assert _same_bytes(xcd, plain) and _same_bytes(warm, xcd)
    assert (xcd["lag"] == _planted(shape.delays)[None, :]).all()
    with capsys.disabled():
        print("\n  k_inv_row_pair4096<false, %d>, shape %s: %d pair-windows, XCD grid = plain grid byte for byte; windows %r vs ob_*: "
              "worst |dcorr|/|corr| %.2e" % (want[1], name.upper(), xcd.size, wids, worst))


@pytest.mark.parametrize("name", ["a", "b"])
def test_refinement_behind_the_xcd_grid(shape_a, shape_b, name):
    """tdoa_process_fine reads the peak's neighbours out of what the row kernel left (V, or the short-lag shares): the fine
    records on the XCD grid are the bytes of the plain grid's, behind the full inverse and behind the FK = 1 short-lag form"""
    import tdoa_amd
    shape = shape_a if name == "a" else shape_b
    assert _no_geometry_env()
    with tdoa_amd.Context(max_lag=300, window_len=shape.wl) as c:
        shape.upload(c)
        for no_short_lag, want in ((True, ("full", 0)), (False, ("short_lag", 1))):
            c.debug_flags(no_segment_form=True, no_short_lag=no_short_lag)
            c.poison_workspace()
            peaks_x, fine_x = c.process_fine(120.0)
            _row_pair_route(c, want, True)
            c.debug_flags(no_segment_form=True, no_short_lag=no_short_lag, no_xcd_rows=True)
            c.poison_workspace()
            peaks_p, fine_p = c.process_fine(120.0)
            _row_pair_route(c, want, False)
            assert _same_bytes(peaks_x, peaks_p) and _same_bytes(fine_x, fine_p), want
            assert (peaks_x["lag"] == _planted(shape.delays)[None, :]).all()
            assert np.isfinite(fine_x["frac"]).all() and np.isfinite(fine_x["y"]).all()      # (no poison in what both grids agree on)


# ---- 2. k_pair_decimate16 on the XCD grid -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_st,name,plan,oracle_window", [(3, "256", (4096, 256), 1), (4, "512", (4096, 512), None)],
                         ids=["3st-4096x256", "4st-4096x512"])
def test_decimation_tiles_on_the_xcd_grid(caps_256, caps_512, monkeypatch, n_st, name, plan, oracle_window, capsys):
    """the tile form of the decimated pair step with a window's pair-windows on one XCD (group_pairs > 0: by default only from
    48 MB of spectra per window on, which no test reaches; TDOA_XCD_PAIR_MB=0 asks for it at any size) against its plain
    (N2 / 2, n_pw) grid: the same bytes.  3 stations on the 4096 x 256 plan (k_pair_decimate16<8>: 3 windows x 128 tile pairs =
    384 groups of 3), every pair of one window against the oracle; 4 stations on the 4096 x 512 plan (<9>, odd window length:
    768 groups of 6): bytes and the planted lags"""
    import tdoa_amd
    shape = _first_stations(caps_256 if name == "256" else caps_512, n_st)
    if oracle_window is not None:
        shape.peaks(oracle_window, ML_DEC)
    assert _no_geometry_env()
    monkeypatch.setenv("TDOA_XCD_PAIR_MB", "0")
    with tdoa_amd.Context(max_lag=ML_DEC, window_len=shape.wl) as c:
        shape.upload(c)
        c.debug_flags(no_dec_cols=True)
        warm = c.process()
        assert tuple(c.plan_info())[1:] == plan

        def route(dec_gp):
            r = c.last_route()
            assert (r["inverse"], r["pair_step"]) == ("decimated", "tiles") and r["dec_gp"] == dec_gp, r
        route(True)
        c.debug_flags(no_dec_cols=True, no_xcd_rows=True)
        c.poison_workspace()
        plain = c.process()
        route(False)
        c.debug_flags(no_dec_cols=True)
        c.poison_workspace()
        xcd = c.process()
        route(True)
        worst = shape.check(c, xcd, () if oracle_window is None else (oracle_window,), ML_DEC, "tiles, xcd grid")
    assert _same_bytes(xcd, plain) and _same_bytes(warm, xcd)
    assert (xcd["lag"] == _planted(shape.delays)[None, :]).all() and (xcd["abs_corr"] > 100.0).all()
    with capsys.disabled():
        print("\n  k_pair_decimate16 on the %d x %d plan, %d stations: XCD grid = plain grid byte for byte; vs ob_*: worst %.2e"
              % (plan + (n_st, worst)))


# ---- 3. the segment form at forced chunk counts -------------------------------------------------------------------------------

SEG_CHUNKS = (1, 2, 3, 5, 7)


@pytest.mark.parametrize("quads", [True, False], ids=["quads", "pairs"])
def test_segment_form_at_forced_chunk_counts(shape_b, monkeypatch, quads, capsys):
    """shape B at 300 lags: pq = 2, hop 3072, 23 frames per window -- k_xcorr_segments_quad one frame per trip, k_xcorr_segments two
    (the last trip holds one frame) -- with TDOA_SEG_CHUNKS = 1, 2, 3, 5 and 7 (the clamp N2 / 2 - 1): chunk c takes the trips
    c, c + chunks, ..., so the first (checked) frame, the ragged last frame and the odd frame fall to another workgroup each
    time.  Every count against the oracle: all 60 lags identical, corr within 1e-5, process_fine's frac within the 1e-4 of
    test_short_lag_form_in_the_batched_path.  The lags are the same for every count.  The corr values are NOT compared byte for
    byte between counts: another count adds a pair-window's frames in another order, by design -- which is also what shows that
    the override took effect (there is no getter): counts 1 and 7 must not return the same corr bytes"""
    import tdoa_amd
    ml, shape = 300, shape_b
    wids = range(shape.n_windows)
    for wid in wids:
        shape.peaks(wid, ml)
        shape.fracs(wid, ml, 120.0)
    assert _no_geometry_env()
    got = {}
    for chunks in SEG_CHUNKS:
        monkeypatch.setenv("TDOA_SEG_CHUNKS", str(chunks))
        with tdoa_amd.Context(max_lag=ml, window_len=shape.wl) as c:
            shape.upload(c)
            c.debug_flags(no_segment_quads=not quads)
            warm, _ = c.process_fine(120.0)
            c.poison_workspace()
            peaks, fine = c.process_fine(120.0)
            r = c.last_route()
            assert tuple(c.plan_info())[1:] == (4096, 16)
            assert (r["inverse"], r["seg_pq"], r["seg_quads"]) == ("segments", 2, quads), (chunks, r)
            worst = shape.check(c, peaks, wids, ml, "%d chunks" % chunks)
        assert _same_bytes(warm, peaks), chunks
        want = np.array([shape.fracs(wid, ml, 120.0) for wid in wids])
        dfrac = np.abs(fine["frac"] - want).max()
        assert dfrac < 1e-4, (chunks, dfrac)
        got[chunks] = (peaks, worst, dfrac)
    for chunks in SEG_CHUNKS:
        assert np.array_equal(got[chunks][0]["lag"], got[1][0]["lag"]), chunks
    assert not np.array_equal(got[1][0]["corr"], got[7][0]["corr"])
    with capsys.disabled():
        print("\n  segment form, %s: " % ("quads" if quads else "one pair-window at a time") +
              "; ".join("%d chunks %.2e (frac %.1e)" % (k, got[k][1], got[k][2]) for k in SEG_CHUNKS))


def test_segment_form_single_pair_pq4_at_forced_chunk_counts(oracle, monkeypatch):
    """one pair of unequal windows (123 457 and 99 991 samples) at 1000 lags: PQ = 4 (hop 2048, 61 frames, 31 trips of
    k_xcorr_segments<4>; the frames of the tail run off the shorter window, then off both) at one chunk and at the most the
    clamp allows (4096 x 16 plan: N2 / 2 - 1 = 7): all 1999 lags against the oracle's lag array"""
    import tdoa_amd
    n1, n2, ml, delay = 123_457, 99_991, 1000, 37
    a = oracle.simulate_delayed_fm(n1, 0, 731, 1)
    b = oracle.simulate_delayed_fm(n2, delay, 731, 2)
    olag, _, want = oracle.b_xcorr_peak_fft(oracle.b_preprocess(a)[0], oracle.b_preprocess(b)[0], ml)
    assert olag == delay
    assert _no_geometry_env()
    got = {}
    for chunks in (1, 7):
        monkeypatch.setenv("TDOA_SEG_CHUNKS", str(chunks))
        with tdoa_amd.Context(max_lag=ml, window_len=max(n1, n2)) as c:
            warm = c.fm_xcorr_lags(a, b, ml)
            c.poison_workspace()
            lags = c.fm_xcorr_lags(a, b, ml)
            r = c.last_route()
            assert tuple(c.plan_info())[1:] == (4096, 16)
            assert (r["inverse"], r["seg_pq"], r["seg_quads"]) == ("segments", 4, False), (chunks, r)
            assert c.fm_xcorr(a, b, ml)[0] == delay
        assert np.array_equal(warm, lags)
        _assert_lags_close(lags, want)
        got[chunks] = lags
    assert not np.array_equal(got[1], got[7])                          # (the override took effect: another order of the sums)


# ---- 4. the staged walk's ring ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def walk_reference(caps_256, caps_512):
    """the per-pair walk (k_pair_decimate_cols: TDOA_DEBUG_DEC_COLS_ALWAYS | NO_DEC_STAGED), which
    tests/test_gpu_column_walk_oracle.py holds against the oracle: one run per batch, shared by that batch's variants"""
    import tdoa_amd
    done = {}

    def reference(name, n_st):
        if (name, n_st) not in done:
            assert _no_geometry_env()
            shape = _first_stations(caps_256 if name == "256" else caps_512, n_st)
            with tdoa_amd.Context(max_lag=ML_DEC, window_len=shape.wl) as c:
                shape.upload(c)
                c.debug_flags(dec_cols_always=True, no_dec_staged=True)
                walk = c.process()
                assert (c.last_route()["inverse"], c.last_route()["pair_step"]) == ("decimated", "columns")
            assert (walk["lag"] == _planted(shape.delays)[None, :]).all()
            walk.setflags(write=False)
            done[(name, n_st)] = walk
        return done[(name, n_st)]
    return reference


STAGED_VARIANTS = (
    [("256", 5, {"TDOA_DEC_STAGED_ROWS": r}) for r in (4, 2)] +
    [("256", 5, {"TDOA_DEC_STAGED_BUFS": b}) for b in (2, 4, 16)] +
    [("256", 5, {"TDOA_DEC_STAGED_LOADERS": w}) for w in (2, 4)] +
    [("256", 5, {"TDOA_DEC_STAGED_ROWS": 2, "TDOA_DEC_STAGED_BUFS": 16})] +
    [("256", 8, {"TDOA_DEC_STAGED_ROWS": r}) for r in (4, 2)] +
    [("256", 8, {"TDOA_DEC_STAGED_BUFS": b}) for b in (2, 3)] +
    [("256", 8, {"TDOA_DEC_STAGED_LOADERS": w}) for w in (2, 4)] +
    [("512", 4, {"TDOA_DEC_STAGED_ROWS": 4})])


@pytest.mark.parametrize("name,n_st,env", STAGED_VARIANTS,
                         ids=["%s-%dst-%s" % (n, s, "-".join("%s%d" % (k[len("TDOA_DEC_STAGED_"):].lower(), v) for k, v in e.items())) for n, s, e in STAGED_VARIANTS])
def test_staged_walk_ring_geometries(caps_256, caps_512, walk_reference, monkeypatch, name, n_st, env):
    """k_pair_decimate_staged with another ring than the library's (8 rows per phase, 2 or 3 phases, one loader wave): 4 and 2
    rows per phase (the <N2, 4> and <N2, 2> instances), another ring depth, 2 and 4 loader waves -- what the A/B numbers of
    DESIGN.md and fm_route.inc were measured with.  5 stations = one group of ten walks, 8 stations = two groups of fourteen
    and eight station slots (with four loader waves a workgroup holds twelve walks: three groups), 4 stations on the 4096 x 512
    plan.  The walk's arithmetic and its order do not depend on the ring: the bytes of the per-pair walk, and the planted lags.
    (The ring's depth is clamped to what the LDS holds and the loader may leave in flight: at 8 rows per phase 5 stations get
    3 phases from TDOA_DEC_STAGED_BUFS = 4 and 16 alike, 8 stations 2 from 3; with 2 rows per phase BUFS = 16 gives 5 stations
    the deepest ring there is, 8 phases.)"""
    import tdoa_amd
    shape = _first_stations(caps_256 if name == "256" else caps_512, n_st)
    walk = walk_reference(name, n_st)
    assert _no_geometry_env()
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    with tdoa_amd.Context(max_lag=ML_DEC, window_len=shape.wl) as c:
        shape.upload(c)
        warm = c.process()
        assert tuple(c.plan_info())[1:] == (4096, int(name))
        assert (c.last_route()["inverse"], c.last_route()["pair_step"]) == ("decimated", "staged")
        c.poison_workspace()
        peaks = c.process()
        assert (c.last_route()["inverse"], c.last_route()["pair_step"]) == ("decimated", "staged")
    assert _same_bytes(peaks, walk) and _same_bytes(warm, peaks)
    assert (peaks["lag"] == _planted(shape.delays)[None, :]).all() and (peaks["abs_corr"] > 100.0).all()


# ---- 5. TZ padding ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def two_sweep_pair(oracle):
    """the single pair of test_two_sweep_plan_padded_rows_in_every_form: 9 000 000 samples, delay 1234"""
    n, delay = 9_000_000, 1234
    return oracle.simulate_delayed_fm(n, 0, 77, 1), oracle.simulate_delayed_fm(n, delay, 77, 2), delay


@pytest.fixture(scope="module")
def two_sweep_default(two_sweep_pair):
    """the lag arrays at the library's own padding (256 elements: what tests/test_gpu_fm.py holds against the oracle)"""
    return _two_sweep_lags(two_sweep_pair, None)


def _two_sweep_lags(pair, zpad):
    import tdoa_amd
    a, b, delay = pair
    assert ("TDOA_ZPAD" in os.environ) == (zpad is not None)
    out = []
    with tdoa_amd.Context() as c:
        # (short-lag rows, the full inverse, the short-lag rows again: every run but the first starts on poisoned workspace)
        for no_short_lag, want in ((False, ("short_lag", 8)), (True, ("full", 0)), (False, ("short_lag", 8))):
            c.debug_flags(no_short_lag=no_short_lag)
            c.poison_workspace()
            lags = c.fm_xcorr_lags(a, b, 3000)
            assert tuple(c.plan_info())[1:] == (4096, 2048)
            assert (c.last_route()["inverse"], c.last_route()["fk"]) == want
            assert int(np.argmax(np.abs(lags))) - 2999 == delay
            out.append(lags)
    assert np.array_equal(out[0], out[2])
    return out[1:][::-1]


@pytest.mark.parametrize("zpad", [0, 16, 4096])
def test_two_sweep_plan_at_other_row_paddings(two_sweep_pair, two_sweep_default, monkeypatch, zpad):
    """N = 2^24 (4096 x 2048): the elements of padding after every 256 rows of TZ (FftPlan.zpad) move rows, they do not touch
    arithmetic -- none, the smallest that keeps rows 128-byte aligned, and the largest the knob allows return the lag arrays of
    the default 256 byte for byte, from the short-lag rows (k_inv_row_pair4096<*, 8>) and from the full inverse"""
    monkeypatch.setenv("TDOA_ZPAD", str(zpad))
    short, full = _two_sweep_lags(two_sweep_pair, zpad)
    assert np.array_equal(short, two_sweep_default[0]) and np.array_equal(full, two_sweep_default[1])
