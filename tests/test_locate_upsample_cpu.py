"""CPU: sub-sample locate (tdoa_locate_set_upsample; include/tdoa_mi355x.h, "sub-sample locate").  The committed taps against
their formula, the numpy statement of the upsampler (tdoa_amd.upsample) against Python integers on rows that touch both edges,
the fine-lag rule and the searches' statement against an enumeration, the noisy case the feature exists for, and the boundary of
the entry points that needs no device.  POSITIONS, window_q(), fine_table() and fine_cell() are shared with
tests/test_gpu_locate_upsample.py, which runs the kernels on the same words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_locate_cpu import FS, GRID, PAIRS4, ST4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdoa_locate_set_upsample", "tdoa_group_locate_set_upsample", "tdoa_locate_upsample_taps", "tdoa_debug_upsample_q")
FACTORS = (2, 4, 8, 16)
ML = 128


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) LocateSetUpsample(", "C.tdoa_locate_set_upsample(", "func (g *Group) LocateSetUpsample(",
                 "C.tdoa_group_locate_set_upsample(", "func LocateUpsampleTaps(", "C.tdoa_locate_upsample_taps("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    assert hasattr(capi.Context, "locate_set_upsample") and hasattr(capi.Context, "upsample_q")
    assert hasattr(capi.Group, "locate_set_upsample") and hasattr(capi, "locate_upsample_taps")
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("n_U = (n - 1) U + 1 words", "Q_U[U l + r] = floor((sum over k = 0 .. 15 of h_r[k] Q[l + k - 7] + 2^14) / 2^15)",
                   "h_r = h16[r 16 / U]", "h16[rho][k] = rint(2^15 sinc(x) kaiser_6(x / 8)), x = k - 7 - rho / 16",
                   "Phase 0 is the delta: Q_U[U l] = Q[l].", "sgn(d) * ((2|d| U + 16) div 32)",
                   "lags are in units of 1/U sample: a range difference is lag / (U * sample_rate) * c.",
                   "4 * P * (stack length in use) > 2^17", "|t| * U >= 2^31",
                   "upsampling comes after the merge", "U not one of 1, 2, 4, 8, 16"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handles_and_a_bad_factor_need_no_device(capi):
    lib = capi.load()
    taps = np.full(16 * 16 + 1, 77, dtype=np.int32)
    pt = taps.ctypes.data_as(C.POINTER(C.c_int32))
    q = np.zeros(7, dtype=np.int64)
    pq = q.ctypes.data_as(C.POINTER(C.c_int64))
    for U in (1, 2, 4, 8, 16, 0, 3, -2, 32):
        assert lib.tdoa_locate_set_upsample(None, U) == 1
        assert lib.tdoa_group_locate_set_upsample(None, U) == 1
        assert lib.tdoa_debug_upsample_q(None, pq, 1, U, pq) == 1
        assert lib.tdoa_locate_upsample_taps(U, None) == 1
    for U in (0, 3, 5, -1, 17, 32):
        assert lib.tdoa_locate_upsample_taps(U, pt) == 1 and (taps == 77).all()
        with pytest.raises(capi.TdoaError) as e:
            capi.locate_upsample_taps(U)
        assert e.value.status == 1


# ---- the taps -------------------------------------------------------------------------------------------------------------
def test_taps_are_the_literals_and_the_formula(capi):
    from tdoa_amd import upsample
    h = upsample.H16
    assert h.shape == (16, 16) and h.dtype == np.int32
    for U in (1,) + FACTORS:
        got = capi.locate_upsample_taps(U)
        assert got.shape == (U, 16) and got.dtype == np.int32
        assert (got == h[::16 // U]).all() and (got == upsample.taps(U)).all(), U
    exact = upsample.formula()
    worst = float(np.abs(h - exact).max())
    print("largest distance of a literal from the float64 formula: %.3f; the phases' sums - 2^15: %s; the largest sum of magnitudes %.4f 2^15"
          % (worst, (h.sum(axis=1) - 2 ** 15).tolist(), np.abs(h).sum(axis=1).max() / 2.0 ** 15))
    assert worst <= 1.0
    assert h[0].tolist() == [0] * 7 + [2 ** 15] + [0] * 8               # phase 0 is the delta
    # the mirror: x(16 - rho, 15 - k) = -x(rho, k) and the window is even.  (k = 15 - k' is the index where both exist for every
    # k; the request's "15 - k + 1" pairs x with -(x - 1), which is no symmetry of the formula.)
    for rho in range(1, 16):
        assert h[rho].tolist() == h[16 - rho][::-1].tolist(), rho
    assert (np.abs(h.sum(axis=1) - 2 ** 15) <= 16).all()
    assert int(np.abs(h.astype(np.int64)).sum(axis=1).max()) <= 4 * 2 ** 15


# ---- hand cases at max_lag 4: n = 7, every output touches an edge --------------------------------------------------------
def edge_rows(n, seed):
    """rows of n lags that the GPU test shares: random words up to 2^60 in magnitude, rows of +-2^60, alternating signs"""
    rng = np.random.default_rng(seed)
    big = 2 ** 60
    rows = [rng.integers(-big, big + 1, size=n, dtype=np.int64) for _ in range(4)]
    rows += [np.full(n, big, dtype=np.int64), np.full(n, -big, dtype=np.int64),
             np.where(np.arange(n) % 2 == 0, big, -big).astype(np.int64), rng.integers(-3, 4, size=n, dtype=np.int64)]
    return np.stack(rows)


@pytest.mark.parametrize("U", FACTORS)
def test_hand_cases_at_max_lag_4(U):
    from tdoa_amd import upsample
    n = 7
    h = upsample.taps(U)
    assert upsample.upsampled_len(n, U) == 6 * U + 1
    for l0 in range(n):                                                  # a delta of 2^15 at each lag gives the taps' columns
        q = np.zeros(n, dtype=np.int64)
        q[l0] = 2 ** 15
        out = upsample.upsample(q, U)
        assert out.shape == (6 * U + 1,) and out.dtype == np.int64
        for u in range(6 * U + 1):
            k = l0 - u // U + 7
            assert out[u] == (h[u % U][k] if 0 <= k < 16 else 0), (l0, u)
    rows = edge_rows(n, 71)
    out = upsample.upsample(rows, U)
    assert (out[:, ::U] == rows).all()                                   # Q_U[U l] = Q[l]
    for row, got in zip(rows, out):
        assert got.tolist() == upsample.upsample_exact(row, U)           # Python integers, straight from the definition
    assert int(np.abs(out).max()) <= 2 * 2 ** 60 + 2 ** 56 + 1           # |Q_U| <= 2.04 |Q| + 1
    assert (upsample.upsample(rows[0], 1) == rows[0]).all()
    with pytest.raises(ValueError):
        upsample.upsample(rows, 3)


def test_rounding_is_half_up_through_the_floor():
    """h_r[7] Q[l] = 2^14 mod 2^15 exactly is a half: it goes up on both signs"""
    from tdoa_amd import upsample
    h = int(upsample.H16[8][7])                                          # phase 8 of U = 2: 20639, odd
    for v in (2 ** 14, -2 ** 14, 3 * 2 ** 14, -3 * 2 ** 14):
        q = np.zeros(33, dtype=np.int64)
        q[16] = v
        assert (h * v) % 2 ** 15 == 2 ** 14
        assert int(upsample.upsample(q, 2)[2 * 16 + 1]) == (h * v + 2 ** 14) // 2 ** 15 == (h * v) // 2 ** 15 + 1


# ---- the searches' statement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", (2, 4, 16))
def test_the_fine_lag_rule_against_an_enumeration(U):
    from tdoa_amd import locate, upsample
    d = np.arange(-300, 301)
    want = []
    for x in d.tolist():                                                 # nearest integer to x U / 16, halves away from zero
        a = (2 * abs(x) * U + 16) // 32
        want.append(-a if x < 0 else a)
    assert upsample.fine_lags(d, U).tolist() == want
    table = np.stack([np.zeros_like(d), d], axis=1)
    t, _, guard, ml = upsample.scaled_args(table, None, 3, 20, U)
    assert locate.pair_lags(t)[:, 0].tolist() == want and guard == 3 * U and ml == 19 * U + 1 and 2 * ml - 1 == 38 * U + 1
    halves = [x for x in d.tolist() if (abs(x) * U) % 16 == 8]           # x U / 16 = m + 1/2
    assert all(abs(want[x + 300]) == (abs(x) * U + 8) // 16 and (want[x + 300] > 0) == (x > 0) for x in halves)
    if U == 16:                                                          # the table's own unit: every difference is a fine lag, no halves
        assert not halves and want == d.tolist()
    else:
        assert {x > 0 for x in halves} == {True, False}
    # with clocks: U (t_j - t_i) + U (k_j - k_i) = U d
    t, k, _, _ = upsample.scaled_args(np.array([[0, 5]]), np.array([0, 3]), 0, 20, U)
    assert locate.pair_lags(t, k).tolist() == [[(2 * 8 * U + 16) // 32]]


@pytest.mark.parametrize("U", (2, 4, 16))
def test_the_statement_against_every_cell_enumerated(U):
    """small random Q, delays that put pairs outside the range: the map of locate.locate on the scaled arguments is the sum of
    |Q_U| at the enumerated fine lags, Q_U in Python integers"""
    from tdoa_amd import locate, upsample
    rng = np.random.default_rng(100 + U)
    for S, ml in ((3, 4), (4, 9)):
        P, n = S * (S - 1) // 2, 2 * ml - 1
        q = rng.integers(-2 ** 40, 2 ** 40, size=(P, n), dtype=np.int64)
        table = rng.integers(-20 * ml, 20 * ml + 1, size=(23, S), dtype=np.int32)
        clock = rng.integers(-40, 41, size=S, dtype=np.int32)
        t, k, _, ml_u = upsample.scaled_args(table, clock, 0, ml, U)
        rec, lags, corr, score_map = locate.locate(upsample.upsample(q, U), t, 5, ml_u, 1, 2, k)
        fine = [upsample.upsample_exact(row, U) for row in q]
        lo, n_u = -(ml - 1) * U, (n - 1) * U + 1
        want, n_out = [], 0
        for c in range(len(table)):
            s, p = 0, 0
            for i in range(S):
                for j in range(i + 1, S):
                    d = int(table[c][j]) - int(table[c][i]) + int(clock[j]) - int(clock[i])
                    a = (2 * abs(d) * U + 16) // 32
                    idx = (-a if d < 0 else a) - lo
                    if 0 <= idx < n_u:
                        s += abs(fine[p][idx])
                    else:
                        n_out += 1
                    p += 1
            want.append(s)
        assert score_map.tolist() == want and n_out > 0
        assert int(rec["cell"]) == want.index(max(want)) and int(rec["score_q"]) == max(want)


# ---- the noisy case -------------------------------------------------------------------------------------------------------
# Twelve emitter positions (latitude, longitude) off the cell centres, anywhere on the 48 x 64 grid of tests/test_locate_cpu.py,
# at the grid's height: numpy's default_rng(2025), latitude lat0 + uniform(0, 47) dlat, then longitude lon0 + uniform(0, 63) dlon,
# rounded to 1e-6 degree; a draw is kept when the coarse search of its noise-free window finds a cell within one row and column of
# the position's own (the first 12 draws all do; of the first 65, 60).
POSITIONS = ((41.346958, -96.039667), (41.315504, -95.896265), (41.343452, -96.135674), (41.219682, -95.87034),
             (41.287063, -96.069965), (41.233234, -96.087481), (41.191389, -96.111668), (41.343129, -96.026473),
             (41.171871, -96.00515), (41.214209, -96.093341), (41.198997, -95.977609), (41.27108, -95.88026))
FINE = 8                    # fine cells per cell
FINE_SIDE = 33              # the fine grid: 33 x 33 cells of 1/8 cell around a cell


def position_ecef(lat, lon):
    from tdoa_amd import locate
    return locate.ecef(lat, lon, GRID["height_m"])


def metres(a, b):
    return float(np.linalg.norm(position_ecef(*a) - position_ecef(*b)))


def window_iq(oracle, k, noise):
    """position k's window of 8 192 samples per station, u8 IQ: station delays rint(4 fs dist / c) quarter samples (minus their
    minimum), realised as simulate_delayed_fm(4 * 8192, d4, 300 + k, 1000 (s + 1) + k, 1.0, noise) with every 4th IQ sample kept"""
    from tdoa_amd import locate
    st = locate.ecef(*np.array(ST4).T)
    dist = np.linalg.norm(st - position_ecef(*POSITIONS[k]), axis=1)
    d4 = np.rint(4 * FS * dist / locate.SPEED_OF_LIGHT).astype(np.int64)
    d4 -= d4.min()
    return [np.ascontiguousarray(oracle.simulate_delayed_fm(4 * 8192, int(d4[s]), 300 + k, 1000 * (s + 1) + k, 1.0, noise)
                                 .reshape(-1, 2)[::4]).reshape(-1) for s in range(4)]


def window_q(oracle, k, noise):
    """... -> Q [6][255] of the float64 pipeline, one window per stack"""
    from tdoa_amd import stacking
    sig = [oracle.b_preprocess(s)[0] for s in window_iq(oracle, k, noise)]
    return np.array([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ML)) for i, j in PAIRS4])


def coarse_table():
    from tdoa_amd import locate
    return locate.grid_table(ST4, sample_rate=FS, **GRID)


def cell_position(cell):
    return GRID["lat0"] + (cell // 64) * GRID["dlat"], GRID["lon0"] + (cell % 64) * GRID["dlon"]


def fine_grid(cell):
    lat, lon = cell_position(cell)
    half = (FINE_SIDE - 1) // 2
    return dict(lat0=lat - half * GRID["dlat"] / FINE, lon0=lon - half * GRID["dlon"] / FINE, dlat=GRID["dlat"] / FINE,
                dlon=GRID["dlon"] / FINE, rows=FINE_SIDE, cols=FINE_SIDE, height_m=GRID["height_m"])


def fine_table(cell):
    from tdoa_amd import locate
    return locate.grid_table(ST4, sample_rate=FS, **fine_grid(cell))


def fine_cell(q, cell, U):
    """the statement: the best cell of the fine grid around `cell` on Q upsampled by U"""
    from tdoa_amd import locate, upsample
    t, _, _, ml = upsample.scaled_args(fine_table(cell), None, 0, ML, U)
    return int(locate.locate(upsample.upsample(q, U), t, FINE_SIDE, ml, 1)[0]["cell"])


def fine_position(cell, f):
    g = fine_grid(cell)
    return g["lat0"] + (f // FINE_SIDE) * g["dlat"], g["lon0"] + (f % FINE_SIDE) * g["dlon"]


def own_cell(k):
    lat, lon = POSITIONS[k]
    return round((lat - GRID["lat0"]) / GRID["dlat"]) * 64 + round((lon - GRID["lon0"]) / GRID["dlon"])


BOUND = 0.5                 # the request's: its measured ratio 0.40 with a 25 % margin (the taps are the request's: 2.039 2^15)


def test_upsampled_surfaces_locate_finer_than_whole_lags(oracle):
    """Four stations, the 48 x 64 grid, one window of 8 192 per stack, max_lag 128, the twelve POSITIONS; the coarse best cell is
    searched again on a 33 x 33 grid of 1/8 cells (55 m x 52 m) around it.  Median distance to the planted position, measured with
    the float64 pipeline at noise 0.3: the coarse cell's centre 203.6 m, the fine grid on whole lags 125.3 m, on Q upsampled x 4
    36.6 m, x 16 34.8 m: a ratio of 0.28 (noise-free 0.30, noise 0.6 0.56; the request measured 283 m, 103 m, 35 m, 31 m: 0.40).  In no
    position is the x 16 fix farther off than the whole-lag one, in 8 of 12 it is nearer.  Over the first 60 kept draws of the same
    generator the medians are 75.1 m and 41.5 m, 0.55.  The whole-lag error depends on where the emitter is: inside the stations'
    polygon a lag's plateau is small (twelve draws from rows 10 .. 38, columns 12 .. 52 gave 41.7 m against 34.4 m, 0.83; sixty 0.70),
    towards the grid's edge the hyperbolae cross at flat angles and it grows to hundreds of metres; the upsampled error stays at
    the case's own floor: the delays are realised to a quarter sample (37 m of range) and the fine cells are 55 m x 52 m."""
    from tdoa_amd import locate
    table = coarse_table()
    for k in range(12):                                                  # the positions' choice holds: noise-free, the coarse cell is near
        c = int(locate.locate(window_q(oracle, k, 0.0), table, 64, ML, 1)[0]["cell"])
        assert abs(c // 64 - own_cell(k) // 64) <= 1 and abs(c % 64 - own_cell(k) % 64) <= 1, k
    d = np.zeros((12, 4))
    for k in range(12):
        q = window_q(oracle, k, 0.3)
        c = int(locate.locate(q, table, 64, ML, 1)[0]["cell"])
        d[k, 0] = metres(POSITIONS[k], cell_position(c))
        for n, U in enumerate((1, 4, 16)):
            d[k, 1 + n] = metres(POSITIONS[k], fine_position(c, fine_cell(q, c, U)))
        print("position %2d: coarse cell (%d, %d) %.0f m; fine grid on whole lags %.0f m, x 4 %.0f m, x 16 %.0f m" % ((k, c // 64, c % 64) + tuple(d[k])))
    med = np.median(d, axis=0)
    print("medians at noise 0.3: coarse cell centre %.1f m, fine grid whole lags %.1f m, upsampled x 4 %.1f m, x 16 %.1f m; ratio %.3f; "
          "x 16 nearer than whole lags in %d positions, farther in %d"
          % (med[0], med[1], med[2], med[3], med[3] / med[1], (d[:, 3] < d[:, 1]).sum(), (d[:, 3] > d[:, 1]).sum()))
    assert med[3] <= BOUND * med[1]
    assert med[1] < med[0]
