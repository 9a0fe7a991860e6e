"""CPU: the numpy statement of the delay-table search (tdoa_amd.locate; include/tdoa_mi355x.h, "delay-table search") on
hand-worked cases, against an enumeration of every cell and pair, and on the noisy case the feature exists for; the host-only
grid table of the library against the numpy one; and the boundary of the entry points that needs no device.  hand_cases(),
noisy_case() and noisy_windows() are shared with tests/test_gpu_locate.py, which runs the kernels on the same words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 2 ** 32
NAMES = ("tdoa_locate_set_table", "tdoa_process_locate", "tdoa_debug_locate_from_q", "tdoa_locate_grid_table",
         "tdoa_group_locate_set_table", "tdoa_group_process_locate")
# the three stations of tests/test_gpu_closure.py and a fourth
ST4 = [(41.18660274289527, -95.96064116595667, 355.69), (41.24669616513154, -96.08366304481238, 329.0),
       (41.32916620016985, -96.03513381562004, 373.18), (41.26, -95.93, 340.0)]
FS = 2e6
GRID = dict(lat0=41.16, lon0=-96.16, dlat=0.004, dlon=0.005, rows=48, cols=64, height_m=350.0)
PAIRS4 = [(i, j) for i in range(4) for j in range(i + 1, 4)]


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import locate
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) LocateSetTable(", "C.tdoa_locate_set_table(", "func (g *gpuCorrelator) ProcessLocate(",
                 "C.tdoa_process_locate(", "func (g *Group) ProcessLocate(", "C.tdoa_group_process_locate(",
                 "C.tdoa_group_locate_set_table(", "C.tdoa_locate_grid_table("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("locate_set_table", "process_locate", "locate_from_q"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.Group, "locate_set_table") and hasattr(capi.Group, "process_locate") and hasattr(capi, "locate_grid_table")
    # the record: the fields of the header in their order, 48 bytes, no padding
    assert capi.LOCATION_DTYPE == locate.LOCATION_DTYPE and capi.LOCATION_DTYPE.itemsize == 48
    assert capi.LOCATION_DTYPE.names == ("cell", "runner_cell", "pairs_in", "reserved", "score_q", "runner_q", "score", "runner_up")
    m = re.search(r"typedef struct \{([^}]*)\} tdoa_location;", hdr)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+([^;]+);", m.group(1))
    assert [(t, [n.strip() for n in names.split(",")]) for t, names in fields] == [
        ("int32_t", ["cell", "runner_cell", "pairs_in", "reserved"]), ("int64_t", ["score_q", "runner_q"]),
        ("double", ["score", "runner_up"])]
    assert re.search(r"#define TDOA_DELAY_UNIT 16\b", hdr) and locate.DELAY_UNIT == 16
    # the definition is in the header in the words the tests hold the library to
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("delay[n_cells][n_stations] is int32, in units of 1/16 sample (TDOA_DELAY_UNIT). 1 <= n_cells <= 2^22.",
                   "row = c div n_cols and col = c mod n_cols. The last row may be short.",
                   "d = t[c][j] - t[c][i], taken in 64 bits.",
                   "lag_p(c) = sgn(d) * ((2|d| + 16) div 32).",
                   "score_q(c) is the sum over all P pairs of M_p[lag_p(c)].",
                   "contributes 0 and is not counted in pairs_in(c).",
                   "Among equal maxima the smaller cell index wins.",
                   "If the largest score is 0, the zero record and zero lags and correlations are returned.",
                   "max(|row - row*|, |col - col*|) > min_separation (>= 1)",
                   "runner_q and runner_cell are 0 when there is none",
                   "TDOA_ERR_UNSUPPORTED when P * (stack length in use) > 2^17"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handle_is_invalid_without_a_device(capi):
    lib = capi.load()
    loc = np.zeros(4, dtype=capi.LOCATION_DTYPE)
    q = np.zeros(3 * 7, dtype=np.int64)
    table = (C.c_int32 * 6)(0, 16, 32, 0, 0, 0)
    pl, pq = loc.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_int64))
    for args in ((table, 2, 2, 3), (None, 0, 1, 0), (table, -1, 2, 3), (table, 2, 0, 3), (table, 2, 2, 65)):
        assert lib.tdoa_locate_set_table(None, *args) == 1
        assert lib.tdoa_group_locate_set_table(None, *args) == 1
    for m, sep in ((0, 1), (2, 3), (-1, 1), (0, 0)):
        assert lib.tdoa_process_locate(None, m, sep, pl, None, None, None) == 1
        assert lib.tdoa_group_process_locate(None, m, sep, pl, None, None, None) == 1
        assert lib.tdoa_debug_locate_from_q(None, pq, 1, 3, 1, sep, pl, None, None, None) == 1
    assert lib.tdoa_process_locate(None, 0, 1, None, None, None, None) == 1
    assert lib.tdoa_debug_locate_from_q(None, None, 0, 1, 0, 1, None, None, None, None) == 1


# ---- hand-worked cases: three stations, max_lag 4 (7 lags, lag l at index l + 3), rows 01, 02, 12 -------------------------
def _q(ml, *peaks):
    """three rows of 2 ml - 1 zeros with (row, lag, value in units of 2^32) set"""
    q = np.zeros((3, 2 * ml - 1), dtype=np.int64)
    for row, lag, value in peaks:
        q[row, lag + ml - 1] = value * ONE
    return q


def hand_cases():
    """[(name, dict(q, ml, table, n_cols, sep, n_w), expected or None for the zero record)]; expected: cell, runner_cell,
    pairs_in, lags (0 for a pair outside), inside, and score, runner and map in units of 2^32"""
    # d = +-8 and +-24 are half-way: 8/16 -> 1, 24/16 -> 2, away from zero on both signs (d12 = -16, -48 are exact);
    # d = +-7 and +-23 are just below: 0 and 1 (d12 = -14 -> -1, -46 -> -3)
    halves = np.array([(0, 8, -8), (0, 24, -24), (0, 7, -7), (0, 23, -23)], dtype=np.int32)
    q_halves = _q(4, (0, 1, 3), (0, 2, 5), (1, -1, 3), (1, -2, 5), (2, -1, 1), (2, -3, 2))
    # cells 0 .. 6: lags (a, 0, -a) for a = -3 .. 3, scoring M_01[a] only; cell 7: lags (0, 3, 3), scoring 2 + 9
    rows = np.array([(0, 16 * a, 0) for a in range(-3, 4)] + [(0, 0, 48)], dtype=np.int32)
    q_rows = _q(4, (0, -3, 1), (0, -2, 1), (0, -1, 4), (0, 0, 2), (0, 1, 6), (0, 2, 1), (0, 3, 5), (1, 3, 9))
    map_rows = [1, 1, 4, 2, 6, 1, 5, 11]
    twins = np.array([(0, 0, 0), (0, 16, 32), (0, 0, 0), (0, 16, 32)], dtype=np.int32)
    q_twins = _q(4, (0, 1, 2), (1, 2, 2), (2, 1, 2))
    return [
        ("half-way differences round away from zero on both signs; n_cols = n_cells",
         dict(q=q_halves, ml=4, table=halves, n_cols=4, sep=1, n_w=1),
         dict(cell=1, runner_cell=3, pairs_in=3, lags=(2, -2, -3), inside=(1, 1, 1), score=12, runner=8, map=[7, 12, 1, 8])),
        ("negative Q counts by its magnitude", dict(q=-q_halves, ml=4, table=halves, n_cols=4, sep=1, n_w=4),
         dict(cell=1, runner_cell=3, pairs_in=3, lags=(2, -2, -3), inside=(1, 1, 1), score=12, runner=8, map=[7, 12, 1, 8])),
        # cell 0: d01 = 48 -> 3, d02 = 96 -> 6 (outside |l| < 4), d12 = 48 -> 3; the other cell is within min_separation
        ("a pair outside the range contributes 0", dict(q=_q(4, (0, 3, 2), (2, 3, 4), (0, 0, 1), (1, 0, 1), (2, 0, 1)), ml=4,
                                                        table=np.array([(0, 48, 96), (0, 0, 0)], dtype=np.int32), n_cols=2, sep=1, n_w=1),
         dict(cell=0, runner_cell=0, pairs_in=2, lags=(3, 0, 3), inside=(1, 0, 1), score=6, runner=0, map=[6, 3])),
        ("equal maxima: the smaller cell, and the runner-up its twin", dict(q=q_twins, ml=4, table=twins, n_cols=4, sep=1, n_w=1),
         dict(cell=1, runner_cell=3, pairs_in=3, lags=(1, 2, 1), inside=(1, 1, 1), score=6, runner=6, map=[0, 6, 0, 6])),
        ("all zeros", dict(q=_q(4), ml=4, table=halves, n_cols=2, sep=1, n_w=1), None),
        # 8 cells in rows of 3: the last row is (6, 7).  The location is cell 7 = (2, 1); cells 3 .. 6 are within one row and
        # column, the 6 of cell 4 and the 5 of cell 6 do not count: the runner-up is the 4 of cell 2 = (0, 2)
        ("the runner-up is excluded by rows and columns at a short last row", dict(q=q_rows, ml=4, table=rows, n_cols=3, sep=1, n_w=2),
         dict(cell=7, runner_cell=2, pairs_in=3, lags=(0, 3, 3), inside=(1, 1, 1), score=11, runner=4, map=map_rows)),
        ("every other cell within min_separation: no runner-up", dict(q=q_rows, ml=4, table=rows, n_cols=3, sep=2, n_w=1),
         dict(cell=7, runner_cell=0, pairs_in=3, lags=(0, 3, 3), inside=(1, 1, 1), score=11, runner=0, map=map_rows)),
        ("n_cols = n_cells: a plain list, columns only", dict(q=q_rows, ml=4, table=rows, n_cols=8, sep=1, n_w=1),
         dict(cell=7, runner_cell=4, pairs_in=3, lags=(0, 3, 3), inside=(1, 1, 1), score=11, runner=6, map=map_rows)),
        # the only cell outside the neighbourhood scores 0: it is the runner-up all the same
        ("a runner-up that scores 0", dict(q=q_twins, ml=4, table=twins[[1, 0, 0, 0, 0]], n_cols=5, sep=2, n_w=1),
         dict(cell=0, runner_cell=3, pairs_in=3, lags=(1, 2, 1), inside=(1, 1, 1), score=6, runner=0, map=[6, 0, 0, 0, 0])),
    ]


def _check_hand_case(got, arg, want):
    """got: (record, lags [P], corr [P], map [n_cells])"""
    from tdoa_amd import locate
    rec, lags, corr, score_map = got
    assert score_map.dtype == np.int64 and lags.dtype == np.int32 and corr.dtype == np.float64
    if want is None:
        assert rec.tobytes() == bytes(locate.LOCATION_DTYPE.itemsize)
        assert not lags.any() and corr.tobytes() == bytes(corr.nbytes) and not score_map.any()
        return
    root = np.sqrt(np.float64(arg["n_w"]))
    assert (int(rec["cell"]), int(rec["runner_cell"]), int(rec["pairs_in"]), int(rec["reserved"])) == \
           (want["cell"], want["runner_cell"], want["pairs_in"], 0)
    assert (int(rec["score_q"]), int(rec["runner_q"])) == (want["score"] * ONE, want["runner"] * ONE)
    assert float(rec["score"]) == want["score"] / root and float(rec["runner_up"]) == want["runner"] / root
    assert score_map.tolist() == [m * ONE for m in want["map"]] and score_map[want["cell"]] == rec["score_q"]
    assert lags.tolist() == list(want["lags"])
    ml = arg["ml"]
    assert corr.tolist() == [float(arg["q"][p, lag + ml - 1]) / ONE / root if inside else 0.0
                             for p, (lag, inside) in enumerate(zip(want["lags"], want["inside"]))]
    assert np.abs(corr).sum() == pytest.approx(float(rec["score"]), rel=1e-15)


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_worked_cases(name, arg, want):
    from tdoa_amd import locate
    got = locate.locate(arg["q"], arg["table"], arg["n_cols"], arg["ml"], arg["sep"], arg["n_w"])
    _check_hand_case(got, arg, want)


def test_pair_lags_rule_and_model_arguments():
    from tdoa_amd import locate, stacking
    d = np.arange(-200, 201)
    lag = locate.pair_lags(np.stack([np.zeros_like(d), d], axis=1))[:, 0]
    assert lag.tolist() == [stacking.shift(int(x), 1, 16) for x in d]          # the slope search's rule
    assert lag[200 + 8] == 1 and lag[200 - 8] == -1 and lag[200 + 24] == 2 and lag[200 - 24] == -2 and lag[200 + 7] == 0
    big = locate.pair_lags(np.array([[-2 ** 31, 2 ** 31 - 1]], dtype=np.int32))        # the difference is taken in 64 bits
    assert big.tolist() == [[(2 * (2 ** 32 - 1) + 16) // 32]]
    assert locate.pair_lags(np.zeros((5, 4), dtype=np.int32)).shape == (5, 6)
    q = np.zeros((3, 7), dtype=np.int64)
    t = np.zeros((2, 3), dtype=np.int32)
    for kw in (dict(min_separation=0), dict(n_cols=0), dict(table=t[:, :1]), dict(q_pairs=q[:, :6]), dict(q_pairs=q[:2])):
        with pytest.raises(ValueError):
            locate.locate(**{"q_pairs": q, "table": t, "n_cols": 2, "max_lag": 4, **kw})


def _brute(q, table, n_cols, ml, sep):
    """every cell and pair by enumeration -> (map, best cell or None, pairs_in, lags, runner cell or None)"""
    n_cells, S = len(table), len(table[0])
    scores, info = [], []
    for c in range(n_cells):
        s, lags, p = 0, [], 0
        for i in range(S):
            for j in range(i + 1, S):
                d = int(table[c][j]) - int(table[c][i])
                a = (2 * abs(d) + 16) // 32
                lag = -a if d < 0 else a
                if -ml < lag < ml:
                    s += abs(int(q[p][lag + ml - 1]))
                    lags.append(lag)
                else:
                    lags.append(None)
                p += 1
        scores.append(s)
        info.append(lags)
    top = max(scores)
    if top == 0:
        return scores, None, 0, None, None
    best = scores.index(top)
    far = [c for c in range(n_cells) if max(abs(c // n_cols - best // n_cols), abs(c % n_cols - best % n_cols)) > sep]
    runner = min((c for c in far if scores[c] == max(scores[f] for f in far)), default=None)
    return scores, best, sum(l is not None for l in info[best]), info[best], runner


def test_model_against_every_cell_enumerated():
    """small random Q with few distinct values, so equal maxima are common; delays that put many pairs outside the range"""
    from tdoa_amd import locate
    rng = np.random.default_rng(23)
    n = n_zero = n_ties = n_out = 0
    for S, ml in ((2, 3), (3, 4), (4, 9), (5, 6)):
        P = S * (S - 1) // 2
        for n_cells, n_cols in ((1, 1), (7, 3), (12, 4), (30, 30), (31, 7)):
            for sep, span in ((1, 16 * ml), (2, 40 * ml)):
                q = rng.integers(-2, 3, size=(P, 2 * ml - 1), dtype=np.int64) * (rng.random() < 0.9)
                table = rng.integers(-span, span + 1, size=(n_cells, S), dtype=np.int32)
                rec, lags, corr, score_map = locate.locate(q, table, n_cols, ml, sep, n_w=2)
                scores, best, pairs_in, want_lags, runner = _brute(q, table, n_cols, ml, sep)
                n += 1
                assert score_map.tolist() == scores
                if best is None:
                    n_zero += 1
                    assert rec.tobytes() == bytes(48) and not lags.any() and not corr.any()
                    continue
                assert (int(rec["cell"]), int(rec["pairs_in"]), int(rec["score_q"])) == (best, pairs_in, scores[best])
                assert lags.tolist() == [l or 0 for l in want_lags]
                assert corr.tolist() == [0.0 if l is None else float(q[p][l + ml - 1]) / ONE / np.sqrt(2.0) for p, l in enumerate(want_lags)]
                assert (int(rec["runner_cell"]), int(rec["runner_q"])) == ((0, 0) if runner is None else (runner, scores[runner]))
                assert rec["runner_q"] <= rec["score_q"] and float(rec["score"]) == float(scores[best]) / ONE / np.sqrt(2.0)
                n_ties += runner is not None and scores[runner] == scores[best]
                n_out += pairs_in < P
    print("%d searches: %d zero records, %d with a runner-up as large as the location, %d with pairs outside" % (n, n_zero, n_ties, n_out))
    assert n_zero >= 2 and n_ties >= 5 and n_out >= 5           # each kind of case occurs


# ---- the host-only grid table --------------------------------------------------------------------------------------------
def test_grid_table_of_the_library_against_numpy(capi):
    """48 x 64 cells, four stations: every entry within 1 unit (1/16 sample) of the float64 numpy value (libm may differ in the
    last place, and an entry may sit on a rounding boundary)"""
    from tdoa_amd import locate
    got = capi.locate_grid_table(ST4, sample_rate=FS, **GRID)
    want = locate.grid_table(ST4, sample_rate=FS, **GRID)
    assert got.shape == want.shape == (48 * 64, 4) and got.dtype == want.dtype == np.int32
    worst = int(np.abs(got.astype(np.int64) - want).max())
    print("largest difference %d unit, %d of %d entries differ; delays %d .. %d units" % (worst, (got != want).sum(), got.size, got.min(), got.max()))
    assert worst <= 1
    assert got.min() > 0 and got.max() < 16 * FS * 60e3 / 299792458.0          # inside 60 km
    # cell r cols + c lies at (lat0 + r dlat, lon0 + c dlon): a station's delay is smallest in the cell next to it
    near = np.unravel_index(np.argmin(got[:, 3]), (48, 64))
    assert near == (round((ST4[3][0] - GRID["lat0"]) / GRID["dlat"]), round((ST4[3][1] - GRID["lon0"]) / GRID["dlon"]))


def test_grid_table_argument_errors(capi):
    lib = capi.load()
    st = np.ascontiguousarray(ST4, dtype=np.float64).reshape(-1)
    out = np.zeros(16, dtype=np.int32)
    ps, po = st.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_int32))
    good = dict(st=ps, n=4, lat0=41.16, lon0=-96.16, dlat=0.004, dlon=0.005, rows=2, cols=2, h=350.0, fs=FS, out=po)
    call = lambda **kw: lib.tdoa_locate_grid_table(*{**good, **kw}.values())
    assert call() == 0 and out.all()
    for kw in (dict(st=None), dict(out=None), dict(n=0), dict(rows=0), dict(cols=0), dict(rows=-1), dict(rows=2049, cols=2049),
               dict(rows=2 ** 22 + 1, cols=1), dict(lat0=float("nan")), dict(lon0=float("inf")), dict(dlat=float("nan")),
               dict(dlon=float("-inf")), dict(h=float("nan")), dict(fs=float("inf")), dict(fs=0.0), dict(fs=1e15)):
        assert call(**kw) == 1, kw                                       # (fs 1e15: the delays do not fit int32)
    bad = st.copy()
    bad[4] = float("nan")
    assert call(st=bad.ctypes.data_as(C.POINTER(C.c_double))) == 1
    with pytest.raises(capi.TdoaError) as e:
        capi.locate_grid_table(ST4, 41.16, -96.16, 0.004, 0.005, 0, 64, 350.0, FS)
    assert e.value.status == 1


# ---- the noisy case ------------------------------------------------------------------------------------------------------
def noisy_case():
    """(table [48 * 64][4], planted cell, station delays in samples, planted pair lags) of the issue's case: a transmitter in
    cell (12, 36) of the 48 x 64 grid; station delays rint(fs dist / c) minus their minimum"""
    from tdoa_amd import locate
    table = locate.grid_table(ST4, sample_rate=FS, **GRID)
    cell = 12 * 64 + 36
    tx = locate.ecef(GRID["lat0"] + 12 * GRID["dlat"], GRID["lon0"] + 36 * GRID["dlon"], GRID["height_m"])
    dist = np.linalg.norm(locate.ecef(*np.array(ST4).T) - tx, axis=1)
    d = np.rint(FS * dist / locate.SPEED_OF_LIGHT).astype(np.int64)
    d -= d.min()
    lags = tuple(int(d[j] - d[i]) for i, j in PAIRS4)
    assert lags == (46, 76, 29, 30, -17, -47)
    return table, cell, [int(x) for x in d], lags


def noisy_windows(oracle, delays, n_windows=12):
    """window w of station s = simulate_delayed_fm(8192, d_s, 300 + w, 1000 (s + 1) + w, 1.0, 0.6) -> [w][s] u8 IQ"""
    return [[oracle.simulate_delayed_fm(8192, delays[s], 300 + w, 1000 * (s + 1) + w, 1.0, 0.6) for s in range(4)]
            for w in range(n_windows)]


def own_lags(q, max_lag):
    """the pairs' independent argmaxes of |Q| (the first of equal maxima) as lags"""
    return tuple(int(np.argmax(np.abs(row))) - (int(max_lag) - 1) for row in q)


def test_the_table_search_finds_the_cell_the_six_argmaxes_miss(oracle):
    """One window per stack, max_lag 128, twelve windows, noise 0.6.  Measured with the float64 pipeline: the six independent
    argmaxes are all right in 0 of 12 windows (40 of 72 pair lags), the best cell is the planted one in 12 of 12."""
    from tdoa_amd import locate, stacking
    ml = 128
    table, planted_cell, delays, planted = noisy_case()
    own_ok = cell_ok = lag_ok = 0
    for w, x in enumerate(noisy_windows(oracle, delays)):
        sig = [oracle.b_preprocess(s)[0] for s in x]
        q = np.array([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ml)) for i, j in PAIRS4])
        rec, lags, corr, score_map = locate.locate(q, table, 64, ml, 1)
        own = own_lags(q, ml)
        own_ok += own == planted
        lag_ok += sum(a == b for a, b in zip(own, planted))
        cell_ok += int(rec["cell"]) == planted_cell
        assert int(rec["pairs_in"]) == 6 and score_map[int(rec["cell"])] == rec["score_q"] and rec["runner_q"] <= rec["score_q"]
        print("window %2d: own %s, cell (%d, %d) lags %s score %.3f runner-up %.3f at (%d, %d)"
              % (w, own, rec["cell"] // 64, rec["cell"] % 64, lags.tolist(), rec["score"], rec["runner_up"],
                 rec["runner_cell"] // 64, rec["runner_cell"] % 64))
    print("the six argmaxes all right in %d of 12 windows (%d of 72 pair lags), the best cell the planted one in %d" % (own_ok, lag_ok, cell_ok))
    assert own_ok <= 2
    assert cell_ok >= 11
