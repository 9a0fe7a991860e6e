"""CPU: the zoom locate (tdoa_process_locate_zoom; include/tdoa_mi355x.h, "zoom locate").  The entries and the header's phrases,
the boundary that needs no device, the numpy statement (tdoa_amd.locate_zoom) against an enumeration in Python integers, the two
consequences of the definition, and the noisy case of tests/test_locate_upsample_cpu.py with one global fine table.
small_case(), global_fine_table() and the noisy helpers are shared with tests/test_gpu_locate_zoom.py, which runs the kernels on
the same words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_locate_cpu import FS, GRID, ST4
from test_locate_upsample_cpu import (BOUND, FINE, FINE_SIDE, ML, POSITIONS, cell_position, coarse_table, fine_cell, metres, window_q)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdoa_locate_set_fine_table", "tdoa_group_locate_set_fine_table", "tdoa_process_locate_zoom", "tdoa_group_process_locate_zoom",
         "tdoa_debug_locate_zoom_from_q")
ZOOM_Z, ZOOM_H = FINE, (FINE_SIDE - 1) // 2           # the noisy case: 8 fine cells per cell, a window of 33 x 33


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import locate_zoom
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) LocateSetFineTable(", "C.tdoa_locate_set_fine_table(", "func (g *Group) LocateSetFineTable(",
                 "C.tdoa_group_locate_set_fine_table(", "func (g *gpuCorrelator) ProcessLocateZoom(", "C.tdoa_process_locate_zoom(",
                 "func (g *Group) ProcessLocateZoom(", "C.tdoa_group_process_locate_zoom("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for name in ("locate_set_fine_table", "process_locate_zoom", "locate_zoom_from_q"):
        assert hasattr(capi.Context, name), name
    assert hasattr(capi.Group, "locate_set_fine_table") and hasattr(capi.Group, "process_locate_zoom")
    assert capi.ZOOM_DTYPE == locate_zoom.ZOOM_DTYPE and capi.ZOOM_DTYPE.itemsize == 64
    assert [capi.ZOOM_DTYPE.fields[n][1] for n in capi.ZOOM_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56]
    assert re.search(r"int32_t cell, runner_cell, pairs_in, n_best;.*?int32_t row_lo, row_hi, col_lo, col_hi;.*?int64_t score_q, runner_q;"
                     r".*?double\s+score, runner_up;.*?\} tdoa_zoom;", hdr, re.S)
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("The coarse stage is tdoa_process_locate on the context's table, clocks, upsample setting and statistics setting",
                   "four outputs are its bytes", "tdoa_locate_last_stats returns what it returns after that call",
                   "The zoom's own map is not judged", "The last row may be short",
                   "a position's fine row is Z r* - H + wa and its fine column is Z c* - H + wb",
                   "competes when its row is >= 0, its column is in 0 .. n_cols_f - 1 and its fine cell index row * n_cols_f + col is < n_cells_f",
                   "score_q of its fine cell exactly as the family defines it", "plus the stack's clock differences where a clock table is set",
                   "sgn(d) * ((2|d| U + 16) div 32) on Q_U", "A pair outside the searched range counts 0",
                   "The words of Q are the same, and so is the overflow bound",
                   "the competing position with the largest score. Among equal maxima the smaller fine cell index wins",
                   "a stack with no location (the zero coarse record) gets the zero tdoa_zoom, zero lags and correlations and a zmap of -1 throughout",
                   "A stack whose window's largest score is 0, or whose window has no competing position, also gets the zero record",
                   "its zmap still holds its scores", "The record, 64 bytes, no padding",
                   "max(|row - row_z|, |col - col_z|) > fine_separation", "are 0 where there is none",
                   "n_best and the box let a caller take the plateau's middle",
                   "zlags and zcorr hold lag_p(cell) in 1/U sample and the signed correlation there, 0 and 0.0 for a pair outside the range",
                   "what tdoa_solve_surface takes", "zmap[s][wa * (2H + 1) + wb] is the position's score, or -1 where it does not compete",
                   "with the fine table equal to the table and Z = 1, the zoom's cell, score_q, lags and correlations are the location's",
                   "lies inside a stack's window, it is the zoom's cell, with the same score, lags and correlations",
                   "The library does not check that", "Its shape (n_cells_f, n_cols_f) is part of a step graph's key; its contents are data",
                   "Scope: the rounds (tdoa_process_locate_multi) and the cell tracks are not zoomed",
                   "The graph's key is the locate's words plus (Z, H, fine_separation, n_cells_f, n_cols_f)",
                   "Z outside 1 .. 64, H outside 0 .. 64, fine_separation < 1, a NULL zoom_host",
                   "TDOA_ERR_STATE: no fine table, or one of another n_stations",
                   "the window maps [n_stacks_total][(2H+1)^2] do not fit", "the same bytes go through the merged sum"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handles_and_bad_arguments_need_no_device(capi):
    lib = capi.load()
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    table = np.zeros((4, 3), dtype=np.int32)
    q = np.zeros((1, 3, 7), dtype=np.int64)
    out = capi._zoom_outputs(1, 3, 4, 1, True, True)
    ptrs = capi._zoom_ptrs(out)
    before = {k: v.tobytes() for k, v in out.items()}
    assert lib.tdoa_locate_set_fine_table(None, table.ctypes.data_as(i32), 4, 2, 3) == 1
    assert lib.tdoa_group_locate_set_fine_table(None, table.ctypes.data_as(i32), 4, 2, 3) == 1
    for Z, H, sep in ((1, 1, 1), (8, 16, 2), (64, 64, 1), (0, 1, 1), (65, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 65, 1), (1, 1, 0), (1, 1, -3)):
        assert lib.tdoa_process_locate_zoom(None, 0, 1, Z, H, sep, *ptrs) == 1
        assert lib.tdoa_group_process_locate_zoom(None, 0, 1, Z, H, sep, *ptrs) == 1
        assert lib.tdoa_debug_locate_zoom_from_q(None, q.ctypes.data_as(i64), 1, 3, 1, 1, Z, H, sep, *ptrs) == 1
    assert lib.tdoa_process_locate_zoom(None, 0, 1, 1, 1, 1, *([None] * 8)) == 1
    assert lib.tdoa_locate_set_fine_table(None, None, 0, 1, 0) == 1
    assert {k: v.tobytes() for k, v in out.items()} == before            # nothing was written
    for Z, H, sep in ((0, 1, 1), (1, 65, 1), (1, 1, 0)):                 # the numpy statement refuses the same ranges
        with pytest.raises(ValueError):
            statement(small_case(3, 4, 1), H, Z=Z, fsep=sep)


# ---- small cases ----------------------------------------------------------------------------------------------------------
COARSE_ROWS, COARSE_COLS, SMALL_Z = 5, 7, 3
FINE_ROWS, FINE_COLS = (COARSE_ROWS - 1) * SMALL_Z + 1, (COARSE_COLS - 1) * SMALL_Z + 1      # 13 x 19
TARGETS = (0, 6, 28, 34, 17)                              # the four corners and cell (2, 3)


def pairs_of(S):
    return [(i, j) for i in range(S) for j in range(i + 1, S)]


def small_case(S, ml, seed, clocked=False, short=False):
    """A coarse 5 x 7 table, Z = 3 and a 13 x 19 fine table with fine (3 r, 3 c) = coarse (r, c) (short: the last fine row holds
    11 cells), and six sets of n_w = 2 windows: set k < 5 has a large word planted at every pair's lag of coarse cell TARGETS[k]
    -- whose delays (plus the set's clocks) are whole samples -- so the sets' best cells are the four corners and (2, 3); set 5
    is all zero.  Every other coarse cell has pair (0, 1) outside the range, the other fine cells have random delays up to
    ml + 2 samples, and the fine cells above and below a target's (where they exist) repeat its delays: a plateau.
    -> dict(q [6][P][2 ml - 1], table, n_cols, fine, n_cols_f, clock or None, ml, n_w, S, Z)"""
    rng = np.random.default_rng(seed)
    pairs = pairs_of(S)
    P, n = len(pairs), 2 * ml - 1
    fine = rng.integers(-8 * (ml + 2), 8 * (ml + 2) + 1, size=(FINE_ROWS, FINE_COLS, S)).astype(np.int64)
    fine[::SMALL_Z, ::SMALL_Z, 1] = fine[::SMALL_Z, ::SMALL_Z, 0] + 16 * (ml + 1) * rng.choice([-1, 1], size=(COARSE_ROWS, COARSE_COLS))
    clock = np.zeros((6, S), dtype=np.int64)
    if clocked:                                           # whole samples; the difference of stations 0 and 1 is the same in every set
        clock = 16 * rng.integers(-1, 2, size=(6, S))
        clock[:, 1] = clock[:, 0] + 16
    q = rng.integers(-2 ** 40, 2 ** 40, size=(6, P, n), dtype=np.int64)
    for k, t in enumerate(TARGETS):
        tau = rng.integers(-1, 2, size=S)                # the target's delays plus set k's clocks, in samples
        tau[0] = 0
        if S > 1:
            tau[1] = k - 2                                # pair (0, 1) tells the targets apart
        r, c = SMALL_Z * (t // COARSE_COLS), SMALL_Z * (t % COARSE_COLS)
        for rr in (r - 1, r, r + 1):
            if 0 <= rr < FINE_ROWS:
                fine[rr, c] = 16 * tau - clock[k]
        for p, (i, j) in enumerate(pairs):
            lag = int(tau[j] - tau[i])
            assert abs(lag) < ml
            q[k, p, lag + ml - 1] = 2 ** 44 * (-1 if (p + k) % 2 else 1)
    q[5] = 0
    table = fine[::SMALL_Z, ::SMALL_Z].reshape(-1, S).astype(np.int32)
    fine = fine.reshape(-1, S).astype(np.int32)
    if short:
        fine = fine[:len(fine) - 8]
    return dict(q=q, table=table, n_cols=COARSE_COLS, fine=fine, n_cols_f=FINE_COLS, clock=clock.astype(np.int32) if clocked else None,
                ml=ml, n_w=2, S=S, Z=SMALL_Z)


def statement(case, H, U=1, sep=1, fsep=1, Z=None, fine=None, n_cols_f=None):
    from tdoa_amd import locate_zoom
    return locate_zoom.zoom_upsampled(case["q"], case["table"], case["n_cols"], case["fine"] if fine is None else fine,
                                      case["n_cols_f"] if n_cols_f is None else n_cols_f, case["ml"], case["Z"] if Z is None else Z, H, U,
                                      sep, fsep, case["n_w"], case["clock"])


def _enumerate_cell(row, clock, fine_q, U, ml):
    """one cell's delays -> (score, pairs inside, lags, words) by the definition, in Python integers"""
    lo, n_u = -(ml - 1) * U, (2 * ml - 2) * U + 1
    score, inside, lags, words = 0, 0, [], []
    for p, (i, j) in enumerate(pairs_of(len(row))):
        d = int(row[j]) - int(row[i]) + (int(clock[j]) - int(clock[i]) if clock is not None else 0)
        a = (2 * abs(d) * U + 16) // 32
        lag = -a if d < 0 else a
        if 0 <= lag - lo < n_u:
            w = fine_q[p][lag - lo]
            score, inside = score + abs(w), inside + 1
            lags.append(lag)
            words.append(w)
        else:
            lags.append(0)
            words.append(None)
    return score, inside, lags, words


def _enumerate_zoom(case, k, H, U, sep, fsep):
    """set k by the definition -> (coarse cell or None, zoom record as a dict or None, zlags, words, zmap)"""
    from tdoa_amd import upsample
    ml, Z = case["ml"], case["Z"]
    fine_q = [upsample.upsample_exact(row, U) for row in case["q"][k]]
    clock = None if case["clock"] is None else case["clock"][k]
    coarse = [_enumerate_cell(row, clock, fine_q, U, ml)[0] for row in case["table"]]
    side = 2 * H + 1
    zmap = [-1] * (side * side)
    if max(coarse) <= 0:
        return None, None, None, None, zmap
    best = coarse.index(max(coarse))
    n_cells_f, n_cols_f = len(case["fine"]), case["n_cols_f"]
    cand = []
    for wa in range(side):
        for wb in range(side):
            row, col = Z * (best // case["n_cols"]) - H + wa, Z * (best % case["n_cols"]) - H + wb
            if row < 0 or not 0 <= col < n_cols_f or row * n_cols_f + col >= n_cells_f:
                continue
            cell = row * n_cols_f + col
            s = _enumerate_cell(case["fine"][cell], clock, fine_q, U, ml)
            zmap[wa * side + wb] = s[0]
            cand.append((s[0], cell, row, col, s))
    if not cand or max(c[0] for c in cand) <= 0:
        return best, None, None, None, zmap
    top = max(c[0] for c in cand)
    tops = [c for c in cand if c[0] == top]
    win = min(tops, key=lambda c: c[1])
    far = [c for c in cand if max(abs(c[2] - win[2]), abs(c[3] - win[3])) > fsep]
    rec = dict(cell=win[1], pairs_in=win[4][1], n_best=len(tops), row_lo=min(c[2] for c in tops), row_hi=max(c[2] for c in tops),
               col_lo=min(c[3] for c in tops), col_hi=max(c[3] for c in tops), score_q=top, runner_cell=0, runner_q=0)
    if far:
        best_far = max(c[0] for c in far)
        rec["runner_q"], rec["runner_cell"] = best_far, min(c[1] for c in far if c[0] == best_far)
    return best, rec, win[4][2], win[4][3], zmap


@pytest.mark.parametrize("U", (1, 4, 16))
@pytest.mark.parametrize("S, ml, clocked, short", [(3, 4, False, False), (4, 9, True, False), (4, 9, False, True), (3, 4, True, True)])
def test_the_statement_against_an_enumeration(S, ml, clocked, short, U):
    from tdoa_amd import stacking
    case = small_case(S, ml, 40 + 7 * S + ml, clocked, short)
    seen_out, seen_plateau, seen_runner = 0, 0, 0
    for H, fsep in ((0, 1), (1, 1), (2, 1), (5, 2)):
        loc, lags, corr, cmap, zoom, zlags, zcorr, zmap = statement(case, H, U, 1, fsep)
        assert zoom.dtype.itemsize == 64 and zmap.shape == (6, (2 * H + 1) ** 2) and zmap.dtype == np.int64
        for k in range(6):
            best, rec, want_lags, words, want_map = _enumerate_zoom(case, k, H, U, 1, fsep)
            assert zmap[k].tolist() == want_map, (H, k)
            if k == 5:
                assert best is None and zoom[k].tobytes() == bytes(64) and loc[k].tobytes() == bytes(48) and (zmap[k] == -1).all()
                continue
            assert best == TARGETS[k] == int(loc[k]["cell"])             # the four corners and (2, 3)
            if rec is None:                                              # the short row's corner with one position: it does not compete
                assert short and k == 3 and H == 0 and zoom[k].tobytes() == bytes(64) and not zlags[k].any() and not zcorr[k].any()
                continue
            for name, value in rec.items():
                assert int(zoom[k][name]) == value, (H, k, name)
            assert zlags[k].tolist() == want_lags
            assert zcorr[k].tolist() == [0.0 if w is None else float(stacking.from_fixed(np.int64(w), case["n_w"])) for w in words]
            assert float(zoom[k]["score"]) == float(stacking.from_fixed(np.int64(rec["score_q"]), case["n_w"]))
            assert float(zoom[k]["runner_up"]) == float(stacking.from_fixed(np.int64(rec["runner_q"]), case["n_w"]))
            seen_out += sum(w is None for w in words) + int((np.asarray(want_map) >= 0).sum() < len(want_map))
            seen_plateau += rec["n_best"] > 1
            seen_runner += rec["runner_q"] > 0
            if H == 0:                                                   # one position: the centre, no runner-up
                assert rec["cell"] == SMALL_Z * (best // 7) * FINE_COLS + SMALL_Z * (best % 7) and rec["n_best"] == 1 and rec["runner_q"] == 0
                assert rec["score_q"] == int(loc[k]["score_q"])          # fine (3 r, 3 c) is coarse (r, c)
            else:
                assert rec["score_q"] >= int(loc[k]["score_q"])
    assert seen_out > 0 and seen_plateau > 0 and seen_runner > 0
    if short:                                                            # the corner (4, 6): its fine cell (12, 18) is past the short row
        _, _, _, _, zoom, _, _, zmap = statement(case, 1, U)
        assert (zmap[3].reshape(3, 3)[1:, 1:] == -1).all() and zmap[3][0] >= 0 and int(zoom[3]["cell"]) // FINE_COLS == 11


def test_windows_without_a_competing_position_or_a_score():
    """a fine table of two rows: the window of target (4, 6) lies below it -- the zero record and a zmap of -1; a fine table whose
    cells all have every pair outside the range: the zero record, and the zmap holds the zeros"""
    case = small_case(3, 9, 77)
    loc, _, _, _, zoom, zlags, zcorr, zmap = statement(case, 2, fine=case["fine"][:2 * FINE_COLS])
    assert int(loc[3]["cell"]) == 34 and zoom[3].tobytes() == bytes(64) and (zmap[3] == -1).all() and not zlags[3].any() and not zcorr[3].any()
    assert int(zoom[0]["score_q"]) > 0 and (zmap[0].reshape(5, 5)[:2] == -1).all() and (zmap[0].reshape(5, 5)[2:4, 2:] >= 0).all() and (zmap[0].reshape(5, 5)[4] == -1).all()
    far = (np.arange(3)[None, :] * 16 * 20 + np.zeros((FINE_ROWS * FINE_COLS, 1))).astype(np.int32)
    loc, _, _, _, zoom, zlags, zcorr, zmap = statement(case, 1, fine=far)
    assert (loc["score_q"][:5] > 0).all() and zoom.tobytes() == bytes(64 * 6) and not zlags.any() and not zcorr.any()
    assert (zmap[0].reshape(3, 3)[1:, 1:] == 0).all() and (zmap[0].reshape(3, 3)[0] == -1).all() and (zmap[5] == -1).all()


@pytest.mark.parametrize("U", (1, 4))
def test_the_two_consequences(U):
    """Z = 1 with the table as the fine table: the location again.  The brute-force best cell of the whole fine table inside the
    window: the zoom's cell"""
    from tdoa_amd import locate, upsample
    case = small_case(4, 9, 91, clocked=True)
    loc, lags, corr, _, zoom, zlags, zcorr, _ = statement(case, 2, U, Z=1, fine=case["table"], n_cols_f=case["n_cols"])
    for name in ("cell", "score_q", "pairs_in", "score"):
        assert zoom[name].tolist() == loc[name].tolist(), name
    assert zlags.tobytes() == lags.tobytes() and zcorr.tobytes() == corr.tobytes()
    t, k, _, ml_u = upsample.scaled_args(case["fine"], case["clock"], 0, case["ml"], U)
    brute = locate.locate_stacks(upsample.upsample(case["q"], U), t, FINE_COLS, ml_u, 1, case["n_w"], k)
    n_inside = 0
    for H in (1, 4, 18):
        loc, _, _, _, zoom, zlags, zcorr, _ = statement(case, H, U)
        for s in range(5):
            r, c = divmod(int(brute[0][s]["cell"]), FINE_COLS)
            r0, c0 = SMALL_Z * (int(loc[s]["cell"]) // 7), SMALL_Z * (int(loc[s]["cell"]) % 7)
            if max(abs(r - r0), abs(c - c0)) > H:
                continue
            n_inside += 1
            assert int(zoom[s]["cell"]) == int(brute[0][s]["cell"]) and int(zoom[s]["score_q"]) == int(brute[0][s]["score_q"])
            assert zlags[s].tobytes() == brute[1][s].tobytes() and zcorr[s].tobytes() == brute[2][s].tobytes()
    assert n_inside >= 10                                                # (H = 18 holds the whole fine table)


# ---- the noisy case -------------------------------------------------------------------------------------------------------
def global_fine_table():
    """the 48 x 64 grid at 1/8 cell: ((48 - 1) 8 + 1) x ((64 - 1) 8 + 1) = 377 x 505 cells -> (table, n_cols_f)"""
    from tdoa_amd import locate
    rows, cols = (GRID["rows"] - 1) * FINE + 1, (GRID["cols"] - 1) * FINE + 1
    g = dict(GRID, dlat=GRID["dlat"] / FINE, dlon=GRID["dlon"] / FINE, rows=rows, cols=cols)
    return locate.grid_table(ST4, sample_rate=FS, **g), cols


def global_position(row, col):
    return GRID["lat0"] + row * GRID["dlat"] / FINE, GRID["lon0"] + col * GRID["dlon"] / FINE


def zoom_counts(zoom_of, brute_of, q_all):
    """the noisy case's figures from any implementation: zoom_of(U) -> ([12] coarse cells, [12] zoom records), brute_of(U) -> [12]
    best cells of the whole fine table -> (distances [12][3] at U = 1, 4, 16, agreements with fine_cell around the same coarse
    cell, agreements with brute force per U, the distances of the plateaus' middles at U = 1)"""
    from tdoa_amd import locate_zoom
    n_cols_f = (GRID["cols"] - 1) * FINE + 1
    d, same_fine, same_brute, mid = np.zeros((12, 3)), 0, [], np.zeros(12)
    for n, U in enumerate((1, 4, 16)):
        (coarse_cells, zoom), brute = zoom_of(U), brute_of(U)
        same_brute.append(int(sum(int(zoom[k]["cell"]) == int(brute[k]) for k in range(12))))
        for k in range(12):
            row, col = locate_zoom.position(zoom[k], n_cols_f)
            c = int(coarse_cells[k])
            d[k, n] = metres(POSITIONS[k], global_position(row, col))
            f = fine_cell(q_all[k], c, U)                                # the host-built 33 x 33 table around the coarse cell
            same_fine += (row - FINE * (c // 64) + ZOOM_H, col - FINE * (c % 64) + ZOOM_H) == divmod(f, FINE_SIDE)
            if U == 1:
                mid[k] = metres(POSITIONS[k], global_position(*locate_zoom.middle(zoom[k])))
    return d, same_fine, same_brute, mid


def test_the_noisy_case_with_one_global_fine_table(oracle):
    """Four stations, the 48 x 64 grid, one window of 8 192 per stack, max_lag 128, the twelve POSITIONS at noise 0.3, a global
    377 x 505 fine table (Z = 8) and H = 16.  Measured with the float64 pipeline: medians 203.6 m at the coarse cell's centre, 125.3
    m for the zoom on whole lags, 36.6 m at x 4 and 34.8 m at x 16 (ratio 0.28); the zoom's position is the host-built fine
    table's in 36 of 36 (position, U) pairs and its cell the brute-force best cell of the whole fine table in 12 of 12 at each U."""
    from tdoa_amd import locate, locate_zoom, upsample
    table = coarse_table()
    fine, n_cols_f = global_fine_table()
    assert fine.shape == (377 * 505, 4) and n_cols_f == 505
    assert (fine.reshape(377, 505, 4)[::FINE, ::FINE].reshape(-1, 4) == table).all()      # word for word
    q_all = np.stack([window_q(oracle, k, 0.3) for k in range(12)])
    out = {U: locate_zoom.zoom_upsampled(q_all, table, 64, fine, n_cols_f, ML, ZOOM_Z, ZOOM_H, U) for U in (1, 4, 16)}
    coarse = out[1][0]["cell"]

    def brute_of(U):
        t, _, _, ml_u = upsample.scaled_args(fine, None, 0, ML, U)
        return [int(locate.locate(upsample.upsample(q_all[k], U), t, n_cols_f, ml_u, 1)[0]["cell"]) for k in range(12)]

    d0 = np.array([metres(POSITIONS[k], cell_position(int(coarse[k]))) for k in range(12)])
    d, same_fine, same_brute, mid = zoom_counts(lambda U: (out[U][0]["cell"], out[U][4]), brute_of, q_all)
    med = np.median(d, axis=0)
    for k in range(12):
        print("position %2d: coarse cell %.0f m; zoom on whole lags %.0f m (plateau of %d cells, its middle %.0f m), x 4 %.0f m, x 16 %.0f m"
              % (k, d0[k], d[k, 0], int(out[1][4][k]["n_best"]), mid[k], d[k, 1], d[k, 2]))
    print("medians at noise 0.3: coarse cell centre %.1f m, zoom on whole lags %.1f m (the plateau boxes' middles %.1f m), x 4 %.1f m, x 16 %.1f m; "
          "ratio %.3f; plateaus of %d .. %d cells at U = 1, %d .. %d at U = 16; zoom = host-built fine table in %d of 36, = brute force in %s of 12"
          % (np.median(d0), med[0], np.median(mid), med[1], med[2], med[2] / med[0], out[1][4]["n_best"].min(), out[1][4]["n_best"].max(),
             out[16][4]["n_best"].min(), out[16][4]["n_best"].max(), same_fine, same_brute))
    assert same_fine == 36
    assert same_brute == [12, 12, 12]
    assert med[2] <= BOUND * med[0]
    assert med[0] < np.median(d0)
