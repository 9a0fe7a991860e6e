"""The zoom locate of tdoa_process_locate_zoom (include/tdoa_mi355x.h, "zoom locate") in int64 numpy: what the GPU kernels
(csrc/stack_locate_zoom.hpp) are held to, byte for byte.  Tests use it; the library does not.

The coarse stage is locate.locate on the table.  A stack with the location cell* = (r*, c*) = divmod(cell*, n_cols) is then
searched again on a second table, fine [n_cells_f][S] in n_cols_f columns, which covers the area at Z cells per cell: over the
window positions (wa, wb), 0 <= wa, wb <= 2 H,

    row = Z r* - H + wa,  col = Z c* - H + wb;   the position competes when row >= 0, 0 <= col < n_cols_f and
    row n_cols_f + col < n_cells_f;   its score is locate's score_q of that fine cell (the same lag rule, clocks and range)

The zoom's cell is the competing position with the largest score, equal maxima: the smaller fine cell.  n_best counts the
competing positions with exactly that score, the box holds their smallest and largest fine row and column, and the runner-up
is the best competing position more than fine_separation fine rows or columns away.  No location, no competing position or a
largest score of 0: the zero record.  zmap holds the positions' scores, -1 where a position does not compete (everywhere for a
stack without a location).

With the setting U > 1 the statement is this function on upsample.upsample(q, U), U table, U fine, U clock and
max_lag' = (max_lag - 1) U + 1 (zoom_upsampled)."""
import numpy as np

from . import locate as _locate
from . import upsample as _upsample
from .stacking import from_fixed

ZOOM_DTYPE = np.dtype([("cell", np.int32), ("runner_cell", np.int32), ("pairs_in", np.int32), ("n_best", np.int32),
                       ("row_lo", np.int32), ("row_hi", np.int32), ("col_lo", np.int32), ("col_hi", np.int32),
                       ("score_q", np.int64), ("runner_q", np.int64),
                       ("score", np.float64), ("runner_up", np.float64)])        # tdoa_zoom
MAX_Z = 64
MAX_H = 64


def position(record, n_cols_f):
    """a zoom record -> (fine row, fine column) of its cell"""
    return divmod(int(record["cell"]), int(n_cols_f))


def middle(record):
    """a zoom record -> (fine row, fine column) of the middle of the box of its equal best positions, halves as they come"""
    return (int(record["row_lo"]) + int(record["row_hi"])) / 2.0, (int(record["col_lo"]) + int(record["col_hi"])) / 2.0


def window(cell, n_cols, n_cells_f, n_cols_f, Z, H):
    """the window of the coarse cell -> (rows [(2H+1)^2], cols, fine cells, competes) in the order of zmap"""
    side = 2 * int(H) + 1
    wa, wb = np.divmod(np.arange(side * side, dtype=np.int64), side)
    rows = int(Z) * (int(cell) // int(n_cols)) - int(H) + wa
    cols = int(Z) * (int(cell) % int(n_cols)) - int(H) + wb
    cells = rows * int(n_cols_f) + cols
    competes = (rows >= 0) & (cols >= 0) & (cols < int(n_cols_f)) & (cells < int(n_cells_f))
    return rows, cols, cells, competes


def zoom(q_pairs, table, n_cols, fine, n_cols_f, max_lag, Z, H, min_separation=1, fine_separation=1, n_w=1, clock=None):
    """One stack -> (locate.locate's four outputs, record ZOOM_DTYPE, zlags [P] int32, zcorr [P] float64, zmap [(2H+1)^2] int64)"""
    ml, Z, H, fsep, n_cols_f = int(max_lag), int(Z), int(H), int(fine_separation), int(n_cols_f)
    if not 1 <= Z <= MAX_Z or not 0 <= H <= MAX_H or fsep < 1:
        raise ValueError("Z must be 1 .. 64, H 0 .. 64 and fine_separation >= 1")
    fine = np.asarray(fine, dtype=np.int64)
    if fine.ndim != 2 or not 1 <= len(fine) <= _locate.MAX_CELLS or n_cols_f < 1:
        raise ValueError("fine must be [n_cells_f][n_stations], 1 .. 2^22 cells, n_cols_f >= 1")
    coarse = _locate.locate(q_pairs, table, n_cols, ml, min_separation, n_w, clock)
    q = np.asarray(q_pairs, dtype=np.int64)
    P = q.shape[0]
    side = 2 * H + 1
    rec = np.zeros((), dtype=ZOOM_DTYPE)
    zlags, zcorr = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.float64)
    zmap = np.full(side * side, -1, dtype=np.int64)
    if int(coarse[0]["score_q"]) == 0:                                   # no location
        return coarse + (rec, zlags, zcorr, zmap)
    rows, cols, cells, competes = window(coarse[0]["cell"], n_cols, len(fine), n_cols_f, Z, H)
    if not competes.any():
        return coarse + (rec, zlags, zcorr, zmap)
    at = np.flatnonzero(competes)
    lag = _locate.pair_lags(fine[cells[at]], clock)
    inside = (lag > -ml) & (lag < ml)
    idx = np.where(inside, lag + ml - 1, 0)
    score = np.where(inside, np.abs(q[np.arange(P)[None, :], idx]), 0).sum(axis=1)
    zmap[at] = score
    b = int(np.argmax(score))                                            # the first of equal maxima: the smaller fine cell
    if score[b] <= 0:
        return coarse + (rec, zlags, zcorr, zmap)
    top = score == score[b]
    r, c = rows[at], cols[at]
    rec["cell"], rec["pairs_in"], rec["n_best"], rec["score_q"] = cells[at[b]], inside[b].sum(), top.sum(), score[b]
    rec["row_lo"], rec["row_hi"], rec["col_lo"], rec["col_hi"] = r[top].min(), r[top].max(), c[top].min(), c[top].max()
    rec["score"] = from_fixed(score[b], n_w)
    far = np.maximum(np.abs(r - r[b]), np.abs(c - c[b])) > fsep
    if far.any():
        u = int(np.argmax(np.where(far, score, -1)))
        rec["runner_cell"], rec["runner_q"], rec["runner_up"] = cells[at[u]], score[u], from_fixed(score[u], n_w)
    zlags[:] = np.where(inside[b], lag[b], 0)
    zcorr[:] = np.where(inside[b], from_fixed(q[np.arange(P), idx[b]], n_w), 0.0)
    return coarse + (rec, zlags, zcorr, zmap)


NAMES = ("loc", "lags", "corr", "map", "zoom", "zlags", "zcorr", "zmap")     # the outputs' order, and capi's dict keys


def zoom_stacks(q, table, n_cols, fine, n_cols_f, max_lag, Z, H, min_separation=1, fine_separation=1, n_w=1, clock=None):
    """q [n_sets][P][2 max_lag - 1] -> the eight outputs with a leading axis of sets; n_w a number or one per set; clock None or
    [n_sets][S]"""
    q = np.asarray(q, dtype=np.int64)
    n = np.broadcast_to(np.asarray(n_w), (q.shape[0],))
    if clock is not None and np.shape(clock)[0] != q.shape[0]:
        raise ValueError("clock must hold one row per set")
    out = [zoom(q[s], table, n_cols, fine, n_cols_f, max_lag, Z, H, min_separation, fine_separation, int(n[s]),
                None if clock is None else clock[s]) for s in range(q.shape[0])]
    return tuple(np.stack([o[k] for o in out]) for k in range(8))


def zoom_upsampled(q, table, n_cols, fine, n_cols_f, max_lag, Z, H, U, min_separation=1, fine_separation=1, n_w=1, clock=None):
    """zoom_stacks with the setting U: on upsample(q, U), U table, U fine, U clock, max_lag' = (max_lag - 1) U + 1"""
    t, k, _, ml_u = _upsample.scaled_args(table, clock, 0, max_lag, U)
    f = np.asarray(fine, dtype=np.int64) * int(U)
    return zoom_stacks(_upsample.upsample(q, U), t, n_cols, f, n_cols_f, ml_u, Z, H, min_separation, fine_separation, n_w, k)
