"""The zoomed cell tracks of tdoa_process_locate_track_zoom (include/tdoa_mi355x.h, "zoomed cell tracks") in int64 numpy:
what the GPU kernels (csrc/stack_locate_track_zoom.hpp) are held to, byte for byte.  Tests use it; the library does not.

The coarse stage is locate_track.track_stacks on the table.  Position j of a track with the coarse cells C_0 .. C_{L-1} then
has the zoom's window (locate_zoom.window) around C_j on the fine table, and w_j[pos] is the family's score_q of that fine
cell under the stack's own clock row, -1 where the position does not compete.  The recurrence runs in fine coordinates, from
the last position back, with Jf = fine_step:

    F_{L-1}[pos] = w_{L-1}[pos]
    F_j[pos]     = w_j[pos] + max over |dr|, |dc| <= Jf of F_{j+1}[pos'], pos' the position of window j + 1 at the fine
                   (row + dr, col + dc), inside that window and with F_{j+1}[pos'] >= 0; -1 where w_j[pos] = -1 or there is
                   no such pos'
    E_j[pos]     = the (dr, dc) of that maximum, the first in the order (rank(dr), rank(dc)), rank(x) = 2 |x| - (x > 0)

f_0 is the position with the largest F_0 (equal maxima: the smaller fine cell), f_{j+1} = f_j + E_j[f_j]; the runner-up is the
largest F_0 >= 0 over the positions more than fine_separation fine rows or columns from f_0.

With the setting U > 1 the statement is this function on upsample.upsample(q, U), U table, U fine, U clock and
max_lag' = (max_lag - 1) U + 1 (track_zoom_upsampled)."""
import numpy as np

from . import locate as _locate
from . import locate_track as _track
from . import locate_zoom as _zoom
from . import upsample as _upsample
from .stacking import from_fixed
from .sync import candidates

MAX_FINE_STEP = 16


def window_scores(q_pairs, fine, cell, n_cols, n_cols_f, max_lag, Z, H, clock=None):
    """One stack and the coarse cell its window lies around -> (w [(2H+1)^2] int64: score_q of the positions' fine cells, -1
    where a position does not compete; rows, cols, cells of the positions)"""
    ml = int(max_lag)
    q = np.asarray(q_pairs, dtype=np.int64)
    P = q.shape[0]
    rows, cols, cells, competes = _zoom.window(cell, n_cols, len(fine), n_cols_f, Z, H)
    w = np.full(len(rows), -1, dtype=np.int64)
    at = np.flatnonzero(competes)
    if len(at):
        lag = _locate.pair_lags(fine[cells[at]], clock)
        inside = (lag > -ml) & (lag < ml)
        idx = np.where(inside, lag + ml - 1, 0)
        w[at] = np.where(inside, np.abs(q[np.arange(P)[None, :], idx]), 0).sum(axis=1)
    return w, rows, cols, cells


def backward(w, origin, H, Jf):
    """w [L][(2H+1)^2]: the windows' scores; origin [L][2]: the fine (row, column) of every window's position (0, 0) ->
    (F [L][(2H+1)^2] int64, E [L][(2H+1)^2][2] int8: (dr, dc), zeros at position L - 1 and where there is no continuation)"""
    w = np.asarray(w, dtype=np.int64)
    origin = np.asarray(origin, dtype=np.int64)
    H, Jf = int(H), int(Jf)
    if not 0 <= Jf <= MAX_FINE_STEP:
        raise ValueError("fine_step must be 0 .. 16")
    L, side = w.shape[0], 2 * H + 1
    wa, wb = np.divmod(np.arange(side * side, dtype=np.int64), side)
    F = np.zeros_like(w)
    E = np.zeros((L, side * side, 2), dtype=np.int8)
    F[L - 1] = w[L - 1]
    for j in range(L - 2, -1, -1):
        off = origin[j + 1] - origin[j]
        m = np.full(side * side, -1, dtype=np.int64)
        for dr in candidates(Jf):
            for dc in candidates(Jf):
                a, b = wa + dr - off[0], wb + dc - off[1]
                inside = (a >= 0) & (a < side) & (b >= 0) & (b < side)
                value = np.where(inside, F[j + 1][np.where(inside, a * side + b, 0)], -1)
                better = value > m                                       # strict: the first of equal maxima stays; -1 never counts
                m = np.where(better, value, m)
                E[j, better] = (dr, dc)
        F[j] = np.where((w[j] >= 0) & (m >= 0), w[j] + m, -1)
    return F, E


def track_zoom(q, fine, n_cols, n_cols_f, max_lag, coarse_cells, Z, H, Jf, fine_separation=1, n_w=1, clock=None):
    """One track that has a coarse record: q [L][P][2 max_lag - 1], coarse_cells [L], n_w [L] or a number, clock None or [L][S]
    -> (record CELL_TRACK_DTYPE, zcells [L] int32, zown [L] int64, zlags [L][P] int32, zcorr [L][P] float64,
    zmap [L][(2H+1)^2] int64, ztotal [(2H+1)^2] int64)"""
    q = np.asarray(q, dtype=np.int64)
    L, P = q.shape[:2]
    n = np.broadcast_to(np.asarray(n_w), (L,))
    side = 2 * int(H) + 1
    w, cells, origin = [], [], []
    for j in range(L):
        s, rows, cols, c = window_scores(q[j], fine, coarse_cells[j], n_cols, n_cols_f, max_lag, Z, H, None if clock is None else clock[j])
        w.append(s)
        cells.append(c)
        origin.append((rows[0], cols[0]))
    w, origin = np.stack(w), np.asarray(origin, dtype=np.int64)
    F, E = backward(w, origin, H, Jf)
    rec = np.zeros((), dtype=_track.CELL_TRACK_DTYPE)
    zcells, zown = np.zeros(L, dtype=np.int32), np.zeros(L, dtype=np.int64)
    zlags, zcorr = np.zeros((L, P), dtype=np.int32), np.zeros((L, P), dtype=np.float64)
    best = int(np.argmax(F[0]))                                          # the first of equal maxima: the smaller fine cell
    if F[0][best] <= 0:
        return rec, zcells, zown, zlags, zcorr, w, F[0]
    pos = best
    for j in range(L):
        zcells[j], zown[j] = cells[j][pos], w[j][pos]
        zlags[j], zcorr[j] = _track.cell_lags(q[j], fine, zcells[j], max_lag, int(n[j]), None if clock is None else clock[j])
        if j + 1 < L:
            off = origin[j + 1] - origin[j]
            a, b = pos // side + int(E[j, pos, 0]) - off[0], pos % side + int(E[j, pos, 1]) - off[1]
            pos = int(a * side + b)
    n_all = int(n.sum())
    rows, cols = origin[0][0] + np.arange(side * side) // side, origin[0][1] + np.arange(side * side) % side
    rec["cell"], rec["positions"], rec["steps"], rec["score_q"] = zcells[0], L, int((zcells[1:] != zcells[:-1]).sum()), F[0][best]
    rec["score"] = from_fixed(F[0][best], n_all)
    far = (np.maximum(np.abs(rows - rows[best]), np.abs(cols - cols[best])) > int(fine_separation)) & (F[0] >= 0)
    if far.any():
        u = int(np.argmax(np.where(far, F[0], -1)))
        rec["runner_cell"], rec["runner_q"], rec["runner_up"] = cells[0][u], F[0][u], from_fixed(F[0][u], n_all)
    return rec, zcells, zown, zlags, zcorr, w, F[0]


NAMES = ("track", "cells", "own", "lags", "corr", "total",
         "ztrack", "zcells", "zown", "zlags", "zcorr", "zmap", "ztotal")      # the outputs' order, and capi's dict keys


def track_zoom_stacks(q, table, n_cols, fine, n_cols_f, max_lag, track_len, J, Z, H, Jf, min_separation=1, fine_separation=1, n_w=1,
                      clock=None):
    """q [n_sets][P][2 max_lag - 1], set t track_len + j position j of track t; n_w a number or one per set; clock None or
    [n_sets][S] -> locate_track.track_stacks' six outputs, then ztrack [n_tracks], zcells [n_tracks][L] int32, zown
    [n_tracks][L] int64, zlags [n_sets][P] int32, zcorr [n_sets][P] float64, zmap [n_sets][(2H+1)^2] int64, ztotal
    [n_tracks][(2H+1)^2] int64"""
    Z, H, Jf, fsep, n_cols_f = int(Z), int(H), int(Jf), int(fine_separation), int(n_cols_f)
    if not 1 <= Z <= _zoom.MAX_Z or not 0 <= H <= _zoom.MAX_H or fsep < 1 or not 0 <= Jf <= MAX_FINE_STEP:
        raise ValueError("Z must be 1 .. 64, H 0 .. 64, fine_step 0 .. 16 and fine_separation >= 1")
    fine = np.asarray(fine, dtype=np.int64)
    if fine.ndim != 2 or not 1 <= len(fine) <= _locate.MAX_CELLS or n_cols_f < 1:
        raise ValueError("fine must be [n_cells_f][n_stations], 1 .. 2^22 cells, n_cols_f >= 1")
    q = np.asarray(q, dtype=np.int64)
    L, P, n_pos = int(track_len), q.shape[1], (2 * H + 1) ** 2
    coarse = _track.track_stacks(q, table, n_cols, max_lag, L, J, min_separation, n_w, clock)
    n = np.broadcast_to(np.asarray(n_w), (q.shape[0],))
    n_tracks = q.shape[0] // L
    ztrack = np.zeros(n_tracks, dtype=_track.CELL_TRACK_DTYPE)
    zcells, zown = np.zeros((n_tracks, L), dtype=np.int32), np.zeros((n_tracks, L), dtype=np.int64)
    zlags, zcorr = np.zeros((q.shape[0], P), dtype=np.int32), np.zeros((q.shape[0], P), dtype=np.float64)
    zmap, ztotal = np.full((q.shape[0], n_pos), -1, dtype=np.int64), np.full((n_tracks, n_pos), -1, dtype=np.int64)
    for t in range(n_tracks):
        if int(coarse[0][t]["score_q"]) == 0:                            # no coarse track
            continue
        s = slice(t * L, (t + 1) * L)
        ztrack[t], zcells[t], zown[t], zlags[s], zcorr[s], zmap[s], ztotal[t] = track_zoom(
            q[s], fine, n_cols, n_cols_f, max_lag, coarse[1][t], Z, H, Jf, fsep, n[s], None if clock is None else np.asarray(clock)[s])
    return coarse + (ztrack, zcells, zown, zlags, zcorr, zmap, ztotal)


def track_zoom_upsampled(q, table, n_cols, fine, n_cols_f, max_lag, track_len, J, Z, H, Jf, U, min_separation=1, fine_separation=1,
                         n_w=1, clock=None):
    """track_zoom_stacks with the setting U: on upsample(q, U), U table, U fine, U clock, max_lag' = (max_lag - 1) U + 1"""
    t, k, _, ml_u = _upsample.scaled_args(table, clock, 0, max_lag, U)
    f = np.asarray(fine, dtype=np.int64) * int(U)
    return track_zoom_stacks(_upsample.upsample(q, U), t, n_cols, f, n_cols_f, ml_u, track_len, J, Z, H, Jf, min_separation,
                             fine_separation, n_w, k)
