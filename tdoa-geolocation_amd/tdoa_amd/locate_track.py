"""The cell tracks of tdoa_process_locate_track (include/tdoa_mi355x.h, "cell tracks") in int64 numpy: what the GPU kernels
(csrc/stack_cell_track.hpp) are held to, byte for byte.  Tests use it; the library does not.

The delay-table search (tdoa_amd.locate) gives every stack of a block a map s_j[c] = score_q(stack j, c) over the table's
cells, row = c div n_cols, col = c mod n_cols.  A track is one cell per stack, consecutive cells at most J rows and columns
apart, with the largest sum of the maps along it:

    T_{L-1}[c] = s_{L-1}[c]
    T_j[c]     = s_j[c] + max over |dr| <= J, |dc| <= J, (row + dr, col + dc) a cell, of T_{j+1}[that cell]
    D_j[c]     = the (dr, dc) of that maximum, the first in the order (rank(dr), rank(dc)), rank(x) = 2 |x| - (x > 0)

L_0 is the cell with the largest T_0 (equal maxima: the smaller cell), L_{j+1} = L_j + D_j[L_j]; the runner-up is the largest
T_0 over the cells more than min_separation rows or columns from L_0."""
import numpy as np

from .locate import locate_stacks, pair_lags
from .stacking import from_fixed
from .sync import candidates

CELL_TRACK_DTYPE = np.dtype([("cell", np.int32), ("runner_cell", np.int32), ("positions", np.int32), ("steps", np.int32),
                             ("score_q", np.int64), ("runner_q", np.int64),
                             ("score", np.float64), ("runner_up", np.float64)])      # tdoa_cell_track

MAX_STEP = 16
MAX_LEN = 4096


def backward(maps, n_cols, J):
    """maps [L][n_cells] integers -> (T [L][n_cells] int64, D [L][n_cells][2] int8: (dr, dc), zeros at position L - 1)"""
    s = np.asarray(maps, dtype=np.int64)
    n_cols, J = int(n_cols), int(J)
    if s.ndim != 2 or s.shape[0] < 1 or s.shape[1] < 1 or n_cols < 1:
        raise ValueError("maps must be [L][n_cells], n_cols >= 1")
    if not 0 <= J <= MAX_STEP:
        raise ValueError("max_step must be 0 .. 16")
    L, n_cells = s.shape
    row, col = np.divmod(np.arange(n_cells), n_cols)
    T = np.zeros_like(s)
    D = np.zeros((L, n_cells, 2), dtype=np.int8)
    T[L - 1] = s[L - 1]
    for j in range(L - 2, -1, -1):
        best = T[j + 1].copy()                                           # (0, 0): always a cell
        for dr in candidates(J):
            for dc in candidates(J):
                r, c = row + dr, col + dc
                cell = r * n_cols + c
                exists = (r >= 0) & (c >= 0) & (c < n_cols) & (cell < n_cells)
                value = T[j + 1][np.where(exists, cell, 0)]
                better = exists & (value > best)                         # strict: the first of equal maxima stays
                best = np.where(better, value, best)
                D[j, better] = (dr, dc)
        T[j] = s[j] + best
    return T, D


def track(maps, n_cols, J, sep=1, n_w=1):
    """One track: maps [L][n_cells], n_w the windows of the whole track -> (record CELL_TRACK_DTYPE, cells [L] int32,
    own [L] int64, total [n_cells] int64 = T_0)"""
    s = np.asarray(maps, dtype=np.int64)
    n_cols, sep = int(n_cols), int(sep)
    if sep < 1:
        raise ValueError("min_separation must be >= 1")
    T, D = backward(s, n_cols, J)
    L, n_cells = s.shape
    rec = np.zeros((), dtype=CELL_TRACK_DTYPE)
    cells, own = np.zeros(L, dtype=np.int32), np.zeros(L, dtype=np.int64)
    best = int(np.argmax(T[0]))                                          # the first of equal maxima: the smaller cell
    if T[0][best] <= 0:
        return rec, cells, own, T[0]
    c = best
    for j in range(L):
        cells[j], own[j] = c, s[j][c]
        if j + 1 < L:
            c += int(D[j, c, 0]) * n_cols + int(D[j, c, 1])
    idx = np.arange(n_cells)
    far = np.maximum(np.abs(idx // n_cols - best // n_cols), np.abs(idx % n_cols - best % n_cols)) > sep
    rec["cell"], rec["positions"], rec["steps"], rec["score_q"] = best, L, int((cells[1:] != cells[:-1]).sum()), T[0][best]
    rec["score"] = from_fixed(T[0][best], n_w)
    if far.any():
        runner = int(np.argmax(np.where(far, T[0], -1)))
        rec["runner_cell"], rec["runner_q"], rec["runner_up"] = runner, T[0][runner], from_fixed(T[0][runner], n_w)
    return rec, cells, own, T[0]


def cell_lags(q_pairs, table, cell, max_lag, n_w=1, clock=None):
    """lag_p(cell) [P] int32 and the signed C there [P] float64 on one stack, 0 for a pair outside the range: what the
    delay-table search reports for its best cell, for any cell"""
    ml = int(max_lag)
    q = np.asarray(q_pairs, dtype=np.int64)
    lag = pair_lags(np.asarray(table)[int(cell):int(cell) + 1], clock)[0]
    inside = (lag > -ml) & (lag < ml)
    idx = np.where(inside, lag + ml - 1, 0)
    return (np.where(inside, lag, 0).astype(np.int32),
            np.where(inside, from_fixed(q[np.arange(len(lag)), idx], n_w), 0.0))


def track_stacks(q, table, n_cols, max_lag, track_len, J, sep=1, n_w=1, clock=None):
    """q [n_sets][P][2 max_lag - 1], set t track_len + j position j of track t; n_w a number or one per set; clock None or
    [n_sets][S] -> (records [n_tracks], cells [n_tracks][L] int32, own [n_tracks][L] int64, lags [n_sets][P] int32,
    corr [n_sets][P] float64, total [n_tracks][n_cells] int64)"""
    q = np.asarray(q, dtype=np.int64)
    L = int(track_len)
    if not 1 <= L <= MAX_LEN or q.shape[0] % L:
        raise ValueError("track_len must be 1 .. 4096 and divide the number of sets")
    n = np.broadcast_to(np.asarray(n_w), (q.shape[0],))
    maps = locate_stacks(q, table, n_cols, max_lag, sep, n, clock)[3]
    recs, cells, own, total = [], [], [], []
    lags, corr = np.zeros(q.shape[:2], dtype=np.int32), np.zeros(q.shape[:2], dtype=np.float64)
    for t in range(q.shape[0] // L):
        sets = range(t * L, (t + 1) * L)
        rec, c, o, tot = track(maps[t * L:(t + 1) * L], n_cols, J, sep, int(n[t * L:(t + 1) * L].sum()))
        if rec["score_q"] > 0:
            for j, sid in enumerate(sets):
                lags[sid], corr[sid] = cell_lags(q[sid], table, c[j], max_lag, int(n[sid]), None if clock is None else clock[sid])
        recs.append(rec)
        cells.append(c)
        own.append(o)
        total.append(tot)
    return np.stack(recs), np.stack(cells), np.stack(own), lags, corr, np.stack(total)
