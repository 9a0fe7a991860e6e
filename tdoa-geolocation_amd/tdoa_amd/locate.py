"""The delay-table search of tdoa_process_locate (include/tdoa_mi355x.h, "delay-table search") in int64 numpy: what the GPU
kernels (csrc/stack_locate.hpp) are held to, byte for byte.  Tests use it; the library does not.

A table t [n_cells][n_stations] of propagation delays in units of 1/16 sample gives every candidate ("cell") c one lag per
pair (i, j), i < j in the library's order:

    d = t[c][j] - t[c][i];   lag_p(c) = sgn(d) ((2 |d| + 16) div 32)      the nearest integer to d / 16, halves away from zero
    score_q(c) = sum over the pairs of M_p[lag_p(c)],  M_p[l] = |Q_p[l]|, a lag outside -max_lag < l < max_lag counting 0

The location is the cell with the largest score_q (equal maxima: the smaller cell); the runner-up is the largest score_q
over the cells more than min_separation rows or columns away, row = c div n_cols, col = c mod n_cols.

With station clocks (tdoa_locate_set_clock: one int32 per station of the stack, in the table's unit) the difference a lag is
made of is d = (t[c][j] - t[c][i]) + (clock[j] - clock[i]); everything else is unchanged."""
import numpy as np

from .stacking import from_fixed

LOCATION_DTYPE = np.dtype([("cell", np.int32), ("runner_cell", np.int32), ("pairs_in", np.int32), ("reserved", np.int32),
                           ("score_q", np.int64), ("runner_q", np.int64),
                           ("score", np.float64), ("runner_up", np.float64)])      # tdoa_location

DELAY_UNIT = 16             # TDOA_DELAY_UNIT: table units per sample
MAX_CELLS = 2 ** 22
SPEED_OF_LIGHT = 299792458.0
WGS84_A = 6378137.0
WGS84_F = 1.0 / 298.257223563


def pair_lags(table, clock=None):
    """table [n_cells][S] integers, clock None or [S] integers in the table's unit -> lag_p(c) [n_cells][P] int64, pairs i < j
    in the library's order"""
    t = np.asarray(table, dtype=np.int64)
    if t.ndim != 2 or t.shape[1] < 2:
        raise ValueError("table must be [n_cells][n_stations], n_stations >= 2")
    S = t.shape[1]
    k = np.zeros(S, dtype=np.int64) if clock is None else np.asarray(clock, dtype=np.int64)
    if k.shape != (S,):
        raise ValueError("clock must hold one integer per station")
    out = np.zeros((t.shape[0], S * (S - 1) // 2), dtype=np.int64)
    p = 0
    for i in range(S):
        for j in range(i + 1, S):
            d = (t[:, j] - t[:, i]) + (k[j] - k[i])
            out[:, p] = np.sign(d) * ((2 * np.abs(d) + DELAY_UNIT) // (2 * DELAY_UNIT))
            p += 1
    return out


def locate(q_pairs, table, n_cols, max_lag, min_separation=1, n_w=1, clock=None):
    """One stack: q_pairs [P][2 max_lag - 1] int64 in the library's pair order, table [n_cells][S], clock None or the stack's
    [S] station clocks in the table's unit -> (record LOCATION_DTYPE, lags [P] int32, corr [P] float64, map [n_cells] int64)"""
    ml, sep, n_cols = int(max_lag), int(min_separation), int(n_cols)
    lag = pair_lags(table, clock)
    n_cells, P = lag.shape
    q = np.asarray(q_pairs, dtype=np.int64)
    if q.shape != (P, 2 * ml - 1):
        raise ValueError("q_pairs must be [S (S-1) / 2][2 max_lag - 1]")
    if not 1 <= n_cells <= MAX_CELLS or n_cols < 1:
        raise ValueError("n_cells must be 1 .. 2^22 and n_cols >= 1")
    if sep < 1:
        raise ValueError("min_separation must be >= 1")
    inside = (lag > -ml) & (lag < ml)
    idx = np.where(inside, lag + ml - 1, 0)
    m = np.where(inside, np.abs(q[np.arange(P)[None, :], idx]), 0)
    score = m.sum(axis=1)
    rec = np.zeros((), dtype=LOCATION_DTYPE)
    lags, corr = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.float64)
    best = int(np.argmax(score))                                         # the first of equal maxima: the smaller cell
    if score[best] <= 0:
        return rec, lags, corr, score
    cells = np.arange(n_cells)
    far = np.maximum(np.abs(cells // n_cols - best // n_cols), np.abs(cells % n_cols - best % n_cols)) > sep
    rec["cell"], rec["pairs_in"], rec["score_q"] = best, inside[best].sum(), score[best]
    rec["score"] = from_fixed(score[best], n_w)
    if far.any():
        runner = int(np.argmax(np.where(far, score, -1)))
        rec["runner_cell"], rec["runner_q"], rec["runner_up"] = runner, score[runner], from_fixed(score[runner], n_w)
    lags[:] = np.where(inside[best], lag[best], 0)
    corr[:] = np.where(inside[best], from_fixed(q[np.arange(P), idx[best]], n_w), 0.0)
    return rec, lags, corr, score


def locate_stacks(q, table, n_cols, max_lag, min_separation=1, n_w=1, clock=None):
    """q [n_sets][P][2 max_lag - 1] -> (records [n_sets], lags [n_sets][P], corr [n_sets][P], map [n_sets][n_cells]);
    n_w a number or one per set; clock None or [n_sets][S]"""
    q = np.asarray(q, dtype=np.int64)
    n = np.broadcast_to(np.asarray(n_w), (q.shape[0],))
    if clock is not None and np.shape(clock)[0] != q.shape[0]:
        raise ValueError("clock must hold one row per set")
    out = [locate(q[s], table, n_cols, max_lag, min_separation, int(n[s]), None if clock is None else clock[s])
           for s in range(q.shape[0])]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def ecef(lat, lon, height):
    """WGS-84 latitude / longitude in degrees and height in metres -> [..., 3] metres"""
    phi, lam, h = np.radians(np.asarray(lat, dtype=np.float64)), np.radians(np.asarray(lon, dtype=np.float64)), np.asarray(height, dtype=np.float64)
    e2 = 2 * WGS84_F - WGS84_F * WGS84_F
    nu = WGS84_A / np.sqrt(1 - e2 * np.sin(phi) ** 2)
    return np.stack(np.broadcast_arrays((nu + h) * np.cos(phi) * np.cos(lam), (nu + h) * np.cos(phi) * np.sin(lam),
                                        (nu * (1 - e2) + h) * np.sin(phi)), axis=-1)


def grid_table(stations_lle, lat0, lon0, dlat, dlon, rows, cols, height_m, sample_rate):
    """tdoa_locate_grid_table in float64 numpy: cell r cols + c at (lat0 + r dlat, lon0 + c dlon, height_m) ->
    [rows cols][S] int32, rint(16 sample_rate |ecef(cell) - ecef(station)| / c)"""
    st = np.asarray(stations_lle, dtype=np.float64).reshape(-1, 3)
    rows, cols = int(rows), int(cols)
    if not 1 <= rows * cols <= MAX_CELLS or rows < 1 or cols < 1:
        raise ValueError("rows cols must be 1 .. 2^22")
    r, c = np.divmod(np.arange(rows * cols), cols)
    x = ecef(lat0 + r * float(dlat), lon0 + c * float(dlon), float(height_m))
    s = ecef(st[:, 0], st[:, 1], st[:, 2])
    d = DELAY_UNIT * float(sample_rate) * np.linalg.norm(x[:, None, :] - s[None, :, :], axis=2) / SPEED_OF_LIGHT
    if not np.isfinite(d).all() or d.max() >= 2 ** 31 - 1:
        raise ValueError("a delay does not fit int32")
    return np.rint(d).astype(np.int32)
