"""The map statistics of tdoa_locate_set_stats (include/tdoa_mi355x.h, "map statistics") in int64 numpy: what the GPU kernels
(csrc/stack_map_stats.hpp) are held to, byte for byte.  Tests use it; the library does not.

Per judged plane of n_cells words v[c] >= 0 -- a map of the delay-table search, T_0 of a cell track -- with the record's
score_q (the plane's largest word) and cell b:

    n_live        = #{c : v[c] > 0}
    quantile_q[i] = sorted(live words)[(ranks[i] (n_live - 1)) div 65535]
    level_q       = q0 + ((best - q0) foot) div 65536,  q0 = quantile_q[0]              (foot > 0)
    foot_cells    = #{c : v[c] > 0 and v[c] >= level_q}; foot_near of them within min_separation rows and columns of b;
                    row_lo .. row_hi, col_lo .. col_hi their bounding box, row = c div n_cols

A zero record (score_q == 0) gives the all-zero statistics."""
import numpy as np

from .stacking import from_fixed

MAX_RANKS = 8               # TDOA_MAP_STATS_MAX_RANKS
HIST_CHUNK = 16384          # kMapChunk: the cells of a plane one workgroup of k_map_hist takes
MAP_STATS_DTYPE = np.dtype([("quantile_q", np.int64, (MAX_RANKS,)), ("quantile", np.float64, (MAX_RANKS,)),
                            ("level_q", np.int64), ("n_live", np.int32), ("foot_cells", np.int32), ("foot_near", np.int32),
                            ("row_lo", np.int32), ("row_hi", np.int32), ("col_lo", np.int32), ("col_hi", np.int32),
                            ("reserved", np.int32)])      # tdoa_map_stats


def level(q0, best, foot):
    """q0 + ((best - q0) foot) div 65536 as the library computes it: no product of more than 64 bits"""
    d = int(best) - int(q0)
    return int(q0) + (d >> 16) * int(foot) + (((d & 0xffff) * int(foot)) >> 16)


def plane_stats(v, n_cols, ranks, foot=0, score_q=None, cell=None, min_separation=1, n_w=1):
    """One plane v [n_cells] int64 -> MAP_STATS_DTYPE.  score_q and cell are the record's (None: the plane's largest word and
    the first cell that holds it); n_w is what the record's score was scaled with"""
    v = np.asarray(v, dtype=np.int64).reshape(-1)
    ranks = [int(r) for r in np.reshape(ranks, -1)]
    if not 1 <= len(ranks) <= MAX_RANKS or min(ranks) < 0 or max(ranks) > 65535:
        raise ValueError("1 .. 8 ranks, each 0 .. 65535")
    if not 0 <= int(foot) <= 65535:
        raise ValueError("foot is 0 .. 65535")
    out = np.zeros((), dtype=MAP_STATS_DTYPE)
    best = int(v.max()) if score_q is None else int(score_q)
    if best <= 0:
        return out
    b = int(np.argmax(v)) if cell is None else int(cell)
    live = np.sort(v[v > 0])
    out["n_live"] = live.size
    for i, r in enumerate(ranks):
        out["quantile_q"][i] = live[(r * (live.size - 1)) // 65535]
        out["quantile"][i] = from_fixed(out["quantile_q"][i], n_w)
    if int(foot) > 0:
        lv = level(out["quantile_q"][0], best, foot)
        c = np.nonzero((v > 0) & (v >= lv))[0]
        row, col = c // int(n_cols), c % int(n_cols)
        out["level_q"], out["foot_cells"] = lv, c.size
        out["foot_near"] = np.count_nonzero((np.abs(row - b // int(n_cols)) <= int(min_separation)) &
                                            (np.abs(col - b % int(n_cols)) <= int(min_separation)))
        out["row_lo"], out["row_hi"], out["col_lo"], out["col_hi"] = row.min(), row.max(), col.min(), col.max()
    return out


def stats(planes, records, n_cols, ranks, foot=0, min_separation=1, n_w=1):
    """planes [...][n_cells] int64 judged by records [...] (LOCATION_DTYPE or CELL_TRACK_DTYPE: score_q and cell are read) ->
    [...] MAP_STATS_DTYPE; n_w a number or one per plane"""
    planes = np.asarray(planes, dtype=np.int64)
    rec = np.asarray(records)
    if planes.shape[:-1] != rec.shape:
        raise ValueError("one record per plane")
    n = np.broadcast_to(np.asarray(n_w), rec.shape).reshape(-1)
    flat, r = planes.reshape(-1, planes.shape[-1]), rec.reshape(-1)
    out = np.zeros(r.size, dtype=MAP_STATS_DTYPE)
    for i in range(r.size):
        out[i] = plane_stats(flat[i], n_cols, ranks, foot, r["score_q"][i], r["cell"][i], min_separation, n[i])
    return out.reshape(rec.shape)


def contrast(stats, floor=0, ref=1, best=None):
    """(best - q[floor]) / (q[ref] - q[floor]) per plane: with ranks (32768, 64880) the peak's height over the median in units
    of the 99 % quantile's.  best: the records' score_q [...]; None: the largest quantile word of the plane, which is score_q
    when rank 65535 is among the ranks.  0.0 where the denominator is not positive (a zero record, equal quantiles)."""
    s = np.asarray(stats)
    q = s["quantile_q"].astype(np.float64)
    lo, hi = q[..., int(floor)], q[..., int(ref)]
    top = q.max(axis=-1) if best is None else np.asarray(best, dtype=np.float64)
    den = hi - lo
    return np.where(den > 0, (top - lo) / np.where(den > 0, den, 1.0), 0.0)
