"""tdoa_process_sync_drift_locate (include/tdoa_mi355x.h, "free-running clocks to fix in one call") as the three numpy
statements it chains, one after another: sync_drift_fine.sync_lines_fine on every line, line_mix.mix_rows on its clock16 and
fine_rate, and the zoomed cell tracks' statement (locate_track_zoom.track_zoom_stacks, with the setting U_loc > 1
track_zoom_upsampled) under those rows.  No arithmetic of its own.  Tests use it; the library does not."""
import numpy as np

from . import line_mix as _mix
from . import locate_track_zoom as _zoom
from . import sync_drift_fine as _fine

TRACK_KEYS = ("track", "cells", "own", "loc_lags", "loc_corr", "total",
              "ztrack", "zcells", "zown", "zlags", "zcorr", "zmap", "ztotal")      # capi's keys for locate_track_zoom.NAMES


def sync_drift_locate(q, track_len, ref_delay, table, n_cols, fine, n_cols_f, max_lag, Z, H, mix=None, gate=0, max_drift=0, drift_den=1,
                      rounds=0, U=16, fine_rounds=2, centre=None, max_step=0, min_separation=1, fine_step=0, fine_separation=1, n_w=1,
                      U_loc=1):
    """q [n_sets][P][2 max_lag - 1], set t track_len + j position j of line and track t -> sync_lines_fine's twelve outputs,
    "mix_rows" [n_sets][S] int32 and the zoomed tracks' thirteen outputs under TRACK_KEYS; mix [n_sets][6] or None (every set
    its own line at its own position); n_w a number or one per set"""
    q = np.asarray(q, dtype=np.int64)
    L = int(track_len)
    out = _fine.sync_lines_fine(q, L, ref_delay, max_lag, gate, max_drift, drift_den, rounds, U, fine_rounds, centre, n_w)
    rows = _mix.mix_rows(out["clock16"], out["fine_rate"], U, drift_den, _mix.own_mix(len(q) // L, L) if mix is None else mix)
    if len(rows) != len(q):
        raise ValueError("mix must hold one entry per set")
    if int(U_loc) == 1:
        z = _zoom.track_zoom_stacks(q, table, n_cols, fine, n_cols_f, max_lag, L, max_step, Z, H, fine_step, min_separation,
                                    fine_separation, n_w, rows)
    else:
        z = _zoom.track_zoom_upsampled(q, table, n_cols, fine, n_cols_f, max_lag, L, max_step, Z, H, fine_step, U_loc, min_separation,
                                       fine_separation, n_w, rows)
    out["mix_rows"] = rows
    out.update(zip(TRACK_KEYS, z))
    return out
