"""tdoa_process_sync_locate (include/tdoa_mi355x.h, "clocks to fix in one call") as the three numpy statements it chains, one
after another: sync_fine.sync_fine_stacks on every stack, clock_mix.mix_rows on its clock16, and the zoom locate's statement
(locate_zoom.zoom_stacks, with the setting U_loc > 1 zoom_upsampled) under those rows.  No arithmetic of its own.  Tests use
it; the library does not."""
import numpy as np

from . import clock_mix as _mix
from . import locate_zoom as _zoom
from . import sync_fine as _fine

ZOOM_KEYS = ("loc", "loc_lags", "loc_corr", "map", "zoom", "zlags", "zcorr", "zmap")     # capi's keys for locate_zoom.NAMES


def sync_locate(q, ref_delay, table, n_cols, fine, n_cols_f, max_lag, Z, H, mix=None, gate=0, rounds=0, U=16, fine_rounds=2, centre=None,
                min_separation=1, fine_separation=1, n_w=1, U_loc=1):
    """q [n_sets][P][2 max_lag - 1] -> sync_fine_stacks' eight outputs, "rows" [n_sets][S] int32 and the zoom's eight outputs
    under ZOOM_KEYS; mix [n_sets][4] or None (every set its own clock); n_w a number or one per set"""
    q = np.asarray(q, dtype=np.int64)
    out = _fine.sync_fine_stacks(q, ref_delay, max_lag, gate, rounds, U, fine_rounds, centre, n_w)
    rows = _mix.mix_rows(out["clock16"], _mix.own_mix(len(q)) if mix is None else mix)
    if len(rows) != len(q):
        raise ValueError("mix must hold one entry per set")
    if int(U_loc) == 1:
        z = _zoom.zoom_stacks(q, table, n_cols, fine, n_cols_f, max_lag, Z, H, min_separation, fine_separation, n_w, rows)
    else:
        z = _zoom.zoom_upsampled(q, table, n_cols, fine, n_cols_f, max_lag, Z, H, U_loc, min_separation, fine_separation, n_w, rows)
    out["rows"] = rows
    out.update(zip(ZOOM_KEYS, z))
    return out
