"""The zoomed rounds of tdoa_process_locate_multi_zoom (include/tdoa_mi355x.h, "zoomed rounds") in int64 numpy: what the GPU
kernels (csrc/stack_locate_multi_zoom.hpp) are held to, byte for byte.  Tests use it; the library does not.

Per stack, rounds r = 0 .. K - 1 of locate_multi.locate_multi, its E_p(r) and M_p^r unchanged: the centres stay the coarse
cells' lags.  Behind round r, locate_zoom.zoom's window of (2 H + 1)^2 fine cells around Z x that round's coarse cell is scored
on M^r, the words round r's coarse scores ran on:

    zscore_q^r(f) = sum over the pairs of M_p^r[lag_p(f)]     lag_p(f) from the fine table, under the zoom's competing rule

Round r's zoom record is the zoom's on those scores; pairs_in counts the pairs inside the range and not excluded at the fine
cell, `reserved` (zpairs[..][1]) the pairs inside the range but excluded there.  An excluded pair reports its lag and 0.0.  A
round with the zero coarse record, a window without a competing position or a largest masked score of 0: the zero record, zero
counts, lags and correlations.  zmap holds a window's scores whenever there was a coarse cell, else -1 throughout.

With the setting U > 1 the statement is this function on upsample.scaled_args' arguments (which scale the guard too) and U fine
(multi_zoom_upsampled)."""
import numpy as np

from . import locate_zoom as _zoom
from . import upsample as _upsample
from .locate import pair_lags
from .locate_multi import MAX_EMITTERS

NAMES = ("loc", "lags", "corr", "map", "zoom", "zpairs", "zlags", "zcorr", "zmap")     # the outputs' order, and capi's dict keys


def multi_zoom(q_pairs, table, n_cols, fine, n_cols_f, max_lag, Z, H, n_emitters=1, guard=0, min_separation=1, fine_separation=1,
               n_w=1, clock=None):
    """One stack -> (locate_multi.locate_multi's four outputs [K][...], records [K] ZOOM_DTYPE, zpairs [K][2] int32, zlags [K][P]
    int32, zcorr [K][P] float64, zmap [K][(2H+1)^2] int64)"""
    K, guard, ml = int(n_emitters), int(guard), int(max_lag)
    if not 1 <= K <= MAX_EMITTERS:
        raise ValueError("n_emitters must be 1 .. 8")
    if guard < 0:
        raise ValueError("guard must be >= 0")
    q = np.asarray(q_pairs, dtype=np.int64)
    lag = pair_lags(table, clock)
    fine = np.asarray(fine, dtype=np.int64)
    P = lag.shape[1]
    at_lag = lambda l: np.where((l > -ml) & (l < ml), l + ml - 1, 0)
    excluded = np.zeros((P, 2 * ml - 1), dtype=bool)                     # E_p as a mask over the range's lags
    out = []
    for _ in range(K):
        rec, lags, corr, score, zrec, zlags, zcorr, zmap = _zoom.zoom(np.where(excluded, 0, q), table, n_cols, fine, n_cols_f, ml, Z, H,
                                                                      min_separation, fine_separation, n_w, clock)
        zpairs = np.zeros(2, dtype=np.int32)
        if zrec["score_q"] > 0:                                          # the fine cell's pairs under E_p(r)
            f = pair_lags(fine[int(zrec["cell"])][None, :], clock)[0]
            inside = (f > -ml) & (f < ml)
            ex = inside & excluded[np.arange(P), at_lag(f)]
            zrec["pairs_in"] = (inside & ~ex).sum()
            zpairs[:] = zrec["pairs_in"], ex.sum()
        if rec["score_q"] > 0:                                           # locate_multi's round: the counts, then the centres
            at = lag[int(rec["cell"])]
            inside = (at > -ml) & (at < ml)
            ex = inside & excluded[np.arange(P), at_lag(at)]
            rec["pairs_in"], rec["reserved"] = (inside & ~ex).sum(), ex.sum()
            for p in np.nonzero(inside)[0]:
                excluded[p, max(at[p] - guard, -(ml - 1)) + ml - 1:min(at[p] + guard, ml - 1) + ml] = True
        out.append((rec, lags, corr, score, zrec, zpairs, zlags, zcorr, zmap))
    return tuple(np.stack([o[k] for o in out]) for k in range(9))


def multi_zoom_stacks(q, table, n_cols, fine, n_cols_f, max_lag, Z, H, n_emitters=1, guard=0, min_separation=1, fine_separation=1,
                      n_w=1, clock=None):
    """q [n_sets][P][2 max_lag - 1] -> the nine outputs [K][n_sets][...]; n_w a number or one per set; clock None or [n_sets][S]"""
    q = np.asarray(q, dtype=np.int64)
    n = np.broadcast_to(np.asarray(n_w), (q.shape[0],))
    if clock is not None and np.shape(clock)[0] != q.shape[0]:
        raise ValueError("clock must hold one row per set")
    out = [multi_zoom(q[s], table, n_cols, fine, n_cols_f, max_lag, Z, H, n_emitters, guard, min_separation, fine_separation, int(n[s]),
                      None if clock is None else clock[s]) for s in range(q.shape[0])]
    return tuple(np.stack([o[k] for o in out], axis=1) for k in range(9))


def multi_zoom_upsampled(q, table, n_cols, fine, n_cols_f, max_lag, Z, H, U, n_emitters=1, guard=0, min_separation=1, fine_separation=1,
                         n_w=1, clock=None):
    """multi_zoom_stacks with the setting U: on upsample(q, U), U table, U fine, U clock, U guard, max_lag' = (max_lag - 1) U + 1"""
    t, k, g, ml_u = _upsample.scaled_args(table, clock, guard, max_lag, U)
    f = np.asarray(fine, dtype=np.int64) * int(U)
    return multi_zoom_stacks(_upsample.upsample(q, U), t, n_cols, f, n_cols_f, ml_u, Z, H, n_emitters, guard=g,
                             min_separation=min_separation, fine_separation=fine_separation, n_w=n_w, clock=k)
