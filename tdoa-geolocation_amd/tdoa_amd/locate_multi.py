"""Several emitters per stack, tdoa_process_locate_multi (include/tdoa_mi355x.h, "several emitters per stack") in int64 numpy:
what the GPU kernels (csrc/stack_locate_multi.hpp) are held to, byte for byte.  Tests use it; the library does not.

Per stack, rounds r = 0 .. K - 1 of the delay-table search (locate.locate) on the same table and the same Q:

    E_p(0) is empty;  E_p(r+1) = E_p(r) united with { l : |l - lag_p(cell*_r)| <= guard } if round r found a cell and
                      lag_p(cell*_r) lies inside the searched range, else E_p(r)
    M_p^r[l] = 0 for l in E_p(r) or outside the range, else |Q_p[l]|;   score_q^r(c) = sum over the pairs of M_p^r[lag_p(c)]

Round r's record is the search's on M^r; pairs_in counts the pairs inside the range and not excluded at the cell, `reserved`
the pairs inside the range but excluded there.  An excluded pair reports its lag and 0.0.  A round whose largest score is 0
returns the zero record and adds nothing to E, so every later round is the zero record too.  Round 0 is locate.locate."""
import numpy as np

from .locate import LOCATION_DTYPE, locate, pair_lags

MAX_EMITTERS = 8            # TDOA_LOCATE_MAX_EMITTERS


def locate_multi(q_pairs, table, n_cols, max_lag, n_emitters=1, guard=0, min_separation=1, n_w=1, clock=None):
    """One stack: q_pairs [P][2 max_lag - 1] int64, table [n_cells][S], clock None or [S] -> (records [K] LOCATION_DTYPE,
    lags [K][P] int32, corr [K][P] float64, map [K][n_cells] int64), K = n_emitters"""
    K, guard, ml = int(n_emitters), int(guard), int(max_lag)
    if not 1 <= K <= MAX_EMITTERS:
        raise ValueError("n_emitters must be 1 .. 8")
    if guard < 0:
        raise ValueError("guard must be >= 0")
    q = np.asarray(q_pairs, dtype=np.int64)
    lag = pair_lags(table, clock)
    P = lag.shape[1]
    excluded = np.zeros((P, 2 * ml - 1), dtype=bool)                     # E_p as a mask over the range's lags
    out = []
    for _ in range(K):
        rec, lags, corr, score = locate(np.where(excluded, 0, q), table, n_cols, ml, min_separation, n_w, clock)
        if rec["score_q"] > 0:
            at = lag[int(rec["cell"])]
            inside = (at > -ml) & (at < ml)
            ex = inside & excluded[np.arange(P), np.where(inside, at + ml - 1, 0)]
            rec["pairs_in"], rec["reserved"] = (inside & ~ex).sum(), ex.sum()
            for p in np.nonzero(inside)[0]:
                excluded[p, max(at[p] - guard, -(ml - 1)) + ml - 1:min(at[p] + guard, ml - 1) + ml] = True
        out.append((rec, lags, corr, score))
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def locate_multi_stacks(q, table, n_cols, max_lag, n_emitters=1, guard=0, min_separation=1, n_w=1, clock=None):
    """q [n_sets][P][2 max_lag - 1] -> (records [K][n_sets], lags [K][n_sets][P], corr [K][n_sets][P], map
    [K][n_sets][n_cells]); n_w a number or one per set; clock None or [n_sets][S]"""
    q = np.asarray(q, dtype=np.int64)
    n = np.broadcast_to(np.asarray(n_w), (q.shape[0],))
    if clock is not None and np.shape(clock)[0] != q.shape[0]:
        raise ValueError("clock must hold one row per set")
    out = [locate_multi(q[s], table, n_cols, max_lag, n_emitters, guard, min_separation, int(n[s]),
                        None if clock is None else clock[s]) for s in range(q.shape[0])]
    return tuple(np.stack([o[k] for o in out], axis=1) for k in range(4))


def near(cell, target, n_cols):
    """cell within one row and one column of target"""
    return abs(int(cell) // n_cols - int(target) // n_cols) <= 1 and abs(int(cell) % n_cols - int(target) % n_cols) <= 1
