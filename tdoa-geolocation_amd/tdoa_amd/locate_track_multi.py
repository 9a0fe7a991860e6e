"""Several emitters per block, tdoa_process_locate_track_multi (include/tdoa_mi355x.h, "several emitters per block") in int64
numpy: what the GPU kernels (csrc/stack_locate_track_multi.hpp) are held to, byte for byte.  Tests use it; the library does not.

Per track (the L stacks of a block), rounds r = 0 .. K - 1 of the cell track (locate_track.track) on the maps the delay-table
search (locate.locate_stacks) gives on a masked copy of Q:

    E_p^j(0) is empty;  if round r found a track, E_p^j(r+1) = E_p^j(r) united with { l : |l - lag_p^j(L_j^r)| <= guard } for
                        every stack j and every pair whose lag at the track's cell L_j^r lies inside the range; else E(r+1) = E(r)
    M_p^{j,r}[l] = 0 for l in E_p^j(r) or outside the range, else |Q_p^j[l]|;   s_j^r(c) = sum over the pairs of M_p^{j,r}[lag_p^j(c)]

Round r's record, cells, own scores and T_0 are the cell track's on s^r.  Per (round, stack) pairs_in counts the pairs inside
the range and not excluded at L_j^r, `reserved` the pairs inside but excluded there; an excluded pair reports its lag and 0.0.
A round whose largest T_0 is 0 returns the zero record and adds nothing to E, so every later round is the zero record too.
Round 0 is locate_track.track_stacks; with one stack per track every round is locate_multi.locate_multi_stacks' round."""
import numpy as np

from .locate import locate_stacks, pair_lags
from .locate_multi import MAX_EMITTERS
from .locate_track import MAX_LEN, cell_lags, track


def track_multi_stacks(q, table, n_cols, max_lag, track_len, J, n_emitters=1, guard=0, sep=1, n_w=1, clock=None):
    """q [n_sets][P][2 max_lag - 1], set t track_len + j position j of track t; n_w a number or one per set; clock None or
    [n_sets][S] -> (records [K][n_tracks], cells [K][n_tracks][L] int32, own [K][n_tracks][L] int64, pairs [K][n_sets][2] int32
    (pairs_in, reserved), lags [K][n_sets][P] int32, corr [K][n_sets][P] float64, total [K][n_tracks][n_cells] int64)"""
    K, guard, ml, L = int(n_emitters), int(guard), int(max_lag), int(track_len)
    if not 1 <= K <= MAX_EMITTERS:
        raise ValueError("n_emitters must be 1 .. 8")
    if guard < 0:
        raise ValueError("guard must be >= 0")
    q = np.asarray(q, dtype=np.int64)
    if not 1 <= L <= MAX_LEN or q.shape[0] % L:
        raise ValueError("track_len must be 1 .. 4096 and divide the number of sets")
    n_sets, P = q.shape[:2]
    n = np.broadcast_to(np.asarray(n_w), (n_sets,))
    excluded = np.zeros((n_sets, P, 2 * ml - 1), dtype=bool)               # E_p^j as a mask over the range's lags
    rounds = []
    for _ in range(K):
        maps = locate_stacks(np.where(excluded, 0, q), table, n_cols, ml, sep, n, clock)[3]
        recs, cells, own, total = [], [], [], []
        pairs = np.zeros((n_sets, 2), dtype=np.int32)
        lags, corr = np.zeros((n_sets, P), dtype=np.int32), np.zeros((n_sets, P), dtype=np.float64)
        for t in range(n_sets // L):
            rec, c, o, tot = track(maps[t * L:(t + 1) * L], n_cols, J, sep, int(n[t * L:(t + 1) * L].sum()))
            recs.append(rec)
            cells.append(c)
            own.append(o)
            total.append(tot)
            if rec["score_q"] <= 0:
                continue
            for j in range(L):
                sid = t * L + j
                k = None if clock is None else clock[sid]
                at = pair_lags(np.asarray(table)[int(c[j]):int(c[j]) + 1], k)[0]
                inside = (at > -ml) & (at < ml)
                ex = inside & excluded[sid][np.arange(P), np.where(inside, at + ml - 1, 0)]
                lags[sid], corr[sid] = cell_lags(q[sid], table, c[j], ml, int(n[sid]), k)
                corr[sid][ex] = 0.0
                pairs[sid] = (inside & ~ex).sum(), ex.sum()
                for p in np.nonzero(inside)[0]:
                    excluded[sid, p, max(at[p] - guard, -(ml - 1)) + ml - 1:min(at[p] + guard, ml - 1) + ml] = True
        rounds.append((np.stack(recs), np.stack(cells), np.stack(own), pairs, lags, corr, np.stack(total)))
    return tuple(np.stack([r[k] for r in rounds]) for k in range(7))
