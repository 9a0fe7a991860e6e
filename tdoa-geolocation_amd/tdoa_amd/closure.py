"""The closure search of tdoa_process_closure (include/tdoa_mi355x.h, "closure search") in int64 numpy: what the GPU kernels
(csrc/stack_closure.hpp) are held to, word for word.  Tests use it; the library does not.

For a triple i < j < k of stations with the pair centres c_ij, c_ik, c_jk (c_p(i,j) = centre[j] - centre[i]) and the gate G:

    cell (u, v):   |u| <= G, |v| <= G, |v-u| <= G;  a = c_ij + u, b = c_ik + v, e = b - a, all inside -max_lag < . < max_lag
    score_q(u,v) = M_ij[a] + M_ik[b] + M_jk[e],  M_p[l] = |Q_p[l]|

The joint cell is the largest score_q; equal maxima: the smaller |u|, then the positive u, then the smaller |v|, then the
positive v."""
import numpy as np

from .stacking import from_fixed

CLOSURE_DTYPE = np.dtype([("lag_ij", np.int32), ("lag_ik", np.int32), ("lag_jk", np.int32), ("residual", np.int32),
                          ("score_q", np.int64), ("own_q", np.int64), ("runner_q", np.int64),
                          ("corr_ij", np.float64), ("corr_ik", np.float64), ("corr_jk", np.float64),
                          ("score", np.float64), ("runner_up", np.float64)])      # tdoa_closure

MAX_GATE = 1023
ABSENT = -1                 # a lag outside the searched range: no magnitude is negative


def triples(n_stations):
    """the triples i < j < k in lexicographic order"""
    S = int(n_stations)
    return [(i, j, k) for i in range(S) for j in range(i + 1, S) for k in range(j + 1, S)]


def num_triples(n_stations):
    S = int(n_stations)
    return S * (S - 1) * (S - 2) // 6


def pair_index(i, j, n_stations):
    """p(i,j) = i S - i (i+1) / 2 + (j - i - 1), i < j: the library's pair order"""
    i, j, S = int(i), int(j), int(n_stations)
    if not 0 <= i < j < S:
        raise ValueError("pair_index needs 0 <= i < j < n_stations")
    return i * S - i * (i + 1) // 2 + (j - i - 1)


def tie_rank(x):
    """0, +1, -1, +2, -2, ... -> 0, 1, 2, 3, 4, ...: the smaller |x|, then the positive x"""
    x = np.asarray(x, dtype=np.int64)
    return 2 * np.abs(x) - (x > 0)


def gated_row(q, centre, gate, max_lag):
    """M_p over the gated window of one pair: [2 G + 1] int64, entry x + G = |Q_p[c_p + x]|, ABSENT outside the range"""
    ml, G = int(max_lag), int(gate)
    lag = int(centre) + np.arange(-G, G + 1, dtype=np.int64)
    inside = (lag > -ml) & (lag < ml)
    row = np.full(2 * G + 1, ABSENT, dtype=np.int64)
    row[inside] = np.abs(np.asarray(q, dtype=np.int64)[lag[inside] + ml - 1])
    return row


def own_peak(row, gate):
    """(x*, maximum) of a gated row; equal maxima: the smaller |x|, then the positive x.  An empty window: (0, 0)"""
    G = int(gate)
    if (row < 0).all():
        return 0, 0
    top = row.max()
    x = np.flatnonzero(row == top) - G
    return int(x[np.argmin(tie_rank(x))]), int(top)


def closure_triple(q_ij, q_ik, q_jk, c_ij, c_ik, c_jk, max_lag, gate, min_separation, n_w=1):
    """One triple: the three pairs' Q [2 max_lag - 1] int64 and centres (c_jk = c_ik - c_ij) -> one CLOSURE_DTYPE record"""
    ml, G, sep = int(max_lag), int(gate), int(min_separation)
    if not 0 <= G <= MAX_GATE:
        raise ValueError("gate must be 0 .. 1023")
    if sep < 1:
        raise ValueError("min_separation must be >= 1")
    if int(c_jk) != int(c_ik) - int(c_ij):
        raise ValueError("the centres do not close")
    rec = np.zeros((), dtype=CLOSURE_DTYPE)
    q = [np.asarray(x, dtype=np.int64) for x in (q_ij, q_ik, q_jk)]
    if any(x.shape != (2 * ml - 1,) for x in q):
        raise ValueError("Q must be [2 max_lag - 1] per pair")
    r_ij, r_ik, r_jk = (gated_row(x, c, G, ml) for x, c in zip(q, (c_ij, c_ik, c_jk)))
    u_in, v_in = np.flatnonzero(r_ij >= 0), np.flatnonzero(r_ik >= 0)      # (a searched range is an interval: so are these)
    if not len(u_in) or not len(v_in):
        return rec
    u0, v0 = int(u_in[0]), int(v_in[0])
    # m_jk[u, v] = r_jk[v - u + G], ABSENT where |v - u| > G: the rows of a sliding window over the padded row, no copy
    pad = np.full(G, ABSENT, dtype=np.int64)
    m_jk = np.lib.stride_tricks.sliding_window_view(np.concatenate([pad, r_jk, pad]), 2 * G + 1)[::-1]
    m_jk = m_jk[u0:int(u_in[-1]) + 1, v0:int(v_in[-1]) + 1]
    score = r_ij[u_in, None] + r_ik[None, v_in] + m_jk
    score[m_jk < 0] = ABSENT                                               # the cells that do not exist
    top = int(score.max())
    if top <= 0:
        return rec
    at = np.argwhere(score == top) + (u0 - G, v0 - G)
    us, vs = (int(x) for x in at[np.argmin(tie_rank(at[:, 0]) * 4096 + tie_rank(at[:, 1]))])
    a, b = int(c_ij) + us, int(c_ik) + vs
    e = b - a
    own = [own_peak(r, G) for r in (r_ij, r_ik, r_jk)]
    iu, iv = us + G - u0, vs + G - v0
    score[max(iu - sep, 0):iu + sep + 1, max(iv - sep, 0):iv + sep + 1] = ABSENT      # what is left is the runner-up's
    runner = max(int(score.max()), 0)
    rec["lag_ij"], rec["lag_ik"], rec["lag_jk"] = a, b, e
    rec["residual"] = (int(c_ij) + own[0][0]) + (int(c_jk) + own[2][0]) - (int(c_ik) + own[1][0])
    rec["score_q"], rec["own_q"], rec["runner_q"] = top, sum(o[1] for o in own), runner
    for name, qq, lag in (("corr_ij", q[0], a), ("corr_ik", q[1], b), ("corr_jk", q[2], e)):
        rec[name] = from_fixed(qq[lag + ml - 1], n_w)
    rec["score"], rec["runner_up"] = from_fixed(np.int64(top), n_w), from_fixed(np.int64(runner), n_w)
    return rec


def closure(q_pairs, n_stations, max_lag, gate, min_separation=1, centre=None, n_w=1):
    """One stack: q_pairs [P][2 max_lag - 1] int64 in the library's pair order -> [T] CLOSURE_DTYPE, one record per triple;
    centre [n_stations] int (None: all 0)"""
    S = int(n_stations)
    q = np.asarray(q_pairs, dtype=np.int64)
    if S < 3 or q.shape != (S * (S - 1) // 2, 2 * int(max_lag) - 1):
        raise ValueError("q_pairs must be [S (S-1) / 2][2 max_lag - 1], S >= 3")
    c = np.zeros(S, dtype=np.int64) if centre is None else np.asarray(centre, dtype=np.int64)
    if c.shape != (S,):
        raise ValueError("centre must be [n_stations]")
    out = np.zeros(num_triples(S), dtype=CLOSURE_DTYPE)
    for t, (i, j, k) in enumerate(triples(S)):
        out[t] = closure_triple(q[pair_index(i, j, S)], q[pair_index(i, k, S)], q[pair_index(j, k, S)],
                                c[j] - c[i], c[k] - c[i], c[k] - c[j], max_lag, gate, min_separation, n_w)
    return out


def closure_stacks(q, n_stations, max_lag, gate, min_separation=1, centre=None, n_w=1):
    """q [n_sets][P][2 max_lag - 1] -> [n_sets][T] CLOSURE_DTYPE; n_w a number or one per set"""
    q = np.asarray(q, dtype=np.int64)
    n = np.broadcast_to(np.asarray(n_w), (q.shape[0],))
    return np.stack([closure(q[s], n_stations, max_lag, gate, min_separation, centre, int(n[s])) for s in range(q.shape[0])])


def independent_lags(q_pairs, n_stations, max_lag, gate, centre=None):
    """the three pairs' own argmax lags of every triple of one stack: [T][3] (ij, ik, jk), by the rule of own_q"""
    S, ml, G = int(n_stations), int(max_lag), int(gate)
    q = np.asarray(q_pairs, dtype=np.int64)
    c = np.zeros(S, dtype=np.int64) if centre is None else np.asarray(centre, dtype=np.int64)
    out = np.zeros((num_triples(S), 3), dtype=np.int64)
    for t, (i, j, k) in enumerate(triples(S)):
        for n, (a, b) in enumerate(((i, j), (i, k), (j, k))):
            cp = int(c[b] - c[a])
            out[t, n] = cp + own_peak(gated_row(q[pair_index(a, b, S)], cp, G, ml), G)[0]
    return out

