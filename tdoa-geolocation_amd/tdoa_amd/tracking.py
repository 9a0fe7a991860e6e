"""The delay track of tdoa_process_track (include/tdoa_mi355x.h, "delay tracks") in int64 numpy: what the GPU kernels
(csrc/stack_track.hpp) are held to, word for word.  Tests use it; the library does not.

    T_{n_w-1}[l] = s q_{n_w-1}[l]
    T_j[l]       = s q_j[l] + max over |d| <= J, l+d inside the range, of T_{j+1}[l+d]
    D_j[l]       = the d of that maximum; equal maxima: the smaller |d|, then the positive d
    L_0          = the l with the largest T_0[l]; equal maxima: the smaller |l|, then the positive l
    L_{j+1}      = L_j + D_j[L_j]

for the polarity s in {+1, -1} with the larger max T_0 (a tie: +1)."""
import numpy as np

from .stacking import PEAK_DTYPE, Q_ONE, from_fixed

ABSENT = np.iinfo(np.int64).min        # a lag outside the range: never larger than a lag inside it


def step_order(max_step):
    """the steps in the order of the tie rule: 0, +1, -1, +2, -2, ..."""
    out = [0]
    for s in range(1, int(max_step) + 1):
        out += [s, -s]
    return out


def backward(q_signed, max_step):
    """q_signed [m][L] int64 (s q_j) -> (T_0 [L] int64, D [m-1][L] int8): the recurrence from the last window back"""
    q = np.asarray(q_signed, dtype=np.int64)
    m, n = q.shape
    T = q[m - 1].copy()
    D = np.zeros((max(m - 1, 0), n), dtype=np.int8)
    for j in range(m - 2, -1, -1):
        best = T.copy()                                  # d = 0 is always inside the range
        for d in step_order(max_step)[1:]:
            if abs(d) >= n:
                continue
            cand = np.full(n, ABSENT, dtype=np.int64)
            if d > 0:
                cand[:n - d] = T[d:]
            else:
                cand[-d:] = T[:n + d]
            better = cand > best                         # strict: the earlier step of the order keeps an equal maximum
            best = np.where(better, cand, best)
            D[j][better] = d
        T = q[j] + best
    return T, D


def first_lag(T0, max_lag):
    """(index, value) of the largest T_0; equal maxima: the smaller |l|, then the positive l"""
    T0 = np.asarray(T0, dtype=np.int64)
    top = T0.max()
    idx = np.flatnonzero(T0 == top)
    lag = idx - (int(max_lag) - 1)
    pick = np.lexsort((lag < 0, np.abs(lag)))[0]
    return int(idx[pick]), int(top)


def track(q_windows, max_step, max_lag):
    """One stack-pair: q_windows [m][2 max_lag - 1] int64, window j of the stack at row j ->
    (score_q, lags [m] int32, values_q [m] int64, total [2 max_lag - 1] int64):
    score_q = s max T_0, the signed sum along the track; lags[j] = L_j; values_q[j] = q_j[L_j]; total = s T_0.
    Nothing but zeros (max T_0 = 0): score_q 0, lags and values 0."""
    q = np.asarray(q_windows, dtype=np.int64)
    J, ml = int(max_step), int(max_lag)
    if q.ndim != 2 or q.shape[0] < 1 or q.shape[1] != 2 * ml - 1:
        raise ValueError("q_windows must be [m >= 1][2 max_lag - 1]")
    if J < 0:
        raise ValueError("max_step must be >= 0")
    m = q.shape[0]
    best = None
    for s in (1, -1):
        T0, D = backward(s * q, J)
        i0, top = first_lag(T0, ml)
        if best is None or top > best[1]:                # a tie keeps +1
            best = (s, top, i0, T0, D)
    s, top, i, T0, D = best
    lags = np.zeros(m, dtype=np.int32)
    values = np.zeros(m, dtype=np.int64)
    if top != 0:
        for j in range(m):
            lags[j] = i - (ml - 1)
            values[j] = q[j, i]
            if j + 1 < m:
                i += int(D[j, i])
    return s * top, lags, values, s * T0


def score_record(score_q, lag, n_w):
    """the tdoa_peak of a track: lag = L_0, corr the double (s max T_0) 2^-32 / sqrt(n_w), abs_corr its float magnitude;
    score_q 0: the zero record"""
    rec = np.zeros((), dtype=PEAK_DTYPE)
    if int(score_q) != 0:
        c = from_fixed(np.int64(score_q), n_w)
        rec["lag"], rec["abs_corr"], rec["corr"] = int(lag), np.float32(abs(c)), c
    return rec


def values_double(values_q):
    """values[j] = (double)q_j[L_j] 2^-32"""
    return np.asarray(values_q, dtype=np.int64).astype(np.float64) * (1.0 / Q_ONE)


def surface(total, n_w):
    """(float)(total 2^-32 / sqrt(n_w))"""
    return from_fixed(total, n_w).astype(np.float32)
