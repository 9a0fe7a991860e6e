"""The stacked correlation of tdoa_process_stacked (include/tdoa_mi355x.h, "stacked correlation") and the slope search of
tdoa_process_stacked_drift ("drift-compensated stacking") in float64 / int64 numpy: what the GPU kernels
(csrc/stack_surfaces.hpp, csrc/stack_drift.hpp) are held to.  Tests use it; the library does not."""
import numpy as np

from .peaks import select_peaks, surface_max

PEAK_DTYPE = np.dtype([("lag", np.int32), ("abs_corr", np.float32), ("corr", np.float64)])      # tdoa_peak

Q_ONE = 2.0 ** 32          # fixed-point units per unit of correlation


def stack_ids(windows_per_block, windows_per_stack=0):
    """(stacks_per_block, [(sid, [window ids])]) of a job of 3 blocks: runs of windows_per_stack consecutive windows of one
    block (0: the whole block), the last run of a block possibly shorter, never across a block boundary"""
    wpb = int(windows_per_block)
    m = wpb if windows_per_stack == 0 else min(int(windows_per_stack), wpb)
    if m < 1:
        raise ValueError("windows_per_stack must be >= 0")
    spb = -(-wpb // m)
    out = []
    for block in range(3):
        for j in range(spb):
            out.append((block * spb + j, [block * wpb + w for w in range(j * m, min((j + 1) * m, wpb))]))
    return spb, out


def to_fixed(c):
    """q = llrint(c * 2^32): int64, round to nearest even"""
    return np.rint(np.asarray(c, dtype=np.float64) * Q_ONE).astype(np.int64)


def from_fixed(q, n_w):
    """C = (double)Q * 2^-32 / sqrt(n_w)"""
    return np.asarray(q, dtype=np.int64).astype(np.float64) * (1.0 / Q_ONE) / np.sqrt(np.float64(n_w))


def stack_surfaces(surfaces, windows_per_block, windows_per_stack=0):
    """surfaces [W][P][L] (reference scale, W = 3 windows_per_block) -> (Q [n_stacks][P][L] int64, C float64, n_w [n_stacks])"""
    s = np.asarray(surfaces, dtype=np.float64)
    if s.ndim != 3 or s.shape[0] != 3 * int(windows_per_block):
        raise ValueError("surfaces must be [3 * windows_per_block][P][L]")
    _, ids = stack_ids(windows_per_block, windows_per_stack)
    q = np.zeros((len(ids),) + s.shape[1:], dtype=np.int64)
    n_w = np.zeros(len(ids), dtype=np.int64)
    for sid, wins in ids:
        q[sid] = to_fixed(s[wins]).sum(axis=0)
        n_w[sid] = len(wins)
    c = np.stack([from_fixed(q[sid], n_w[sid]) for sid in range(len(ids))]) if len(ids) else q.astype(np.float64)
    return q, c, n_w


def stacked_peaks(c, max_lag, k=1, min_separation=1):
    """the selection rule of tdoa_process_peaks on (float32)C of one stack-pair -> [(lag, C[lag] as float64)]"""
    c = np.asarray(c, dtype=np.float64)
    picked = select_peaks(c.astype(np.float32), -(int(max_lag) - 1), k, min_separation)
    return [(lag, float(c[lag + int(max_lag) - 1])) for lag, _ in picked]


def refine(c, max_lag, lag):
    """the parabola of tdoa_process_fine on C[lag-1], C[lag], C[lag+1] -> lag + frac (frac 0 at the edge of the range)"""
    c = np.asarray(c, dtype=np.float64)
    i = int(lag) + int(max_lag) - 1
    if i <= 0 or i + 1 >= len(c):
        return float(lag)
    sg = -1.0 if c[i] < 0 else 1.0
    ym, y0, yp = sg * c[i - 1], sg * c[i], sg * c[i + 1]
    den = ym - 2.0 * y0 + yp
    fr = 0.5 * (ym - yp) / den if den < 0 else 0.0
    return float(lag) + float(np.clip(fr, -0.5, 0.5))


def shift(h, j, den):
    """shift(h, j) = sgn(h) ((2 |h| j + D) div (2 D)): the nearest integer to h j / D, halves away from zero"""
    h, j, den = int(h), int(j), int(den)
    if den < 1 or j < 0:
        raise ValueError("den must be >= 1 and j >= 0")
    a = (2 * abs(h) * j + den) // (2 * den)
    return -a if h < 0 else a


def sheared_sum(q_windows, h, den):
    """q_windows [m][L] int64, window j of a stack at row j -> Q_h[L] = sum_j q_j[L + shift(h, j)], a term outside the
    searched range contributing 0"""
    q = np.asarray(q_windows, dtype=np.int64)
    n = q.shape[-1]
    out = np.zeros(n, dtype=np.int64)
    for j in range(q.shape[0]):
        s = shift(h, j, den)
        lo, hi = max(0, -s), min(n, n - s)              # L with 0 <= L + s < n
        if lo < hi:
            out[lo:hi] += q[j, lo + s:hi + s]
    return out


def drift_search(q_windows, max_drift, den, max_lag):
    """the slope search on one stack-pair's windows q_windows [m][2 max_lag - 1] int64 -> (h*, profile [2 max_drift + 1]
    PEAK_DTYPE, Q_h*): per hypothesis the maximum of |float32(C_h)| (ties: smaller |lag|, then the positive lag), h* the
    hypothesis with the largest abs_corr (ties: smaller |h|, then the positive h; nothing but zeros: 0)"""
    q = np.asarray(q_windows, dtype=np.int64)
    H, ml = int(max_drift), int(max_lag)
    if q.ndim != 2 or q.shape[1] != 2 * ml - 1:
        raise ValueError("q_windows must be [m][2 max_lag - 1]")
    if shift(H, max(q.shape[0] - 1, 0), den) > ml - 1:
        raise ValueError("the largest shift exceeds max_lag - 1")
    profile = np.zeros(2 * H + 1, dtype=PEAK_DTYPE)
    sums = {}
    best = None
    for h in sorted(range(-H, H + 1), key=lambda x: (abs(x), x < 0)):       # 0, +1, -1, +2, -2, ...
        sums[h] = sheared_sum(q, h, den)
        T, top = surface_max(from_fixed(sums[h], q.shape[0]).astype(np.float32), -(ml - 1))
        if T and top != 0:
            profile[h + H] = (T[0], np.abs(top), np.float64(top))
            if best is None or profile[h + H]["abs_corr"] > profile[best + H]["abs_corr"]:
                best = h
    best = 0 if best is None else best
    return best, profile, sums[best]


def drift_ppm(h, den, window_len):
    """the relative clock rate a slope of h / den lags per window of window_len samples stands for, in parts per million"""
    return 1e6 * float(h) / (float(den) * float(window_len))
