"""The peak-selection rule of tdoa_process_peaks (include/tdoa_mi355x.h) in float64 numpy: what the GPU kernel
(csrc/peak_select.hpp) is held to."""
import numpy as np


def select_peaks(surface, lag_lo, k, min_separation):
    """[(lag, value)] of the k strongest separate peaks of `surface` (lags lag_lo, lag_lo + 1, ...), strongest first.

    A lag is a candidate when |c| there is >= |c| at both neighbours (a neighbour outside the range counts as smaller; a
    NaN neighbour fails the comparison) and c is neither NaN nor 0.  Each round takes the largest |c| among the candidates
    more than min_separation lags from every peak already chosen; ties go to the smaller |lag|, then the positive lag."""
    if not 1 <= k <= 16 or min_separation < 1:
        raise ValueError("k must be in 1..16 and min_separation >= 1")
    c = np.asarray(surface, dtype=np.float64)
    a = np.abs(c)
    left = np.concatenate([[-np.inf], a[:-1]])
    right = np.concatenate([a[1:], [-np.inf]])
    with np.errstate(invalid="ignore"):
        cand = (a > 0) & (a >= left) & (a >= right)
    idx = np.nonzero(cand)[0]
    lags = idx + int(lag_lo)
    order = np.lexsort((lags <= 0, np.abs(lags), -a[idx]))      # primary |c| descending, then |lag|, then positive first
    out = []
    for o in order:
        lag = int(lags[o])
        if all(abs(lag - q) > min_separation for q, _ in out):
            out.append((lag, float(c[idx[o]])))
            if len(out) == k:
                break
    return out
