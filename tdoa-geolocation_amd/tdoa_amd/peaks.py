"""The peak-selection rule of tdoa_process_peaks (include/tdoa_mi355x.h) in float64 numpy: what the GPU kernel
(csrc/peak_select.hpp) is held to; and the exact relation between a peak record and the float32 surface of the same
pair-window (csrc/peak_key.hpp: one step offers a value to the key and writes it to the surface)."""
import numpy as np


def surface_max(surface, lag_lo):
    """(T, value) of one returned float32 surface (lags lag_lo, lag_lo + 1, ...): T = the lags l with |s[l]| == max |s|, in
    the order of the peak key (smaller |lag| first, then the positive lag), and the signed value at T[0].  NaN never counts;
    an empty or all-NaN surface gives ([], 0.0)."""
    s = np.asarray(surface, dtype=np.float32)
    a = np.abs(s)
    if not np.any(a == a):
        return [], np.float32(0.0)
    top = np.nanmax(a)
    lags = np.nonzero(a == top)[0] + int(lag_lo)
    order = np.lexsort((lags <= 0, np.abs(lags)))
    T = [int(l) for l in lags[order]]
    return T, s[T[0] - int(lag_lo)]


def record_is_surface_max(rec, surface, max_lag):
    """assert, without a tolerance, that the peak record `rec` (lag, abs_corr, corr) is the maximum of |surface|, the float32
    surface of the same pair-window over the lags -(max_lag - 1) .. max_lag - 1; returns T of surface_max.

    Exact because the record is (double)|raw| x scale (x gain) with the sign put back and the surface element is
    (float)((double)raw x scale (x gain)) of the same raw float in the same order, and scale and gain are positive: rounding
    to float32 is monotone, so it can merge two magnitudes into a tie but cannot reorder them -- the record's lag is in T.
    It is held to the first of T, the key's choice among equal raw values; a caller whose surface could hold two raw values
    that only the rounding made equal checks len(T) == 1 on what comes back."""
    s = np.asarray(surface, dtype=np.float32)
    ml = int(max_lag)
    assert s.shape == (2 * ml - 1,)
    lag, corr, abs_corr = int(rec["lag"]), float(rec["corr"]), np.float32(rec["abs_corr"])
    T, top = surface_max(s, -(ml - 1))
    if not T or top == 0:
        assert (lag, corr, float(abs_corr)) == (0, 0.0, 0.0), "a record on a surface without a peak"
        return T
    assert -(ml - 1) <= lag <= ml - 1, lag
    at = s[lag + ml - 1]
    assert np.float32(corr) == at and np.signbit(np.float32(corr)) == np.signbit(at), (lag, corr, float(at))
    assert abs_corr == np.abs(at), (lag, float(abs_corr), float(at))
    assert np.abs(at) == np.abs(top), ("the record is not the surface's maximum", lag, float(at), T[0], float(top))
    assert lag == T[0], ("the tie went to the wrong lag", lag, T)
    return T


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
