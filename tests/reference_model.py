"""numpy restatement of the oracle's timeDomainCorrelation (oracle/tdoa_oracle.c: tdc_one_lag,
o_time_domain_correlation; processor.go:646-736) with the block size as an argument -- the oracle fixes it at 1000,
the library takes it from tdoa_params.corr_block.  tests/test_reference_model_cpu.py holds the model to the oracle at
block = 1000 before tests/test_gpu_reference_edges.py uses it to judge the GPU at other block sizes."""
import math

import numpy as np


def tdc_model(s1, s2, max_lag, block=1000):
    """-> (delay, corr, all_lags): the reference's answer and its value at every searched lag.

    Per lag: f32 products f32(f32(tr*sr) + f32(ti*si)), widened to f64 and summed SEQUENTIALLY inside a block
    (np.add.accumulate, never np.sum: pairwise summation has another rounding), / block, the sequential sum over
    blocks, / nb, * sqrt(nb * block); the first strictly greater |corr| over ascending lag wins."""
    t = np.ascontiguousarray(s1, dtype=np.complex64)
    s = np.ascontiguousarray(s2, dtype=np.complex64)
    if t.size > s.size:                                   # :650-655 the shorter input is the template
        t, s = s, t
    tl, sl, block = t.size, s.size, int(block)
    ml = max(1, min(int(max_lag), sl - tl))               # :668-675
    nb_all = len(range(0, tl - block, block))             # block starts below tl - block
    all_lags = np.zeros(ml, dtype=np.float64)
    delay, best = 0, 0.0
    tr = np.ascontiguousarray(t.real[:nb_all * block])
    ti = np.ascontiguousarray(t.imag[:nb_all * block])
    sr_all = np.ascontiguousarray(s.real)
    si_all = np.ascontiguousarray(s.imag)
    for d in range(ml):
        nb = min(nb_all, max(0, (sl - d) // block))       # a block that would run off the signal ends the lag's loop
        if nb == 0:
            continue
        m = nb * block
        p = tr[:m] * sr_all[d:d + m] + ti[:m] * si_all[d:d + m]            # float32 throughout
        assert p.dtype == np.float32
        bc = np.add.accumulate(p.astype(np.float64).reshape(nb, block), axis=1)[:, -1] / np.float64(block)
        c = np.add.accumulate(bc)[-1]
        c = c / np.float64(nb)
        c = float(c * np.float64(math.sqrt(float(nb * block))))
        all_lags[d] = c
        if abs(c) > abs(best):                            # :722-725 strictly greater
            delay, best = d, c
    return delay, best, all_lags


# ---- constructed inputs with EXACT ties: integer samples, so every sum is exact in any order ------------------------
TIE_LAGS = 2560                                           # ten 256-lag tiles


def tie_pattern(support=2001, n=2001, seed=5):
    """n complex64 samples, the first `support` of them integers in -2..2 per component, the rest +0.0"""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=np.complex64)
    p[:support] = rng.integers(-2, 3, support) + 1j * rng.integers(-2, 3, support)
    return p


def tie_signal(pattern, copies, support=None):
    """zeros of len(pattern) + TIE_LAGS samples with sign * pattern[:support] added at every (offset, sign) of `copies`"""
    support = pattern.size if support is None else support
    s = np.zeros(pattern.size + TIE_LAGS, dtype=np.complex64)
    for off, sign in copies:
        s[off:off + support] += np.complex64(sign) * pattern[:support]
    return s


def tie_cases():
    """[(name, template, signal, tying lags, sign of corr)]: two maximal lags with identical windows under the template.
    200 | 2304 = 9 * 256: the lowest tying lag sits in thread 200 of the first-max kernel, the later one in thread 0.
    0 | 2304 and 0 | 256: both in thread 0 (the 256 case with a 256-sample pattern, so that the copies do not overlap)."""
    dense, short = tie_pattern(), tie_pattern(support=256, seed=6)
    return [
        ("two_copies", dense, tie_signal(dense, [(200, 1), (2304, 1)]), (200, 2304), 1),
        ("first_negated", dense, tie_signal(dense, [(200, -1), (2304, 1)]), (200, 2304), -1),
        ("same_thread_far", dense, tie_signal(dense, [(0, 1), (2304, 1)]), (0, 2304), 1),
        ("same_thread_256", short, tie_signal(short, [(0, 1), (256, 1)], support=256), (0, 256), 1),
    ]
