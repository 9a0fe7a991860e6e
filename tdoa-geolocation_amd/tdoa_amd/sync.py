"""The clock search of tdoa_process_sync (include/tdoa_mi355x.h, "clock search") in int64 numpy: what the GPU kernels
(csrc/stack_sync.hpp) are held to, byte for byte.  Tests use it; the library does not.

A block whose emitter is known gives every pair (i, j), i < j in the library's order, the lag its propagation alone would
have, e_ij = sgn(d) ((2 |d| + 16) div 32) with d = ref_delay[j] - ref_delay[i] in units of 1/16 sample.  What is left of a
pair's peak is the stations' clocks: k_s = centre[s] + x_s samples, |x_s| <= G, x_0 = 0, and

    F(k) = sum over the pairs of M_ij[e_ij + k_j - k_i],   M_p[l] = |Q_p[l]|, a lag outside -max_lag < l < max_lag counting 0

is searched in three phases: a joint start of (x_1, x_2) over the whole square, the placing of stations 3 .. S-1 one after
the other against the stations before them, and R Gauss-Seidel sweeps over stations 1 .. S-1 against all the others.
Candidates are always taken in the order rank(x) = 2 |x| - (x > 0) -- 0, +1, -1, +2, -2 ... -- and the first of equal
maxima wins."""
import numpy as np

from .closure import pair_index
from .locate import DELAY_UNIT, pair_lags
from .stacking import from_fixed

SYNC_DTYPE = np.dtype([("moved", np.int32), ("pairs_in", np.int32), ("score_q", np.int64), ("start_q", np.int64),
                       ("score", np.float64)])      # tdoa_sync

MAX_GATE = 1023
MAX_ROUNDS = 16


def candidates(gate):
    """x in rank order: 0, +1, -1, +2, -2 ... +G, -G"""
    r = np.arange(2 * int(gate) + 1, dtype=np.int64)
    return np.where(r & 1, (r + 1) >> 1, -(r >> 1))


def _m(q, p, lag, ml):
    """M_p at the lags `lag` (any shape), 0 outside the range"""
    lag = np.asarray(lag, dtype=np.int64)
    inside = (lag > -ml) & (lag < ml)
    return np.where(inside, np.abs(q[p][np.where(inside, lag + ml - 1, 0)]), 0)


def objective(q, e, k, ml):
    """(F(k), pairs inside the range, the pairs' lags [P] int64, inside [P] bool)"""
    i, j = np.triu_indices(len(k), 1)                                    # the library's pair order
    lag = e + k[j] - k[i]
    inside = (lag > -ml) & (lag < ml)
    m = np.where(inside, np.abs(q[np.arange(len(lag)), np.where(inside, lag + ml - 1, 0)]), 0)
    return int(m.sum()), int(inside.sum()), lag, inside


def _place(q, e, k, centre, s, partners, xs, ml):
    """x_s: the first largest, in rank order, of the sum over the partners of M at the pair's lag with k_s = centre[s] + x"""
    S = len(k)
    i = np.asarray(partners, dtype=np.int64)
    lo, hi = np.minimum(i, s), np.maximum(i, s)
    p = lo * S - lo * (lo + 1) // 2 + (hi - lo - 1)
    sign = np.where(i < s, 1, -1)                                        # i < s: e_is + k_s - k_i; i > s: e_si + k_i - k_s
    lag = e[p][:, None] + sign[:, None] * ((centre[s] + xs)[None, :] - k[i][:, None])
    inside = (lag > -ml) & (lag < ml)
    total = np.where(inside, np.abs(q[p[:, None], np.where(inside, lag + ml - 1, 0)]), 0).sum(axis=0)
    return int(xs[int(np.argmax(total))])


def sync(q_pairs, ref_delay, max_lag, gate=0, rounds=0, centre=None, n_w=1):
    """One stack: q_pairs [P][2 max_lag - 1] int64 in the library's pair order, ref_delay [S] in units of 1/16 sample ->
    (record SYNC_DTYPE, clock [S] int32 in samples, lags [P] int32, corr [P] float64)"""
    ml, G, R = int(max_lag), int(gate), int(rounds)
    ref = np.asarray(ref_delay, dtype=np.int64)
    if ref.ndim != 1 or not 2 <= len(ref) <= 64:
        raise ValueError("ref_delay must hold one delay for each of 2 .. 64 stations")
    S = len(ref)
    P = S * (S - 1) // 2
    q = np.asarray(q_pairs, dtype=np.int64)
    if q.shape != (P, 2 * ml - 1):
        raise ValueError("q_pairs must be [S (S-1) / 2][2 max_lag - 1]")
    if not 0 <= G <= MAX_GATE or not 0 <= R <= MAX_ROUNDS:
        raise ValueError("gate must be 0 .. 1023 and rounds 0 .. 16")
    c = np.zeros(S, dtype=np.int64) if centre is None else np.asarray(centre, dtype=np.int64)
    if c.shape != (S,):
        raise ValueError("centre must hold one integer per station")
    e = pair_lags(ref[None, :])[0]
    xs = candidates(G)
    k = c.copy()                                                         # x_0 = 0: station 0 is the gauge
    if S == 2:
        k[1] = c[1] + _place(q, e, k, c, 1, [0], xs, ml)
    else:
        k1, k2 = c[1] + xs, c[2] + xs
        total = (_m(q, 0, e[0] + k1 - k[0], ml)[:, None] + _m(q, 1, e[1] + k2 - k[0], ml)[None, :] +
                 _m(q, pair_index(1, 2, S), e[pair_index(1, 2, S)] + k2[None, :] - k1[:, None], ml))
        r1, r2 = np.unravel_index(int(np.argmax(total)), total.shape)    # the first: the smaller rank(x_1), then rank(x_2)
        k[1], k[2] = k1[r1], k2[r2]
        for s in range(3, S):
            k[s] = c[s] + _place(q, e, k, c, s, range(s), xs, ml)
    start_q = objective(q, e, k, ml)[0]
    moved = 0
    for _ in range(R):
        moved = 0
        for s in range(1, S):
            new = c[s] + _place(q, e, k, c, s, [i for i in range(S) if i != s], xs, ml)
            moved += int(new != k[s])
            k[s] = new
    score_q, pairs_in, lag, inside = objective(q, e, k, ml)
    rec = np.zeros((), dtype=SYNC_DTYPE)
    clock, lags, corr = np.zeros(S, dtype=np.int32), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.float64)
    if score_q <= 0:
        return rec, clock, lags, corr
    rec["moved"], rec["pairs_in"], rec["score_q"], rec["start_q"] = moved, pairs_in, score_q, start_q
    rec["score"] = from_fixed(score_q, n_w)
    clock[:] = k.astype(np.int32)
    lags[:] = np.where(inside, lag, 0)
    corr[:] = np.where(inside, from_fixed(q[np.arange(P), np.where(inside, lag + ml - 1, 0)], n_w), 0.0)
    return rec, clock, lags, corr


def sync_stacks(q, ref_delay, max_lag, gate=0, rounds=0, centre=None, n_w=1):
    """q [n_sets][P][2 max_lag - 1] -> (records [n_sets], clock [n_sets][S], lags [n_sets][P], corr [n_sets][P]); n_w a number
    or one per set"""
    q = np.asarray(q, dtype=np.int64)
    n = np.broadcast_to(np.asarray(n_w), (q.shape[0],))
    out = [sync(q[s], ref_delay, max_lag, gate, rounds, centre, int(n[s])) for s in range(q.shape[0])]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def midpoint_clock(clock_before, clock_after):
    """the clock table of the block between two reference blocks, in units of 1/16 sample: 8 (k_before + k_after), the exact
    midpoint of the two blocks' clocks in samples -> int32, the shape of the inputs"""
    a, b = np.asarray(clock_before, dtype=np.int64), np.asarray(clock_after, dtype=np.int64)
    if a.shape != b.shape:
        raise ValueError("the two clock tables must have the same shape")
    return ((DELAY_UNIT // 2) * (a + b)).astype(np.int32)


def ramp_clock(k_before, k_after, n):
    """the clocks of the n positions of the block between two reference blocks, in units of 1/16 sample, linear between the
    centres of the two reference blocks (blocks of equal length, position j's centre (n + 2 j + 1) / (4 n) of the way):

        clock_j = 16 k_before + r(16 (k_after - k_before) (n + 2 j + 1), 4 n)

    r(a, b) the nearest integer to a / b, halves away from zero, in integers only.  k_before, k_after [S] in samples ->
    [n][S] int32; its mean over j is midpoint_clock's value up to the rounding"""
    a, b, n = np.asarray(k_before, dtype=np.int64), np.asarray(k_after, dtype=np.int64), int(n)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("the two clocks must hold one integer per station")
    if n < 1:
        raise ValueError("n must be >= 1")
    num = DELAY_UNIT * (b - a)[None, :] * (n + 2 * np.arange(n, dtype=np.int64) + 1)[:, None]
    return (DELAY_UNIT * a[None, :] + np.sign(num) * ((2 * np.abs(num) + 4 * n) // (8 * n))).astype(np.int32)
