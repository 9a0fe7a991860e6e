"""The clock-line search of tdoa_process_sync_drift (include/tdoa_mi355x.h, "clock lines") in int64 numpy: what the GPU
kernels (csrc/stack_sync_drift.hpp) are held to, byte for byte.  Tests use it; the library does not.

A line is one block; its positions j = 0 .. L-1 are the block's stacks in order.  Station s has the clock
k_s(j) = k_s + shift(h_s, j) at position j, k_s = centre[s] + x_s with |x_s| <= G and a slope of h_s / D lags per position,
|h_s| <= H, shift(h, j) = sgn(h) ((2 |h| j + D) div (2 D)); station 0 is the gauge (x_0 = h_0 = 0).  The signed words are
summed along the line,

    A_ij = sum over j of Q_{j,ij}[e_ij + k_j(j) - k_i(j)],     F = sum over the pairs of |A_ij|,

a term outside -max_lag < lag < max_lag adding 0.  Stations 1 .. S-1 are placed one after the other against the stations
before them, then R Gauss-Seidel sweeps run over stations 1 .. S-1 against all the others.  A station's candidates (h, x)
are taken in the order r = rank(h) (2 G + 1) + rank(x), rank(x) = 2 |x| - (x > 0), and the first of equal maxima wins."""
import numpy as np

from .locate import DELAY_UNIT, pair_lags
from .stacking import Q_ONE, from_fixed
from .sync import MAX_GATE, MAX_ROUNDS, candidates

SYNC_LINE_DTYPE = np.dtype([("moved", np.int32), ("terms_in", np.int32), ("positions", np.int32), ("reserved", np.int32),
                            ("score_q", np.int64), ("start_q", np.int64), ("score", np.float64)])      # tdoa_sync_line

MAX_DRIFT = 512


def shift(h, j, den):
    """sgn(h) ((2 |h| j + D) div (2 D)) for integer arrays h and j: the nearest integer to h j / D, halves away from zero"""
    h, j, d = np.asarray(h, dtype=np.int64), np.asarray(j, dtype=np.int64), int(den)
    return np.sign(h) * ((2 * np.abs(h) * j + d) // (2 * d))


def _clocks(k, h, n_pos, den):
    """k_s(j): [L][S]"""
    return k[None, :] + shift(h[None, :], np.arange(n_pos, dtype=np.int64)[:, None], den)


def objective(q, e, k, h, den, ml):
    """(F, terms inside the range, A [P], the lags [L][P] int64, inside [L][P] bool) at the clocks k and the slopes h"""
    n_pos, S = q.shape[0], len(k)
    i, j = np.triu_indices(S, 1)                                         # the library's pair order
    kj = _clocks(k, h, n_pos, den)
    lag = e[None, :] + kj[:, j] - kj[:, i]
    inside = (lag > -ml) & (lag < ml)
    w = np.where(inside, q[np.arange(n_pos)[:, None], np.arange(len(e))[None, :], np.where(inside, lag + ml - 1, 0)], 0)
    a = w.sum(axis=0)
    return int(np.abs(a).sum()), int(inside.sum()), a, lag, inside


def _place(q, e, k, h, centre, s, partners, xs, hs, den, ml):
    """(x_s, h_s): the first largest, in the candidates' order, of the sum over the partners of |A| with station s on the
    candidate's line and the partners where they are"""
    n_pos, S = q.shape[0], len(k)
    i = np.asarray(partners, dtype=np.int64)
    lo, hi = np.minimum(i, s), np.maximum(i, s)
    p = lo * S - lo * (lo + 1) // 2 + (hi - lo - 1)
    sign = np.where(i < s, 1, -1)                                        # i < s: e_is + k_s(j) - k_i(j); i > s: e_si + k_i(j) - k_s(j)
    pos = np.arange(n_pos, dtype=np.int64)
    mine = (centre[s] + xs)[None, None, :] + shift(hs[None, :, None], pos[:, None, None], den)          # [L][V][W]
    theirs = _clocks(k, h, n_pos, den)[:, i]                                                             # [L][partners]
    lag = e[p][None, :, None, None] + sign[None, :, None, None] * (mine[:, None, :, :] - theirs[:, :, None, None])
    inside = (lag > -ml) & (lag < ml)
    w = np.where(inside, q[pos[:, None, None, None], p[None, :, None, None], np.where(inside, lag + ml - 1, 0)], 0)
    total = np.abs(w.sum(axis=0)).sum(axis=0)                            # [V][W], rank(h) major: the candidates' order
    r = int(np.argmax(total))
    return int(xs[r % len(xs)]), int(hs[r // len(xs)])


def sync_line(q, ref_delay, max_lag, gate=0, max_drift=0, drift_den=1, rounds=0, centre=None, n_w=1):
    """One line: q [L][P][2 max_lag - 1] int64, position j's pairs in the library's order; ref_delay [S] in units of 1/16
    sample; n_w the windows of a position, a number or one per position ->
    (record SYNC_LINE_DTYPE, clock [S] int32 in samples, rate [S] int32, rows [L][S] int32 = 16 k_s(j), lags [L][P] int32,
    corr [L][P] float64)"""
    ml, G, H, D, R = int(max_lag), int(gate), int(max_drift), int(drift_den), int(rounds)
    ref = np.asarray(ref_delay, dtype=np.int64)
    if ref.ndim != 1 or not 2 <= len(ref) <= 64:
        raise ValueError("ref_delay must hold one delay for each of 2 .. 64 stations")
    S = len(ref)
    P = S * (S - 1) // 2
    q = np.asarray(q, dtype=np.int64)
    if q.ndim != 3 or q.shape[0] < 1 or q.shape[1:] != (P, 2 * ml - 1):
        raise ValueError("q must be [L][S (S-1) / 2][2 max_lag - 1]")
    if not 0 <= G <= MAX_GATE or not 0 <= R <= MAX_ROUNDS or not 0 <= H <= MAX_DRIFT or D < 1:
        raise ValueError("gate must be 0 .. 1023, rounds 0 .. 16, max_drift 0 .. 512 and drift_den >= 1")
    c = np.zeros(S, dtype=np.int64) if centre is None else np.asarray(centre, dtype=np.int64)
    if c.shape != (S,):
        raise ValueError("centre must hold one integer per station")
    n_pos = q.shape[0]
    n = np.broadcast_to(np.asarray(n_w, dtype=np.int64), (n_pos,))
    e = pair_lags(ref[None, :])[0]
    xs, hs = candidates(G), candidates(H)
    k, h = c.copy(), np.zeros(S, dtype=np.int64)                         # station 0 is the gauge
    for s in range(1, S):
        x, h[s] = _place(q, e, k, h, c, s, np.arange(s), xs, hs, D, ml)
        k[s] = c[s] + x
    start_q = objective(q, e, k, h, D, ml)[0]
    moved = 0
    for _ in range(R):
        moved = 0
        for s in range(1, S):
            x, hn = _place(q, e, k, h, c, s, np.array([i for i in range(S) if i != s]), xs, hs, D, ml)
            moved += int(c[s] + x != k[s] or hn != h[s])
            k[s], h[s] = c[s] + x, hn
    score_q, terms_in, _, lag, inside = objective(q, e, k, h, D, ml)
    rec = np.zeros((), dtype=SYNC_LINE_DTYPE)
    clock, rate = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
    rows = np.zeros((n_pos, S), dtype=np.int32)
    lags, corr = np.zeros((n_pos, P), dtype=np.int32), np.zeros((n_pos, P), dtype=np.float64)
    if score_q <= 0:
        return rec, clock, rate, rows, lags, corr
    rec["moved"], rec["terms_in"], rec["positions"] = moved, terms_in, n_pos
    rec["score_q"], rec["start_q"] = score_q, start_q
    rec["score"] = from_fixed(score_q, int(n.sum()))
    clock[:], rate[:] = k.astype(np.int32), h.astype(np.int32)
    rows[:] = (DELAY_UNIT * _clocks(k, h, n_pos, D)).astype(np.int32)
    lags[:] = np.where(inside, lag, 0)
    word = q[np.arange(n_pos)[:, None], np.arange(P)[None, :], np.where(inside, lag + ml - 1, 0)]
    corr[:] = np.where(inside, word.astype(np.float64) * (1.0 / Q_ONE) / np.sqrt(n.astype(np.float64))[:, None], 0.0)      # from_fixed, per position
    return rec, clock, rate, rows, lags, corr


def sync_lines(q, track_len, ref_delay, max_lag, gate=0, max_drift=0, drift_den=1, rounds=0, centre=None, n_w=1):
    """q [n_sets][P][2 max_lag - 1], set t track_len + j position j of line t -> (records [n_lines], clock [n_lines][S],
    rate [n_lines][S], rows [n_sets][S], lags [n_sets][P], corr [n_sets][P]); n_w a number or one per set"""
    q = np.asarray(q, dtype=np.int64)
    L = int(track_len)
    if q.ndim != 3 or L < 1 or q.shape[0] % L:
        raise ValueError("q must be [n_sets][P][2 max_lag - 1] and track_len a divisor of n_sets")
    n = np.broadcast_to(np.asarray(n_w, dtype=np.int64), (q.shape[0],))
    out = [sync_line(q[t:t + L], ref_delay, max_lag, gate, max_drift, drift_den, rounds, centre, n[t:t + L])
           for t in range(0, q.shape[0], L)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3)) + tuple(np.concatenate([o[i] for o in out]) for i in range(3, 6))


def line_clock(clock, rate, drift_den, first_position, n_positions):
    """tdoa_sync_line_clock: the line continued over positions first .. first + n - 1 at the table's 1/16 sample,
    16 k_s + r(16 h_s j, D), r(a, b) the nearest integer to a / b, halves away from zero, in integers only.  clock, rate [S]
    -> [n][S] int32, what tdoa_locate_set_clock takes.  Blocks that follow one another without a gap are assumed"""
    k, h = np.asarray(clock, dtype=np.int64), np.asarray(rate, dtype=np.int64)
    D, first, n = int(drift_den), int(first_position), int(n_positions)
    if k.shape != h.shape or k.ndim != 1:
        raise ValueError("clock and rate must hold one integer per station")
    if D < 1 or first < 0 or n < 1:
        raise ValueError("drift_den >= 1, first_position >= 0 and n_positions >= 1")
    num = DELAY_UNIT * h[None, :] * (first + np.arange(n, dtype=np.int64))[:, None]
    return (DELAY_UNIT * k[None, :] + np.sign(num) * ((2 * np.abs(num) + D) // (2 * D))).astype(np.int32)
