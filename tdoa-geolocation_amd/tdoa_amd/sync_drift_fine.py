"""The clock-line refinement of tdoa_process_sync_drift_fine (include/tdoa_mi355x.h, "fine clock lines") in int64 numpy: what
the GPU kernels (csrc/stack_sync_drift_fine.hpp) are held to, byte for byte.  Tests use it; the library does not.

The coarse stage is sync_drift.sync_line and stays what it is: clocks k_s in whole samples, rates h_s in 1/D lag per position.
The refinement works on the lag grid of 1/U sample, U in {2, 4, 8, 16}.  A fine lag lam is inside when |lam| <= (max_lag - 1) U,
and its word is Q_U[lam + (max_lag - 1) U] of that (position, pair) row, Q_U = upsample.upsample(Q, U); an outside term adds 0
and is not counted.  The pair delays are e^U_ij = upsample.fine_lags(ref_delay[j] - ref_delay[i], U).  The unknowns are

    kappa_s = U k_s + y_s in 1/U sample, |y_s| <= U        eta_s = U h_s + g_s in 1/(U D) lag per position, |g_s| <= U

with station 0 the gauge (y_0 = g_0 = 0); the clock at position x is kappa_s(x) = kappa_s + shift(eta_s, x) in 1/U sample,
shift the slope search's rule with the same D, and

    A^U_ij = sum over x of Q_U,x,ij[e^U_ij + kappa_j(x) - kappa_i(x)]        F_U = sum over i < j of |A^U_ij|

is raised by Rf Gauss-Seidel sweeps over stations 1 .. S-1 (there is no placing): station s takes the (g, y) of the largest
sum over i != s of |A^U_pair(i,s)| with the others where they stand.  Candidates compete in the order
r = rank(g) (2 U + 1) + rank(y), rank(x) = 2 |x| - (x > 0), and the first of equal maxima wins.  The window stays centred on
(U k_s, U h_s) in every sweep, so the standing value is always a candidate and F_U never decreases.  start_q is F_U at
y = g = 0; because of the rounding (of e^U and of shift at the finer unit) it is not the coarse line's F."""
import numpy as np

from . import sync as _sync
from . import sync_drift as _line
from . import upsample as _up
from .stacking import Q_ONE, from_fixed
from .sync_fine import CLOCK_UNIT, FACTORS, MAX_FINE_ROUNDS, _check

__all__ = ["FACTORS", "MAX_FINE_ROUNDS", "refine_line", "sync_line_fine", "sync_lines_fine", "line_clock16"]


def _zero(n_pos, S, P):
    return (np.zeros((), dtype=_line.SYNC_LINE_DTYPE), np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32),
            np.zeros((n_pos, S), dtype=np.int32), np.zeros((n_pos, P), dtype=np.int32), np.zeros((n_pos, P), dtype=np.float64))


def refine_line(q, ref_delay, clock, rate, max_lag, drift_den, U, fine_rounds, n_w=1):
    """One line: q [L][P][2 max_lag - 1] int64, ref_delay [S] in 1/16 sample, clock and rate [S] the coarse stage's k and h,
    n_w the windows of a position (a number or one per position) ->
    (record SYNC_LINE_DTYPE, clock16 [S] int32 in 1/16 sample, fine_rate [S] int32, fine_rows [L][S] int32 in 1/16 sample,
    fine_lags [L][P] int32 in 1/U sample, fine_corr [L][P] float64)"""
    U, Rf = _check(U, fine_rounds)
    ml, D = int(max_lag), int(drift_den)
    ref = np.asarray(ref_delay, dtype=np.int64)
    k, h = np.asarray(clock, dtype=np.int64), np.asarray(rate, dtype=np.int64)
    S = len(ref)
    P = S * (S - 1) // 2
    q = np.asarray(q, dtype=np.int64)
    if ref.ndim != 1 or not 2 <= S <= 64 or k.shape != (S,) or h.shape != (S,) or q.ndim != 3 or q.shape[1:] != (P, 2 * ml - 1):
        raise ValueError("ref_delay, clock and rate must be [S], 2 <= S <= 64, and q [L][S (S-1) / 2][2 max_lag - 1]")
    if D < 1:
        raise ValueError("drift_den >= 1")
    n_pos = q.shape[0]
    n = np.broadcast_to(np.asarray(n_w, dtype=np.int64), (n_pos,))
    qu, ml_u = _up.upsample(q, U), (ml - 1) * U + 1
    i, j = np.triu_indices(S, 1)
    e = _up.fine_lags(ref[j] - ref[i], U)
    centre, mid = U * k, U * h
    kappa, eta = centre.copy(), mid.copy()
    ys = _sync.candidates(U)
    start_q = _line.objective(qu, e, kappa, eta, D, ml_u)[0]
    moved = 0
    for _ in range(Rf):
        moved = 0
        for s in range(1, S):
            y, new_eta = _line._place(qu, e, kappa, eta, centre, s, np.array([p for p in range(S) if p != s]), ys, mid[s] + ys, D, ml_u)
            moved += int(centre[s] + y != kappa[s] or new_eta != eta[s])
            kappa[s], eta[s] = centre[s] + y, new_eta
    score_q, terms_in, _, lag, inside = _line.objective(qu, e, kappa, eta, D, ml_u)
    out = _zero(n_pos, S, P)
    if score_q <= 0:
        return out
    rec, clock16, fine_rate, rows, lags, corr = out
    rec["moved"], rec["terms_in"], rec["positions"] = moved, terms_in, n_pos
    rec["score_q"], rec["start_q"] = score_q, start_q
    rec["score"] = from_fixed(score_q, int(n.sum()))
    clock16[:] = (kappa * (CLOCK_UNIT // U)).astype(np.int32)
    fine_rate[:] = eta.astype(np.int32)
    rows[:] = (_line._clocks(kappa, eta, n_pos, D) * (CLOCK_UNIT // U)).astype(np.int32)
    lags[:] = np.where(inside, lag, 0)
    word = qu[np.arange(n_pos)[:, None], np.arange(P)[None, :], np.where(inside, lag + ml_u - 1, 0)]
    corr[:] = np.where(inside, word.astype(np.float64) * (1.0 / Q_ONE) / np.sqrt(n.astype(np.float64))[:, None], 0.0)
    return out


_KEYS = ("line", "clock", "rate", "rows", "lags", "corr", "fine", "clock16", "fine_rate", "fine_rows", "fine_lags", "fine_corr")


def sync_line_fine(q, ref_delay, max_lag, gate=0, max_drift=0, drift_den=1, rounds=0, U=16, fine_rounds=2, centre=None, n_w=1):
    """One line: sync_drift.sync_line, then refine_line on its clocks and rates -> {"line", "clock", "rate", "rows", "lags",
    "corr"} (the coarse stage's) and {"fine", "clock16", "fine_rate", "fine_rows", "fine_lags", "fine_corr"}; a zero coarse
    record gives zero fine outputs"""
    _check(U, fine_rounds)
    coarse = _line.sync_line(q, ref_delay, max_lag, gate, max_drift, drift_den, rounds, centre, n_w)
    if int(coarse[0]["score_q"]) == 0:
        fine = _zero(coarse[3].shape[0], coarse[3].shape[1], coarse[4].shape[1])
    else:
        fine = refine_line(q, ref_delay, coarse[1], coarse[2], max_lag, drift_den, U, fine_rounds, n_w)
    return dict(zip(_KEYS, coarse + fine))


def sync_lines_fine(q, track_len, ref_delay, max_lag, gate=0, max_drift=0, drift_den=1, rounds=0, U=16, fine_rounds=2, centre=None,
                    n_w=1):
    """q [n_sets][P][2 max_lag - 1], set t track_len + j position j of line t -> sync_line_fine's outputs, the per-line ones
    with a leading [n_lines], the per-stack ones [n_sets]; n_w a number or one per set"""
    q = np.asarray(q, dtype=np.int64)
    L = int(track_len)
    if q.ndim != 3 or L < 1 or q.shape[0] % L:
        raise ValueError("q must be [n_sets][P][2 max_lag - 1] and track_len a divisor of n_sets")
    n = np.broadcast_to(np.asarray(n_w, dtype=np.int64), (q.shape[0],))
    out = [sync_line_fine(q[t:t + L], ref_delay, max_lag, gate, max_drift, drift_den, rounds, U, fine_rounds, centre, n[t:t + L])
           for t in range(0, q.shape[0], L)]
    per_line = ("line", "clock", "rate", "fine", "clock16", "fine_rate")
    return {key: (np.stack if key in per_line else np.concatenate)([o[key] for o in out]) for key in _KEYS}


def line_clock16(clock16, fine_rate, U, drift_den, first_position, n_positions):
    """tdoa_sync_line_clock16: the fine line continued over positions first .. first + n - 1 in 1/16 sample,
    clock16[s] + r(16 eta_s x, U D), r(a, b) the nearest integer to a / b, halves away from zero, in integers only.
    clock16, fine_rate [S] -> [n][S] int32, what tdoa_locate_set_clock takes"""
    k, h = np.asarray(clock16, dtype=np.int64), np.asarray(fine_rate, dtype=np.int64)
    U, D, first, n = int(U), int(drift_den), int(first_position), int(n_positions)
    if k.shape != h.shape or k.ndim != 1 or k.shape[0] < 1:
        raise ValueError("clock16 and fine_rate must hold one integer per station")
    if U not in FACTORS or D < 1 or first < 0 or n < 1:
        raise ValueError("U one of 2, 4, 8, 16, drift_den >= 1, first_position >= 0 and n_positions >= 1")
    num = CLOCK_UNIT * h[None, :] * (first + np.arange(n, dtype=np.int64))[:, None]
    den = U * D
    return (k[None, :] + np.sign(num) * ((2 * np.abs(num) + den) // (2 * den))).astype(np.int32)
