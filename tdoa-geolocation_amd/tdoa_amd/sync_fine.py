"""The clock refinement of tdoa_process_sync_fine (include/tdoa_mi355x.h, "fine clock search") in int64 numpy: what the GPU
kernel (csrc/stack_sync_fine.hpp) is held to, byte for byte.  Tests use it; the library does not.

The coarse stage is sync.sync and stays what it is: clocks k_s in whole samples.  The refinement works on the lag grid of
1/U sample, U in {2, 4, 8, 16}.  A fine lag lam is inside when |lam| <= (max_lag - 1) U, and its word is
Q_U[lam + (max_lag - 1) U] of the pair's row, Q_U = upsample.upsample(Q, U); M_p(lam) is the word's magnitude, an outside lag
adds 0 and is not counted.  The pair delays are e^U_ij = upsample.fine_lags(ref_delay[j] - ref_delay[i], U), the upsampled
locate's lag rule.  The unknowns are kappa_s = U k_s + y_s, |y_s| <= U, y_0 = 0, and

    F_U(kappa) = sum over i < j of M_ij(e^U_ij + kappa_j - kappa_i)

is raised by Rf Gauss-Seidel sweeps over stations 1 .. S-1: station s takes the y of the largest sum over its S - 1 partners
with the others where they stand.  Candidates compete in the order rank(y) = 2 |y| - (y > 0) and the first of equal maxima
wins.  The window stays centred on U k_s in every sweep, so the standing value is always a candidate and F_U never
decreases."""
import numpy as np

from . import sync as _sync
from . import upsample as _up
from .stacking import from_fixed

FACTORS = (2, 4, 8, 16)
MAX_FINE_ROUNDS = 16
CLOCK_UNIT = 16             # clock16 is in 1/16 sample: tdoa_locate_set_clock's unit


def _check(U, fine_rounds):
    U, Rf = int(U), int(fine_rounds)
    if U not in FACTORS:
        raise ValueError("U must be one of 2, 4, 8, 16")
    if not 0 <= Rf <= MAX_FINE_ROUNDS:
        raise ValueError("fine_rounds must be 0 .. 16")
    return U, Rf


def sweep(qu, e, kappa, centre, ml_u, U):
    """one Gauss-Seidel sweep over stations 1 .. S-1 on the upsampled rows qu, in place on kappa -> the stations it changed"""
    S, ys, moved = len(kappa), _sync.candidates(U), 0
    for s in range(1, S):
        new = centre[s] + _sync._place(qu, e, kappa, centre, s, [i for i in range(S) if i != s], ys, ml_u)
        moved += int(new != kappa[s])
        kappa[s] = new
    return moved


def refine(q_pairs, ref_delay, clock, max_lag, U, fine_rounds, n_w=1):
    """One stack: q_pairs [P][2 max_lag - 1] int64, ref_delay [S] in 1/16 sample, clock [S] the coarse stage's k in samples ->
    (record SYNC_DTYPE, clock16 [S] int32 in 1/16 sample, lags [P] int32 in 1/U sample, corr [P] float64)"""
    U, Rf = _check(U, fine_rounds)
    ml = int(max_lag)
    ref, k = np.asarray(ref_delay, dtype=np.int64), np.asarray(clock, dtype=np.int64)
    S = len(ref)
    P = S * (S - 1) // 2
    q = np.asarray(q_pairs, dtype=np.int64)
    if ref.ndim != 1 or not 2 <= S <= 64 or k.shape != (S,) or q.shape != (P, 2 * ml - 1):
        raise ValueError("ref_delay and clock must be [S], 2 <= S <= 64, and q_pairs [S (S-1) / 2][2 max_lag - 1]")
    qu, ml_u = _up.upsample(q, U), (ml - 1) * U + 1
    i, j = np.triu_indices(S, 1)
    e = _up.fine_lags(ref[j] - ref[i], U)
    centre = U * k
    kappa = centre.copy()
    start_q = _sync.objective(qu, e, kappa, ml_u)[0]
    moved = 0
    for _ in range(Rf):
        moved = sweep(qu, e, kappa, centre, ml_u, U)
    score_q, pairs_in, lag, inside = _sync.objective(qu, e, kappa, ml_u)
    rec = np.zeros((), dtype=_sync.SYNC_DTYPE)
    clock16, lags, corr = np.zeros(S, dtype=np.int32), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.float64)
    if score_q <= 0:
        return rec, clock16, lags, corr
    rec["moved"], rec["pairs_in"], rec["score_q"], rec["start_q"] = moved, pairs_in, score_q, start_q
    rec["score"] = from_fixed(score_q, n_w)
    clock16[:] = (kappa * (CLOCK_UNIT // U)).astype(np.int32)
    lags[:] = np.where(inside, lag, 0)
    corr[:] = np.where(inside, from_fixed(qu[np.arange(P), np.where(inside, lag + ml_u - 1, 0)], n_w), 0.0)
    return rec, clock16, lags, corr


def sync_fine(q_pairs, ref_delay, max_lag, gate=0, rounds=0, U=16, fine_rounds=2, centre=None, n_w=1):
    """One stack: sync.sync, then refine on its clocks -> {"sync", "clock", "lags", "corr"} (the coarse stage's) and {"fine",
    "clock16", "fine_lags", "fine_corr"}; a zero coarse record gives zero fine outputs"""
    _check(U, fine_rounds)
    rec, clock, lags, corr = _sync.sync(q_pairs, ref_delay, max_lag, gate, rounds, centre, n_w)
    out = {"sync": rec, "clock": clock, "lags": lags, "corr": corr}
    if int(rec["score_q"]) == 0:
        S, P = len(clock), len(lags)
        fine = (np.zeros((), dtype=_sync.SYNC_DTYPE), np.zeros(S, dtype=np.int32), np.zeros(P, dtype=np.int32),
                np.zeros(P, dtype=np.float64))
    else:
        fine = refine(q_pairs, ref_delay, clock, max_lag, U, fine_rounds, n_w)
    out["fine"], out["clock16"], out["fine_lags"], out["fine_corr"] = fine
    return out


def sync_fine_stacks(q, ref_delay, max_lag, gate=0, rounds=0, U=16, fine_rounds=2, centre=None, n_w=1):
    """q [n_sets][P][2 max_lag - 1] -> sync_fine's outputs with a leading [n_sets]; n_w a number or one per set"""
    q = np.asarray(q, dtype=np.int64)
    n = np.broadcast_to(np.asarray(n_w), (q.shape[0],))
    out = [sync_fine(q[s], ref_delay, max_lag, gate, rounds, U, fine_rounds, centre, int(n[s])) for s in range(q.shape[0])]
    return {key: np.stack([o[key] for o in out]) for key in out[0]}


def midpoint_clock16(a16, b16):
    """the clock row of the target block between two refined reference blocks, in 1/16 sample: the nearest integer to
    (a + b) / 2, halves away from zero -> int32, the shape of the inputs"""
    a, b = np.asarray(a16, dtype=np.int64), np.asarray(b16, dtype=np.int64)
    if a.shape != b.shape:
        raise ValueError("the two clock rows must have the same shape")
    t = a + b
    return (np.sign(t) * ((np.abs(t) + 1) // 2)).astype(np.int32)
