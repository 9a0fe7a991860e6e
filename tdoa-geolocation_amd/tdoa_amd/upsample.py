"""Sub-sample locate (tdoa_locate_set_upsample; include/tdoa_mi355x.h, "sub-sample locate") in int64 numpy: what the GPU kernel
(csrc/stack_upsample.hpp) is held to, byte for byte.  Tests use it; the library does not.

A row Q[l], -max_lag < l < max_lag, of n = 2 max_lag - 1 lags becomes n_U = (n - 1) U + 1 words on a lag grid of 1/U sample,
U in {1, 2, 4, 8, 16}; index u stands for lag u / U - (max_lag - 1):

    Q_U[U l + r] = floor((sum over k = 0 .. 15 of h_r[k] Q[l + k - 7]  +  2^14) / 2^15)      r = 0 .. U - 1, Q outside the range = 0
    h_r = H16[r 16 / U],   H16[rho][k] = rint(2^15 sinc(x) kaiser_6(x / 8)),  x = k - 7 - rho / 16

H16 is normative: the literals below are the ones of csrc/stack_upsample.hpp, and nothing computes a tap at run time.  Phase 0
is the delta, so Q_U[U l] = Q[l].  The sum is exact and rounded half up by the floor.

The statement of every search of the delay-table family with U > 1 is the existing numpy function (locate.locate,
locate_multi.locate_multi, locate_track.track_stacks, locate_track_multi.track_multi_stacks) on the arguments of scaled_args:
upsample(q, U), U table, U clock, U guard, max_lag' = (max_lag - 1) U + 1.  The lag rule sgn(d) ((2 |d| + 16) div 32) on
d' = U d is sgn(d) ((2 |d| U + 16) div 32): the nearest 1/U lag, halves away from zero (fine_lags)."""
import numpy as np

FACTORS = (1, 2, 4, 8, 16)
TAPS = 16
BEFORE = 7                  # tap k of a window is the word at lag l + k - 7
SHIFT = 15                  # the taps' scale
SPLIT = 31                  # Q = hi 2^31 + lo

H16 = np.array([
    [0, 0, 0, 0, 0, 0, 0, 32768, 0, 0, 0, 0, 0, 0, 0, 0],
    [-18, 52, -119, 236, -439, 820, -1825, 32552, 2090, -893, 473, -256, 130, -59, 21, -4],
    [-33, 97, -223, 445, -828, 1544, -3360, 31911, 4414, -1828, 964, -522, 267, -122, 45, -10],
    [-44, 133, -308, 620, -1158, 2151, -4593, 30859, 6933, -2773, 1454, -788, 406, -186, 70, -16],
    [-51, 159, -374, 757, -1419, 2629, -5517, 29423, 9600, -3692, 1923, -1043, 540, -250, 95, -23],
    [-55, 176, -419, 855, -1606, 2970, -6136, 27636, 12362, -4544, 2350, -1275, 663, -310, 120, -30],
    [-56, 184, -444, 911, -1717, 3172, -6460, 25543, 15162, -5291, 2714, -1473, 769, -363, 142, -38],
    [-54, 184, -448, 928, -1755, 3237, -6510, 23192, 17942, -5893, 2994, -1625, 852, -406, 162, -45],
    [-50, 176, -435, 907, -1722, 3174, -6311, 20639, 20639, -6311, 3174, -1722, 907, -435, 176, -50],
    [-45, 162, -406, 852, -1625, 2994, -5893, 17942, 23192, -6510, 3237, -1755, 928, -448, 184, -54],
    [-38, 142, -363, 769, -1473, 2714, -5291, 15162, 25543, -6460, 3172, -1717, 911, -444, 184, -56],
    [-30, 120, -310, 663, -1275, 2350, -4544, 12362, 27636, -6136, 2970, -1606, 855, -419, 176, -55],
    [-23, 95, -250, 540, -1043, 1923, -3692, 9600, 29423, -5517, 2629, -1419, 757, -374, 159, -51],
    [-16, 70, -186, 406, -788, 1454, -2773, 6933, 30859, -4593, 2151, -1158, 620, -308, 133, -44],
    [-10, 45, -122, 267, -522, 964, -1828, 4414, 31911, -3360, 1544, -828, 445, -223, 97, -33],
    [-4, 21, -59, 130, -256, 473, -893, 2090, 32552, -1825, 820, -439, 236, -119, 52, -18],
], dtype=np.int32)
H16.setflags(write=False)


def _factor(U):
    U = int(U)
    if U not in FACTORS:
        raise ValueError("U must be one of 1, 2, 4, 8, 16")
    return U


def formula():
    """H16 from its definition in float64 (numpy's sinc and i0): for the tests, which hold the literals to within 1 of it"""
    k, rho = np.arange(TAPS)[None, :], np.arange(16)[:, None]
    x = k - BEFORE - rho / 16.0
    t = x / 8.0
    return 2.0 ** SHIFT * np.sinc(x) * np.i0(6.0 * np.sqrt(np.maximum(0.0, 1.0 - t * t))) / np.i0(6.0)


def taps(U):
    """[U][16] int32: h_r = H16[r 16 / U]"""
    U = _factor(U)
    return H16[::16 // U].copy()


def upsampled_len(n, U):
    return (int(n) - 1) * _factor(U) + 1


def upsample(q, U):
    """q [..., n] int64, |q| <= 2^60 -> [..., (n - 1) U + 1] int64, in split int64 arithmetic: A = sum h hi, B = sum h lo,
    the word is A 2^16 + ((B + 2^14) >> 15)"""
    U = _factor(U)
    q = np.asarray(q, dtype=np.int64)
    if U == 1:
        return q.copy()
    n = q.shape[-1]
    pad = np.zeros(q.shape[:-1] + (n + TAPS - 1,), dtype=np.int64)
    pad[..., BEFORE:BEFORE + n] = q
    hi, lo = pad >> SPLIT, pad & ((1 << SPLIT) - 1)
    out = np.zeros(q.shape[:-1] + (n, U), dtype=np.int64)
    h = taps(U).astype(np.int64)
    for r in range(U):
        a = np.zeros(q.shape, dtype=np.int64)
        b = np.full(q.shape, 1 << (SHIFT - 1), dtype=np.int64)
        for k in range(TAPS):
            a += h[r, k] * hi[..., k:k + n]
            b += h[r, k] * lo[..., k:k + n]
        out[..., r] = a * (1 << (SPLIT - SHIFT)) + (b >> SHIFT)
    return out.reshape(q.shape[:-1] + (n * U,))[..., :(n - 1) * U + 1]


def upsample_exact(row, U):
    """one row in Python integers, straight from the definition (any magnitude): a list of (n - 1) U + 1 integers"""
    U = _factor(U)
    row = [int(v) for v in row]
    n, h = len(row), taps(U).tolist()
    at = lambda l: row[l] if 0 <= l < n else 0
    return [(sum(h[u % U][k] * at(u // U + k - BEFORE) for k in range(TAPS)) + (1 << (SHIFT - 1))) >> SHIFT for u in range((n - 1) * U + 1)]


def fine_lags(d, U):
    """d: table differences in 1/16 sample -> the nearest 1/U lag, sgn(d) ((2 |d| U + 16) div 32), halves away from zero"""
    d = np.asarray(d, dtype=np.int64)
    return np.sign(d) * ((2 * np.abs(d) * _factor(U) + 16) // 32)


def scaled_args(table, clock, guard, max_lag, U):
    """-> (U table int64, U clock or None, U guard, (max_lag - 1) U + 1): what the searches' numpy statements take with
    upsample(q, U)"""
    U = _factor(U)
    t = np.asarray(table, dtype=np.int64) * U
    k = None if clock is None else np.asarray(clock, dtype=np.int64) * U
    return t, k, int(guard) * U, (int(max_lag) - 1) * U + 1
