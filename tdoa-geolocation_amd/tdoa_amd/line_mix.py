"""The line mix of tdoa_process_sync_drift_locate (include/tdoa_mi355x.h, "free-running clocks to fix in one call") in int64
numpy: what the GPU kernel (csrc/stack_line_mix.hpp) and tdoa_line_mix_rows are held to, byte for byte.  Tests use it; the
library does not.

clock16, fine_rate [n_lines][S] are the fine clock lines' offsets (1/16 sample) and rates (1/(U drift_den) lag per position).  A
mix is [m][6] int32, one (a, xa, b, xb, wa, wb) per row:

    cont(l, x) = clock16[l] + r(16 fine_rate[l] x, U drift_den)       row = clock_mix's mean of cont(a, xa), cont(b, xb) by wa, wb

r the nearest integer, halves away from zero: sync_drift_fine.line_clock16's rule with x of either sign, and clock_mix.mix_rows'
mean.  (l, x, l, x, 1, 0) is line l continued to x."""
import numpy as np

from .clock_mix import MAX_DEN, pair_differences  # noqa: F401  (the differences are the clock mix's)

MAX_X = 65535
FACTORS = (2, 4, 8, 16)
CLOCK_UNIT = 16
MIX_DTYPE = np.dtype([("a", np.int32), ("xa", np.int32), ("b", np.int32), ("xb", np.int32), ("wa", np.int32), ("wb", np.int32)])   # tdoa_line_mix


def as_mix(mix, n_lines):
    """a mix as [m][6] int64, checked as the library checks it against n_lines lines"""
    m = np.asarray(mix)
    if m.dtype == MIX_DTYPE:
        m = np.stack([m[k] for k in MIX_DTYPE.names], axis=-1)
    m = np.asarray(m, dtype=np.int64)
    if m.ndim != 2 or m.shape[1] != 6 or len(m) < 1:
        raise ValueError("mix must be [m][6]: a, xa, b, xb, wa, wb")
    lines, x, w = m[:, [0, 2]], m[:, [1, 3]], m[:, 4:]
    den = w.sum(axis=1)
    if ((lines < 0).any() or (lines >= int(n_lines)).any() or (np.abs(x) > MAX_X).any() or (w < 0).any() or (den < 1).any() or
            (den > MAX_DEN).any()):
        raise ValueError("a, b must be 0 .. n_lines - 1, |xa|, |xb| <= 65535, wa, wb >= 0 and 1 <= wa + wb <= 65536")
    return m


def continued(clock16, fine_rate, x, U, drift_den):
    """clock16, fine_rate [...] int, x [...] -> clock16 + r(16 fine_rate x, U drift_den), int64"""
    num = CLOCK_UNIT * np.asarray(fine_rate, dtype=np.int64) * np.asarray(x, dtype=np.int64)
    den = int(U) * int(drift_den)
    return np.asarray(clock16, dtype=np.int64) + np.sign(num) * ((2 * np.abs(num) + den) // (2 * den))


def mix_rows(clock16, fine_rate, U, drift_den, mix):
    """clock16, fine_rate [n_lines][S], mix [m][6] -> rows [m][S] int32"""
    c, h = np.asarray(clock16, dtype=np.int64), np.asarray(fine_rate, dtype=np.int64)
    if c.ndim != 2 or c.shape != h.shape:
        raise ValueError("clock16 and fine_rate must be [n_lines][S]")
    if int(U) not in FACTORS or int(drift_den) < 1:
        raise ValueError("U one of 2, 4, 8, 16 and drift_den >= 1")
    m = as_mix(mix, len(c))
    ca = continued(c[m[:, 0]], h[m[:, 0]], m[:, 1, None], U, drift_den)
    cb = continued(c[m[:, 2]], h[m[:, 2]], m[:, 3, None], U, drift_den)
    if max(np.abs(ca).max(), np.abs(cb).max()) > 2 ** 31 - 1:
        raise ValueError("a continued clock does not fit int32")
    den = (m[:, 4] + m[:, 5])[:, None]
    t = m[:, 4, None] * ca + m[:, 5, None] * cb
    return (np.sign(t) * ((2 * np.abs(t) + den) // (2 * den))).astype(np.int32)


def own_mix(n_lines, L):
    """n_lines lines of L stacks, every stack its own line at its own position: what mix = None means"""
    n_lines, L = int(n_lines), int(L)
    if n_lines < 1 or L < 1:
        raise ValueError("n_lines and L must be >= 1")
    line, x = np.divmod(np.arange(n_lines * L, dtype=np.int32), np.int32(L))
    return np.stack([line, x, line, x, np.ones_like(x), np.zeros_like(x)], axis=1)


def forward_mix(L):
    """[reference | target | reference] blocks of L stacks: blocks 0 and 2 their own entries, stack j of block 1 the line of
    block 0 continued to L + j"""
    m = own_mix(3, L)
    x = int(L) + np.arange(int(L), dtype=np.int32)
    z = np.zeros_like(x)
    m[int(L):2 * int(L)] = np.stack([z, x, z, x, z + 1, z], axis=1)
    return m


def bridge_mix(L):
    """[reference | target | reference] blocks of L stacks: blocks 0 and 2 their own entries, stack j of block 1 the line of
    block 0 continued forwards to L + j and the line of block 2 continued backwards to j - L, weighted by nearness: L - j and
    j + 1"""
    m = own_mix(3, L)
    L = int(L)
    j = np.arange(L, dtype=np.int32)
    m[L:2 * L] = np.stack([0 * j, L + j, 0 * j + 2, j - L, L - j, j + 1], axis=1)
    return m
