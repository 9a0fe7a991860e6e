"""The clock mix of tdoa_process_sync_locate (include/tdoa_mi355x.h, "clocks to fix in one call") in int64 numpy: what the GPU
kernel (csrc/stack_line_mix.hpp) and tdoa_clock_mix_rows are held to, byte for byte.  Tests use it; the library does not.

clock16 [n][S] are the fine clock search's clocks in 1/16 sample.  A mix is [m][4] int32, one (a, b, wa, wb) per row:

    den = wa + wb,  T = wa clock16[a] + wb clock16[b],  row = sgn(T) ((2 |T| + den) // (2 den))

the nearest integer to T / den, halves away from zero.  (t, t, 1, 0) is a stack's own clock and (a, b, 1, 1) is
sync_fine.midpoint_clock16(clock16[a], clock16[b]).  The sum is rounded, not an increment, so a ramp made of this is not
sync.ramp_clock's on exact halves of opposite sign."""
import numpy as np

MAX_DEN = 65536
MIX_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("wa", np.int32), ("wb", np.int32)])        # tdoa_clock_mix


def as_mix(mix, n):
    """a mix as [m][4] int64, checked as the library checks it against n stacks"""
    m = np.asarray(mix)
    if m.dtype == MIX_DTYPE:
        m = np.stack([m[k] for k in MIX_DTYPE.names], axis=-1)
    m = np.asarray(m, dtype=np.int64)
    if m.ndim != 2 or m.shape[1] != 4 or len(m) < 1:
        raise ValueError("mix must be [m][4]: a, b, wa, wb")
    den = m[:, 2] + m[:, 3]
    if (m[:, :2] < 0).any() or (m[:, :2] >= int(n)).any() or (m[:, 2:] < 0).any() or (den < 1).any() or (den > MAX_DEN).any():
        raise ValueError("a, b must be 0 .. n - 1, wa, wb >= 0 and 1 <= wa + wb <= 65536")
    return m


def mix_rows(clock16, mix):
    """clock16 [n][S], mix [m][4] -> rows [m][S] int32"""
    c = np.asarray(clock16, dtype=np.int64)
    if c.ndim != 2:
        raise ValueError("clock16 must be [n][S]")
    m = as_mix(mix, len(c))
    den = (m[:, 2] + m[:, 3])[:, None]
    t = m[:, 2, None] * c[m[:, 0]] + m[:, 3, None] * c[m[:, 1]]
    return (np.sign(t) * ((2 * np.abs(t) + den) // (2 * den))).astype(np.int32)


def pair_differences(rows):
    """rows [m][S] -> [m][P] int64: row[j] - row[i] over i < j, i first: what tdoa_locate_set_clock makes of a clock table"""
    r = np.asarray(rows, dtype=np.int64)
    i, j = np.triu_indices(r.shape[1], 1)
    return r[:, j] - r[:, i]


def own_mix(n):
    """every one of n stacks its own clock"""
    t = np.arange(int(n), dtype=np.int32)
    return np.stack([t, t, np.ones_like(t), np.zeros_like(t)], axis=1)


def midpoint_mix(stacks_per_block):
    """[reference | target | reference] blocks of stacks_per_block stacks: blocks 1 and 3 their own rows, stack j of block 2 the
    (1, 1) mix of stack j of blocks 1 and 3"""
    L = int(stacks_per_block)
    if L < 1:
        raise ValueError("stacks_per_block must be >= 1")
    m = own_mix(3 * L)
    j = np.arange(L, dtype=np.int32)
    m[L:2 * L] = np.stack([j, 2 * L + j, np.ones_like(j), np.ones_like(j)], axis=1)
    return m
