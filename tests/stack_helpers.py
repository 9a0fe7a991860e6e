"""What the stacked GPU tests (stacks, drift stacks, delay tracks, the closure and the delay-table search) share: byte
comparison, and the exact fixed-point words their numpy models start from."""
import numpy as np


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def windows_q(c):
    """q of every pair-window [W][P][L], word for word"""
    return c.process_stacked(1, 1, 1, want_partial=True)["partial"]


def stacks_q(c, q, m):
    """(Q [n_stacks][P][L], n_w [n_stacks]) of stacks of m windows from the windows' q"""
    from tdoa_amd import stacking
    wpb, _ = c.num_windows()
    _, ids = stacking.stack_ids(wpb, m)
    return np.stack([q[wins].sum(axis=0) for _, wins in ids]), [len(wins) for _, wins in ids]
