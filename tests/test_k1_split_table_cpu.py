"""CPU: the split half-plane angle table of the fused column kernels (csrc/k1_discriminator.hpp, k1_split_angle2) as the
library's host code builds it (tdoa_debug_k1_split_table: no device needed).

A numpy model of the kernels' look-up runs on the library's two arrays for all 65 536 byte pairs -- reflect the sample where
Q < 0, index both arrays with the reflected 16-bit word, combine hi << 16 | lo << 8, add the half turn of a reflected sample
as bit 31 -- and must give the oracle's angle code ob_angle_code(I, Q) modulo 2^24 (the kernels' angles are scaled by 256,
modulo 2^32)."""
import numpy as np


def _tables():
    import tdoa_amd
    return tdoa_amd.capi.k1_split_table()


def test_every_byte_pair_looks_up_the_oracles_angle(oracle):
    hi, lo = _tables()
    word = np.arange(65536, dtype=np.uint32)                      # b_I | b_Q << 8
    b_i, b_q = word & 0xff, word >> 8
    pm = np.where(b_q < 128, 0xffff, 0).astype(np.uint32)         # reflect: Q = 2 b_Q - 255 < 0
    fw = word ^ pm
    assert (fw >= 0x8000).all()                                   # so word + 0x8000 / 2 word + 0x8000 are the LDS addresses
    lo_addr, hi_addr = fw + 0x8000, 2 * fw + 0x8000               # lo at 0x10000, hi at 0x18000
    assert lo_addr.min() == 0x10000 and lo_addr.max() == 0x17fff and hi_addr.min() == 0x18000 and hi_addr.max() == 0x27ffe
    h, l = hi[(hi_addr - 0x18000) // 2].astype(np.uint64), lo[lo_addr - 0x10000].astype(np.uint64)
    scaled = (h << 16 | l << 8 | (pm.astype(np.uint64) & 1) << 31) & 0xffffffff
    assert (scaled & 0xff == 0).all()
    got = (scaled >> 8).astype(np.int64)
    want = np.array([oracle.b_angle_code(2 * int(i) - 255, 2 * int(q) - 255) for i, q in zip(b_i, b_q)], dtype=np.int64) % (1 << 24)
    assert np.array_equal(got, want)


def test_parts_are_in_range_and_no_entry_is_zero():
    hi, lo = _tables()
    assert hi.dtype == np.uint16 and lo.dtype == np.uint8 and hi.shape == lo.shape == (32768,)
    assert (hi < (1 << 15)).all()                                 # bit 31 of the scaled angle is free for the half turn
    assert ((hi.astype(np.uint32) << 8 | lo) != 0).all()          # Q > 0: 0 < angle < half a turn
