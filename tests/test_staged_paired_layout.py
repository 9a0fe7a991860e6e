"""CPU: the paired block layout of the staged column walk's spectra (stg_paired_at, csrc/dec_staged.hpp) as the library's own
map gives it (tdoa_debug_stg_paired_index: host only, no device needed).

U[cb (32)][k2 (N2)][128]: line [cb][k2] is the KB the LDS ring holds for a station and row -- the 64 columns of block cb of row
k2, then the 64 columns 4032 - 64 cb .. 4095 - 64 cb of the partner row (N2 - k2) mod N2, ascending.  The row pass, both loaders
and the walk's row-0 reads all go through this one map."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    return tdoa_amd.capi


@pytest.fixture(scope="module", params=[256, 512])
def table(request, capi):
    """(N2, index of every (row, column))"""
    n2 = request.param
    L = capi.load()
    idx = np.array([[L.tdoa_debug_stg_paired_index(n2, r, c) for c in range(4096)] for r in range(n2)], dtype=np.int64)
    idx.setflags(write=False)
    return n2, idx


def test_the_map_is_a_bijection_onto_the_spectrum(table):
    n2, idx = table
    assert idx.min() == 0 and idx.max() == 4096 * n2 - 1
    assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(4096 * n2))


def test_a_line_holds_a_rows_block_and_its_partner_rows_mirror_block(table):
    n2, idx = table
    inv = np.empty((4096 * n2, 2), dtype=np.int64)          # element index -> (row, column)
    rows, cols = np.meshgrid(np.arange(n2), np.arange(4096), indexing="ij")
    inv[idx.reshape(-1), 0] = rows.reshape(-1)
    inv[idx.reshape(-1), 1] = cols.reshape(-1)
    lines = inv.reshape(32, n2, 128, 2)
    for cb in range(32):
        for k2 in range(n2):
            fwd, par = lines[cb, k2, :64], lines[cb, k2, 64:]
            assert (fwd[:, 0] == k2).all() and np.array_equal(fwd[:, 1], np.arange(64 * cb, 64 * cb + 64))
            assert (par[:, 0] == (n2 - k2) % n2).all() and np.array_equal(par[:, 1], np.arange(4032 - 64 * cb, 4096 - 64 * cb))


def test_rows_0_and_half_pair_with_themselves(table):
    n2, idx = table
    for r in (0, n2 // 2):
        assert np.array_equal(np.unique(idx[r] // 128 % n2), [r])          # every column of the row lies in lines [.][r]
    for r in range(1, n2 // 2):                                            # every other row: forward in [.][r], partner in [.][N2 - r]
        assert np.array_equal(np.unique(idx[r, :2048] // 128 % n2), [r])
        assert np.array_equal(np.unique(idx[r, 2048:] // 128 % n2), [n2 - r])


def test_the_python_wrapper_and_the_argument_checks(capi):
    assert capi.stg_paired_index(256, 0, 0) == 0 and capi.stg_paired_index(256, 0, 4095) == 127
    assert capi.stg_paired_index(512, 511, 64) == (1 * 512 + 511) * 128
    L = capi.load()
    for bad in ((128, 0, 0), (256, 256, 0), (256, -1, 0), (512, 0, 4096), (512, 0, -1)):
        assert L.tdoa_debug_stg_paired_index(*bad) == -1
        with pytest.raises(ValueError):
            capi.stg_paired_index(*bad)
