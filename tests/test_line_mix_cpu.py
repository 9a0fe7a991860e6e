"""CPU: the line mix of tdoa_process_sync_drift_locate (include/tdoa_mi355x.h, "free-running clocks to fix in one call").

1. line_mix.mix_rows against fractions.Fraction, halves away from zero, on the corners -- x of both signs, 0 and +-65535, exact
   halves of both signs in the continuation and in the mean, wb = 0, wa = 0, den = 65536, rates of both signs up to 16 x 513,
   U in {2, 4, 8, 16}, D in {1, 4, 7} and 16 (the one with halves at every U) -- and a few thousand random entries;
2. (l, x, l, x, 1, 0) with x >= 0 is tdoa_sync_line_clock16 / sync_drift_fine.line_clock16 byte for byte, and with both rates
   zero the rule is clock_mix.mix_rows;
3. tdoa_line_mix_rows (host only) returns mix_rows' bytes and refuses what the header says;
4. forward_mix(L) reproduces the clock table tests/test_gpu_sync_drift_fine.py's CLI test and tdoa_processor build by hand;
5. the chain's statement (tdoa_amd.sync_drift_locate) on the measured case of tests/test_sync_drift_fine_cpu.py is the three
   statements called one after another; under forward_mix the target block's fix has that case's medians, and the medians under
   bridge_mix (a reference block after the target, from the same generators) are printed beside them;
6. the entries are declared, bound and exported; the record states the header's order.
corner_cases() is shared with tests/test_gpu_sync_drift_locate.py, which runs the kernel on the same words."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from test_locate_cpu import FS, GRID, ST4
from test_locate_upsample_cpu import ML, coarse_table
from test_sync_drift_fine_cpu import (KEYS as LINE_KEYS, LINE, M_POS, _prototypes, _quarter_window, block_fix_metres, float64_words,
                                      reference_windows_iq, slide4, target_windows_iq, true_rows16)
from test_sync_fine_cpu import CLOCK4, measured_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdoa_process_sync_drift_locate", "tdoa_group_process_sync_drift_locate", "tdoa_debug_sync_drift_locate_from_q",
         "tdoa_line_mix_rows", "tdoa_debug_line_mix")
TRACK_KEYS = ("track", "cells", "own", "loc_lags", "loc_corr", "total", "ztrack", "zcells", "zown", "zlags", "zcorr", "zmap", "ztotal")
KEYS = tuple(LINE_KEYS) + ("mix_rows",) + TRACK_KEYS
MAX_RATE = 16 * 513             # |fine_rate| <= U (max_drift + 1) at U = 16, max_drift = 512
FORWARD_MEDIAN_M = 81.6         # tests/test_sync_drift_fine_cpu.py: the median fix under the fine line continued, twelve blocks


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def _round(num, den):
    """the nearest integer to num / den, halves away from zero, in rationals"""
    x = Fraction(int(num), int(den))
    n = abs(x) + Fraction(1, 2)
    r = n.numerator // n.denominator
    return -r if x < 0 else r


def exact_row(ca, ha, xa, cb, hb, xb, wa, wb, U, D):
    a = int(ca) + _round(16 * int(ha) * int(xa), U * D)
    b = int(cb) + _round(16 * int(hb) * int(xb), U * D)
    return _round(int(wa) * a + int(wb) * b, int(wa) + int(wb))


def _exact(clock16, rate, U, D, mix):
    return np.array([[exact_row(clock16[a][s], rate[a][s], xa, clock16[b][s], rate[b][s], xb, wa, wb, U, D) for s in range(clock16.shape[1])]
                     for a, xa, b, xb, wa, wb in np.asarray(mix).tolist()], dtype=np.int64)


def corner_cases(U, D):
    """-> (clock16 [n][1], fine_rate [n][1], mix [m][6]), int32: every corner as one entry on one-station lines, two lines each.
    r(16 rate x, U D) is an exact half when 32 rate x = (2 k + 1) U D.  With e = 32 / U (16, 8, 4 or 2) that is e rate x = (2 k + 1) D,
    which has solutions only where e divides D: of D in 1, 4, 7 at (U, D) = (16, 4) and (8, 4); D = 16 has them at every U"""
    den, e = U * D, 32 // U
    halves = []                                                              # (rate, x) with 16 rate x / (U D) an odd number of halves
    for odd in ((1, 3, -1, -3, 5, -7) if D % e == 0 else ()):
        prod = odd * (D // e)
        halves += [(prod, 1), (1, prod), (-prod, -1), (-1, prod)]
    cases = []                                                               # (ca, ha, xa, cb, hb, xb, wa, wb)
    for h, x in halves + [(7, 3), (-7, 3), (7, -3), (-7, -3), (MAX_RATE, 1), (-MAX_RATE, 1), (MAX_RATE, -1)]:
        for c in (0, 5, -5):
            cases += [(c, h, x, c, h, x, 1, 0), (c, h, x, -c, -h, x, 1, 1), (c, h, x, c + 1, h, -x, 1, 1), (c, h, x, c, 0, 0, 3, 1)]
    for x in (0, 1, -1, 65535, -65535):                                      # x at its ends; the largest rate where the row still fits int32
        for h in (0, 1, -1, 13, -13, MAX_RATE if abs(x) <= 1 or 16 * MAX_RATE * 65535 // den < 2 ** 31 - 2 ** 20 else 97, -97):
            cases += [(100, h, x, -100, -h, -x, 1, 0), (100, h, x, -100, -h, -x, 0, 1), (100, h, x, -100, h, -x, 1, 1),
                      (100, h, x, 101, h, x, 65535, 1), (100, h, x, 101, h, x, 1, 65535), (100, h, x, 103, -h, x, 32768, 32768),
                      (100, h, x, 0, 0, 0, 65536, 0), (0, 0, 0, 100, h, x, 0, 65536)]
    for a, b in ((3, 4), (-3, -4), (3, -4), (-3, 4), (1, 0), (-1, 0), (5, -5), (1, -2)):          # exact halves in the mean, rates zero
        cases += [(a, 0, 9, b, 0, -9, 1, 1), (a, 0, 9, b, 0, -9, 3, 1), (a, 0, 9, b, 0, -9, 4, 4), (a, 5, 0, b, -5, 0, 1, 1)]
    for dn in (2, 8, 65536):                                                 # ... and their neighbours at every den
        for t in (dn // 2, -(dn // 2), dn // 2 + 1, -(dn // 2) - 1, dn // 2 - 1, -(dn // 2) + 1, 3 * dn // 2, -3 * dn // 2):
            cases += [(t, 0, 1, 0, 0, 1, 1, dn - 1), (0, 0, 1, t, 0, 1, dn - 1, 1)]
    clock16 = np.array([[v] for c in cases for v in (c[0], c[3])], dtype=np.int32)
    rate = np.array([[v] for c in cases for v in (c[1], c[4])], dtype=np.int32)
    mix = np.array([[2 * k, c[2], 2 * k + 1, c[5], c[6], c[7]] for k, c in enumerate(cases)], dtype=np.int32)
    return clock16, rate, mix


def random_cases(seed, n, U, D):
    """n random entries over 64 three-station lines; every fourth line small numbers (many exact halves)"""
    rng = np.random.default_rng(seed)
    clock16 = rng.integers(-2 ** 29, 2 ** 29, size=(64, 3)).astype(np.int32)
    rate = rng.integers(-MAX_RATE, MAX_RATE + 1, size=(64, 3)).astype(np.int32)
    clock16[::4] = rng.integers(-9, 10, size=(16, 3))
    rate[::4] = rng.integers(-4, 5, size=(16, 3)) * (D // (32 // U) if D % (32 // U) == 0 else D)      # halves where there are any
    den = np.where(rng.random(n) < 0.5, rng.integers(1, 9, size=n), rng.integers(1, 65537, size=n))
    wa = (rng.random(n) * (den + 1)).astype(np.int64).clip(0, den)
    reach = min(65535, (2 ** 29) * U * D // (16 * MAX_RATE))                  # |16 rate x / (U D)| <= 2^29: the rows fit int32
    x = rng.integers(-reach, reach + 1, size=(n, 2))
    x[::5] = rng.integers(-3, 4, size=x[::5].shape)
    lines = rng.integers(0, 64, size=(n, 2))
    lines[::3] = 4 * rng.integers(0, 16, size=lines[::3].shape)              # the small lines among themselves
    return clock16, rate, np.stack([lines[:, 0], x[:, 0], lines[:, 1], x[:, 1], wa, den - wa], axis=1).astype(np.int32)


def _halves(clock16, rate, U, D, mix):
    """-> (exact halves in a continuation: positive, negative; in the mean: positive, negative), counts over all stations"""
    from tdoa_amd import line_mix
    m, den = np.asarray(mix, dtype=np.int64), U * D
    out = []
    num = np.concatenate([16 * rate[m[:, 0]].astype(np.int64) * m[:, 1, None], 16 * rate[m[:, 2]].astype(np.int64) * m[:, 3, None]])
    half = (2 * np.abs(num)) % (2 * den) == den
    out += [int((half & (num > 0)).sum()), int((half & (num < 0)).sum())]
    ca = line_mix.continued(clock16[m[:, 0]], rate[m[:, 0]], m[:, 1, None], U, D)
    cb = line_mix.continued(clock16[m[:, 2]], rate[m[:, 2]], m[:, 3, None], U, D)
    t, dn = m[:, 4, None] * ca + m[:, 5, None] * cb, (m[:, 4] + m[:, 5])[:, None]
    half = (2 * np.abs(t)) % (2 * dn) == dn
    return out + [int((half & (t > 0)).sum()), int((half & (t < 0)).sum())]


@pytest.mark.parametrize("U", [2, 4, 8, 16])
def test_mix_rows_against_fractions(U):
    from tdoa_amd import line_mix
    seen = np.zeros(4, dtype=np.int64)
    for D in (1, 4, 7, 16):
        clock16, rate, mix = corner_cases(U, D)
        got = line_mix.mix_rows(clock16, rate, U, D, mix)
        assert got.dtype == np.int32 and (got == _exact(clock16, rate, U, D, mix)).all(), (U, D)
        x = mix[:, [1, 3]]
        assert (x == 65535).any() and (x == -65535).any() and (x == 0).any() and (x > 0).any() and (x < 0).any()      # the corners are there
        assert (mix[:, 4] == 0).sum() >= 10 and (mix[:, 5] == 0).sum() >= 10 and (mix[:, 4] + mix[:, 5] == 65536).sum() >= 20
        assert rate.max() == MAX_RATE and rate.min() == -MAX_RATE
        corners = np.array(_halves(clock16, rate, U, D, mix))
        assert (corners[2:] >= 5).all(), (U, D, corners)                     # halves of both signs in the mean
        seen += corners
        clock16, rate, mix = random_cases(10 * U + D, 1200, U, D)
        got = line_mix.mix_rows(clock16, rate, U, D, mix)
        assert (got == _exact(clock16, rate, U, D, mix)).all(), (U, D)
        seen += _halves(clock16, rate, U, D, mix)
    assert (seen >= 20).all(), seen                                          # ... and, over the four D, in the continuation
    c, h = np.zeros((3, 2), dtype=np.int32), np.ones((3, 2), dtype=np.int32)
    for bad in ([[0, 0, 3, 0, 1, 1]], [[3, 0, 0, 0, 1, 1]], [[-1, 0, 0, 0, 1, 1]], [[0, 65536, 0, 0, 1, 1]], [[0, 0, 0, -65536, 1, 1]],
                [[0, 0, 0, 0, -1, 2]], [[0, 0, 0, 0, 0, 0]], [[0, 0, 0, 0, 65536, 1]], [[0, 0, 1, 1]], []):
        with pytest.raises(ValueError):
            line_mix.mix_rows(c, h, U, 1, bad)
    for kw in (dict(U=3), dict(U=1), dict(U=32), dict(drift_den=0)):
        with pytest.raises(ValueError):
            line_mix.mix_rows(c, h, **{**dict(U=U, drift_den=1, mix=[[0, 0, 0, 0, 1, 0]]), **kw})
    with pytest.raises(ValueError):                                          # a continued clock that leaves int32
        line_mix.mix_rows(np.full((1, 1), 2 ** 31 - 1), np.full((1, 1), U), U, 1, [[0, 1, 0, 0, 1, 0]])


def test_one_line_is_line_clock16_and_still_lines_are_the_clock_mix(capi):
    from tdoa_amd import clock_mix, line_mix, sync_drift_fine
    rng = np.random.default_rng(3)
    n_half = 0
    for U in (2, 4, 8, 16):
        for D in (1, 3, 4, 7, 32):
            k, h = rng.integers(-5000, 5001, size=(4, 6)).astype(np.int32), rng.integers(-300, 301, size=(4, 6)).astype(np.int32)
            h[0] = rng.integers(-3, 4, size=6) * D
            for line in range(4):
                mix = np.array([[line, x, line, x, 1, 0] for x in range(9, 49)], dtype=np.int32)
                got = line_mix.mix_rows(k, h, U, D, mix)
                want = sync_drift_fine.line_clock16(k[line], h[line], U, D, 9, 40)
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes() == capi.sync_line_clock16(k[line], h[line], U, D, 9, 40).tobytes()
                num = 16 * h[line].astype(np.int64)[None, :] * np.arange(9, 49)[:, None]
                n_half += int(((2 * np.abs(num)) % (2 * U * D) == U * D).sum())
            # a negative x is the mirrored rate's positive one: the rule is odd in rate x
            back = line_mix.mix_rows(k, h, U, D, [[1, -x, 1, -x, 1, 0] for x in range(1, 30)])
            assert back.tobytes() == line_mix.mix_rows(k, -h, U, D, [[1, x, 1, x, 1, 0] for x in range(1, 30)]).tobytes()
            # ... and with both rates zero nothing of x is left
            a, b = np.divmod(np.arange(16), 4)
            w = rng.integers(0, 9, size=(16, 2)) + [1, 0]
            mix = np.stack([a, rng.integers(-65535, 65536, size=16), b, rng.integers(-65535, 65536, size=16), w[:, 0], w[:, 1]], axis=1)
            still = line_mix.mix_rows(k, np.zeros_like(h), U, D, mix)
            assert still.tobytes() == clock_mix.mix_rows(k, mix[:, [0, 2, 4, 5]]).tobytes()
    assert n_half >= 50
    assert (line_mix.own_mix(2, 3) == [[0, 0, 0, 0, 1, 0], [0, 1, 0, 1, 1, 0], [0, 2, 0, 2, 1, 0], [1, 0, 1, 0, 1, 0], [1, 1, 1, 1, 1, 0],
                                       [1, 2, 1, 2, 1, 0]]).all()


def test_line_mix_rows_in_c_returns_the_statements_bytes_and_refuses(capi):
    from tdoa_amd import line_mix
    for U, D in ((2, 7), (4, 1), (8, 4), (16, 4), (16, 1)):
        for clock16, rate, mix in (corner_cases(U, D), random_cases(5 + U, 2000, U, D)):
            got = capi.line_mix_rows(clock16, rate, U, D, mix)
            want = line_mix.mix_rows(clock16, rate, U, D, mix)
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (U, D)
    lib = capi.load()
    i32p = C.POINTER(C.c_int32)
    c16 = np.arange(12, dtype=np.int32).reshape(4, 3)
    eta = np.array([[0, 4, -4]] * 4, dtype=np.int32)
    rows = np.zeros((2, 3), dtype=np.int32)
    pc, pe, pr = c16.ctypes.data_as(i32p), eta.ctypes.data_as(i32p), rows.ctypes.data_as(i32p)

    def call(mix, pc=pc, pe=pe, pr=pr, n=4, S=3, U=16, D=8, m=2, null_mix=False):
        mm = np.array(mix, dtype=np.int32)
        return lib.tdoa_line_mix_rows(pc, pe, n, S, U, D, None if null_mix else mm.ctypes.data_as(i32p), m, pr)

    ok = [[0, 1, 0, 1, 1, 0], [0, 1, 3, -1, 1, 1]]
    # 16 eta x / (U D) = eta x / 8: +-4 at x = 1 is a half, away from zero; line 3 backwards is (9, 10 - 1, 11 + 1)
    assert call(ok) == 0 and rows.tolist() == [[0, 2, 1], [5, 6, 7]]         # (0 + 9 + 1) div 2, (2 + 9 + 1) div 2, (1 + 12 + 1) div 2
    for bad in ([0, 0, 4, 0, 1, 1], [4, 0, 0, 0, 1, 1], [-1, 0, 0, 0, 1, 1], [0, 0, -1, 0, 1, 1], [0, 65536, 0, 0, 1, 1], [0, -65536, 0, 0, 1, 1],
                [0, 0, 0, 65536, 1, 1], [0, 0, 0, -65536, 1, 1], [0, 0, 0, 0, -1, 2], [0, 0, 0, 0, 2, -1], [0, 0, 0, 0, 0, 0],
                [0, 0, 0, 0, 65536, 1], [0, 0, 0, 0, 1, 65536], [0, 0, 0, 0, 2 ** 31 - 1, 2 ** 31 - 1]):
        assert call([ok[0], bad]) == 1, bad
    assert call([ok[0], [3, 65535, 3, -65535, 65535, 1]]) == 0               # every field at its end
    assert call(ok, pc=None) == 1 and call(ok, pe=None) == 1 and call(ok, pr=None) == 1 and call(ok, null_mix=True) == 1
    assert call(ok, n=0) == 1 and call(ok, S=0) == 1 and call(ok, m=0) == 1
    for U in (0, 1, 3, 5, 12, 32, -2):
        assert call(ok, U=U) == 1, U
    assert call(ok, D=0) == 1 and call(ok, D=-1) == 1 and call(ok, U=2, D=1) == 0
    top = np.full((1, 1), 2 ** 31 - 1, dtype=np.int32)                       # a continued clock that does not fit int32: refused, either sign
    one = np.full((1, 1), 16, dtype=np.int32)
    pt, po = top.ctypes.data_as(i32p), one.ctypes.data_as(i32p)
    assert call([[0, 0, 0, 0, 1, 0]], pc=pt, pe=po, n=1, S=1, D=1, m=1) == 0 and rows[0, 0] == 2 ** 31 - 1
    assert call([[0, 1, 0, 0, 1, 0]], pc=pt, pe=po, n=1, S=1, D=1, m=1) == 1
    assert call([[0, 0, 0, 1, 0, 1]], pc=pt, pe=po, n=1, S=1, D=1, m=1) == 1
    assert call([[0, -1, 0, -1, 1, 0]], pc=pt, pe=po, n=1, S=1, D=1, m=1) == 0 and rows[0, 0] == 2 ** 31 - 17
    with pytest.raises(capi.TdoaError) as e:
        capi.line_mix_rows(c16, eta, 16, 8, [[0, 0, 9, 0, 1, 1]])
    assert e.value.status == 1
    with pytest.raises(ValueError):
        capi.line_mix_rows(c16, eta, 16, 8, [[0, 0, 1, 1]])                   # a clock mix is not a line mix


@pytest.mark.parametrize("L", [1, 2, 5])
def test_forward_mix_reproduces_the_hand_built_clock_table(capi, L):
    """tests/test_gpu_sync_drift_fine.py::test_cli_sync_drift_fine_prints_the_library_result and tdoa_processor: np.concatenate(
    [fine_rows[:L], sync_line_clock16(clock16[0], fine_rate[0], U, D, L, L), fine_rows[2 L:]]).  fine_rows[l L + x] is
    16 / U x (kappa + shift(eta, x)) in 1/U sample, which at U = 16 is the own entry's row; at U < 16 the two differ by less than
    1/U sample = 16 / U sixteenths"""
    from tdoa_amd import line_mix, sync_drift
    rng = np.random.default_rng(40 + L)
    for U, D in ((16, 2), (16, 7), (8, 2), (2, 3)):
        kappa, eta = rng.integers(-40 * U, 40 * U + 1, size=(3, 3)), rng.integers(-3 * U, 3 * U + 1, size=(3, 3))
        c16, rate = (kappa * (16 // U)).astype(np.int32), eta.astype(np.int32)
        fine_rows = np.concatenate([(kappa[l] + np.array([[sync_drift.shift(int(e), x, D) for e in eta[l]] for x in range(L)])) * (16 // U)
                                    for l in range(3)]).astype(np.int32)
        by_hand = np.concatenate([fine_rows[:L], capi.sync_line_clock16(c16[0], rate[0], U, D, L, L), fine_rows[2 * L:]])
        mix = line_mix.forward_mix(L)
        assert mix.shape == (3 * L, 6) and mix.dtype == np.int32
        got = line_mix.mix_rows(c16, rate, U, D, mix)
        assert got[L:2 * L].tobytes() == by_hand[L:2 * L].tobytes()
        if U == 16:
            assert got.tobytes() == by_hand.tobytes()
            assert line_mix.mix_rows(c16, rate, U, D, line_mix.own_mix(3, L)).tobytes() == fine_rows.tobytes()
        else:
            assert np.abs(got.astype(np.int64) - by_hand).max() < 16 // U
    assert line_mix.forward_mix(2).tolist() == [[0, 0, 0, 0, 1, 0], [0, 1, 0, 1, 1, 0], [0, 2, 0, 2, 1, 0], [0, 3, 0, 3, 1, 0],
                                               [2, 0, 2, 0, 1, 0], [2, 1, 2, 1, 1, 0]]
    assert line_mix.bridge_mix(2).tolist() == [[0, 0, 0, 0, 1, 0], [0, 1, 0, 1, 1, 0], [0, 2, 2, -2, 2, 1], [0, 3, 2, -1, 1, 2],
                                              [2, 0, 2, 0, 1, 0], [2, 1, 2, 1, 1, 0]]
    assert line_mix.pair_differences(np.array([[1, 4, 9]])).tolist() == [[3, 8, 5]]          # pairs (0,1), (0,2), (1,2)


# ---- 5. the measured case ------------------------------------------------------------------------------------------------
def after_windows_iq(oracle, b):
    """[w - 24][s] u8 IQ of a reference block after block b's target: windows w = 24 .. 35 from reference_windows_iq's generator,
    the clocks sliding on"""
    d4 = measured_case()[1]
    return [_quarter_window(oracle, d4 + CLOCK4 + slide4(w) + 400, 300 + 50 * b + w, 1300 + 50 * b + w) for w in range(2 * M_POS, 3 * M_POS)]


def test_the_chains_statement_is_the_three_statements_one_after_another(oracle):
    """[reference | target | reference] = block 0 of the measured case with a reference block behind it, three lines of twelve
    one-window stacks: sync_drift_locate under forward_mix(12) and bridge_mix(12) returns what sync_lines_fine, mix_rows and
    track_zoom_stacks return when the caller chains them, and the target's track moves when the clocks are dropped"""
    from tdoa_amd import line_mix, locate, locate_track_zoom, sync_drift_fine, sync_drift_locate
    ref_delay = measured_case()[0]
    q = np.concatenate([float64_words(oracle, reference_windows_iq(oracle, 0)), float64_words(oracle, target_windows_iq(oracle, 0)),
                        float64_words(oracle, after_windows_iq(oracle, 0))])
    Z, H, J, Jf = 2, 3, 1, 2
    table = coarse_table()
    grid = dict(GRID, dlat=GRID["dlat"] / Z, dlon=GRID["dlon"] / Z, rows=(GRID["rows"] - 1) * Z + 1, cols=(GRID["cols"] - 1) * Z + 1)
    fine = locate.grid_table(ST4, sample_rate=FS, **grid)
    args = (LINE["G"], LINE["H"], LINE["D"], LINE["R"], LINE["U"], LINE["Rf"])
    found = sync_drift_fine.sync_lines_fine(q, M_POS, ref_delay, ML, *args)
    bare = locate_track_zoom.track_zoom_stacks(q, table, 64, fine, grid["cols"], ML, M_POS, J, Z, H, Jf, 1, 1, 1, None)
    for name, mix in (("forward", line_mix.forward_mix(M_POS)), ("bridge", line_mix.bridge_mix(M_POS)), ("own", None)):
        got = sync_drift_locate.sync_drift_locate(q, M_POS, ref_delay, table, 64, fine, grid["cols"], ML, Z, H, mix, *args, None, J, 1, Jf, 1, 1, 1)
        rows = line_mix.mix_rows(found["clock16"], found["fine_rate"], LINE["U"], LINE["D"], line_mix.own_mix(3, M_POS) if mix is None else mix)
        z = locate_track_zoom.track_zoom_stacks(q, table, 64, fine, grid["cols"], ML, M_POS, J, Z, H, Jf, 1, 1, 1, rows)
        assert set(got) == set(KEYS)
        for k in LINE_KEYS:
            assert got[k].dtype == found[k].dtype and got[k].tobytes() == found[k].tobytes(), (name, k)
        assert got["mix_rows"].tobytes() == rows.tobytes() and got["mix_rows"].any()
        for k, want in zip(sync_drift_locate.TRACK_KEYS, z):
            assert got[k].dtype == want.dtype and got[k].tobytes() == want.tobytes(), (name, k)
        assert (got["ztrack"]["score_q"] > 0).all()
        assert (got["zcells"] != bare[7]).any(), name                        # a dropped clock would show
        if name == "own":
            assert got["mix_rows"].tobytes() == got["fine_rows"].tobytes()   # U = 16
        if name == "forward":
            assert rows[M_POS:2 * M_POS].tobytes() == sync_drift_fine.line_clock16(found["clock16"][0], found["fine_rate"][0], LINE["U"], LINE["D"],
                                                                                   M_POS, M_POS).tobytes()
    assert sync_drift_locate.TRACK_KEYS == TRACK_KEYS


def test_the_block_fix_under_the_forward_and_the_bridge_mix(oracle):
    """The measured case, twelve blocks, each with a reference block behind its target (windows 24 .. 35 of the same generators).
    Under forward_mix the target's rows are the fine line continued, so the median fix is that case's 81.6 m and the worst row
    error 9/16 sample.  Under bridge_mix the rows are the weighted mean of that line continued forwards and the later block's line
    continued backwards.  Measured with the numpy statement: bridge 176.8 m, worst row error 1972.5/16 sample.  That is the later
    block's line, not the rule: the case slides stations 1 and 2 apart by 35/16 sample per window, by windows 24 .. 35 they are
    about 140 samples apart, beyond max_lag 128, so pair (1, 2) has left the lag range, station 2's later line is not found
    (clock16 between 205 and 1799 over the blocks where -1367 is true) and the bridge inherits half of that error.  The case was
    built for a line before the target; it says nothing about a bridge between two good lines, which nobody has measured.  No
    assertion on which is better.  Every block's figures are printed."""
    from tdoa_amd import line_mix, sync_drift_fine
    ref_delay = measured_case()[0]
    args = (LINE["G"], LINE["H"], LINE["D"], LINE["R"], LINE["U"], LINE["Rf"])
    truth = true_rows16(M_POS, M_POS)
    d, err = [], []
    for b in range(12):
        q_tgt = float64_words(oracle, target_windows_iq(oracle, b))
        lines = [sync_drift_fine.sync_line_fine(float64_words(oracle, w), ref_delay, ML, *args)
                 for w in (reference_windows_iq(oracle, b), after_windows_iq(oracle, b))]
        c16 = np.stack([lines[0]["clock16"], np.zeros(4, dtype=np.int32), lines[1]["clock16"]])
        rate = np.stack([lines[0]["fine_rate"], np.zeros(4, dtype=np.int32), lines[1]["fine_rate"]])
        rows = [line_mix.mix_rows(c16, rate, LINE["U"], LINE["D"], m(M_POS))[M_POS:2 * M_POS] for m in (line_mix.forward_mix, line_mix.bridge_mix)]
        assert rows[0].tobytes() == sync_drift_fine.line_clock16(c16[0], rate[0], LINE["U"], LINE["D"], M_POS, M_POS).tobytes()
        d.append([block_fix_metres(q_tgt, b, r) for r in rows])
        err.append([int(np.abs(r.astype(np.int64) - truth).max()) for r in rows])
        print("block %2d: line after clock16 %s rate %s; worst row error forward %d/16, bridge %d/16; fix forward %.0f m, bridge %.0f m"
              % (b, c16[2].tolist(), rate[2].tolist(), err[-1][0], err[-1][1], d[-1][0], d[-1][1]))
    med, med_err = np.median(np.array(d), axis=0), np.median(np.array(err, dtype=np.float64), axis=0)
    print("medians over 12 blocks: fix under the forward mix %.1f m, the bridge mix %.1f m; worst row error %.1f/16 and %.1f/16"
          % (med[0], med[1], med_err[0], med_err[1]))
    assert abs(med[0] - FORWARD_MEDIAN_M) < 0.05 and med_err[0] == 9.0        # that case's medians
    assert np.isfinite(med[1]) and med[1] >= 0.0


# ---- 6. the entries ----------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported(capi):
    import tdoa_amd
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessSyncDriftLocate(", "C.tdoa_process_sync_drift_locate(", "func (g *Group) ProcessSyncDriftLocate(",
                 "C.tdoa_group_process_sync_drift_locate(", "func LineMixRows(", "C.tdoa_line_mix_rows(", "func ForwardMix("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_sync_drift_locate", "sync_drift_locate_from_q", "debug_line_mix"):
        assert getattr(capi.Context, method).__doc__, method
    assert capi.Group.process_sync_drift_locate.__doc__ and capi.line_mix_rows.__doc__
    for name in ("as_mix", "mix_rows", "own_mix", "forward_mix", "bridge_mix"):
        assert callable(getattr(tdoa_amd.line_mix, name)), name
    assert len(capi.SEARCHES) == 9 and list(capi.LATER_SEARCHES) == ["sync_drift_fine"]
    assert list(capi.TRACK_ZOOM_SEARCHES) == ["locate_track_zoom", "sync_locate", "sync_drift_locate"]
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]
    text = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("cont(l, x)[s] = c16[l][s] + r(16 eta[l][s] x, U drift_den)", "(l, x, l, x, 1, 0) is line l continued to x",
                   "a negative x continues a line backwards", "is neither read nor changed",
                   "mix == NULL: stack l L + x takes (l, x, l, x, 1, 0)", "At U = 16 these rows are fine_rows byte for byte.",
                   "At U < 16 they differ from fine_rows by less than 1/U sample", "|xa| or |xb| above 65535", "wa + wb outside 1 .. 65536",
                   "|centre| + gate + 2 + ((max_drift + 1) X) div drift_den >= 2^27", "16 times that sum times U_loc >= 2^31"):
        assert phrase in text, phrase
    assert tdoa_amd.line_mix.MIX_DTYPE.itemsize == 24


def test_the_record_states_the_headers_order_and_types(capi):
    lib, protos = capi.load(), _prototypes()
    s = capi._search("sync_drift_locate")
    assert s.entries == {"own": NAMES[0], "group": NAMES[1], "q": NAMES[2]}
    assert s.ints == ("gate", "max_drift", "drift_den", "rounds", "U", "fine_rounds") and s.inputs == ("ref_delay", "centre", "mix")
    assert s.late_ints == ("max_step", "min_separation", "Z", "H", "fine_step", "fine_separation")
    assert s.track_len and s.stats == "track" and not s.bare and s.mix_width == 6 and capi._search("sync_locate").mix_width == 4
    keys = [o.key for o in s.outputs]
    assert keys == list(KEYS) and len(keys) == 26
    c_types = {"int": C.c_int, "int32_t *": C.POINTER(C.c_int32), "double *": C.POINTER(C.c_double), "int64_t *": C.POINTER(C.c_int64)}
    records = {"tdoa_sync_line *": capi.SYNC_LINE_DTYPE, "tdoa_cell_track *": capi.CELL_TRACK_DTYPE}
    scalars = {"int32_t *": np.int32, "double *": np.float64, "int64_t *": np.int64}
    for route, lead in (("own", ["ctx", "windows_per_stack"]), ("group", ["g", "windows_per_stack"]),
                        ("q", ["ctx", "q", "n_sets", "track_len", "n_stations", "n_w"])):
        entry = s.entries[route]
        names = lead + list(s.ints) + list(s.inputs) + list(s.late_ints) + [k + "_host" for k in keys]
        assert [n for _, n in protos[entry]] == names, route
        argtypes = getattr(lib, entry).argtypes
        assert len(argtypes) == len(names), route
        first_out = len(names) - len(keys)
        for k, ((ctype, name), argtype) in enumerate(zip(protos[entry], argtypes)):
            if k == 0:
                assert ctype == ("tdoa_group *" if route == "group" else "tdoa_ctx *") and argtype is C.c_void_p
            elif name == "mix":
                assert ctype == "tdoa_line_mix *" and argtype is C.POINTER(C.c_int32)
            elif ctype in c_types:
                assert argtype is c_types[ctype], (entry, name)
            else:
                assert ctype in records and argtype is C.c_void_p, (entry, name)
            if k >= first_out:
                dtype = np.dtype(s.outputs[k - first_out].dtype)
                assert dtype == (records[ctype] if ctype in records else np.dtype(scalars[ctype])), (entry, name)
    assert [n for _, n in protos[NAMES[3]]] == ["clock16", "fine_rate", "n_lines", "n_stations", "U", "drift_den", "mix", "n_rows", "rows"]
    assert [n for _, n in protos[NAMES[4]]] == ["ctx", "clock16", "fine_rate", "n_lines", "n_stations", "U", "drift_den", "mix", "n_rows", "U_loc",
                                                "rows", "cdiff", "cdiff_up"]
    assert len(lib.tdoa_line_mix_rows.argtypes) == 9 and len(lib.tdoa_debug_line_mix.argtypes) == 13


def test_null_handle_is_invalid_without_a_device(capi):
    lib = capi.load()
    n_out = len(capi._search("sync_drift_locate").outputs)
    ref = (C.c_int32 * 3)(0, 16, 32)
    q = np.zeros(3 * 7, dtype=np.int64)
    ints = (1, 1, 1, 1, 16, 2)
    late = (0, 1, 2, 2, 0, 1)
    assert lib.tdoa_process_sync_drift_locate(None, 0, *ints, ref, None, None, *late, *[None] * n_out) == 1
    assert lib.tdoa_group_process_sync_drift_locate(None, 0, *ints, ref, None, None, *late, *[None] * n_out) == 1
    assert lib.tdoa_debug_sync_drift_locate_from_q(None, q.ctypes.data_as(C.POINTER(C.c_int64)), 1, 1, 3, 1, *ints, ref, None, None, *late,
                                                   *[None] * n_out) == 1
    assert lib.tdoa_debug_line_mix(None, ref, ref, 1, 3, 16, 1, None, 1, 1, None, None, None) == 1
