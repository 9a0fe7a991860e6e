"""GPU: free-running clocks to fix in one call (tdoa_process_sync_drift_locate, tdoa_group_process_sync_drift_locate,
tdoa_debug_sync_drift_locate_from_q, tdoa_debug_line_mix; include/tdoa_mi355x.h, "free-running clocks to fix in one call").

Every comparison is byte for byte.

1. debug_line_mix, the kernel alone, against line_mix.mix_rows: the corner list of tests/test_line_mix_cpu.py, 2, 3, 5 and 64
   stations (2 016 pairs: several passes of the workgroup), 1 and 7 lines, 1 and 300 rows, U 2 and 16, U_loc 1 and 16; the
   differences are row[j] - row[i] in tdoa_locate_set_clock's pair order and the scaled ones exactly U_loc x them; the same
   kernel without rates (debug_clock_mix) against itself with rates at position zero and against clock_mix.mix_rows;
2. the chain identity: process_sync_drift_fine, line_mix_rows, locate_set_clock, process_locate_track_zoom on one context, then
   the clock table forgotten and process_sync_drift_locate: the same twenty-six outputs, for three mixes, three upsample
   settings, two fine searches, two pairs of steps, one-window, two-window and whole-block stacks, with and without map
   statistics;
3. the context's clock table is neither read nor changed, whatever its shape, and the neighbours keep their bytes;
4. the caller's-Q route and the numpy statement; groups of one and of two members, twice;
5. the step graph replays on poisoned workspace and under new delays, centres, mixes, tables and fine tables; other Z, H, J, Jf,
   U, Rf, max_drift are other keys; the first call's bytes come back;
6. what the call refuses, both bounds at their exact edge;
7. tdoa_processor --one-call prints what the run without the flag prints."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from stack_helpers import same_bytes as _same_bytes, stacks_q as _stacks_q, windows_q as _windows_q
from test_line_mix_cpu import KEYS, MAX_RATE, corner_cases, random_cases
from test_locate_cpu import ST4

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TX = (41.20, -96.00, 400.0)
ML, WL, WPB, S = 64, 2048, 4, 4
G, R, HD, D = 4, 2, 2, 4                                   # gate, rounds, max_drift, drift_den
Z, H = 4, 2
REF = np.array([0, 16, 40, 72], dtype=np.int32)
OTHER_REF = np.array([5, -30, 11, 64], dtype=np.int32)
CENTRE = np.array([0, 1, -2, 1], dtype=np.int32)
TABLE = np.random.default_rng(19).integers(0, 16 * 30, size=(8 * 8, S), dtype=np.int32)            # 8 x 8 cells
FINE = np.random.default_rng(23).integers(0, 16 * 30, size=(29 * 29, S), dtype=np.int32)           # Z = 4: 29 x 29 fine cells
RANKS = (32768, 64880)
FOOT = 49152


def _differ(got, want):
    return [k for k in set(got) | set(want) if k not in got or k not in want or not _same_bytes(got[k], want[k])]


def _mixes(L):
    from tdoa_amd import line_mix
    return (("own", None), ("forward", line_mix.forward_mix(L)), ("bridge", line_mix.bridge_mix(L)))


def _renamed(z):
    return {("loc_" + k if k in ("lags", "corr") else k): v for k, v in z.items()}


def _chain(c, m, mix, ref=REF, centre=CENTRE, U=16, Rf=2, hd=HD, z=Z, h=H, J=1, Jf=2, sep=2, fsep=1):
    """the four calls the one call replaces, the clock table forgotten afterwards"""
    import tdoa_amd
    from tdoa_amd import line_mix
    out = c.process_sync_drift_fine(ref, m, G, hd, D, R, U, Rf, centre)
    L = c.num_stacks(m)[0]
    out["mix_rows"] = tdoa_amd.capi.line_mix_rows(out["clock16"], out["fine_rate"], U, D, line_mix.own_mix(3, L) if mix is None else mix)
    c.locate_set_clock(out["mix_rows"])
    out.update(_renamed(c.process_locate_track_zoom(z, h, m, J, sep, Jf, fsep, want_total=True)))
    c.locate_set_clock(None)
    return out


def _one(c, m, mix, ref=REF, centre=CENTRE, U=16, Rf=2, hd=HD, z=Z, h=H, J=1, Jf=2, sep=2, fsep=1):
    return c.process_sync_drift_locate(ref, z, h, m, G, hd, D, R, U, Rf, centre, mix, J, sep, Jf, fsep, want_total=True)


def _statement(c, q, m, mix, ref=REF, centre=CENTRE, U=16, Rf=2, hd=HD, z=Z, h=H, J=1, Jf=2, sep=2, fsep=1, U_loc=1, table=TABLE, fine=FINE):
    from tdoa_amd import sync_drift_locate
    Q, n_w = _stacks_q(c, q, m)
    return sync_drift_locate.sync_drift_locate(Q, c.num_stacks(m)[0], ref, table, 8, fine, 29, ML, z, h, mix, G, hd, D, R, U, Rf, centre, J, sep,
                                               Jf, fsep, n_w, U_loc)


def _synth(c):
    for s in range(S):
        c.synth_capture(s, WPB * WL, ST4[s], TX, 0x57AC0000 + s)


def _reset(c):
    c.locate_set_stats(None)
    c.locate_set_upsample(1)
    c.locate_set_clock(None)
    c.locate_set_table(TABLE, 8)
    c.locate_set_fine_table(FINE, 29)


@pytest.fixture(scope="module")
def ctx():
    """one context on synthetic captures of four stations, 3 blocks of 4 windows; the windows' words"""
    import tdoa_amd
    with tdoa_amd.Context(max_lag=ML, window_len=WL) as c:
        _synth(c)
        assert c.num_windows() == (WPB, 3 * WPB)
        _reset(c)
        yield c, _windows_q(c)


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------
def _check_mix(c, clock16, rate, U, Dd, mix, U_loc):
    from tdoa_amd import line_mix
    rows, cdiff, up = c.debug_line_mix(clock16, rate, U, Dd, mix, U_loc)
    want = line_mix.mix_rows(clock16, rate, U, Dd, mix)
    assert _same_bytes(rows, want)
    d = line_mix.pair_differences(want)
    assert _same_bytes(cdiff, d) and _same_bytes(up, U_loc * d)
    return rows


@pytest.mark.parametrize("U_loc", [1, 16])
@pytest.mark.parametrize("U", [2, 16])
def test_debug_line_mix_is_the_numpy_statement(ctx, U, U_loc):
    c, _ = ctx
    for Dd in (1, 4, 7, 16):
        clock16, rate, mix = corner_cases(U, Dd)                             # one station per line would be refused: two, the second mirrored
        rows = _check_mix(c, np.concatenate([clock16, -clock16], axis=1), np.concatenate([rate, -rate], axis=1), U, Dd, mix, U_loc)
        assert (rows[:, 0] == -rows[:, 1]).all()                             # halves go away from zero on both sides
    rng = np.random.default_rng(31 + U)
    for n_st in (2, 3, 5, 64):
        for n, m in ((1, 1), (7, 300), (1, 300), (7, 1)):
            Dd = int(rng.integers(1, 9))
            c16 = rng.integers(-2 ** 29, 2 ** 29, size=(n, n_st)).astype(np.int32)
            eta = rng.integers(-MAX_RATE, MAX_RATE + 1, size=(n, n_st)).astype(np.int32)
            c16[::2] = rng.integers(-9, 10, size=c16[::2].shape)
            reach = min(65535, (2 ** 29) * U * Dd // (16 * MAX_RATE))        # the continued clocks fit int32
            den = rng.integers(1, 65537, size=m)
            den[::3] = rng.integers(1, 9, size=len(den[::3]))
            wa = rng.integers(0, den + 1)
            mx = np.stack([rng.integers(0, n, size=m), rng.integers(-reach, reach + 1, size=m), rng.integers(0, n, size=m),
                           rng.integers(-reach, reach + 1, size=m), wa, den - wa], axis=1).astype(np.int32)
            _check_mix(c, c16, eta, U, Dd, mx, U_loc)
    clock16, rate, mix = random_cases(7, 300, U, 4)
    _check_mix(c, clock16, rate, U, 4, mix, U_loc)


@pytest.mark.parametrize("U_loc", [1, 16])
def test_the_kernel_in_its_clock_role_is_its_line_role_at_position_zero(ctx, U_loc):
    """one kernel serves both calls: without rates it takes the clocks as they are, and a clock-mix entry (a, b, wa, wb) is the
    line-mix entry (a, 0, b, 0, wa, wb), whatever the rates and U D.  2 stations: one pair; 3: the fewest with several; 64: the
    whole LDS row and 2 016 pairs, more than the workgroup's 256 threads.  Clocks up to +-(2^31 - 16), every other source small."""
    from tdoa_amd import clock_mix
    c, _ = ctx
    rng = np.random.default_rng(37 + U_loc)
    for n_st in (2, 3, 64):
        for n in (1, 7):
            for m in (1, 300):
                c16 = rng.integers(-(2 ** 31 - 16), 2 ** 31 - 15, size=(n, n_st)).astype(np.int32)
                c16[::2] = rng.integers(-9, 10, size=c16[::2].shape)
                rate = (rng.integers(1, MAX_RATE + 1, size=(n, n_st)) * rng.choice([-1, 1], size=(n, n_st))).astype(np.int32)
                den = rng.integers(1, 65537, size=m)
                den[::3] = rng.integers(1, 9, size=len(den[::3]))
                wa = rng.integers(0, den + 1)
                a, b, zero = rng.integers(0, n, size=m), rng.integers(0, n, size=m), np.zeros(m, dtype=np.int64)
                narrow = np.stack([a, b, wa, den - wa], axis=1).astype(np.int32)
                wide = np.stack([a, zero, b, zero, wa, den - wa], axis=1).astype(np.int32)
                want = clock_mix.mix_rows(c16, narrow)
                d = clock_mix.pair_differences(want)
                as_clocks = c.debug_clock_mix(c16, narrow, U_loc)
                for U, Dd in ((2, 1), (16, 7)):
                    as_lines = c.debug_line_mix(c16, rate, U, Dd, wide, U_loc)
                    for got in (as_clocks, as_lines):
                        assert _same_bytes(got[0], want) and _same_bytes(got[1], d) and _same_bytes(got[2], U_loc * d)
                    assert all(_same_bytes(x, y) for x, y in zip(as_clocks, as_lines))


# ---- 2. the chain identity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U_loc", [1, 4, 16])
def test_the_one_call_is_the_chain(ctx, U_loc):
    c, q = ctx
    _reset(c)
    c.locate_set_upsample(U_loc)
    seen = moved_cells = 0
    for m in (1, 2, 0):                                                      # lines and tracks of 4, 2 and 1 stacks
        L = c.num_stacks(m)[0]
        assert L == {1: 4, 2: 2, 0: 1}[m]
        for J, Jf in ((1, 2), (0, 0)):
            bare = c.process_locate_track_zoom(Z, H, m, J, 2, Jf, 1)         # no clocks
            for U, Rf in ((16, 2), (4, 1)):
                for name, mix in _mixes(L):
                    want = _chain(c, m, mix, U=U, Rf=Rf, J=J, Jf=Jf)
                    got = _one(c, m, mix, U=U, Rf=Rf, J=J, Jf=Jf)
                    assert set(got) == set(KEYS) and not _differ(got, want), (m, J, Jf, U, Rf, name, _differ(got, want))
                    # (on these random tables a block's best summed score may be 0, the zero record: the chain's bytes all the same)
                    assert got["mix_rows"].any() and (got["fine"]["score_q"] > 0).all() and (got["ztrack"]["score_q"] > 0).any()
                    assert not _same_bytes(got["zmap"], bare["zmap"]), (m, J, Jf, U, Rf, name)      # a dropped clock would show
                    moved_cells += int((got["zcells"] != bare["zcells"]).sum())
                    if name == "own" and U == 16:
                        assert _same_bytes(got["mix_rows"], got["fine_rows"])
                    if name == "own" and U == 4:                             # less than 1/U sample apart
                        assert np.abs(got["mix_rows"].astype(np.int64) - got["fine_rows"]).max() < 16 // U
                    seen += 1
        if U_loc == 1 and m == 2:                                            # ... and the statement, once
            want = _statement(c, q, m, mix, U=4, Rf=1, J=0, Jf=0)
            assert not _differ(got, want), _differ(got, want)
    assert seen == 36 and moved_cells > 0                                    # at least one zoomed cell differs from the clock-less call's
    c.locate_set_stats(RANKS, FOOT)                                          # map statistics on: the chain's, as after process_locate_track_zoom
    for m in (1, 0):
        for name, mix in _mixes(c.num_stacks(m)[0]):
            want = _chain(c, m, mix)
            got = _one(c, m, mix)
            assert set(got) == set(KEYS) | {"stats"} and not _differ(got, want), (m, name, _differ(got, want))
            assert _same_bytes(c.locate_last_stats().reshape(got["stats"].shape), want["stats"]) and want["stats"]["n_live"].all()
    _reset(c)


# ---- 3. the context's clock table -----------------------------------------------------------------------------------------
def test_the_contexts_clock_table_is_left_alone(ctx):
    import tdoa_amd
    from tdoa_amd import line_mix
    c, _ = ctx
    _reset(c)
    M = 2
    mix = line_mix.bridge_mix(2)
    fine0 = c.process_sync_drift_fine(REF, M, G, HD, D, R, 16, 2, CENTRE)
    zoom0 = c.process_locate_track_zoom(Z, H, M, 1, 2, 2, 1, want_total=True)
    want = _chain(c, M, mix)
    other = np.random.default_rng(5).integers(-64, 65, size=(6, S)).astype(np.int32)
    c.locate_set_clock(other)
    plain = c.process_locate_track(M, 1, 2, want_total=True)
    got = _one(c, M, mix)
    assert not _differ(got, want), _differ(got, want)                       # test 2's bytes: that table has no say
    again = c.process_locate_track(M, 1, 2, want_total=True)
    assert not _differ(again, plain) and not _same_bytes(plain["total"], zoom0["total"])
    c.locate_set_clock(other[:3])                                            # a table of another shape: not asked about either
    got = _one(c, M, mix)
    assert not _differ(got, want), _differ(got, want)
    with pytest.raises(tdoa_amd.TdoaError) as e:                             # ... and still there for the call that reads it
        c.process_locate_track(M, 1, 2)
    assert e.value.status == 6
    c.locate_set_clock(None)
    assert not _differ(c.process_sync_drift_fine(REF, M, G, HD, D, R, 16, 2, CENTRE), fine0)
    assert not _differ(c.process_locate_track_zoom(Z, H, M, 1, 2, 2, 1, want_total=True), zoom0)


# ---- 4. routes ------------------------------------------------------------------------------------------------------------
def test_the_callers_q_route_and_the_statement(ctx):
    from tdoa_amd import line_mix
    c, q = ctx
    _reset(c)
    for m, U_loc, mix in ((2, 1, line_mix.bridge_mix(2)), (1, 4, line_mix.forward_mix(4))):
        L = c.num_stacks(m)[0]
        Q = c.process_stacked(m, 1, 1, want_partial=True)["partial"]
        c.locate_set_upsample(U_loc)
        own = _one(c, m, mix, U=4, Rf=1)
        b = c.sync_drift_locate_from_q(Q, REF, L, Z, H, m, G, HD, D, R, 4, 1, CENTRE, mix, 1, 2, 2, 1)
        assert not _differ(b, own), _differ(b, own)
        want = _statement(c, q, m, mix, U=4, Rf=1, U_loc=U_loc)
        assert not _differ(own, want), (U_loc, _differ(own, want))
    _reset(c)


@pytest.mark.parametrize("n_members", [1, 2])
def test_group_returns_a_single_contexts_bytes(ctx, n_members):
    import tdoa_amd
    from tdoa_amd import line_mix
    c, _ = ctx
    _reset(c)
    with tdoa_amd.Group([0] * n_members, max_lag=ML, window_len=WL) as g:
        for k in range(n_members):
            _synth(g.member(k))
        g.locate_set_table(TABLE, 8)
        g.locate_set_fine_table(FINE, 29)
        for m, U_loc, mix in ((2, 4, line_mix.bridge_mix(2)), (1, 1, line_mix.forward_mix(4)), (0, 1, None)):
            c.locate_set_upsample(U_loc)
            g.locate_set_upsample(U_loc)
            want = _one(c, m, mix)
            args = (REF, Z, H, m, G, HD, D, R, 16, 2, CENTRE, mix, 1, 2, 2, 1)
            got = g.process_sync_drift_locate(*args, want_total=True)
            again = g.process_sync_drift_locate(*args, want_total=True)
            assert got["mix_rows"].any() and not _differ(got, want) and not _differ(again, want), (m, U_loc, _differ(got, want))
        with pytest.raises(tdoa_amd.TdoaError) as e:
            g.process_sync_drift_locate(REF, Z, H, 0, G, HD, D, R, 16, 2, CENTRE, [[0, 0, 3, 0, 1, 1]] * 3)
        assert e.value.status == 1
    _reset(c)


# ---- 5. the step graph ----------------------------------------------------------------------------------------------------
def test_the_step_graph(ctx):
    from tdoa_amd import line_mix
    c, q = ctx
    _reset(c)
    c.locate_set_upsample(4)
    M = 2
    mix = line_mix.bridge_mix(2)
    kw0 = dict(U=4, Rf=1)                                                    # (the numpy statement of U = 16 is the slow one)
    a = _one(c, M, mix, **kw0)
    first = c.graph_info()
    assert first["memsets"] == 0 and first["roots"] == 1
    want = _statement(c, q, M, mix, U_loc=4, **kw0)
    assert not _differ(a, want), _differ(a, want)
    c.poison_workspace()
    again = _one(c, M, mix, **kw0)                                           # the same key: replayed, on poisoned workspace
    assert c.graph_info() == first and not _differ(again, a)
    moved = _one(c, M, mix, ref=OTHER_REF, **kw0)                            # new delays
    want = _statement(c, q, M, mix, ref=OTHER_REF, U_loc=4, **kw0)
    assert c.graph_info() == first and not _differ(moved, want) and not _same_bytes(moved["mix_rows"], a["mix_rows"]), _differ(moved, want)
    moved = _one(c, M, mix, centre=-CENTRE, **kw0)                           # new centres
    want = _statement(c, q, M, mix, centre=-CENTRE, U_loc=4, **kw0)
    assert c.graph_info() == first and not _differ(moved, want), _differ(moved, want)
    far = np.array([[0, 40, 2, -40, 7, 2]] * 6, dtype=np.int32)              # new mixes of the same length (NULL: the own mix)
    for other in (line_mix.forward_mix(2), far, None):
        moved = _one(c, M, other, **kw0)
        want = _statement(c, q, M, other, U_loc=4, **kw0)
        assert c.graph_info() == first and not _differ(moved, want), _differ(moved, want)
    table2, fine2 = np.ascontiguousarray(TABLE[::-1]), np.ascontiguousarray(FINE[::-1])
    c.locate_set_table(table2, 8)                                            # a new table of the same shape
    moved = _one(c, M, mix, **kw0)
    want = _statement(c, q, M, mix, U_loc=4, table=table2, **kw0)
    assert c.graph_info() == first and not _differ(moved, want) and not _same_bytes(moved["total"], a["total"]), _differ(moved, want)
    c.locate_set_fine_table(fine2, 29)                                       # ... and a new fine table
    moved2 = _one(c, M, mix, **kw0)
    want = _statement(c, q, M, mix, U_loc=4, table=table2, fine=fine2, **kw0)
    assert c.graph_info() == first and not _differ(moved2, want) and not _same_bytes(moved2["zmap"], moved["zmap"]), _differ(moved2, want)
    c.locate_set_table(TABLE, 8)
    c.locate_set_fine_table(FINE, 29)
    for kw in (dict(z=2), dict(h=3), dict(J=0), dict(Jf=1), dict(U=8), dict(Rf=0), dict(hd=1)):     # other keys
        got = _one(c, M, mix, **{**kw0, **kw})
        want = _statement(c, q, M, mix, U_loc=4, **{**kw0, **kw})
        assert not _differ(got, want), (kw, _differ(got, want))
    back = _one(c, M, mix, **kw0)
    assert not _differ(back, a)
    _reset(c)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    import tdoa_amd
    capi = tdoa_amd.capi
    wl = 1024
    ref = np.array([0, 16, 40], dtype=np.int32)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        f = c._L.tdoa_process_sync_drift_locate
        line, fine = np.zeros(3, dtype=capi.SYNC_LINE_DTYPE), np.zeros(3, dtype=capi.SYNC_LINE_DTYPE)
        track, ztrack = np.zeros(3, dtype=capi.CELL_TRACK_DTYPE), np.zeros(3, dtype=capi.CELL_TRACK_DTYPE)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        pref = ref.ctypes.data_as(i32p)

        def tail(pline, pfine, ptrack, pztrack):
            return (pline, None, None, None, None, None, pfine, None, None, None, None, None, None, ptrack, None, None, None, None, None,
                    pztrack, None, None, None, None, None, None)

        def call(m=0, g=1, hd=1, dd=1, r=1, U=16, Rf=2, pref=pref, centre=None, mix=None, J=1, sep=1, z=2, h=2, jf=1, fsep=1, pline=p(line),
                 pfine=p(fine), ptrack=p(track), pztrack=p(ztrack)):
            mm = None if mix is None else np.array(mix, dtype=np.int32)
            cc = None if centre is None else np.array(centre, dtype=np.int32)
            return f(c._h, m, g, hd, dd, r, U, Rf, pref, None if cc is None else cc.ctypes.data_as(i32p),
                     None if mm is None else mm.ctypes.data_as(i32p), J, sep, z, h, jf, fsep, *tail(pline, pfine, ptrack, pztrack))

        c.locate_set_table(TABLE[:, :3], 8)
        c.locate_set_fine_table(FINE[:225, :3], 15)
        assert call() == 6                                                   # no captures
        for s in range(3):
            c.synth_capture(s, 4 * wl, ST4[s], TX, 0x10CA7E00 + s)
        assert call() == 0 and fine["score_q"].all() and ztrack["score_q"].any()
        own = [[0, 0, 0, 0, 1, 0], [1, 0, 1, 0, 1, 0], [2, 0, 2, 0, 1, 0]]     # whole-block stacks: three lines of one stack
        assert call(mix=own) == 0
        for bad in ([3, 0, 0, 0, 1, 1], [-1, 0, 0, 0, 1, 1], [0, 65536, 0, 0, 1, 1], [0, -65536, 0, 0, 1, 1], [0, 0, 3, 0, 1, 1], [0, 0, -1, 0, 1, 1],
                    [0, 0, 0, 65536, 1, 1], [0, 0, 0, -65536, 1, 1], [0, 0, 0, 0, -1, 2], [0, 0, 0, 0, 2, -1], [0, 0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 65536, 1], [0, 0, 0, 0, 2 ** 31 - 1, 2 ** 31 - 1]):
            for at in range(3):
                mix = [row[:] for row in own]
                mix[at] = bad
                assert call(mix=mix) == 1, (bad, at)
        assert call(mix=[[0, 65535, 2, -65535, 65535, 1], [2, -65535, 0, 65535, 0, 65536], [1, 0, 1, 0, 1, 0]]) == 0      # every field at its end
        for kw in (dict(m=-1), dict(g=-1), dict(g=1024), dict(hd=-1), dict(hd=513), dict(dd=0), dict(r=17), dict(r=-1), dict(U=3), dict(U=1),
                   dict(Rf=17), dict(Rf=-1), dict(pref=None), dict(J=-1), dict(J=17), dict(sep=0), dict(z=0), dict(z=65), dict(h=-1), dict(h=65),
                   dict(jf=-1), dict(jf=17), dict(fsep=0),
                   dict(pline=None), dict(pfine=None), dict(ptrack=None), dict(pztrack=None)):      # each required output
            assert call(**kw) == 1, kw
        # the rows' bound: |centre| + gate + 2 + ((max_drift + 1) X) div drift_den < 2^27.  Gate 1, max_drift 2, drift_den 2 and a
        # mix whose largest |x| is 9 (whole-block stacks: L - 1 = 0): 3 + (3 x 9) div 2 = 16, so |centre| <= 2^27 - 17
        reach = [[0, 9, 0, 0, 1, 0], [1, 0, 1, -3, 1, 1], [2, 0, 2, 0, 1, 0]]
        back = [[0, 0, 0, 0, 1, 0], [1, 0, 2, -9, 1, 1], [2, 0, 2, 0, 1, 0]]   # ... of either sign, in either place
        edge = 2 ** 27 - 16
        for mix in (reach, back):
            assert call(hd=2, dd=2, mix=mix, centre=[0, edge - 1, -(edge - 1)]) == 0
            assert call(hd=2, dd=2, mix=mix, centre=[0, edge, 0]) == 1 and call(hd=2, dd=2, mix=mix, centre=[0, 0, -edge]) == 1
            assert "would not fit int32" in c._L.tdoa_last_error(c._h).decode()
        assert call(hd=2, dd=2, centre=[0, edge, -edge]) == 0                # without the mix's reach the same centres pass
        assert call(hd=2, dd=2, centre=[0, 2 ** 27 - 4, 0]) == 0 and call(hd=2, dd=2, centre=[0, 2 ** 27 - 3, 0]) == 1
        # the U_loc bound: 16 x the same sum x U_loc < 2^31: with U_loc = 16 the sum stays below 2^23
        far = 2 ** 23 - 16
        assert call(hd=2, dd=2, mix=reach, centre=[0, far, -far]) == 0
        c.locate_set_upsample(16)
        assert call() == 0
        assert call(hd=2, dd=2, mix=reach, centre=[0, far, 0]) == 5 and call(hd=2, dd=2, mix=back, centre=[0, 0, -far]) == 5
        assert "clock table entry times the upsampling factor" in c._L.tdoa_last_error(c._h).decode()
        assert call(hd=2, dd=2, mix=reach, centre=[0, far - 1, -(far - 1)]) == 0
        assert call(hd=2, dd=2, centre=[0, far, -far]) == 0
        c.locate_set_upsample(1)
        c.locate_set_fine_table(None)                                        # no fine table: the zoomed tracks' status
        with pytest.raises(tdoa_amd.TdoaError) as e:
            c.process_locate_track_zoom(2, 2)
        assert call() == e.value.status == 6
        c.locate_set_fine_table(FINE[:225, :3], 15)
        c.locate_set_table(None)
        assert call() == 6
        c.locate_set_table(TABLE[:, :3], 8)
        # the debug entries
        d = c._L.tdoa_debug_sync_drift_locate_from_q
        q = np.zeros((4, 3, 2 * ML - 1), dtype=np.int64)
        pq = q.ctypes.data_as(i64p)
        t = tail(p(line), p(fine), p(track), p(ztrack))
        ints, late = (1, 1, 1, 1, 16, 2), (1, 1, 2, 2, 1, 1)
        two = np.array([[1, 0, 0, 5, 1, 1], [0, 1, 0, 1, 1, 0], [1, 0, 1, 0, 1, 0], [0, -3, 1, 1, 0, 1]], dtype=np.int32)      # two lines of two sets
        assert d(c._h, pq, 4, 2, 3, 1, *ints, pref, None, two.ctypes.data_as(i32p), *late, *t) == 0
        assert d(c._h, pq, 4, 2, 3, 1, *ints, pref, None, None, *late, *t) == 0
        bad = two.copy()
        bad[3, 2] = 2                                                        # line 2 of 2
        assert d(c._h, pq, 4, 2, 3, 1, *ints, pref, None, bad.ctypes.data_as(i32p), *late, *t) == 1
        assert d(c._h, pq, 4, 4, 3, 1, *ints, pref, None, two.ctypes.data_as(i32p), *late, *t) == 1      # one line of four: line 1 is outside
        assert d(c._h, None, 4, 2, 3, 1, *ints, pref, None, None, *late, *t) == 1
        assert d(c._h, pq, 4, 0, 3, 1, *ints, pref, None, None, *late, *t) == 1
        assert d(c._h, pq, 4, 3, 3, 1, *ints, pref, None, None, *late, *t) == 1                          # not a divisor of n_sets
        assert d(c._h, pq, 0, 1, 3, 1, *ints, pref, None, None, *late, *t) == 1
        assert d(c._h, pq, 4, 2, 1, 1, *ints, pref, None, None, *late, *t) == 1
        assert d(c._h, pq, 4, 2, 3, 5462, *ints, pref, None, None, *late, *t) == 5                       # the fine lines' overflow bound
        c16 = np.zeros((2, 3), dtype=np.int32)
        pc = c16.ctypes.data_as(i32p)
        pm = two[:2].ctypes.data_as(i32p)
        rows, cd = np.zeros((2, 65), dtype=np.int32), np.zeros((2, 2080), dtype=np.int64)
        pr, pd = rows.ctypes.data_as(i32p), cd.ctypes.data_as(i64p)
        dm = c._L.tdoa_debug_line_mix
        assert dm(c._h, pc, pc, 2, 3, 16, 1, pm, 2, 1, pr, pd, pd) == 0
        for n, n_st, U, dd, m, U_loc in ((0, 3, 16, 1, 2, 1), (2, 1, 16, 1, 2, 1), (2, 65, 16, 1, 2, 1), (2, 3, 16, 1, 0, 1), (2, 3, 16, 1, 2, 3),
                                         (2, 3, 16, 1, 2, 32), (65536, 3, 16, 1, 2, 1), (2, 3, 16, 1, 65536, 1), (2, 3, 1, 1, 2, 1), (2, 3, 3, 1, 2, 1),
                                         (2, 3, 32, 1, 2, 1), (2, 3, 16, 0, 2, 1), (1, 3, 16, 1, 2, 1)):
            assert dm(c._h, pc, pc, n, n_st, U, dd, pm, m, U_loc, pr, pd, pd) == 1, (n, n_st, U, dd, m, U_loc)
        for args in ((None, pc, pm, pr, pd, pd), (pc, None, pm, pr, pd, pd), (pc, pc, None, pr, pd, pd), (pc, pc, pm, None, pd, pd),
                     (pc, pc, pm, pr, None, pd), (pc, pc, pm, pr, pd, None)):
            assert dm(c._h, args[0], args[1], 2, 3, 16, 1, args[2], 2, 1, *args[3:]) == 1
        with pytest.raises(tdoa_amd.TdoaError) as e:
            c.debug_line_mix(c16, c16, 16, 1, [[0, 0, 2, 0, 1, 1]])
        assert e.value.status == 1
        with pytest.raises(tdoa_amd.TdoaError) as e:                         # a continued clock that leaves int32: refused on the host
            c.debug_line_mix(np.full((1, 2), 2 ** 31 - 1, dtype=np.int32), np.full((1, 2), 16, dtype=np.int32), 16, 1, [[0, 1, 0, 0, 1, 0]])
        assert e.value.status == 1
    with tdoa_amd.Context(max_lag=ML, window_len=wl, lag_mode=capi.LAGS_GO) as c:
        for s in range(3):
            c.synth_capture(s, 5 * wl, ST4[s], TX, 0x10CA7E00 + s)
        c.locate_set_table(TABLE[:, :3], 8)
        c.locate_set_fine_table(FINE[:225, :3], 15)
        with pytest.raises(tdoa_amd.TdoaError) as e:
            c.process_sync_drift_locate(ref, 2, 2)
        assert e.value.status == 5


# ---- 7. the command line --------------------------------------------------------------------------------------------------
def test_cli_one_call_prints_what_the_chain_prints(tmp_path):
    """tdoa_processor --stack=1 --locate=32x32/30 --sync=LAT,LON,HEIGHT/64/2 --sync-drift=3/2 --sync-drift-fine=16/2 --locate-track=1
    --locate-track-zoom=4/2/1 on the golden three-station captures, with and without --one-call: the same stdout, SYNCLINE,
    SYNCLINEFINE, LOCATE-TRACK and TRACKZOOM lines among it; the refusal and the combinations that get it are what they were"""
    import tdoa_amd
    tdoa_amd.build.build()
    cli = tdoa_amd.build.build_cli()
    csv = tmp_path / "lat-lon-table.csv"
    csv.write_text("Name,Latitude,Longitude,Elevation\nKEVO,41.30888549464701,-96.02619229605524,356.0\n"
                   "162400000,41.25703803095629,-95.95512763589404,349.07\nkx0u,41.18660274289527,-95.96064116595667,355.69\n"
                   "n3pay,41.24669616513154,-96.08366304481238,329.0\nkf0mtl,41.32916620016985,-96.03513381562004,373.18\n")
    dats = [os.path.join(GOLD, "sim-%s-1754900000.dat" % n) for n in ("kx0u", "n3pay", "kf0mtl")]
    opts = ["--window", "2000", "--max-lag", "150"]
    tail = ["162400000", "101700000", str(csv)] + dats
    flag = "--sync=%r,%r,%r/64/2" % (41.25703803095629, -95.95512763589404, 349.07)
    args = ["--stack=1", "--locate=32x32/30", flag, "--sync-drift=3/2", "--sync-drift-fine=16/2", "--locate-track=1", "--locate-track-zoom=4/2/1"]
    chain = subprocess.run([cli] + args + opts + tail, capture_output=True, text=True, timeout=300)
    one = subprocess.run([cli] + args + ["--one-call"] + opts + tail, capture_output=True, text=True, timeout=300)
    assert chain.returncode in (0, 3) and one.returncode == chain.returncode, (chain.stderr, one.stderr)
    for word in ("SYNCLINE block 1", "SYNCLINE block 3", "SYNCLINEFINE block 1", "SYNCLINEFINE block 3", "LOCATE block 2", "LOCATE-TRACK block 2",
                 "TRACKZOOM block 2"):
        assert word in chain.stdout, (word, chain.stdout)
    assert one.stdout == chain.stdout
    for bad in (["--stack", "--locate=32x32/30", "--sync=%r,%r,%r/64/2" % (41.25703803095629, -95.95512763589404, 349.07), "--sync-fine=16/2",
                 "--one-call"],
                ["--stack", "--locate=32x32/30", "--locate-zoom=4/2", "--one-call"],
                args[:5] + ["--locate-track=1", "--one-call"],                # the fine lines without the zoomed tracks
                args[:4] + args[5:] + ["--one-call"]):                       # the zoomed tracks without the fine lines
        r = subprocess.run([cli] + bad + opts + tail, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "--one-call needs --stack --locate --sync --sync-fine --locate-zoom" in r.stderr, (bad, r.stderr)
