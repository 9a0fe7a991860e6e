"""GPU: clocks to fix in one call (tdoa_process_sync_locate, tdoa_group_process_sync_locate, tdoa_debug_sync_locate_from_q,
tdoa_debug_clock_mix; include/tdoa_mi355x.h, "clocks to fix in one call").

Every comparison is byte for byte.

1. debug_clock_mix, the kernel alone, against clock_mix.mix_rows: the corner list of tests/test_clock_mix_cpu.py, 2, 3, 5 and 64
   stations (2 016 pairs: several passes of the workgroup), 1 and 300 stacks, U_loc 1 and 16; the differences are row[j] - row[i]
   in tdoa_locate_set_clock's pair order and the scaled ones exactly U_loc x them;
2. the chain identity: process_sync_fine, clock_mix_rows, locate_set_clock, process_locate_zoom on one context, then the clock
   table forgotten and process_sync_locate: the same sixteen outputs and rows, for three mixes, three upsample settings, two
   fine searches, whole-block and two-window stacks, with and without map statistics;
3. the context's clock table is neither read nor changed, whatever its shape, and the neighbours keep their bytes;
4. the caller's-Q route and the numpy statement; groups of one and of two members;
5. the step graph replays under new delays, centres, mixes and tables; other Z, H, U, Rf are other keys;
6. what the call refuses;
7. tdoa_processor --one-call prints what the run without the flag prints."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from stack_helpers import same_bytes as _same_bytes, stacks_q as _stacks_q, windows_q as _windows_q
from test_clock_mix_cpu import corner_cases, random_cases
from test_locate_cpu import ST4
from test_sync_fine_cpu import FINE_KEYS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TX = (41.20, -96.00, 400.0)
ML, WL, WPB, M, S = 64, 2048, 4, 2, 4
G, R = 4, 2
Z, H = 4, 2
REF = np.array([0, 16, 40, 72], dtype=np.int32)
OTHER_REF = np.array([5, -30, 11, 64], dtype=np.int32)
CENTRE = np.array([0, 1, -2, 1], dtype=np.int32)
TABLE = np.random.default_rng(19).integers(0, 16 * 30, size=(8 * 8, S), dtype=np.int32)            # 8 x 8 cells
FINE = np.random.default_rng(23).integers(0, 16 * 30, size=(29 * 29, S), dtype=np.int32)           # Z = 4: 29 x 29 fine cells
ZOOM_KEYS = ("loc", "loc_lags", "loc_corr", "map", "zoom", "zlags", "zcorr", "zmap")
KEYS = FINE_KEYS + ("rows",) + ZOOM_KEYS
RANKS = (32768, 64880)
FOOT = 49152


def _differ(got, want):
    return [k for k in set(got) | set(want) if k not in got or k not in want or not _same_bytes(got[k], want[k])]


def _ramp_mix(n):
    """between the first and the last stack, den = 8, every weight 0 .. 8 among them"""
    w = (3 * np.arange(n) + 1) % 9
    return np.stack([np.zeros(n), np.full(n, n - 1), 8 - w, w], axis=1).astype(np.int32)


def _mixes(n_stacks):
    from tdoa_amd import clock_mix
    return (("own", None), ("midpoint", clock_mix.midpoint_mix(n_stacks // 3)), ("ramp", _ramp_mix(n_stacks)))


def _renamed(z):
    return {("loc_" + k if k in ("lags", "corr") else k): v for k, v in z.items()}


def _chain(c, m, mix, ref=REF, centre=CENTRE, U=16, Rf=2, z=Z, h=H, sep=2, fsep=1):
    """the four calls the one call replaces, the clock table forgotten afterwards"""
    import tdoa_amd
    from tdoa_amd import clock_mix
    out = c.process_sync_fine(ref, m, G, R, U, Rf, centre)
    n = out["clock16"].shape[0]
    out["rows"] = tdoa_amd.capi.clock_mix_rows(out["clock16"], clock_mix.own_mix(n) if mix is None else mix)
    c.locate_set_clock(out["rows"])
    out.update(_renamed(c.process_locate_zoom(z, h, m, sep, fsep, want_map=True)))
    c.locate_set_clock(None)
    return out


def _one(c, m, mix, ref=REF, centre=CENTRE, U=16, Rf=2, z=Z, h=H, sep=2, fsep=1):
    return c.process_sync_locate(ref, z, h, m, G, R, U, Rf, centre, mix, sep, fsep, want_map=True)


def _statement(c, q, m, mix, ref=REF, centre=CENTRE, U=16, Rf=2, z=Z, h=H, sep=2, fsep=1, U_loc=1, table=TABLE, fine=FINE):
    from tdoa_amd import sync_locate
    Q, n_w = _stacks_q(c, q, m)
    return sync_locate.sync_locate(Q, ref, table, 8, fine, 29, ML, z, h, mix, G, R, U, Rf, centre, sep, fsep, n_w, U_loc)


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
def _check_mix(c, clock16, mix, U_loc):
    from tdoa_amd import clock_mix
    rows, cdiff, up = c.debug_clock_mix(clock16, mix, U_loc)
    want = clock_mix.mix_rows(clock16, mix)
    assert _same_bytes(rows, want)
    d = clock_mix.pair_differences(want)
    assert _same_bytes(cdiff, d) and _same_bytes(up, U_loc * d)
    return rows


@pytest.mark.parametrize("U_loc", [1, 16])
def test_debug_clock_mix_is_the_numpy_statement(ctx, U_loc):
    c, _ = ctx
    clock16, mix = corner_cases()                                            # one station per stack would be refused: two, the second mirrored
    two = np.concatenate([clock16, -clock16], axis=1)
    rows = _check_mix(c, two, mix, U_loc)
    assert (rows[:, 0] == -rows[:, 1]).all()                                 # halves go away from zero on both sides
    rng = np.random.default_rng(31)
    for n_st in (2, 3, 5, 64):
        for n, m in ((1, 1), (7, 300), (300, 300)):
            c16 = rng.integers(-(2 ** 31 - 16), 2 ** 31 - 15, size=(n, n_st)).astype(np.int32)
            c16[::2] = rng.integers(-9, 10, size=c16[::2].shape)
            den = rng.integers(1, 65537, size=m)
            den[::3] = rng.integers(1, 9, size=len(den[::3]))
            wa = rng.integers(0, den + 1)
            mx = np.stack([rng.integers(0, n, size=m), rng.integers(0, n, size=m), wa, den - wa], axis=1).astype(np.int32)
            _check_mix(c, c16, mx, U_loc)
    clock16, mix = random_cases(7, 300)
    _check_mix(c, clock16, mix, U_loc)


# ---- 2. the chain identity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U_loc", [1, 4, 16])
def test_the_one_call_is_the_chain(ctx, U_loc):
    c, q = ctx
    _reset(c)
    c.locate_set_upsample(U_loc)
    seen = 0
    for m in (M, 0):
        n_stacks = c.num_stacks(m)[1]
        bare = c.process_locate_zoom(Z, H, m, 2, 1)                          # no clocks
        for U, Rf in ((16, 2), (4, 1)):
            for name, mix in _mixes(n_stacks):
                want = _chain(c, m, mix, U=U, Rf=Rf)
                got = _one(c, m, mix, U=U, Rf=Rf)
                assert set(got) == set(KEYS) and not _differ(got, want), (m, U, Rf, name, _differ(got, want))
                assert got["rows"].any() and (got["fine"]["score_q"] > 0).all() and (got["zoom"]["score_q"] > 0).all()
                assert (got["zoom"]["cell"] != bare["zoom"]["cell"]).any(), (m, U, Rf, name)       # a dropped clock would show
                if name == "own":
                    assert _same_bytes(got["rows"], got["clock16"])
                seen += 1
        if U_loc == 1 and m == M:                                            # ... and the statement, once per stack length
            want = _statement(c, q, m, _ramp_mix(n_stacks), U=4, Rf=1)
            assert not _differ(got, want), _differ(got, want)
    assert seen == 12
    c.locate_set_stats(RANKS, FOOT)                                          # map statistics on: the chain's, as after process_locate_zoom
    for name, mix in _mixes(c.num_stacks(M)[1]):
        want = _chain(c, M, mix)
        got = _one(c, M, mix)
        assert set(got) == set(KEYS) | {"stats"} and not _differ(got, want), (name, _differ(got, want))
        assert _same_bytes(c.locate_last_stats().reshape(got["stats"].shape), want["stats"]) and want["stats"]["n_live"].all()
    _reset(c)


# ---- 3. the context's clock table -----------------------------------------------------------------------------------------
def test_the_contexts_clock_table_is_left_alone(ctx):
    import tdoa_amd
    from tdoa_amd import clock_mix
    c, _ = ctx
    _reset(c)
    mix = clock_mix.midpoint_mix(2)
    fine0 = c.process_sync_fine(REF, M, G, R, 16, 2, CENTRE)
    zoom0 = c.process_locate_zoom(Z, H, M, 2, 1, want_map=True)
    want = _chain(c, M, mix)
    other = np.random.default_rng(5).integers(-64, 65, size=(6, S)).astype(np.int32)
    c.locate_set_clock(other)
    plain = c.process_locate(M, 2, want_map=True)
    got = _one(c, M, mix)
    assert not _differ(got, want), _differ(got, want)                       # test 2's bytes: that table has no say
    again = c.process_locate(M, 2, want_map=True)
    assert not _differ(again, plain) and not _same_bytes(plain["map"], zoom0["map"])
    c.locate_set_clock(other[:3])                                            # a table of another shape: not asked about either
    got = _one(c, M, mix)
    assert not _differ(got, want), _differ(got, want)
    with pytest.raises(tdoa_amd.TdoaError) as e:                             # ... and still there for the call that reads it
        c.process_locate(M, 2)
    assert e.value.status == 6
    c.locate_set_clock(None)
    assert not _differ(c.process_sync_fine(REF, M, G, R, 16, 2, CENTRE), fine0)
    assert not _differ(c.process_locate_zoom(Z, H, M, 2, 1, want_map=True), zoom0)


# ---- 4. routes ------------------------------------------------------------------------------------------------------------
def test_the_callers_q_route_and_the_statement(ctx):
    from tdoa_amd import clock_mix
    c, q = ctx
    _reset(c)
    Q = c.process_stacked(M, 1, 1, want_partial=True)["partial"]
    for U_loc, mix in ((1, clock_mix.midpoint_mix(2)), (4, _ramp_mix(6))):
        c.locate_set_upsample(U_loc)
        own = _one(c, M, mix)
        b = c.sync_locate_from_q(Q, REF, Z, H, M, G, R, 16, 2, CENTRE, mix, 2, 1)
        assert not _differ(b, own), _differ(b, own)
        want = _statement(c, q, M, mix, U_loc=U_loc)
        assert not _differ(own, want), (U_loc, _differ(own, want))
    _reset(c)


@pytest.mark.parametrize("n_members", [1, 2])
def test_group_returns_a_single_contexts_bytes(ctx, n_members):
    import tdoa_amd
    from tdoa_amd import clock_mix
    c, _ = ctx
    _reset(c)
    with tdoa_amd.Group([0] * n_members, max_lag=ML, window_len=WL) as g:
        for k in range(n_members):
            _synth(g.member(k))
        g.locate_set_table(TABLE, 8)
        g.locate_set_fine_table(FINE, 29)
        for m, U_loc, mix in ((M, 4, clock_mix.midpoint_mix(2)), (0, 1, None)):
            c.locate_set_upsample(U_loc)
            g.locate_set_upsample(U_loc)
            want = _one(c, m, mix)
            got = g.process_sync_locate(REF, Z, H, m, G, R, 16, 2, CENTRE, mix, 2, 1, want_map=True)
            again = g.process_sync_locate(REF, Z, H, m, G, R, 16, 2, CENTRE, mix, 2, 1, want_map=True)
            assert got["rows"].any() and not _differ(got, want) and not _differ(again, want), (m, U_loc, _differ(got, want))
        with pytest.raises(tdoa_amd.TdoaError) as e:
            g.process_sync_locate(REF, Z, H, 0, G, R, 16, 2, CENTRE, [[0, 3, 1, 1]] * 3)
        assert e.value.status == 1
    _reset(c)


# ---- 5. the step graph ----------------------------------------------------------------------------------------------------
def test_the_step_graph(ctx):
    from tdoa_amd import clock_mix
    c, q = ctx
    _reset(c)
    c.locate_set_upsample(4)
    mix = clock_mix.midpoint_mix(2)
    a = _one(c, M, mix)
    first = c.graph_info()
    assert first["memsets"] == 0 and first["roots"] == 1
    want = _statement(c, q, M, mix, U_loc=4)
    assert not _differ(a, want), _differ(a, want)
    c.poison_workspace()
    again = _one(c, M, mix)                                                  # the same key: replayed, on poisoned workspace
    assert c.graph_info() == first and not _differ(again, a)
    moved = _one(c, M, mix, ref=OTHER_REF)                                   # new delays
    want = _statement(c, q, M, mix, ref=OTHER_REF, U_loc=4)
    assert c.graph_info() == first and not _differ(moved, want) and not _same_bytes(moved["rows"], a["rows"]), _differ(moved, want)
    moved = _one(c, M, mix, centre=-CENTRE)                                  # new centres
    want = _statement(c, q, M, mix, centre=-CENTRE, U_loc=4)
    assert c.graph_info() == first and not _differ(moved, want), _differ(moved, want)
    for other in (_ramp_mix(6), None):                                       # new mixes of the same length (NULL: the own mix)
        moved = _one(c, M, other)
        want = _statement(c, q, M, other, U_loc=4)
        assert c.graph_info() == first and not _differ(moved, want), _differ(moved, want)
    table2, fine2 = np.ascontiguousarray(TABLE[::-1]), np.ascontiguousarray(FINE[::-1])
    c.locate_set_table(table2, 8)                                            # new tables of the same shape
    c.locate_set_fine_table(fine2, 29)
    moved = _one(c, M, mix)
    want = _statement(c, q, M, mix, U_loc=4, table=table2, fine=fine2)
    assert c.graph_info() == first and not _differ(moved, want) and not _same_bytes(moved["map"], a["map"]), _differ(moved, want)
    c.locate_set_table(TABLE, 8)
    c.locate_set_fine_table(FINE, 29)
    for kw in (dict(z=2), dict(h=3), dict(U=8), dict(Rf=0)):                 # other keys
        got = _one(c, M, mix, **kw)
        want = _statement(c, q, M, mix, U_loc=4, **kw)
        assert not _differ(got, want), (kw, _differ(got, want))
    back = _one(c, M, mix)
    assert not _differ(back, a)
    _reset(c)


# ---- 6. errors ------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors():
    import tdoa_amd
    capi = tdoa_amd.capi
    wl = 1024
    ref = np.array([0, 16, 40], dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        f = c._L.tdoa_process_sync_locate
        sync, fine = np.zeros(3, dtype=capi.SYNC_DTYPE), np.zeros(3, dtype=capi.SYNC_DTYPE)
        loc, zoom = np.zeros(3, dtype=capi.LOCATION_DTYPE), np.zeros(3, dtype=capi.ZOOM_DTYPE)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        pref = ref.ctypes.data_as(i32p)

        def call(m=0, g=1, r=1, U=16, Rf=2, pref=pref, centre=None, mix=None, sep=1, z=2, h=2, fsep=1, psync=p(sync), pfine=p(fine), ploc=p(loc),
                 pzoom=p(zoom)):
            mm = None if mix is None else np.array(mix, dtype=np.int32)
            cc = None if centre is None else np.array(centre, dtype=np.int32)
            return f(c._h, m, g, r, U, Rf, pref, None if cc is None else cc.ctypes.data_as(i32p), None if mm is None else mm.ctypes.data_as(i32p),
                     sep, z, h, fsep, psync, None, None, None, pfine, None, None, None, None, ploc, None, None, None, pzoom, None, None, None)

        c.locate_set_table(TABLE[:, :3], 8)
        c.locate_set_fine_table(FINE[:225, :3], 15)
        assert call() == 6                                                   # no captures
        for s in range(3):
            c.synth_capture(s, 4 * wl, ST4[s], TX, 0x10CA7E00 + s)
        assert call() == 0 and fine["score_q"].all() and zoom["score_q"].all()
        own = [[0, 0, 1, 0], [1, 1, 1, 0], [2, 2, 1, 0]]
        assert call(mix=own) == 0
        for bad in ([0, 3, 1, 1], [3, 0, 1, 1], [-1, 0, 1, 1], [0, -1, 1, 1], [0, 0, -1, 2], [0, 0, 2, -1], [0, 0, 0, 0], [0, 0, 65536, 1],
                    [0, 0, 2 ** 31 - 1, 2 ** 31 - 1]):
            for at in range(3):
                mix = [row[:] for row in own]
                mix[at] = bad
                assert call(mix=mix) == 1, (bad, at)
        assert call(mix=[[0, 2, 65535, 1], [2, 0, 0, 65536], [1, 1, 1, 0]]) == 0          # the largest den
        for kw in (dict(m=-1), dict(g=-1), dict(g=1024), dict(r=17), dict(U=3), dict(U=1), dict(Rf=17), dict(Rf=-1), dict(pref=None),
                   dict(sep=0), dict(z=0), dict(z=65), dict(h=-1), dict(h=65), dict(fsep=0),
                   dict(psync=None), dict(pfine=None), dict(ploc=None), dict(pzoom=None)):     # each required output
            assert call(**kw) == 1, kw
        # the U_loc bound: 16 (|centre| + gate + 1) U_loc < 2^31: with gate 1 and U_loc = 16, |centre| <= 2^23 - 3
        far = [0, 2 ** 23 - 2, -(2 ** 23 - 2)]
        assert call(centre=far) == 0
        c.locate_set_upsample(16)
        assert call() == 0
        assert call(centre=far) == 5 and "clock table entry times the upsampling factor" in c._L.tdoa_last_error(c._h).decode()
        assert call(centre=[0, 2 ** 23 - 3, -(2 ** 23 - 3)]) == 0
        c.locate_set_upsample(1)
        c.locate_set_fine_table(None)                                        # no fine table: the zoom's status
        with pytest.raises(tdoa_amd.TdoaError) as e:
            c.process_locate_zoom(2, 2)
        assert call() == e.value.status == 6
        c.locate_set_fine_table(FINE[:225, :3], 15)
        c.locate_set_table(None)
        assert call() == 6
        c.locate_set_table(TABLE[:, :3], 8)
        # the debug entries
        d = c._L.tdoa_debug_sync_locate_from_q
        q = np.zeros((2, 3, 2 * ML - 1), dtype=np.int64)
        pq = q.ctypes.data_as(C.POINTER(C.c_int64))
        tail = (p(sync), None, None, None, p(fine), None, None, None, None, p(loc), None, None, None, p(zoom), None, None, None)
        two = np.array([[1, 0, 1, 1], [0, 0, 1, 0]], dtype=np.int32)
        assert d(c._h, pq, 2, 3, 1, 1, 1, 16, 2, pref, None, two.ctypes.data_as(i32p), 1, 2, 2, 1, *tail) == 0
        bad = np.array([[2, 0, 1, 1], [0, 0, 1, 0]], dtype=np.int32)         # set 2 of 2
        assert d(c._h, pq, 2, 3, 1, 1, 1, 16, 2, pref, None, bad.ctypes.data_as(i32p), 1, 2, 2, 1, *tail) == 1
        assert d(c._h, None, 2, 3, 1, 1, 1, 16, 2, pref, None, None, 1, 2, 2, 1, *tail) == 1
        assert d(c._h, pq, 2, 3, 10923, 1, 1, 16, 2, pref, None, None, 1, 2, 2, 1, *tail) == 5      # the fine search's overflow bound
        c16 = np.zeros((2, 3), dtype=np.int32)
        for n, n_st, m, U_loc in ((0, 3, 2, 1), (2, 1, 2, 1), (2, 65, 2, 1), (2, 3, 0, 1), (2, 3, 2, 3), (2, 3, 2, 32), (65536, 3, 2, 1)):
            rows, cd = np.zeros((2, 65), dtype=np.int32), np.zeros((2, 2080), dtype=np.int64)
            assert c._L.tdoa_debug_clock_mix(c._h, c16.ctypes.data_as(i32p), n, n_st, two.ctypes.data_as(i32p), m, U_loc, rows.ctypes.data_as(i32p),
                                             cd.ctypes.data_as(C.POINTER(C.c_int64)), cd.ctypes.data_as(C.POINTER(C.c_int64))) == 1, (n, n_st, m, U_loc)
        with pytest.raises(tdoa_amd.TdoaError) as e:
            c.debug_clock_mix(c16, [[0, 2, 1, 1]])
        assert e.value.status == 1
    with tdoa_amd.Context(max_lag=ML, window_len=wl, lag_mode=capi.LAGS_GO) as c:
        for s in range(3):
            c.synth_capture(s, 5 * wl, ST4[s], TX, 0x10CA7E00 + s)
        c.locate_set_table(TABLE[:, :3], 8)
        c.locate_set_fine_table(FINE[:225, :3], 15)
        with pytest.raises(tdoa_amd.TdoaError) as e:
            c.process_sync_locate(ref, 2, 2)
        assert e.value.status == 5


# ---- 7. the command line --------------------------------------------------------------------------------------------------
def test_cli_one_call_prints_what_the_chain_prints(tmp_path):
    """tdoa_processor --stack --locate=32x32/30 --sync=LAT,LON,HEIGHT/64/2 --sync-fine=16/2 --locate-zoom=4/2 on the golden
    three-station captures, with and without --one-call: the same stdout, SYNC, SYNCFINE, LOCATE and ZOOM lines among it"""
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
    args = ["--stack", "--locate=32x32/30", flag, "--sync-fine=16/2", "--locate-zoom=4/2"]
    chain = subprocess.run([cli] + args + opts + tail, capture_output=True, text=True, timeout=300)
    one = subprocess.run([cli] + args + ["--one-call"] + opts + tail, capture_output=True, text=True, timeout=300)
    assert chain.returncode in (0, 3) and one.returncode == chain.returncode, (chain.stderr, one.stderr)
    for word in ("SYNC block 1", "SYNC block 3", "SYNCFINE block 1", "SYNCFINE block 3", "LOCATE block 2", "ZOOM block 2"):
        assert word in chain.stdout, (word, chain.stdout)
    assert one.stdout == chain.stdout
    for bad in (["--stack", "--locate=32x32/30", flag, "--sync-fine=16/2", "--one-call"],
                ["--stack", "--locate=32x32/30", flag, "--locate-zoom=4/2", "--one-call"],
                ["--stack", "--locate=32x32/30", "--locate-zoom=4/2", "--one-call"]):
        r = subprocess.run([cli] + bad + opts + tail, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "--one-call needs --stack --locate --sync --sync-fine --locate-zoom" in r.stderr, (bad, r.stderr)
