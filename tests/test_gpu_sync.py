"""GPU: the clock search (tdoa_process_sync, tdoa_group_process_sync, tdoa_debug_sync_from_q) and the station clocks of the
delay-table search (tdoa_locate_set_clock, tdoa_group_locate_set_clock); include/tdoa_mi355x.h, "clock search".

Every comparison with the numpy models (tdoa_amd.sync, tdoa_amd.locate) is exact: process_stacked(1, 1, 1,
want_partial=True) returns each window's fixed-point q word for word, their sums are the stacks' Q, the models turn those
into records, clocks, lags and correlations.

1. sync_from_q: the hand-worked cases of tests/test_sync_cpu.py; random few-valued words on 2, 3, 5, 16 and 64 stations over
   the gates, rounds and centres at which the kernels take another path; the largest start; words of 2^62 div P;
2. the noisy case of tests/test_sync_cpu.py end to end: the clocks from the reference block, then the target block located
   with them and without;
3. the step graph replays under new delays, centres and clocks, and its neighbours keep their bytes; a stack over several
   launch groups;
4. a group of members on one device returns a single context's bytes;
5. argument and state errors on a live context;
6. tdoa_processor --stack --locate --sync prints what the library returns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from stack_helpers import same_bytes as _same_bytes, stacks_q as _stacks_q, windows_q as _windows_q
from test_locate_cpu import FS, GRID, ST4
from test_sync_cpu import (CLOCKS, _check_hand_case, count_noisy_case, hand_cases, noisy_sync_case, noisy_sync_windows)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ST = ST4[:3]
TX = (41.20, -96.00, 400.0)
SYNC_KEYS = ("sync", "clock", "lags", "corr")
LOC_KEYS = ("loc", "lags", "corr", "map")


def _synth(c, n_stations, block):
    for s in range(n_stations):
        c.synth_capture(s, block, ST[s % 3], TX, 0x10CA7E00 + s)


def _same(got, want, keys):
    """got: a call's dict; want: the model's tuple in the order of keys"""
    return all(_same_bytes(got[k], w) for k, w in zip(keys, want) if k in got)


def _sync_model(c, q, m, ref, G, R, centre=None):
    from tdoa_amd import sync
    Q, n_w = _stacks_q(c, q, m)
    return sync.sync_stacks(Q, ref, c.params.max_lag, G, R, centre, n_w)


def _locate_model(c, q, m, table, n_cols, sep, clock=None):
    from tdoa_amd import locate
    Q, n_w = _stacks_q(c, q, m)
    return locate.locate_stacks(Q, table, n_cols, c.params.max_lag, sep, n_w, clock)


@pytest.fixture(scope="module")
def tiny():
    """contexts of max_lag 4 .. 8 for the hand-worked cases, made on demand"""
    import tdoa_amd
    made = {}

    def get(ml):
        if ml not in made:
            made[ml] = tdoa_amd.Context(max_lag=ml, window_len=1024)
        return made[ml]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_sync_from_q_hand_worked_cases(tiny, name, arg, want):
    from tdoa_amd import sync
    c = tiny(arg["ml"])
    got = c.sync_from_q(arg["q"], arg["ref"], arg["n_w"], arg["G"], arg["R"], arg["centre"])
    assert got["sync"].shape == (1,)
    _check_hand_case((got["sync"][0], got["clock"][0], got["lags"][0], got["corr"][0]), arg, want)
    model = sync.sync(arg["q"], arg["ref"], arg["ml"], arg["G"], arg["R"], arg["centre"], arg["n_w"])
    assert _same(got, [x[None] for x in model], SYNC_KEYS)


@pytest.fixture(scope="module")
def lag64():
    import tdoa_amd
    with tdoa_amd.Context(max_lag=64, window_len=1024) as c:
        yield c


@pytest.mark.parametrize("S", [2, 3, 5, 16, 64])
def test_sync_from_q_random_few_valued_words(lag64, S):
    """3 sets, max_lag 64, words -3 .. 3 with many zeros (equal maxima everywhere).  G 0 and 1: one and nine cells, a partial
    tile; G 37: 5625 cells, 22 tiles, the last one partial; G 63 with centres up to +-70: windows partly and wholly outside
    the range.  R 0, 1 and 3.  S = 2 has no start kernel, S = 3 no placing, S = 64 more pairs than the workgroup has threads"""
    from tdoa_amd import sync
    rng = np.random.default_rng(100 + S)
    ml, P = 64, S * (S - 1) // 2
    q = rng.integers(-3, 4, size=(3, P, 2 * ml - 1), dtype=np.int64) * (rng.random((3, P, 2 * ml - 1)) < 0.5)
    q[2] *= 0 if S == 5 else 1                                           # one set of zeros
    ref = rng.integers(-16 * 20, 16 * 20 + 1, size=S, dtype=np.int32)
    near = rng.integers(-5, 6, size=S, dtype=np.int32)
    far = rng.integers(-70, 71, size=S, dtype=np.int32)
    n_out = n_moved = 0
    for G, centre in ((0, None), (0, near), (1, None), (1, near), (37, None), (37, near), (63, far)):
        for R in (0, 1, 3):
            for n_w in ((1, 5) if R == 1 else (1,)):
                got = lag64.sync_from_q(q, ref, n_w, G, R, centre)
                want = sync.sync_stacks(q, ref, ml, G, R, centre, n_w)
                assert _same(got, want, SYNC_KEYS), (S, G, R, n_w, got["sync"], want[0], got["clock"], want[1])
                rec = got["sync"]
                assert (rec["score_q"] >= rec["start_q"]).all() and (rec["pairs_in"] <= P).all()
                if G == 0:
                    live = rec["score_q"] > 0
                    assert (got["clock"][live] == (0 if centre is None else centre)).all()
                if S == 5:
                    assert rec[2].tobytes() == bytes(32) and not got["clock"][2].any() and not got["lags"][2].any()
                n_out += int((rec["pairs_in"][rec["score_q"] > 0] < P).sum())
                n_moved += int((rec["moved"] > 0).sum())
    one = lag64.sync_from_q(q[1], ref, 1, 37, 1, near)
    assert all(one[k][0].tobytes() == lag64.sync_from_q(q, ref, 1, 37, 1, near)[k][1].tobytes() for k in one)
    print("S %d: %d results with pairs outside the range, %d whose last sweep moved a station" % (S, n_out, n_moved))
    assert n_out >= 1 or S in (2, 5)             # (two stations: the one pair outside leaves F = 0; five: these inputs have none)


def test_sync_from_q_the_largest_start():
    """G = 1023 at max_lag 1024, three stations, two sets: 2047^2 = 4.2 M cells, 16 369 tiles per set, the last one partial.
    Set 0: few distinct values; set 1: one large word per row, far out, so the winner is a cell of large ranks"""
    import tdoa_amd
    from tdoa_amd import sync
    rng = np.random.default_rng(131)
    ml, G = 1024, 1023
    q = rng.integers(-3, 4, size=(2, 3, 2 * ml - 1), dtype=np.int64)
    q[1] = rng.integers(-2, 3, size=(3, 2 * ml - 1))
    q[1, 0, 1010 + ml - 1] = q[1, 1, -990 + ml - 1] = 50                 # (pair 12 would be at lag -2000: outside, it adds 0)
    ref = np.array([0, 16 * 3, -16 * 7], dtype=np.int32)
    with tdoa_amd.Context(max_lag=ml, window_len=4096) as c:
        for R, n_w in ((0, 1), (2, 3)):
            got = c.sync_from_q(q, ref, n_w, G, R)
            assert _same(got, sync.sync_stacks(q, ref, ml, G, R, None, n_w), SYNC_KEYS), (R, got["sync"], got["clock"])
        assert got["clock"][1].tolist() == [0, 1010 - 3, -990 + 7]


def test_sync_from_q_large_words_do_not_overflow():
    """words of magnitude 2^62 div P: F with every pair at the largest word is P (2^62 div P) <= 2^62"""
    import tdoa_amd
    from tdoa_amd import sync
    rng = np.random.default_rng(137)
    S, ml, P = 4, 9, 6
    big = 2 ** 62 // P
    q = rng.choice(np.array([-big, -big + 1, 0, 5, big - 1, big], dtype=np.int64), size=(2, P, 2 * ml - 1))
    q[0, :, ml - 1] = (big, -big, big, -big, big, -big)            # set 0: equal clocks reach the bound
    with tdoa_amd.Context(max_lag=ml, window_len=1024) as c:
        got = c.sync_from_q(q, (0, 0, 0, 0), 3, 4, 2)
        assert _same(got, sync.sync_stacks(q, (0, 0, 0, 0), ml, 4, 2, None, 3), SYNC_KEYS)
        assert int(got["sync"]["score_q"][0]) == P * big and (got["sync"]["score_q"] > 0).all()


def test_the_clock_search_finds_the_clocks_and_the_cell(oracle):
    """the inputs of tests/test_sync_cpu.py as captures of [12 reference | 12 target | 12 reference] windows: process_sync is
    the model on every stack, one window per stack and whole blocks; the target block located with the clocks of the first
    reference block is the model with clock=; the counts of the CPU test hold"""
    import tdoa_amd
    from tdoa_amd import locate
    wl, ml, G, R = 8192, 256, 120, 2
    table, ref_delay, d_ref, planted_cell, d_tgt = noisy_sync_case()
    e = locate.pair_lags(ref_delay[None, :])[0]
    wins_ref, wins_tgt = noisy_sync_windows(oracle, d_ref, d_tgt)
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        for s in range(4):
            c.capture_upload(s, np.concatenate([w[s] for w in wins_ref] + [w[s] for w in wins_tgt] + [w[s] for w in wins_ref]))
        assert c.num_windows() == (12, 36)
        q = _windows_q(c)
        c.locate_set_table(table, 64)
        for m in (1, 0):
            n = c.num_stacks(m)[1]
            got = c.process_sync(ref_delay, m, G, R)
            assert got["sync"].shape == (n,) and got["clock"].shape == (n, 4) and got["lags"].shape == got["corr"].shape == (n, 6)
            assert _same(got, _sync_model(c, q, m, ref_delay, G, R), SYNC_KEYS), (m, got["sync"], got["clock"])
            per = n // 3
            clock = 16 * np.tile(got["clock"][:per], (3, 1))             # every block searched with the first block's clocks
            c.locate_set_clock(clock)
            clocked = c.process_locate(m, 1, want_map=True)
            assert _same(clocked, _locate_model(c, q, m, table, 64, 1, clock), LOC_KEYS), m
            c.locate_set_clock(None)
            plain = c.process_locate(m, 1, want_map=True)
            assert _same(plain, _locate_model(c, q, m, table, 64, 1), LOC_KEYS), m
            if m == 1:
                counts = count_noisy_case(q[:12], q[12:24], (got["sync"][:12], got["clock"][:12]), clocked["loc"][12:24],
                                          plain["loc"][12:24], e, planted_cell, ml)
            else:                                                        # twelve windows stacked: found outright
                assert tuple(got["clock"][0].tolist()) == CLOCKS and tuple(got["clock"][2].tolist()) == CLOCKS
                assert int(clocked["loc"]["cell"][1]) == planted_cell and int(plain["loc"]["cell"][1]) != planted_cell
        own_ok, sync_ok, with_ok, without_ok = counts
        assert own_ok <= 4
        assert sync_ok >= 9
        assert with_ok >= 9
        assert without_ok <= 1


def _grid_table(stations, **kw):
    from tdoa_amd import locate
    return locate.grid_table(stations, sample_rate=FS, **{**GRID, **kw})


def test_graph_replays_and_leaves_its_neighbours_alone():
    import tdoa_amd
    wl, wpb, ml = 10_000, 5, 700
    stations = [ST[s % 3] for s in range(4)]
    grid = _grid_table(stations)
    ref, other_ref = grid[40 * 64 + 10], grid[7 * 64 + 50]
    centre = np.array([0, 3, -4, 2], dtype=np.int32)
    rng = np.random.default_rng(139)
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        _synth(c, 4, wpb * wl)
        q = _windows_q(c)
        n = c.num_stacks(2)[1]
        base = c.process()
        clos = c.process_closure(2, 37, 1)
        stack = c.process_stacked(2, 8, 8, want_surface=True, want_partial=True)
        stack_nodes = c.graph_info()["nodes"]                    # the step, the stack's accumulation and its four finishing kernels
        a = c.process_sync(ref, 2, 37, 2)
        first = c.graph_info()                                   # ... the accumulation, the start and the steps
        assert first["memsets"] == 0 and first["roots"] == 1 and first["nodes"] == stack_nodes - 2
        assert _same(a, _sync_model(c, q, 2, ref, 37, 2), SYNC_KEYS)
        c.poison_workspace()
        b = c.process_sync(ref, 2, 37, 2)                        # the same key: replayed, on poisoned workspace
        assert c.graph_info() == first and all(_same_bytes(a[k], b[k]) for k in a)
        moved = c.process_sync(other_ref, 2, 37, 2)              # new delays: the same graph
        assert c.graph_info() == first
        assert _same(moved, _sync_model(c, q, 2, other_ref, 37, 2), SYNC_KEYS) and not _same_bytes(moved["lags"], a["lags"])
        shifted = c.process_sync(ref, 2, 37, 2, centre)          # new centres: the same graph
        assert c.graph_info() == first
        assert _same(shifted, _sync_model(c, q, 2, ref, 37, 2, centre), SYNC_KEYS)
        assert all(_same_bytes(c.process_sync(ref, 2, 37, 2)[k], a[k]) for k in a)        # ... and back
        for G, R in ((36, 2), (37, 1)):                          # another gate, other rounds: other keys
            assert _same(c.process_sync(ref, 2, G, R), _sync_model(c, q, 2, ref, G, R), SYNC_KEYS), (G, R)
        assert _same_bytes(c.process(), base)
        assert _same_bytes(c.process_closure(2, 37, 1), clos)
        mid = c.process_stacked(2, 8, 8, want_surface=True, want_partial=True)
        assert all(_same_bytes(mid[k], stack[k]) for k in stack)
        # the delay-table search with and without clocks
        c.locate_set_table(grid, 64)
        plain = c.process_locate(2, 1, want_map=True)
        loc_graph = c.graph_info()
        assert _same(plain, _locate_model(c, q, 2, grid, 64, 1), LOC_KEYS)              # today's bytes
        c.locate_set_clock(np.zeros((n, 4), dtype=np.int32))     # a zero clock: the clocked kernel, today's bytes
        zero = c.process_locate(2, 1, want_map=True)
        clocked_graph = c.graph_info()
        assert clocked_graph == loc_graph and all(_same_bytes(zero[k], plain[k]) for k in plain)
        k1 = rng.integers(-16 * 60, 16 * 60 + 1, size=(n, 4), dtype=np.int32)
        k2 = rng.integers(-16 * 60, 16 * 60 + 1, size=(n, 4), dtype=np.int32)
        for k in (k1, k2, k1):                                   # new clocks of the same shape: the same graph
            c.locate_set_clock(k)
            got = c.process_locate(2, 1, want_map=True)
            assert c.graph_info() == clocked_graph
            assert _same(got, _locate_model(c, q, 2, grid, 64, 1, k), LOC_KEYS)
        assert not _same_bytes(got["map"], plain["map"])
        c.locate_set_clock(None)                                 # forgotten: the clock-less kernel again
        assert all(_same_bytes(c.process_locate(2, 1, want_map=True)[k], plain[k]) for k in plain)
        c.locate_set_clock(k2)
        assert _same(c.process_locate(2, 1, want_map=True), _locate_model(c, q, 2, grid, 64, 1, k2), LOC_KEYS)
        assert all(_same_bytes(c.process_sync(ref, 2, 37, 2)[k], a[k]) for k in a)        # the clocks are the locate's alone
        assert _same_bytes(c.process(), base)
        assert _same_bytes(c.process_closure(2, 37, 1), clos)
        after = c.process_stacked(2, 8, 8, want_surface=True, want_partial=True)
        assert all(_same_bytes(after[k], stack[k]) for k in stack)
        far = c.process_locate(2, 1, want_map=True)
    with tdoa_amd.Context(max_lag=ml, window_len=wl, windows_per_batch=1) as c:     # a stack spans several launch groups
        _synth(c, 4, wpb * wl)
        assert all(_same_bytes(c.process_sync(ref, 2, 37, 2)[k], a[k]) for k in a)
        assert all(_same_bytes(c.process_sync(ref, 2, 37, 2, centre)[k], shifted[k]) for k in a)
        c.locate_set_table(grid, 64)
        c.locate_set_clock(k2)
        assert all(_same_bytes(c.process_locate(2, 1, want_map=True)[k], far[k]) for k in far)


@pytest.mark.parametrize("n_members", [1, 2, 3])
def test_group_returns_a_single_contexts_bytes(n_members):
    import tdoa_amd
    block, wl, ml = 50_000, 10_000, 300
    rng = np.random.default_rng(149)
    table, n_cols = rng.integers(-16 * 350, 16 * 350 + 1, size=(700, 4), dtype=np.int32), 29
    ref = rng.integers(0, 16 * 100, size=4, dtype=np.int32)
    centre = np.array([0, -2, 5, 1], dtype=np.int32)
    with tdoa_amd.Group([0] * n_members, max_lag=ml, window_len=wl) as g, tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        for target in [g.member(k) for k in range(n_members)] + [c]:
            _synth(target, 4, block)
        g.locate_set_table(table, n_cols)
        c.locate_set_table(table, n_cols)
        for m in (2, 0):
            for G, R, cen in ((40, 2, None), (9, 0, centre)):
                want = c.process_sync(ref, m, G, R, cen)
                got = g.process_sync(ref, m, G, R, cen)
                again = g.process_sync(ref, m, G, R, cen)            # the members replay their steps
                assert (want["sync"]["score_q"] > 0).all()
                assert all(_same_bytes(got[k], want[k]) and _same_bytes(again[k], want[k]) for k in want), (m, G, R)
            clock = 16 * want["clock"] + rng.integers(-8, 9, size=want["clock"].shape, dtype=np.int32)
            g.locate_set_clock(clock)
            c.locate_set_clock(clock)
            want = c.process_locate(m, 2, want_map=True)
            got = g.process_locate(m, 2, want_map=True)
            assert all(_same_bytes(got[k], want[k]) for k in want), m
            g.locate_set_clock(None)
            c.locate_set_clock(None)
            want = c.process_locate(m, 2, want_map=True)
            assert all(_same_bytes(g.process_locate(m, 2, want_map=True)[k], want[k]) for k in want), m
        g.locate_set_clock(np.zeros((2, 4), dtype=np.int32))         # a clock table of another n_stacks
        with pytest.raises(tdoa_amd.TdoaError) as e:
            g.process_locate(0, 1)
        assert e.value.status == 6
        with pytest.raises(tdoa_amd.TdoaError) as e:
            g.process_sync(ref, 0, 1024, 0)
        assert e.value.status == 1


def test_argument_and_state_errors():
    import tdoa_amd
    wl, ml = 1024, 64
    rng = np.random.default_rng(151)
    table = rng.integers(-16 * 40, 16 * 40 + 1, size=(50, 3), dtype=np.int32)
    ref = np.array([0, 16, 40], dtype=np.int32)

    def status(fn, *a, **kw):
        with pytest.raises(tdoa_amd.TdoaError) as e:
            fn(*a, **kw)
        return e.value.status

    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        f = c._L.tdoa_process_sync
        rec = np.zeros(3, dtype=tdoa_amd.capi.SYNC_DTYPE)
        pref, prec = ref.ctypes.data_as(f.argtypes[4]), rec.ctypes.data_as(C.c_void_p)
        assert f(c._h, 0, 1, 1, pref, None, prec, None, None, None) == 6          # no captures
        _synth(c, 3, 4 * wl)
        assert c.process_sync(ref, 0, 5, 1)["sync"].shape == (3,)
        for m, G, R in ((-1, 1, 1), (0, -1, 1), (0, 1024, 1), (0, 1, -1), (0, 1, 17)):
            assert f(c._h, m, G, R, pref, None, prec, None, None, None) == 1, (m, G, R)
        assert f(c._h, 0, 1, 1, None, None, prec, None, None, None) == 1 and f(c._h, 0, 1, 1, pref, None, None, None, None, None) == 1
        assert f(c._h, 0, 1023, 16, pref, None, prec, None, None, None) == 0      # the largest gate and rounds
        # the clock table
        c.locate_set_table(table, 10)
        k = rng.integers(-99, 100, size=(3, 3), dtype=np.int32)
        c.locate_set_clock(k)
        assert c.process_locate(0, 1)["loc"].shape == (3,)
        g = c._L.tdoa_locate_set_clock
        pk = k.ctypes.data_as(g.argtypes[1])
        for n_stacks, S in ((-1, 3), (65536, 3), (3, 1), (3, 65)):
            assert g(c._h, pk, n_stacks, S) == 1, (n_stacks, S)
        assert c.process_locate(0, 1)["loc"].shape == (3,)           # refused clocks leave the old ones
        c.locate_set_clock(k[:2])                                    # another n_stacks
        assert status(c.process_locate, 0, 1) == 6
        c.locate_set_clock(np.zeros((3, 4), dtype=np.int32))         # another n_stations
        assert status(c.process_locate, 0, 1) == 6
        assert g(c._h, pk, 0, 3) == 0 and c.process_locate(0, 1)["loc"].shape == (3,)        # n_stacks == 0 forgets
        c.locate_set_clock(k)
        assert status(c.process_locate, 1, 1) == 6                   # twelve stacks now
        # the debug entries
        q = np.zeros((1, 3, 2 * ml - 1), dtype=np.int64)
        assert status(c.locate_from_q, q, 3) == 6                    # one set, three rows of clocks
        c.locate_set_clock(k[:1])
        assert c.locate_from_q(q, 3)["loc"].shape == (1,)
        c.locate_set_clock(None)
        d = c._L.tdoa_debug_sync_from_q
        pq = q.ctypes.data_as(d.argtypes[1])
        for n_sets, S, n_w, G, R in ((0, 3, 1, 1, 1), (65536, 3, 1, 1, 1), (1, 1, 1, 1, 1), (1, 65, 1, 1, 1), (1, 3, 0, 1, 1),
                                     (1, 3, 1, 1024, 1), (1, 3, 1, 1, 17)):
            assert d(c._h, pq, n_sets, S, n_w, G, R, pref, None, prec, None, None, None) == 1, (n_sets, S, n_w, G, R)
        assert d(c._h, None, 1, 3, 1, 1, 1, pref, None, prec, None, None, None) == 1
        assert d(c._h, pq, 1, 3, 1, 1, 1, None, None, prec, None, None, None) == 1
        assert d(c._h, pq, 1, 3, 1, 1, 1, pref, None, None, None, None, None) == 1
        # the overflow bound: P n_w <= 2^17; 3 * 43 690 = 131 070, 3 * 43 691 = 131 073
        assert d(c._h, pq, 1, 3, 43690, 1, 1, pref, None, prec, None, None, None) == 0
        assert d(c._h, pq, 1, 3, 43691, 1, 1, pref, None, prec, None, None, None) == 5
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:           # one station: no pair
        _synth(c, 1, 4 * wl)
        rec = np.zeros(3, dtype=tdoa_amd.capi.SYNC_DTYPE)
        assert c._L.tdoa_process_sync(c._h, 0, 1, 1, pref, None, rec.ctypes.data_as(C.c_void_p), None, None, None) == 5
    with tdoa_amd.Context(max_lag=ml, window_len=wl, lag_mode=tdoa_amd.capi.LAGS_GO) as c:
        _synth(c, 3, 5 * wl)
        assert status(c.process_sync, ref, 0, 1, 1) == 5


def test_cli_sync_prints_the_library_result(tmp_path):
    """tdoa_processor --stack --locate=32x32/30 --sync=LAT,LON,HEIGHT/64/2 on the golden three-station captures: a SYNC line for
    blocks 1 and 3 with what process_sync returns for the one-cell table of that position, and the LOCATE lines of
    process_locate under the clock table made of them (block 2: the midpoint); the usage errors; without --sync no line changes"""
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
    emitter = (41.25703803095629, -95.95512763589404, 349.07)
    flag = "--sync=%r,%r,%r/64/2" % emitter
    r = subprocess.run([cli, "--stack", "--locate=32x32/30", flag] + opts + tail, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stderr            # (the 3-station solve may fail on these captures: tests/test_processor_cli.py)
    sync_rows = re.findall(r"^SYNC block (\d): clock=(-?\d+),(-?\d+),(-?\d+) moved=(\d+) score=([\d.]+)$", r.stdout, flags=re.M)
    loc_rows = re.findall(r"^LOCATE block (\d) stack (\d+): cell=(\d+) lat=(-?[\d.]+) lon=(-?[\d.]+) pairs=(\d+) score=([\d.]+) "
                          r"runner=([\d.]+)$", r.stdout, flags=re.M)
    assert [row[0] for row in sync_rows] == ["1", "3"] and sorted(row[0] for row in loc_rows) == ["1", "2", "3"], r.stdout
    # the tool's grid: 30 km on a side around the stations' centroid at their mean height, 111.32 km per degree of latitude
    lat_c, lon_c, h_c = (sum(s[k] / 3 for s in ST) for k in range(3))
    dlat, dlon = 30.0 / 111.32 / 31, 30.0 / (111.32 * np.cos(lat_c * np.pi / 180)) / 31
    lat0, lon0 = lat_c - dlat * 31 / 2, lon_c - dlon * 31 / 2
    with tdoa_amd.Context(max_lag=150, window_len=2000) as c:
        from tdoa_amd import sync
        for s, p in enumerate(dats):
            c.capture_upload_file(s, p)
        assert c.num_stacks(0) == (1, 3)
        fs = c.params.sample_rate
        ref = tdoa_amd.capi.locate_grid_table(ST, emitter[0], emitter[1], 0.0, 0.0, 1, 1, emitter[2], fs)[0]
        found = c.process_sync(ref, 0, 64, 2)
        clock = np.stack([16 * found["clock"][0], sync.midpoint_clock(found["clock"][0], found["clock"][2]), 16 * found["clock"][2]])
        c.locate_set_table(tdoa_amd.capi.locate_grid_table(ST, lat0, lon0, dlat, dlon, 32, 32, h_c, fs), 32)
        c.locate_set_clock(clock)
        out = c.process_locate(0, 1)["loc"]
    for row in sync_rows:
        sid = int(row[0]) - 1
        assert [int(x) for x in row[1:4]] == found["clock"][sid].tolist() and int(row[4]) == int(found["sync"]["moved"][sid])
        assert abs(float(row[5]) - float(found["sync"]["score"][sid])) <= 5.1e-7 and float(row[5]) > 0
    for row in loc_rows:
        rec = out[int(row[0]) - 1]
        cell = int(rec["cell"])
        assert int(row[1]) == 0 and int(row[2]) == cell and int(row[5]) == int(rec["pairs_in"])
        assert abs(float(row[3]) - (lat0 + (cell // 32) * dlat)) <= 5.1e-7 and abs(float(row[4]) - (lon0 + (cell % 32) * dlon)) <= 5.1e-7
        for text, value in ((row[6], float(rec["score"])), (row[7], float(rec["runner_up"]))):
            assert abs(float(text) - value) <= 5.1e-7
    plain = subprocess.run([cli, "--stack", "--locate=32x32/30"] + opts + tail, capture_output=True, text=True, timeout=300)
    assert plain.returncode in (0, 3) and "SYNC" not in plain.stdout
    keep = lambda text: [l for l in text.splitlines() if not l.startswith(("SYNC ", "LOCATE "))]
    assert keep(plain.stdout) == keep(r.stdout)
    for args, what in ((["--stack", flag], "--sync needs --stack --locate"), (["--stack=2", "--locate=32x32/30", flag], "whole-block stacks"),
                       (["--stack", "--locate=32x32/30", "--sync=41.2,-95.9"], "--sync=LAT,LON,HEIGHT"),
                       (["--stack", "--locate=32x32/30", "--sync=41.2,-95.9,300/1024"], "--sync=LAT,LON,HEIGHT")):
        bad = subprocess.run([cli] + args + opts + tail, capture_output=True, text=True, timeout=300)
        assert bad.returncode == 1 and what in bad.stderr, (args, bad.stderr)
