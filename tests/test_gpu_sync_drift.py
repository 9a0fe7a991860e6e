"""GPU: the clock-line search (tdoa_process_sync_drift, tdoa_group_process_sync_drift, tdoa_debug_sync_drift_from_q);
include/tdoa_mi355x.h, "clock lines".

Every comparison with the numpy model (tdoa_amd.sync_drift) is exact: process_stacked(1, 1, 1, want_partial=True) returns
each window's fixed-point q word for word, their sums are the stacks' Q, the model turns those into records, clocks, rates,
rows, lags and correlations.

1. sync_drift_from_q: the hand-worked cases of tests/test_sync_drift_cpu.py; random few-valued words on 2, 3, 5, 16 and 64
   stations over the lines, gates, slopes and rounds at which the kernels take another path; the largest candidate count;
   words of 2^62 div (P L);
2. the noisy case of tests/test_sync_drift_cpu.py end to end: the line from the reference block, then the target block
   tracked under the line continued;
3. the step graph replays under new delays and centres, and its neighbours keep their bytes; a stack over several launch
   groups;
4. a group of members on one device returns a single context's bytes;
5. argument and state errors on a live context;
6. tdoa_processor --stack=M --locate --sync --sync-drift prints what the library returns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from stack_helpers import same_bytes as _same_bytes, stacks_q as _stacks_q, windows_q as _windows_q
from test_locate_cpu import FS, GRID, ST4
from test_sync_cpu import CLOCKS, noisy_sync_case
from test_sync_drift_cpu import (NOISY, RATES, check_hand_case, hand_cases, noisy_drift_windows, random_lines, true_clocks)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ST = ST4[:3]
TX = (41.20, -96.00, 400.0)
KEYS = ("line", "clock", "rate", "rows", "lags", "corr")


def _synth(c, n_stations, block):
    for s in range(n_stations):
        c.synth_capture(s, block, ST[s % 3], TX, 0x10CA7E00 + s)


def _same(got, want):
    """got: a call's dict; want: the model's tuple in the order of KEYS"""
    return all(_same_bytes(got[k], w) for k, w in zip(KEYS, want))


def _model(c, q, m, ref, G, H, D, R, centre=None):
    from tdoa_amd import sync_drift
    Q, n_w = _stacks_q(c, q, m)
    return sync_drift.sync_lines(Q, len(Q) // 3, ref, c.params.max_lag, G, H, D, R, centre, n_w)


@pytest.fixture(scope="module")
def tiny():
    """contexts of max_lag 3 .. 8 for the hand-worked cases, made on demand"""
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
def test_from_q_hand_worked_cases(tiny, name, arg, want):
    from tdoa_amd import sync_drift
    c = tiny(arg["ml"])
    L = len(arg["q"])
    got = c.sync_drift_from_q(arg["q"], arg["ref"], L, arg["n_w"], arg["G"], arg["H"], arg["D"], arg["R"], arg["centre"])
    assert got["line"].shape == (1,)
    check_hand_case((got["line"][0], got["clock"][0], got["rate"][0], got["rows"], got["lags"], got["corr"]), arg, want)
    assert _same(got, sync_drift.sync_lines(arg["q"], L, arg["ref"], arg["ml"], arg["G"], arg["H"], arg["D"], arg["R"], arg["centre"],
                                            arg["n_w"]))


@pytest.fixture(scope="module")
def lag64():
    import tdoa_amd
    with tdoa_amd.Context(max_lag=64, window_len=1024) as c:
        yield c


@pytest.mark.parametrize("S", [2, 3, 5, 16, 64])
def test_from_q_random_few_valued_words(lag64, S):
    """3 lines of L = 1, 2 and 7 positions, max_lag 64, words -3 .. 3 with many zeros (equal maxima everywhere).  G 0 with H 0:
    one candidate; G 1 and H 1: nine, a partial tile; G 37 with H 5: 825 candidates, four tiles, the last one partial; centres
    up to +-70: windows partly and wholly outside the range.  D 1 and 4, R 0, 1 and 3.  S = 5 has a line of zeros, S = 64 more
    pairs than a workgroup has threads"""
    from tdoa_amd import sync_drift
    rng = np.random.default_rng(200 + S)
    ml, P = 64, S * (S - 1) // 2
    near = rng.integers(-5, 6, size=S, dtype=np.int32)
    n_out = n_moved = n_sloped = n = 0
    for L in (1, 2, 7):
        q, ref, far = random_lines(rng, S, ml, 3, L, span=70, zero_line=2 if S == 5 else None, ref_span=16 * 20)
        combos = [(0, 0, 1, 0, None), (1, 1, 1, 1, near), (37, 5, 4, 3, near), (37, 0, 1, 1, far), (0, 5, 4, 1, None),
                  (1, 5, 1, 0, far), (37, 1, 4, 1, None), (1, 0, 4, 3, near), (0, 1, 1, 3, far)]
        if S == 64:                                                  # (the model's time: the many-tile search on the long lines only)
            combos = combos[:2] + (combos[2:3] if L == 7 else []) + [combos[3], combos[7]]
        for G, H, D, R, centre in combos:
            for n_w in ((1, 5) if R == 1 else (1,)):
                got = lag64.sync_drift_from_q(q, ref, L, n_w, G, H, D, R, centre)
                want = sync_drift.sync_lines(q, L, ref, ml, G, H, D, R, centre, n_w)
                assert _same(got, want), (S, L, G, H, D, R, n_w, got["line"], want[0], got["clock"], want[1], got["rate"], want[2])
                rec = got["line"]
                live = rec["score_q"] > 0
                assert (rec["score_q"] >= rec["start_q"]).all() and (rec["terms_in"] <= L * P).all() and (rec["positions"][live] == L).all()
                if G == 0:
                    assert (got["clock"][live] == (0 if centre is None else centre)).all()
                if H == 0 or L == 1:
                    assert not got["rate"].any()
                if S == 5:
                    assert rec[2].tobytes() == bytes(40) and not got["rows"][2 * L:].any() and not got["lags"][2 * L:].any()
                n += 1
                n_out += int((rec["terms_in"][live] < L * P).sum())
                n_moved += int((rec["moved"] > 0).sum())
                n_sloped += int(got["rate"].any(axis=1).sum())
    one = lag64.sync_drift_from_q(q[7:14], ref, 7, 1, 37, 5, 4, 1, near)
    three = lag64.sync_drift_from_q(q, ref, 7, 1, 37, 5, 4, 1, near)
    assert all(one[k][0].tobytes() == three[k][1].tobytes() for k in KEYS[:3])
    assert all(one[k].tobytes() == three[k][7:14].tobytes() for k in KEYS[3:])
    print("S %d: %d calls, %d lines with terms outside the range, %d whose last sweep moved a station, %d with a slope"
          % (S, n, n_out, n_moved, n_sloped))
    assert n_out >= 1 and n_sloped >= 1 and (n_moved >= 1 or S == 2)


def test_from_q_the_largest_candidate_count():
    """G = 1023 with H = 2 at max_lag 1024, three stations, two lines of three positions: 2047 x 5 = 10 235 candidates, 40 tiles,
    the last one partial.  Line 0: few distinct values; line 1: one large word per row and position along slopes +2 and -1,
    far out, so the winners are candidates of large ranks"""
    import tdoa_amd
    from tdoa_amd import sync_drift
    rng = np.random.default_rng(231)
    ml, G, H, L = 1024, 1023, 2, 3
    q = rng.integers(-3, 4, size=(2 * L, 3, 2 * ml - 1), dtype=np.int64)
    q[L:] = rng.integers(-2, 3, size=(L, 3, 2 * ml - 1))
    for j in range(L):
        q[L + j, 0, 1010 + 2 * j + ml - 1] = q[L + j, 1, -990 - j + ml - 1] = 50       # (pair 12 would be near lag -2000: outside)
    ref = np.array([0, 16 * 3, -16 * 7], dtype=np.int32)
    with tdoa_amd.Context(max_lag=ml, window_len=4096) as c:
        for R, n_w in ((0, 1), (2, 3)):
            got = c.sync_drift_from_q(q, ref, L, n_w, G, H, 1, R)
            assert _same(got, sync_drift.sync_lines(q, L, ref, ml, G, H, 1, R, None, n_w)), (R, got["line"], got["clock"], got["rate"])
        assert got["clock"][1].tolist() == [0, 1010 - 3, -990 + 7] and got["rate"][1].tolist() == [0, 2, -1]


def test_from_q_large_words_do_not_overflow():
    """words of magnitude 2^62 div (P L): F with every term at the largest word is P L (2^62 div (P L)) <= 2^62"""
    import tdoa_amd
    from tdoa_amd import sync_drift
    rng = np.random.default_rng(237)
    S, ml, P, L = 4, 9, 6, 3
    big = 2 ** 62 // (P * L)
    q = rng.choice(np.array([-big, -big + 1, 0, 5, big - 1, big], dtype=np.int64), size=(2 * L, P, 2 * ml - 1))
    q[:L, :, ml - 1] = (big, -big, big, -big, big, -big)           # line 0: equal clocks without a slope reach the bound
    with tdoa_amd.Context(max_lag=ml, window_len=1024) as c:
        got = c.sync_drift_from_q(q, (0, 0, 0, 0), L, 3, 4, 2, 3, 2)
        assert _same(got, sync_drift.sync_lines(q, L, (0, 0, 0, 0), ml, 4, 2, 3, 2, None, 3))
        assert int(got["line"]["score_q"][0]) == P * L * big and (got["line"]["score_q"] > 0).all()


def test_the_line_finds_sliding_clocks_and_the_cell(oracle):
    """the inputs of tests/test_sync_drift_cpu.py as captures of [12 reference | 12 target | 12 reference] windows of 8 192, the
    clocks sliding on through all 36: process_sync_drift on one-window stacks is the model on the library's own words, in
    every block; the counts of the CPU test hold over twelve such captures -- the line's offsets and rates exact, the clock
    search on one-window stacks (three captures) and on the whole block not, and the J = 0 cell track of the target block (six
    captures) on the planted cell under the line continued over positions 12 .. 23, not under the whole block's clocks"""
    import tdoa_amd
    from tdoa_amd import sync_drift
    wl = 8192
    ml, G, H, D, R, M = (NOISY[k] for k in ("ml", "G", "H", "D", "R", "M"))
    table, ref_delay, d_ref, planted_cell, d_tgt = noisy_sync_case()
    line_ok = whole_ok = per_ok = track_line = track_whole = 0
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        c.locate_set_table(table, 64)
        for b in range(12):
            blocks = [noisy_drift_windows(oracle, d_ref, b, 0, 300), noisy_drift_windows(oracle, d_tgt, b, M, 700),
                      noisy_drift_windows(oracle, d_ref, b, 2 * M, 300) if b == 0 else None]
            blocks[2] = blocks[2] or blocks[0]
            for s in range(4):
                c.capture_upload(s, np.concatenate([w[s] for blk in blocks for w in blk]))
            assert c.num_windows() == (M, 3 * M) and c.num_stacks(1) == (M, 3 * M)
            c.locate_set_clock(None)
            got = c.process_sync_drift(ref_delay, 1, G, H, D, R)
            assert got["line"].shape == (3,) and got["clock"].shape == got["rate"].shape == (3, 4)
            assert got["rows"].shape == (3 * M, 4) and got["lags"].shape == got["corr"].shape == (3 * M, 6)
            if b < 2:
                assert _same(got, _model(c, _windows_q(c), 1, ref_delay, G, H, D, R)), (b, got["line"], got["clock"], got["rate"])
            rec = got["line"][0]
            assert rec["score_q"] >= rec["start_q"] > 0 and rec["terms_in"] == 6 * M and rec["positions"] == M
            exact = got["clock"][0].tolist() == list(CLOCKS) and got["rate"][0].tolist() == list(RATES)
            line_ok += exact
            if b == 0:                                               # the third block continues the slide: its own line
                assert exact and got["clock"][2].tolist() == true_clocks(2 * M)[0] and got["rate"][2].tolist() == list(RATES)
                assert got["rows"][2 * M:].tolist() == (16 * np.array(true_clocks(2 * M))).tolist()
            whole = c.process_sync(ref_delay, 0, G, R)["clock"][0]
            whole_ok += whole.tolist() == list(CLOCKS)
            if b < 3:
                per = c.process_sync(ref_delay, 1, G, R)["clock"][:M]
                per_ok += sum(per[w].tolist() == true_clocks(0)[w] for w in range(M))
            if b < 6:
                cont = tdoa_amd.capi.sync_line_clock(got["clock"][0], got["rate"][0], D, M, M)
                assert _same_bytes(cont, sync_drift.line_clock(got["clock"][0], got["rate"][0], D, M, M))
                c.locate_set_clock(np.tile(cont, (3, 1)))
                track_line += int(c.process_locate_track(1, 0, 1)["track"]["cell"][1] == planted_cell)
                c.locate_set_clock(np.tile(16 * whole.astype(np.int32), (3 * M, 1)))
                track_whole += int(c.process_locate_track(1, 0, 1)["track"]["cell"][1] == planted_cell)
    print("offsets and rates exact in %d of 12 captures; the clock search right in %d of 36 one-window stacks and at %d of 12 "
          "whole-block stacks; the target block's track on the planted cell in %d of 6 with the line's clocks, %d with the whole "
          "block's" % (line_ok, per_ok, whole_ok, track_line, track_whole))
    assert line_ok >= 10
    assert per_ok <= 6
    assert whole_ok <= 1
    assert track_line >= 5
    assert track_whole <= 1


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
    args = (37, 2, 2, 2)                                         # G, H, D, R
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        _synth(c, 4, wpb * wl)
        q = _windows_q(c)
        assert c.num_stacks(2) == (3, 9)                         # lines of three positions, the last stack one window short
        base = c.process()
        sync = c.process_sync(ref, 2, 37, 2)
        stack = c.process_stacked(2, 8, 8, want_surface=True, want_partial=True)
        c.locate_set_table(grid, 64)
        loc = c.process_locate(2, 1, want_map=True)
        a = c.process_sync_drift(ref, 2, *args)
        first = c.graph_info()
        assert first["memsets"] == 0 and first["roots"] == 1
        assert _same(a, _model(c, q, 2, ref, *args)) and (a["line"]["score_q"] > 0).all() and (a["line"]["positions"] == 3).all()
        c.poison_workspace()
        b = c.process_sync_drift(ref, 2, *args)                  # the same key: replayed, on poisoned workspace
        assert c.graph_info() == first and all(_same_bytes(a[k], b[k]) for k in a)
        moved = c.process_sync_drift(other_ref, 2, *args)        # new delays: the same graph
        assert c.graph_info() == first
        assert _same(moved, _model(c, q, 2, other_ref, *args)) and not _same_bytes(moved["lags"], a["lags"])
        shifted = c.process_sync_drift(ref, 2, *args, centre)    # new centres: the same graph
        assert c.graph_info() == first
        assert _same(shifted, _model(c, q, 2, ref, *args, centre))
        assert all(_same_bytes(c.process_sync_drift(ref, 2, *args)[k], a[k]) for k in a)          # ... and back
        for other in ((36, 2, 2, 2), (37, 3, 2, 2), (37, 2, 3, 2), (37, 2, 2, 1)):                # another G, H, D or R: other keys
            assert _same(c.process_sync_drift(ref, 2, *other), _model(c, q, 2, ref, *other)), other
        assert c.graph_info()["nodes"] < first["nodes"]          # (one sweep fewer: fewer launches)
        whole = c.process_sync_drift(ref, 0, *args)              # whole blocks: lines of one position, no slope
        assert _same(whole, _model(c, q, 0, ref, *args)) and not whole["rate"].any()
        assert all(_same_bytes(c.process_sync_drift(ref, 2, *args)[k], a[k]) for k in a)
        assert _same_bytes(c.process(), base)
        assert all(_same_bytes(c.process_sync(ref, 2, 37, 2)[k], sync[k]) for k in sync)
        after = c.process_stacked(2, 8, 8, want_surface=True, want_partial=True)
        assert all(_same_bytes(after[k], stack[k]) for k in stack)
        assert all(_same_bytes(c.process_locate(2, 1, want_map=True)[k], loc[k]) for k in loc)
    with tdoa_amd.Context(max_lag=ml, window_len=wl, windows_per_batch=1) as c:     # a stack spans several launch groups
        _synth(c, 4, wpb * wl)
        assert all(_same_bytes(c.process_sync_drift(ref, 2, *args)[k], a[k]) for k in a)
        assert all(_same_bytes(c.process_sync_drift(ref, 2, *args, centre)[k], shifted[k]) for k in a)


@pytest.mark.parametrize("n_members", [1, 2, 3])
def test_group_returns_a_single_contexts_bytes(n_members):
    import tdoa_amd
    block, wl, ml = 50_000, 10_000, 300
    rng = np.random.default_rng(249)
    ref = rng.integers(0, 16 * 100, size=4, dtype=np.int32)
    centre = np.array([0, -2, 5, 1], dtype=np.int32)
    with tdoa_amd.Group([0] * n_members, max_lag=ml, window_len=wl) as g, tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        for target in [g.member(k) for k in range(n_members)] + [c]:
            _synth(target, 4, block)
        for m in (1, 2, 0):
            for G, H, D, R, cen in ((40, 2, 3, 2, None), (9, 1, 1, 0, centre)):
                want = c.process_sync_drift(ref, m, G, H, D, R, cen)
                got = g.process_sync_drift(ref, m, G, H, D, R, cen)
                again = g.process_sync_drift(ref, m, G, H, D, R, cen)           # the members replay their steps
                assert (want["line"]["score_q"] > 0).all()
                assert all(_same_bytes(got[k], want[k]) and _same_bytes(again[k], want[k]) for k in want), (m, G, H, D, R)
        with pytest.raises(tdoa_amd.TdoaError) as e:
            g.process_sync_drift(ref, 0, 1, 513, 1, 0)
        assert e.value.status == 1


def test_argument_and_state_errors():
    import tdoa_amd
    wl, ml = 1024, 64
    ref = np.array([0, 16, 40], dtype=np.int32)

    def status(fn, *a, **kw):
        with pytest.raises(tdoa_amd.TdoaError) as e:
            fn(*a, **kw)
        return e.value.status

    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        f = c._L.tdoa_process_sync_drift
        rec = np.zeros(3, dtype=tdoa_amd.capi.SYNC_LINE_DTYPE)
        pref, prec = ref.ctypes.data_as(f.argtypes[6]), rec.ctypes.data_as(C.c_void_p)
        none = (None,) * 5
        assert f(c._h, 0, 1, 1, 1, 1, pref, None, prec, *none) == 6                # no captures
        _synth(c, 3, 4 * wl)
        assert c.process_sync_drift(ref, 1, 5, 2, 3, 1)["line"].shape == (3,)
        for m, G, H, D, R in ((-1, 1, 1, 1, 1), (0, -1, 1, 1, 1), (0, 1024, 1, 1, 1), (0, 1, -1, 1, 1), (0, 1, 513, 1, 1), (0, 1, 1, 0, 1),
                              (0, 1, 1, -3, 1), (0, 1, 1, 1, -1), (0, 1, 1, 1, 17)):
            assert f(c._h, m, G, H, D, R, pref, None, prec, *none) == 1, (m, G, H, D, R)
        assert f(c._h, 0, 1, 1, 1, 1, None, None, prec, *none) == 1 and f(c._h, 0, 1, 1, 1, 1, pref, None, None, *none) == 1
        assert f(c._h, 2, 1023, 512, 1, 1, pref, None, prec, *none) == 0           # the largest gate and slope
        # the debug entry
        q = np.zeros((2, 3, 2 * ml - 1), dtype=np.int64)
        d = c._L.tdoa_debug_sync_drift_from_q
        pq = q.ctypes.data_as(d.argtypes[1])
        for n_sets, L, S, n_w, G, H, D, R in ((0, 1, 3, 1, 1, 1, 1, 1), (65536, 1, 3, 1, 1, 1, 1, 1), (2, 0, 3, 1, 1, 1, 1, 1),
                                              (2, 3, 3, 1, 1, 1, 1, 1), (2, 1, 1, 1, 1, 1, 1, 1), (2, 1, 65, 1, 1, 1, 1, 1),
                                              (2, 1, 3, 0, 1, 1, 1, 1), (2, 1, 3, 1, 1024, 1, 1, 1), (2, 1, 3, 1, 1, 513, 1, 1),
                                              (2, 1, 3, 1, 1, 1, 0, 1), (2, 1, 3, 1, 1, 1, 1, 17)):
            assert d(c._h, pq, n_sets, L, S, n_w, G, H, D, R, pref, None, prec, *none) == 1, (n_sets, L, S, n_w, G, H, D, R)
        assert d(c._h, None, 2, 2, 3, 1, 1, 1, 1, 1, pref, None, prec, *none) == 1
        assert d(c._h, pq, 2, 2, 3, 1, 1, 1, 1, 1, None, None, prec, *none) == 1
        assert d(c._h, pq, 2, 2, 3, 1, 1, 1, 1, 1, pref, None, None, *none) == 1
        # the overflow bound: P N_w <= 2^17 with N_w = track_len n_w; 3 * 2 * 21 845 = 131 070, 3 * 2 * 21 846 = 131 076
        assert d(c._h, pq, 2, 2, 3, 21845, 1, 1, 1, 1, pref, None, prec, *none) == 0
        assert d(c._h, pq, 2, 2, 3, 21846, 1, 1, 1, 1, pref, None, prec, *none) == 5
        assert d(c._h, pq, 2, 1, 3, 43690, 1, 1, 1, 1, pref, None, prec, *none) == 0
        assert d(c._h, pq, 2, 1, 3, 43691, 1, 1, 1, 1, pref, None, prec, *none) == 5
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:           # one station: no pair
        _synth(c, 1, 4 * wl)
        assert c._L.tdoa_process_sync_drift(c._h, 0, 1, 1, 1, 1, pref, None, prec, *none) == 5
    with tdoa_amd.Context(max_lag=ml, window_len=wl, lag_mode=tdoa_amd.capi.LAGS_GO) as c:
        _synth(c, 3, 5 * wl)
        assert status(c.process_sync_drift, ref, 0, 1, 1, 1, 1) == 5


def test_cli_sync_drift_prints_the_library_result(tmp_path):
    """tdoa_processor --stack=1 --locate=32x32/30 --sync=LAT,LON,HEIGHT/64/2 --sync-drift=3/2 on the golden three-station
    captures: a SYNCLINE line for blocks 1 and 3 with what process_sync_drift returns for the one-cell table of that position,
    and the LOCATE lines of process_locate under the clock table made of them (block 2: block 1's line continued); the usage
    errors; without --sync-drift no other line changes"""
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
    sync_flag = "--sync=%r,%r,%r/64/2" % emitter
    r = subprocess.run([cli, "--stack=1", "--locate=32x32/30", sync_flag, "--sync-drift=3/2"] + opts + tail, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode in (0, 3), r.stderr            # (the 3-station solve may fail on these captures: tests/test_processor_cli.py)
    line_rows = re.findall(r"^SYNCLINE block (\d): clock=(-?\d+),(-?\d+),(-?\d+) rate=(-?\d+),(-?\d+),(-?\d+)/2 moved=(\d+) score=([\d.]+)$",
                           r.stdout, flags=re.M)
    loc_rows = re.findall(r"^LOCATE block (\d) stack (\d+): cell=(\d+) lat=(-?[\d.]+) lon=(-?[\d.]+) pairs=(\d+) score=([\d.]+) "
                          r"runner=([\d.]+)$", r.stdout, flags=re.M)
    assert [row[0] for row in line_rows] == ["1", "3"] and "SYNC block" not in r.stdout, r.stdout
    lat_c, lon_c, h_c = (sum(s[k] / 3 for s in ST) for k in range(3))
    dlat, dlon = 30.0 / 111.32 / 31, 30.0 / (111.32 * np.cos(lat_c * np.pi / 180)) / 31
    lat0, lon0 = lat_c - dlat * 31 / 2, lon_c - dlon * 31 / 2
    with tdoa_amd.Context(max_lag=150, window_len=2000) as c:
        for s, p in enumerate(dats):
            c.capture_upload_file(s, p)
        L, n = c.num_stacks(1)
        assert (L, n) == (2, 6) and len(loc_rows) == n          # two windows of 2 000 per block
        fs = c.params.sample_rate
        ref = tdoa_amd.capi.locate_grid_table(ST, emitter[0], emitter[1], 0.0, 0.0, 1, 1, emitter[2], fs)[0]
        found = c.process_sync_drift(ref, 1, 64, 3, 2, 2)
        clock = np.concatenate([found["rows"][:L], tdoa_amd.capi.sync_line_clock(found["clock"][0], found["rate"][0], 2, L, L),
                                found["rows"][2 * L:]])
        c.locate_set_table(tdoa_amd.capi.locate_grid_table(ST, lat0, lon0, dlat, dlon, 32, 32, h_c, fs), 32)
        c.locate_set_clock(clock)
        out = c.process_locate(1, 1)["loc"]
    for row in line_rows:
        b = int(row[0]) - 1
        assert [int(x) for x in row[1:4]] == found["clock"][b].tolist() and [int(x) for x in row[4:7]] == found["rate"][b].tolist()
        assert int(row[7]) == int(found["line"]["moved"][b])
        assert abs(float(row[8]) - float(found["line"]["score"][b])) <= 5.1e-7 and float(row[8]) > 0
    for row in loc_rows:
        rec = out[(int(row[0]) - 1) * L + int(row[1])]
        cell = int(rec["cell"])
        assert int(row[2]) == cell and int(row[5]) == int(rec["pairs_in"])
        assert abs(float(row[3]) - (lat0 + (cell // 32) * dlat)) <= 5.1e-7 and abs(float(row[4]) - (lon0 + (cell % 32) * dlon)) <= 5.1e-7
        for text, value in ((row[6], float(rec["score"])), (row[7], float(rec["runner_up"]))):
            assert abs(float(text) - value) <= 5.1e-7
    plain = subprocess.run([cli, "--stack=1", "--locate=32x32/30"] + opts + tail, capture_output=True, text=True, timeout=300)
    assert plain.returncode in (0, 3) and "SYNCLINE" not in plain.stdout
    keep = lambda text: [l for l in text.splitlines() if not l.startswith(("SYNCLINE ", "LOCATE "))]
    assert keep(plain.stdout) == keep(r.stdout)
    for args, what in ((["--stack=1", "--locate=32x32/30", "--sync-drift=3/2"], "--sync-drift needs --stack --locate --sync"),
                       (["--stack=1", "--locate=32x32/30", sync_flag], "whole-block stacks"),
                       (["--stack=1", "--locate=32x32/30", sync_flag, "--sync-drift=513"], "--sync-drift=H[/D]"),
                       (["--stack=1", "--locate=32x32/30", sync_flag, "--sync-drift=3/0"], "--sync-drift=H[/D]"),
                       (["--stack=1", "--locate=32x32/30", sync_flag, "--sync-drift=x"], "--sync-drift=H[/D]")):
        bad = subprocess.run([cli] + args + opts + tail, capture_output=True, text=True, timeout=300)
        assert bad.returncode == 1 and what in bad.stderr, (args, bad.stderr)
