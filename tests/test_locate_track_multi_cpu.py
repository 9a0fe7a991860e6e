"""CPU: the numpy statement of several emitters per block (tdoa_amd.locate_track_multi; include/tdoa_mi355x.h, "several
emitters per block") against a plain enumeration of every path, round, cell and pair, on hand-worked cases, on the identities
the header states and on the two-emitter case the feature exists for; and the boundary of the entry points that needs no
device.  hand_cases(), check_hand_case(), claim_windows() and claim_counts() are shared with
tests/test_gpu_locate_track_multi.py, which runs the kernels on the same words."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from test_locate_cpu import FS, GRID, ONE, PAIRS4, ST4, _q
from test_locate_track_cpu import cell_delays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdoa_process_locate_track_multi", "tdoa_debug_locate_track_multi_from_q", "tdoa_group_process_locate_track_multi")


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessLocateTrackMulti(", "C.tdoa_process_locate_track_multi(",
                 "func (g *Group) ProcessLocateTrackMulti(", "C.tdoa_group_process_locate_track_multi("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_locate_track_multi", "locate_track_multi_from_q"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.Group, "process_locate_track_multi")
    # the definition is in the header in the words the tests hold the library to
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("E_p^j(r) is the set of excluded lags of pair p in stack j of the track. E_p^j(0) is empty.",
                   "M_p^{j,r}[l] = 0 for l in E_p^j(r) or outside the range, else |Q_p^j[l]|.",
                   "s_j^r(c) = the sum over all P pairs of M_p^{j,r}[lag_p^j(c)].",
                   "Round r's track is the cell track on the maps s_0^r .. s_{L-1}^r: T^r, D^r, L_0^r the cell of the largest T_0^r, "
                   "equal maxima going to the smaller cell.",
                   "The walk is L_{j+1}^r = L_j^r + D_j^r[L_j^r].",
                   "The runner-up is the largest T_0^r beyond min_separation of L_0^r.", "own_j^r = s_j^r[L_j^r].",
                   "If max T_0^r > 0: E_p^j(r+1) = E_p^j(r) united with { l : |l - lag_p^j(L_j^r)| <= guard } for every stack j and "
                   "every pair whose lag there lies inside the range.",
                   "Intervals are clipped at the range edges and may overlap.",
                   "Otherwise E(r+1) = E(r): the round returns the zero record and zero per-position outputs, and so does every later "
                   "round.",
                   "pairs_in counts the pairs inside the range and not excluded at L_j^r, reserved the pairs inside but excluded there.",
                   "An excluded pair reports its lag and 0.0; a pair outside reports 0 and 0.0.",
                   "Q is never written.",
                   "Round 0 is tdoa_process_locate_track's bytes: record, cells, own, lags, corr, total. So is the whole call with K = 1.",
                   "There pairs_in is the count of pairs inside and reserved is 0.",
                   "With one stack per track (L = 1), every round equals tdoa_process_locate_multi's round",
                   "positions = 1 and steps = 0.",
                   "Outputs are laid out [round][...].",
                   "what tdoa_process_locate_track refuses, n_emitters outside 1 .. 8, guard < 0.",
                   # the sentence about the older call stays, and points on
                   "It joins nothing across stacks: combining it with tdoa_process_locate_track is out of scope. "
                   "tdoa_process_locate_track_multi below is the call that runs the rounds on a block's tracks."):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handle_and_argument_errors_need_no_device(capi):
    lib = capi.load()
    rec = np.zeros(8 * 3, dtype=capi.CELL_TRACK_DTYPE)
    q = np.zeros(2 * 3 * 7, dtype=np.int64)
    pr, pq = rec.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_int64))
    none = (None,) * 6
    for m, J, k, guard, sep in ((0, 0, 1, 0, 1), (2, 16, 8, 3, 2), (0, 0, 0, 0, 1), (0, 0, 9, 0, 1), (0, 0, 2, -1, 1), (-1, 0, 2, 0, 1),
                                (0, 0, 2, 0, 0), (0, 17, 2, 0, 1), (0, -1, 2, 0, 1)):
        assert lib.tdoa_process_locate_track_multi(None, m, J, k, guard, sep, pr, *none) == 1
        assert lib.tdoa_group_process_locate_track_multi(None, m, J, k, guard, sep, pr, *none) == 1
        assert lib.tdoa_debug_locate_track_multi_from_q(None, pq, 2, 2, 3, 1, J, k, guard, sep, pr, *none) == 1
    assert lib.tdoa_process_locate_track_multi(None, 0, 0, 2, 0, 1, None, *none) == 1
    assert lib.tdoa_debug_locate_track_multi_from_q(None, None, 0, 0, 1, 0, 0, 2, 0, 1, None, *none) == 1


def test_model_argument_errors():
    from tdoa_amd import locate_track_multi
    q = np.zeros((2, 3, 7), dtype=np.int64)
    t = np.zeros((2, 3), dtype=np.int32)
    for kw in (dict(n_emitters=0), dict(n_emitters=9), dict(guard=-1), dict(sep=0), dict(track_len=0), dict(track_len=3), dict(J=17),
               dict(q=q[:, :, :6])):
        with pytest.raises(ValueError):
            locate_track_multi.track_multi_stacks(**{"q": q, "table": t, "n_cols": 2, "max_lag": 4, "track_len": 2, "J": 0, **kw})


# ---- every path, round, cell and pair enumerated ----------------------------------------------------------------------------
def _rank_order(J):
    return [0] + [x for k in range(1, J + 1) for x in (k, -k)]


def _brute(q, table, n_cols, ml, L, J, sep, K, guard, clock):
    """-> [round][track]: (T_0, None) for the zero record, else (T_0, path, own, per position (pairs_in, reserved), per position
    the lags (None: outside), per position the excluded flags, runner cell or None); E as Python sets per (stack, pair)"""
    n_sets, (n_cells, S) = len(q), table.shape
    pairs = [(i, j) for i in range(S) for j in range(i + 1, S)]

    def lag(sid, c, p):
        i, j = pairs[p]
        d = int(table[c][j]) - int(table[c][i]) + (0 if clock is None else int(clock[sid][j]) - int(clock[sid][i]))
        a = (2 * abs(d) + 16) // 32
        return -a if d < 0 else a

    E = [[set() for _ in pairs] for _ in range(n_sets)]
    moves = [(dr, dc) for dr in _rank_order(J) for dc in _rank_order(J)]              # rank order, dr first
    rounds = []
    for _ in range(K):
        maps = [[sum(abs(int(q[sid][p][lag(sid, c, p) + ml - 1])) for p in range(len(pairs))
                     if -ml < lag(sid, c, p) < ml and lag(sid, c, p) not in E[sid][p]) for c in range(n_cells)] for sid in range(n_sets)]
        tracks = []
        for t in range(n_sets // L):
            s = maps[t * L:(t + 1) * L]
            best = []
            for c0 in range(n_cells):
                top = None
                for seq in itertools.product(moves, repeat=L - 1):                    # lexicographic in that order
                    r, c, path, total = c0 // n_cols, c0 % n_cols, [c0], s[0][c0]
                    for j, (dr, dc) in enumerate(seq):
                        r, c = r + dr, c + dc
                        if not (r >= 0 and 0 <= c < n_cols and r * n_cols + c < n_cells):
                            break
                        path.append(r * n_cols + c)
                        total += s[j + 1][path[-1]]
                    else:
                        if top is None or total > top[0]:                             # strict: the first maximum
                            top = (total, path)
                best.append(top)
            T0 = [b[0] for b in best]
            if max(T0) == 0:
                tracks.append((T0, None))
                continue
            c0 = T0.index(max(T0))
            path = best[c0][1]
            far = [c for c in range(n_cells) if max(abs(c // n_cols - c0 // n_cols), abs(c % n_cols - c0 % n_cols)) > sep]
            runner = min((c for c in far if T0[c] == max(T0[f] for f in far)), default=None)
            counts, lags, flags = [], [], []
            for j, c in enumerate(path):
                sid = t * L + j
                at = [lag(sid, c, p) for p in range(len(pairs))]
                inside = [-ml < l < ml for l in at]
                ex = [ins and l in E[sid][p] for p, (l, ins) in enumerate(zip(at, inside))]
                counts.append((sum(i and not e for i, e in zip(inside, ex)), sum(ex)))
                lags.append([l if ins else None for l, ins in zip(at, inside)])
                flags.append(ex)
            for j, c in enumerate(path):                                              # after every position has been read
                for p, l in enumerate(lags[j]):
                    if l is not None:
                        E[t * L + j][p] |= {x for x in range(l - guard, l + guard + 1) if -ml < x < ml}
            tracks.append((T0, path, [s[j][c] for j, c in enumerate(path)], counts, lags, flags, runner))
        rounds.append(tracks)
    return rounds


def test_model_against_every_path_round_cell_and_pair_enumerated():
    """tiny grids, small integers so that equal maxima are common, delays that put pairs outside the range, with and without
    clocks; n_w differs from stack to stack"""
    from tdoa_amd import locate_track_multi
    rng = np.random.default_rng(41)
    n = n_zero = n_excl = n_out = n_ties = n_moved = 0
    for S, ml in ((2, 3), (3, 4), (4, 5)):
        P = S * (S - 1) // 2
        for n_cells, n_cols in ((1, 1), (7, 3), (12, 4), (10, 4), (6, 6)):
            for L, J, sep, K, guard, span, clocked in ((1, 0, 1, 3, 0, 16 * ml, False), (2, 1, 1, 2, 1, 24 * ml, True),
                                                       (3, 1, 2, 3, 0, 16 * ml, False), (3, 0, 1, 3, 2 * ml, 16 * ml, True),
                                                       (2, 1, 1, 3, 1, 40 * ml, False)):
                q = rng.integers(-2, 3, size=(2 * L, P, 2 * ml - 1), dtype=np.int64) * (rng.random() < 0.9)
                table = rng.integers(-span, span + 1, size=(n_cells, S), dtype=np.int32)
                clock = rng.integers(-24, 25, size=(2 * L, S), dtype=np.int32) if clocked else None
                n_w = rng.integers(1, 4, size=2 * L)
                recs, cells, own, pairs, lags, corr, total = locate_track_multi.track_multi_stacks(
                    q, table, n_cols, ml, L, J, K, guard, sep, n_w, clock)
                assert recs.shape == (K, 2) and cells.shape == own.shape == (K, 2, L) and pairs.shape == (K, 2 * L, 2)
                assert lags.shape == corr.shape == (K, 2 * L, P) and total.shape == (K, 2, n_cells)
                for r, tracks in enumerate(_brute(q, table, n_cols, ml, L, J, sep, K, guard, clock)):
                    for t, want in enumerate(tracks):
                        n += 1
                        sets = slice(t * L, (t + 1) * L)
                        assert total[r, t].tolist() == want[0], (r, t)
                        if want[1] is None:
                            n_zero += 1
                            assert recs[r, t].tobytes() == bytes(48) and not cells[r, t].any() and not own[r, t].any()
                            assert not pairs[r, sets].any() and not lags[r, sets].any() and not corr[r, sets].any()
                            continue
                        T0, path, own_w, counts, lags_w, flags, runner = want
                        rec = recs[r, t]
                        root = np.sqrt(np.float64(n_w[sets].sum()))
                        assert cells[r, t].tolist() == path and own[r, t].tolist() == own_w
                        assert (int(rec["cell"]), int(rec["positions"]), int(rec["score_q"])) == (path[0], L, T0[path[0]])
                        assert int(rec["steps"]) == sum(a != b for a, b in zip(path, path[1:])) and int(rec["score_q"]) == sum(own_w)
                        assert (int(rec["runner_cell"]), int(rec["runner_q"])) == ((0, 0) if runner is None else (runner, T0[runner]))
                        assert float(rec["score"]) == float(T0[path[0]]) / ONE / root
                        assert pairs[r, sets].tolist() == [list(c) for c in counts]
                        for j in range(L):
                            sid = t * L + j
                            assert lags[r, sid].tolist() == [l or 0 for l in lags_w[j]]
                            assert corr[r, sid].tolist() == [0.0 if l is None or e else float(q[sid][p][l + ml - 1]) / ONE / np.sqrt(float(n_w[sid]))
                                                             for p, (l, e) in enumerate(zip(lags_w[j], flags[j]))]
                        n_excl += any(c[1] for c in counts)
                        n_out += any(sum(c) < P for c in counts)
                        n_ties += r > 0 and T0.count(T0[path[0]]) > 1
                        n_moved += r > 0 and len(set(path)) > 1
    print("%d (round, track)s: %d zero records, %d tracks with an excluded pair, %d with pairs outside, %d later rounds with equal maxima, "
          "%d later rounds whose track moves" % (n, n_zero, n_excl, n_out, n_ties, n_moved))
    assert min(n_zero, n_excl, n_out, n_ties, n_moved) >= 5                          # each kind of case occurs


# ---- hand-worked cases: three stations, max_lag 4 (7 lags), rows 01, 02, 12; lists (n_cols = n_cells), so columns only ------
def _track(cells, pairs, lags, corr, score, runner_cell, runner, total):
    return dict(cells=cells, pairs=pairs, lags=lags, corr=corr, score=score, runner_cell=runner_cell, runner=runner, total=total)


def hand_cases():
    """[(name, dict(q [n_sets][3][7], ml, table, n_cols, L, J, sep, n_w, k, guard), [round][track]: expected or (None, total) for
    the zero record)]; expected: cells, per position (pairs_in, reserved), the lags (0 for a pair outside) and corr (0 for a
    pair outside or excluded), score, runner_cell, runner, total; corr, score, runner and total in units of 2^32"""
    # cells' lags: (1, 2, 1), (-1, -1, 0)
    two = np.array([(0, 16, 32), (0, -16, -16)], dtype=np.int32)
    strong = _q(4, (0, 1, 5), (1, 2, 4), (2, 1, 3), (0, -1, 1), (1, -1, 1), (2, 0, 1))          # cell 0: 12, cell 1: 3
    weak = _q(4, (0, 1, 2))                                                                      # cell 0: 2, cell 1: 0
    zero2 = (None, [0, 0])
    a0 = _track([0, 0], [(3, 0)] * 2, [(1, 2, 1)] * 2, [(5, 4, 3)] * 2, 24, 0, 0, [24, 15])
    # cells' lags: (3, 6 outside, 3), (4 outside, 3, -1)
    out = np.array([(0, 48, 96), (0, 64, 48)], dtype=np.int32)
    q_out = _q(4, (0, 3, 4), (1, 3, 5), (2, 3, 4), (2, -1, 2))                                   # cell 0: 4 + 4, cell 1: 5 + 2
    # cells' lags: (1, 2, 1), (1, 3, 2), (2, 3, 1), (-1, -1, 0)
    three = np.array([(0, 16, 32), (0, 16, 48), (0, 32, 48), (0, -16, -16)], dtype=np.int32)
    q_three = _q(4, (0, 1, 5), (0, 2, 3), (0, -1, 1), (1, 2, 4), (1, 3, 2), (1, -1, 1), (2, 1, 3), (2, 2, 1), (2, 0, 1))
    return [
        # track 0 (two strong stacks): round 0 takes cell 0's lags {1}, {2}, {1} out of both stacks, round 1 finds cell 1
        # (T_0 = 0 + 3, 3 + 3) and takes {-1}, {-1}, {0}, round 2 has nothing left.  Track 1 (two weak stacks) has nothing
        # left after round 0: it ends a round earlier
        ("a round that ends early in one track and not in the other",
         dict(q=np.stack([strong, strong, weak, weak]), ml=4, table=two, n_cols=2, L=2, J=1, sep=1, n_w=1, k=3, guard=0),
         [[a0, _track([0, 0], [(3, 0)] * 2, [(1, 2, 1)] * 2, [(2, 0, 0)] * 2, 4, 0, 0, [4, 2])],
          [_track([1, 1], [(3, 0)] * 2, [(-1, -1, 0)] * 2, [(1, 1, 1)] * 2, 6, 0, 0, [3, 6]), zero2],
          [zero2, zero2]]),
        # guard 100 around lags inside a range of 7: every pair of both stacks loses its whole range
        ("a guard that covers the range", dict(q=np.stack([strong, -strong]), ml=4, table=two, n_cols=2, L=2, J=1, sep=1, n_w=2, k=2, guard=100),
         [[dict(a0, corr=[(5, 4, 3), (-5, -4, -3)])], [zero2]]),
        # cell 0's pair 02 has lag 6, outside: with guard 3 an interval around 6 would take lag 3 of pair 02 from cell 1.  Pairs 01
        # and 12 lose {0 .. 3}; cell 1's pair 12 at lag -1 stays
        ("a pair outside the range adds no exclusion", dict(q=np.stack([q_out, q_out]), ml=4, table=out, n_cols=2, L=2, J=1, sep=1, n_w=1, k=2, guard=3),
         [[_track([0, 0], [(2, 0)] * 2, [(3, 0, 3)] * 2, [(4, 0, 4)] * 2, 16, 0, 0, [16, 15])],
          [_track([1, 1], [(2, 0)] * 2, [(0, 3, -1)] * 2, [(0, 5, 2)] * 2, 14, 0, 0, [7, 14])]]),
        # J = 0: T_0 is twice the map.  Round 1's cell 2 keeps 3 + 2 and has its pair 12 (lag 1) excluded in both stacks
        ("the track's cell has an excluded pair in every stack",
         dict(q=np.stack([q_three, q_three]), ml=4, table=three, n_cols=4, L=2, J=0, sep=1, n_w=1, k=2, guard=0),
         [[_track([0, 0], [(3, 0)] * 2, [(1, 2, 1)] * 2, [(5, 4, 3)] * 2, 24, 2, 16, [24, 16, 16, 6])],
          [_track([2, 2], [(2, 1)] * 2, [(2, 3, 1)] * 2, [(3, 2, 0)] * 2, 10, 0, 0, [0, 6, 10, 6])]]),
    ]


def check_hand_case(got, arg, want):
    """got: (records [K][n_tracks], cells, own, pairs [K][n_sets][2], lags [K][n_sets][3], corr, total [K][n_tracks][n_cells])"""
    recs, cells, own, pairs, lags, corr, total = got
    L, K, n_sets = arg["L"], arg["k"], len(arg["q"])
    assert recs.shape == (K, n_sets // L) and cells.shape == own.shape == (K, n_sets // L, L) and pairs.shape == (K, n_sets, 2)
    assert lags.shape == corr.shape == (K, n_sets, 3) and total.shape == (K, n_sets // L, len(arg["table"]))
    assert (total.dtype, own.dtype, cells.dtype, pairs.dtype, lags.dtype, corr.dtype) == (np.int64, np.int64, np.int32, np.int32, np.int32, np.float64)
    root, track_root = np.sqrt(np.float64(arg["n_w"])), np.sqrt(np.float64(arg["n_w"] * L))
    for r, tracks in enumerate(want):
        for t, w in enumerate(tracks):
            sets = slice(t * L, (t + 1) * L)
            rec = recs[r, t]
            if isinstance(w, tuple):
                assert rec.tobytes() == bytes(48) and not cells[r, t].any() and not own[r, t].any() and not pairs[r, sets].any(), (r, t)
                assert not lags[r, sets].any() and corr[r, sets].tobytes() == bytes(corr[r, sets].nbytes), (r, t)
                assert total[r, t].tolist() == [x * ONE for x in w[1]], (r, t)
                continue
            assert cells[r, t].tolist() == w["cells"] and total[r, t].tolist() == [x * ONE for x in w["total"]], (r, t)
            assert (int(rec["cell"]), int(rec["runner_cell"]), int(rec["positions"])) == (w["cells"][0], w["runner_cell"], L), (r, t)
            assert int(rec["steps"]) == sum(a != b for a, b in zip(w["cells"], w["cells"][1:])), (r, t)
            assert (int(rec["score_q"]), int(rec["runner_q"])) == (w["score"] * ONE, w["runner"] * ONE), (r, t)
            assert int(own[r, t].sum()) == w["score"] * ONE == int(total[r, t][w["cells"][0]]), (r, t)
            assert float(rec["score"]) == w["score"] / track_root and float(rec["runner_up"]) == w["runner"] / track_root, (r, t)
            assert pairs[r, sets].tolist() == [list(p) for p in w["pairs"]], (r, t)
            assert lags[r, sets].tolist() == [list(x) for x in w["lags"]], (r, t)
            assert corr[r, sets].tolist() == [[c / root for c in x] for x in w["corr"]], (r, t)


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_worked_cases(name, arg, want):
    from tdoa_amd import locate_track_multi
    got = locate_track_multi.track_multi_stacks(arg["q"], arg["table"], arg["n_cols"], arg["ml"], arg["L"], arg["J"], arg["k"],
                                                arg["guard"], arg["sep"], arg["n_w"])
    check_hand_case(got, arg, want)


# ---- the identities of the header -------------------------------------------------------------------------------------------
def test_identities_on_random_integers():
    from tdoa_amd import locate_multi, locate_track, locate_track_multi
    rng = np.random.default_rng(13)
    for S, ml, n_cells, n_cols, L, J, K, guard in ((3, 6, 40, 7, 4, 2, 3, 1), (4, 9, 33, 33, 3, 1, 2, 0), (2, 5, 50, 8, 5, 16, 4, 2),
                                                   (4, 7, 29, 5, 1, 3, 8, 1), (3, 8, 31, 6, 1, 0, 3, 0)):
        P = S * (S - 1) // 2
        q = rng.integers(-50, 51, size=(2 * L, P, 2 * ml - 1), dtype=np.int64)
        table = rng.integers(-16 * ml, 16 * ml + 1, size=(n_cells, S), dtype=np.int32)
        clock = rng.integers(-40, 41, size=(2 * L, S), dtype=np.int32)
        n_w = rng.integers(1, 4, size=2 * L)
        for sep in (1, 2):
            got = locate_track_multi.track_multi_stacks(q, table, n_cols, ml, L, J, K, guard, sep, n_w, clock)
            one = locate_track_multi.track_multi_stacks(q, table, n_cols, ml, L, J, 1, guard, sep, n_w, clock)
            plain = locate_track.track_stacks(q, table, n_cols, ml, L, J, sep, n_w, clock)
            # 1: round 0, and the whole call with K = 1, are the cell track's bytes
            for k, b in zip((0, 1, 2, 4, 5, 6), plain):
                assert one[k].shape == (1,) + b.shape and one[k].dtype == b.dtype
                assert one[k][0].tobytes() == b.tobytes() == got[k][0].tobytes(), k
            inside = (got[4][0] != 0) | (got[5][0] != 0)
            assert (got[3][0, :, 1] == 0).all() and (got[3][0, :, 0] >= inside.sum(axis=1)).all()
            # every round: score_q = total[cell] = the sum of own; pairs_in + reserved <= P
            recs, cells, own, pairs, lags, corr, total = got
            assert (recs["score_q"] == np.take_along_axis(total, recs["cell"][..., None].astype(np.int64), axis=2)[..., 0]).all()
            assert (recs["score_q"] == own.sum(axis=2)).all() and (pairs.sum(axis=2) <= P).all()
            assert (np.diff(recs["score_q"], axis=0) <= 0).all()                                   # masking never adds
            if L == 1:                                                                             # 2: the rounds of locate_multi
                loc, mlags, mcorr, mmap = locate_multi.locate_multi_stacks(q, table, n_cols, ml, K, guard, sep, n_w, clock)
                for name in ("cell", "runner_cell", "score_q", "runner_q", "score", "runner_up"):
                    assert recs[name].tobytes() == loc[name].tobytes(), name
                assert lags.tobytes() == mlags.tobytes() and corr.tobytes() == mcorr.tobytes() and total.tobytes() == mmap.tobytes()
                assert (pairs[..., 0] == loc["pairs_in"]).all() and (pairs[..., 1] == loc["reserved"]).all()
                found = recs["score_q"] > 0
                assert (recs["positions"] == found).all() and (recs["steps"] == 0).all()
                assert (cells[..., 0] == recs["cell"]).all() and (own[..., 0] == recs["score_q"]).all()


# ---- the two-emitter case ---------------------------------------------------------------------------------------------------
N_STACKS, PER_STACK, NOISE = 12, 3, 0.6
A_PATH = [(12 + t, 30 + t) for t in range(N_STACKS)]
B_PATHS = {"B moving": [(40 - t, 50 - t) for t in range(N_STACKS)], "B still": [(30, 50)] * N_STACKS}
ROUND1_AT_LEAST = {"B moving": 8, "B still": 10}            # measured 10 and 12 of 12: a margin of two stacks
CLAIM = dict(J=1, guard=2, sep=2, K=2)


def claim_windows(oracle, b_path):
    """A time-shared channel: stack t = 0 .. 11 holds the windows w = 16 t + k, k = 0, 1 with A's delays at (12 + t, 30 + t)
    and k = 2 with B's at b_path[t].  Window w of station s = simulate_delayed_fm(8192, d_s, 300 + w, 1000 (s + 1) + w, 1.0,
    0.6) -> [stack][k][s] u8 IQ"""
    out = []
    for t in range(N_STACKS):
        da, db = cell_delays(*A_PATH[t]), cell_delays(*b_path[t])
        out.append([[oracle.simulate_delayed_fm(8192, (da if k < 2 else db)[s], 300 + 16 * t + k, 1000 * (s + 1) + 16 * t + k, 1.0, NOISE)
                     for s in range(4)] for k in range(PER_STACK)])
    return out


def claim_counts(b_path, multi_cells, track_rec, track_cells):
    """multi_cells [12]: round 2's cell of the per-stack rounds (None: none); track_rec [2], track_cells [2][12]: the rounds of
    the block's track -> (stacks whose per-stack round 2 is near B, whose round-0 track cell is A's, whose round-1 track cell is
    near B, whether round 0's runner-up is near B's first cell)"""
    from tdoa_amd import locate_multi
    b = [r * 64 + c for r, c in b_path]
    a = [r * 64 + c for r, c in A_PATH]
    per_stack = sum(c is not None and locate_multi.near(c, b[t], 64) for t, c in enumerate(multi_cells))
    on_a = sum(int(c) == a[t] for t, c in enumerate(track_cells[0]))
    near_b = sum(track_rec[1]["score_q"] > 0 and locate_multi.near(c, b[t], 64) for t, c in enumerate(track_cells[1]))
    runner = bool(track_rec[0]["runner_q"] > 0 and locate_multi.near(track_rec[0]["runner_cell"], b[0], 64))
    return int(per_stack), int(on_a), int(near_b), runner


def check_claim(name, counts):
    per_stack, on_a, near_b, runner = counts
    print("%s: per-stack round 2 near B in %d of 12 stacks, round-0 track on A in %d, round-1 track near B in %d, round 0's runner-up "
          "near B's first cell: %s" % (name, per_stack, on_a, near_b, runner))
    assert per_stack <= 3
    assert on_a >= 10
    assert near_b >= ROUND1_AT_LEAST[name]
    assert not runner


@pytest.mark.parametrize("name", list(B_PATHS))
def test_the_second_emitter_no_stack_shows_is_the_second_track(oracle, name):
    """Four stations, windows of 8 192, max_lag 128, the 48 x 64 grid, noise 0.6, twelve stacks of 2 windows of A and 1 of B,
    J 1, guard 2, min_separation 2.  Measured with the float64 pipeline: B moving: the per-stack round 2 is near B in 1 of 12
    stacks, the round-0 track is on A in 12, the round-1 track near B in 10; B still: 1, 12 and 12.  Round 0's runner-up is
    near B's first cell in neither."""
    from tdoa_amd import locate, locate_multi, locate_track_multi, stacking
    ml = 128
    table = locate.grid_table(ST4, sample_rate=FS, **GRID)
    Q = []
    for stack in claim_windows(oracle, B_PATHS[name]):
        total = np.zeros((6, 2 * ml - 1), dtype=np.int64)
        for x in stack:
            sig = [oracle.b_preprocess(s)[0] for s in x]
            total += np.array([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ml)) for i, j in PAIRS4])
        Q.append(total)
    Q = np.array(Q)
    loc = locate_multi.locate_multi_stacks(Q, table, 64, ml, CLAIM["K"], CLAIM["guard"], CLAIM["sep"], PER_STACK)[0]
    multi_cells = [int(loc["cell"][1, t]) if loc["score_q"][1, t] > 0 else None for t in range(N_STACKS)]
    out = locate_track_multi.track_multi_stacks(Q, table, 64, ml, N_STACKS, CLAIM["J"], CLAIM["K"], CLAIM["guard"], CLAIM["sep"], PER_STACK)
    check_claim(name, claim_counts(B_PATHS[name], multi_cells, out[0][:, 0], out[1][:, 0]))
