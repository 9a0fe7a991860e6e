"""CPU: the numpy statement of several emitters per stack (tdoa_amd.locate_multi; include/tdoa_mi355x.h, "several emitters
per stack") on hand-worked cases, against a plain enumeration of every round, cell and pair, and on the two-emitter case the
feature exists for; and the boundary of the entry points that needs no device.  hand_cases(), check_hand_case() and the
two-emitter helpers are shared with tests/test_gpu_locate_multi.py, which runs the kernels on the same words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_locate_cpu import FS, GRID, ONE, PAIRS4, ST4, _q, noisy_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdoa_process_locate_multi", "tdoa_debug_locate_multi_from_q", "tdoa_group_process_locate_multi")


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import locate_multi
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessLocateMulti(", "C.tdoa_process_locate_multi(", "func (g *Group) ProcessLocateMulti(",
                 "C.tdoa_group_process_locate_multi("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_locate_multi", "locate_multi_from_q"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.Group, "process_locate_multi")
    assert re.search(r"#define TDOA_LOCATE_MAX_EMITTERS 8\b", hdr) and locate_multi.MAX_EMITTERS == 8
    # the definition is in the header in the words the tests hold the library to
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("E_p(r) is the set of excluded lags of pair p. E_p(0) is empty.",
                   "E_p(r+1) = E_p(r) united with { l : |l - lag_p(cell*_r)| <= guard } if round r found a cell and lag_p(cell*_r) lies "
                   "inside the searched range; otherwise E_p(r+1) = E_p(r).",
                   "Intervals are clipped at the range edges. They may overlap.",
                   "M_p^r[l] = 0 for l in E_p(r) or outside the range, else |Q_p[l]|.",
                   "score_q^r(c) = the sum over all P pairs of M_p^r[lag_p(c)].",
                   "the largest score_q^r, equal maxima going to the smaller cell",
                   "the runner-up of that round's map beyond min_separation of that round's cell",
                   "pairs_in counts the pairs inside the range and not excluded at the cell",
                   "reserved carries the number of pairs inside the range but excluded at the cell.",
                   "a pair outside the range reports lag 0 and 0.0. An excluded pair reports its lag and 0.0, so tdoa_solve_surface "
                   "gives it no weight.",
                   "If the largest score of a round is 0, the result is the zero record, zero lags and zero correlations, and nothing "
                   "is added to E. Every later round is then the zero record too.",
                   "Q is never written.",
                   "round 0, and therefore the whole call with K = 1, returns tdoa_process_locate's bytes",
                   "reserved is 0 there.",
                   "The outputs are laid out [round][stack][...].",
                   "It joins nothing across stacks: combining it with tdoa_process_locate_track is out of scope.",
                   "n_emitters outside 1 .. 8, guard < 0"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handle_and_argument_errors_need_no_device(capi):
    lib = capi.load()
    loc = np.zeros(8 * 4, dtype=capi.LOCATION_DTYPE)
    q = np.zeros(3 * 7, dtype=np.int64)
    pl, pq = loc.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_int64))
    for m, k, guard, sep in ((0, 1, 0, 1), (2, 8, 3, 2), (0, 0, 0, 1), (0, 9, 0, 1), (0, 2, -1, 1), (-1, 2, 0, 1), (0, 2, 0, 0)):
        assert lib.tdoa_process_locate_multi(None, m, k, guard, sep, pl, None, None, None) == 1
        assert lib.tdoa_group_process_locate_multi(None, m, k, guard, sep, pl, None, None, None) == 1
        assert lib.tdoa_debug_locate_multi_from_q(None, pq, 1, 3, 1, k, guard, sep, pl, None, None, None) == 1
    assert lib.tdoa_process_locate_multi(None, 0, 2, 0, 1, None, None, None, None) == 1
    assert lib.tdoa_debug_locate_multi_from_q(None, None, 0, 1, 0, 2, 0, 1, None, None, None, None) == 1


def test_model_argument_errors():
    from tdoa_amd import locate_multi
    q = np.zeros((3, 7), dtype=np.int64)
    t = np.zeros((2, 3), dtype=np.int32)
    for kw in (dict(n_emitters=0), dict(n_emitters=9), dict(guard=-1), dict(min_separation=0), dict(q_pairs=q[:, :6])):
        with pytest.raises(ValueError):
            locate_multi.locate_multi(**{"q_pairs": q, "table": t, "n_cols": 2, "max_lag": 4, **kw})


# ---- hand-worked cases: three stations, max_lag 4 (7 lags, lag l at index l + 3), rows 01, 02, 12 -------------------------
def _round(cell, runner_cell, pairs_in, reserved, lags, corr, score, runner, score_map):
    return dict(cell=cell, runner_cell=runner_cell, pairs_in=pairs_in, reserved=reserved, lags=lags, corr=corr, score=score,
                runner=runner, map=score_map)


def hand_cases():
    """[(name, dict(q, ml, table, n_cols, sep, n_w, k, guard), [per round: expected or None for the zero record])]; expected:
    cell, runner_cell, pairs_in, reserved, lags (0 for a pair outside), corr (0 for a pair outside or excluded), score, runner
    and map, the last four in units of 2^32"""
    # cells' lags: (1, 2, 1), (1, 3, 2), (2, 3, 1), (-1, -1, 0); a list (n_cols = n_cells), so columns only
    three = np.array([(0, 16, 32), (0, 16, 48), (0, 32, 48), (0, -16, -16)], dtype=np.int32)
    q_three = _q(4, (0, 1, 5), (0, 2, 3), (0, -1, 1), (1, 2, 4), (1, 3, 2), (1, -1, 1), (2, 1, 3), (2, 2, 1), (2, 0, 1))
    first = _round(0, 2, 3, 0, (1, 2, 1), (5, 4, 3), 12, 8, [12, 8, 8, 3])
    # cells' lags: (0, 0, 0), (2, 2, 0), (1, 1, 0), (-3, -3, 0)
    lap = np.array([(0, 0, 0), (0, 32, 32), (0, 16, 16), (0, -48, -48)], dtype=np.int32)
    q_lap = _q(4, (0, 0, 9), (0, 2, 6), (0, 1, 4), (0, -3, 1), (1, 0, 9), (1, 2, 6), (1, 1, 4), (1, -3, 1), (2, 0, 1))
    # cells' lags: (3, 0, -3), (1, 0, -1), (0, 0, 0)
    edge = np.array([(0, 48, 0), (0, 16, 0), (0, 0, 0)], dtype=np.int32)
    q_edge = _q(4, (0, 3, 5), (0, 1, 3), (0, 0, 2), (1, 0, 1), (2, -3, 5), (2, -1, 3), (2, 0, 2))
    # cells' lags: (3, 6 outside, 3), (4 outside, 3, -1)
    out = np.array([(0, 48, 96), (0, 64, 48)], dtype=np.int32)
    q_out = _q(4, (0, 3, 4), (1, 3, 5), (2, 3, 4), (2, -1, 2))
    # cells' lags: (0, 0, 0), (1, 2, 1) twice, (0, 0, 0)
    twins = np.array([(0, 0, 0), (0, 16, 32), (0, 16, 32), (0, 0, 0)], dtype=np.int32)
    q_twins = _q(4, (0, 0, 3), (1, 0, 3), (2, 0, 3), (0, 1, 2), (1, 2, 2), (2, 1, 2))
    return [
        # E after round 0: {1}, {2}, {1}.  Round 1: cell 1 keeps 2 + 1, cell 2 keeps 3 + 2 and has its pair 12 excluded.
        # E after round 1: {1, 2}, {2, 3}, {1}.  Round 2: cell 1 keeps the 1 of M_12[2], cell 3 is untouched
        ("guard 0: only the found lags go", dict(q=q_three, ml=4, table=three, n_cols=4, sep=1, n_w=1, k=3, guard=0),
         [first, _round(2, 0, 2, 1, (2, 3, 1), (3, 2, 0), 5, 0, [0, 3, 5, 3]),
          _round(3, 1, 3, 0, (-1, -1, 0), (1, 1, 1), 3, 1, [0, 1, 0, 3])]),
        # E after round 0: {0, 1, 2}, {1, 2, 3}, {0, 1, 2}: only cell 3 keeps anything, and its pair 12 (lag 0) is excluded.
        # After round 1 nothing is left: the maximum of round 2 is 0, and round 3 is the zero record too
        ("guard 1, and a round with maximum 0 zeroes every later round",
         dict(q=-q_three, ml=4, table=three, n_cols=4, sep=1, n_w=4, k=4, guard=1),
         [dict(first, corr=(-5, -4, -3)), _round(3, 0, 2, 1, (-1, -1, 0), (-1, -1, 0), 2, 0, [0, 0, 0, 2]), None, None]),
        # E after round 0: {-1, 0, 1} in every pair; after round 1 pairs 01 and 02 have {-1, 0, 1} and {1, 2, 3}, which share
        # lag 1: {-1 .. 3}.  Cell 3 at lags (-3, -3, 0) is what is left
        ("two emitters' intervals overlap", dict(q=q_lap, ml=4, table=lap, n_cols=4, sep=1, n_w=1, k=3, guard=1),
         [_round(0, 2, 3, 0, (0, 0, 0), (9, 9, 1), 19, 9, [19, 13, 9, 3]),
          _round(1, 3, 2, 1, (2, 2, 0), (6, 6, 0), 12, 2, [0, 12, 0, 2]),
          _round(3, 0, 2, 1, (-3, -3, 0), (1, 1, 0), 2, 0, [0, 0, 0, 2])]),
        # guard 2 around lags 3 and -3 of a range that ends at +-3: {1, 2, 3} and {-3, -2, -1}; pair 02 loses {-2 .. 2}
        ("an interval is clipped at the range edge", dict(q=q_edge, ml=4, table=edge, n_cols=3, sep=1, n_w=2, k=2, guard=2),
         [_round(0, 2, 3, 0, (3, 0, -3), (5, 1, 5), 11, 5, [11, 7, 5]),
          _round(2, 0, 2, 1, (0, 0, 0), (2, 0, 2), 4, 0, [0, 0, 4])]),
        # cell 0's pair 02 has lag 6, outside: with guard 3 an interval around 6 would take lag 3 of pair 02 from cell 1
        ("an emitter's pair outside the range adds no exclusion", dict(q=q_out, ml=4, table=out, n_cols=2, sep=1, n_w=1, k=2, guard=3),
         [_round(0, 0, 2, 0, (3, 0, 3), (4, 0, 4), 8, 0, [8, 7]),
          _round(1, 0, 2, 0, (0, 3, -1), (0, 5, 2), 7, 0, [0, 7])]),
        ("equal maxima in round 1 go to the smaller cell", dict(q=q_twins, ml=4, table=twins, n_cols=4, sep=1, n_w=1, k=2, guard=0),
         [_round(0, 3, 3, 0, (0, 0, 0), (3, 3, 3), 9, 9, [9, 6, 6, 9]),
          _round(1, 3, 3, 0, (1, 2, 1), (2, 2, 2), 6, 0, [0, 6, 6, 0])]),
        ("all zeros: every round is the zero record", dict(q=_q(4), ml=4, table=three, n_cols=2, sep=1, n_w=1, k=3, guard=1),
         [None, None, None]),
    ]


def check_hand_case(got, arg, want):
    """got: (records [K], lags [K][P], corr [K][P], map [K][n_cells])"""
    from tdoa_amd import locate
    recs, lags, corr, score_map = got
    assert recs.shape == (arg["k"],) and lags.shape == corr.shape == (arg["k"], 3) and score_map.shape == (arg["k"], len(arg["table"]))
    assert score_map.dtype == np.int64 and lags.dtype == np.int32 and corr.dtype == np.float64 and recs.dtype == locate.LOCATION_DTYPE
    root = np.sqrt(np.float64(arg["n_w"]))
    for r, w in enumerate(want):
        rec = recs[r]
        if w is None:
            assert rec.tobytes() == bytes(48), r
            assert not lags[r].any() and corr[r].tobytes() == bytes(corr[r].nbytes) and not score_map[r].any(), r
            continue
        assert (int(rec["cell"]), int(rec["runner_cell"]), int(rec["pairs_in"]), int(rec["reserved"])) == \
               (w["cell"], w["runner_cell"], w["pairs_in"], w["reserved"]), r
        assert (int(rec["score_q"]), int(rec["runner_q"])) == (w["score"] * ONE, w["runner"] * ONE), r
        assert float(rec["score"]) == w["score"] / root and float(rec["runner_up"]) == w["runner"] / root, r
        assert score_map[r].tolist() == [m * ONE for m in w["map"]] and score_map[r][w["cell"]] == rec["score_q"], r
        assert lags[r].tolist() == list(w["lags"]), r
        assert corr[r].tolist() == [c / root for c in w["corr"]], r
        assert np.abs(corr[r]).sum() == pytest.approx(float(rec["score"]), rel=1e-15), r


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_worked_cases(name, arg, want):
    from tdoa_amd import locate_multi
    got = locate_multi.locate_multi(arg["q"], arg["table"], arg["n_cols"], arg["ml"], arg["k"], arg["guard"], arg["sep"], arg["n_w"])
    check_hand_case(got, arg, want)


def _brute(q, table, n_cols, ml, sep, K, guard):
    """every round, cell and pair by enumeration -> per round (map, best cell or None, pairs_in, excluded pairs, lags (None:
    outside), excluded flags, runner cell or None)"""
    n_cells, S = len(table), len(table[0])
    pairs = [(i, j) for i in range(S) for j in range(i + 1, S)]
    lag = []
    for c in range(n_cells):
        row = []
        for i, j in pairs:
            d = int(table[c][j]) - int(table[c][i])
            a = (2 * abs(d) + 16) // 32
            row.append(-a if d < 0 else a)
        lag.append(row)
    E = [set() for _ in pairs]
    rounds = []
    for _ in range(K):
        scores = [sum(abs(int(q[p][l + ml - 1])) for p, l in enumerate(lag[c]) if -ml < l < ml and l not in E[p]) for c in range(n_cells)]
        top = max(scores)
        if top == 0:
            rounds.append((scores, None, 0, 0, None, None, None))
            continue
        best = scores.index(top)
        inside = [-ml < l < ml for l in lag[best]]
        ex = [ins and l in E[p] for p, (l, ins) in enumerate(zip(lag[best], inside))]
        far = [c for c in range(n_cells) if max(abs(c // n_cols - best // n_cols), abs(c % n_cols - best % n_cols)) > sep]
        runner = min((c for c in far if scores[c] == max(scores[f] for f in far)), default=None)
        rounds.append((scores, best, sum(i and not e for i, e in zip(inside, ex)), sum(ex),
                       [l if ins else None for l, ins in zip(lag[best], inside)], ex, runner))
        for p, (l, ins) in enumerate(zip(lag[best], inside)):
            if ins:
                E[p] |= {x for x in range(l - guard, l + guard + 1) if -ml < x < ml}
    return rounds


def test_model_against_every_round_cell_and_pair_enumerated():
    """small random Q with few distinct values, so equal maxima are common; delays that put many pairs outside the range; the
    model with K = 1 is locate.locate byte for byte, and round 0 of every K is too"""
    from tdoa_amd import locate, locate_multi
    rng = np.random.default_rng(29)
    n = n_zero = n_excl = n_out = n_ties = 0
    for S, ml in ((2, 3), (3, 4), (4, 9), (5, 6)):
        P = S * (S - 1) // 2
        for n_cells, n_cols in ((1, 1), (7, 3), (12, 4), (30, 30), (31, 7)):
            for sep, span, K, guard in ((1, 16 * ml, 2, 0), (2, 40 * ml, 4, 1), (1, 24 * ml, 8, 2), (1, 16 * ml, 3, 2 * ml)):
                q = rng.integers(-2, 3, size=(P, 2 * ml - 1), dtype=np.int64) * (rng.random() < 0.9)
                table = rng.integers(-span, span + 1, size=(n_cells, S), dtype=np.int32)
                recs, lags, corr, score_map = locate_multi.locate_multi(q, table, n_cols, ml, K, guard, sep, n_w=2)
                one = locate_multi.locate_multi(q, table, n_cols, ml, 1, guard, sep, n_w=2)
                plain = locate.locate(q, table, n_cols, ml, sep, n_w=2)
                for a, b, c in zip(one, plain, (recs, lags, corr, score_map)):
                    assert a.shape == (1,) + b.shape and a[0].tobytes() == b.tobytes() == c[0].tobytes() and a.dtype == b.dtype
                assert recs["reserved"][0] == 0
                zero_seen = False
                for r, (scores, best, pairs_in, n_ex, want_lags, ex, runner) in enumerate(_brute(q, table, n_cols, ml, sep, K, guard)):
                    n += 1
                    assert score_map[r].tolist() == scores, (r, K, guard)
                    if best is None:
                        n_zero += 1
                        zero_seen = True
                        assert recs[r].tobytes() == bytes(48) and not lags[r].any() and not corr[r].any()
                        continue
                    assert not zero_seen                                      # a zero round is never followed by a find
                    rec = recs[r]
                    assert (int(rec["cell"]), int(rec["pairs_in"]), int(rec["reserved"]), int(rec["score_q"])) == \
                           (best, pairs_in, n_ex, scores[best])
                    assert lags[r].tolist() == [l or 0 for l in want_lags]
                    assert corr[r].tolist() == [0.0 if l is None or e else float(q[p][l + ml - 1]) / ONE / np.sqrt(2.0)
                                                for p, (l, e) in enumerate(zip(want_lags, ex))]
                    assert (int(rec["runner_cell"]), int(rec["runner_q"])) == ((0, 0) if runner is None else (runner, scores[runner]))
                    assert float(rec["score"]) == float(scores[best]) / ONE / np.sqrt(2.0)
                    n_excl += n_ex > 0
                    n_out += pairs_in + n_ex < P
                    n_ties += r > 0 and scores.count(scores[best]) > 1
    print("%d rounds: %d zero records, %d best cells with an excluded pair, %d with pairs outside, %d later rounds with equal maxima"
          % (n, n_zero, n_excl, n_out, n_ties))
    assert n_zero >= 5 and n_excl >= 5 and n_out >= 5 and n_ties >= 5          # each kind of case occurs


# ---- the two-emitter case ------------------------------------------------------------------------------------------------
A_CELL = 12 * 64 + 36
B_CELLS = (30 * 64 + 50, 34 * 64 + 14)
ROUND2_AT_LEAST = {B_CELLS[0]: 10, B_CELLS[1]: 8}          # measured 12 and 10 of 12: a margin of two stacks
N_A, N_B, NOISE, N_STACKS = 8, 2, 0.5, 12


def emitter_delays(cell):
    """station delays in samples of a transmitter in `cell` of the 48 x 64 grid: rint(fs dist / c) minus their minimum"""
    from tdoa_amd import locate
    tx = locate.ecef(GRID["lat0"] + (cell // 64) * GRID["dlat"], GRID["lon0"] + (cell % 64) * GRID["dlon"], GRID["height_m"])
    dist = np.linalg.norm(locate.ecef(*np.array(ST4).T) - tx, axis=1)
    d = np.rint(FS * dist / locate.SPEED_OF_LIGHT).astype(np.int64)
    return [int(x) for x in d - d.min()]


def two_emitter_windows(oracle, b_cell):
    """A time-shared channel: stack t = 0 .. 11 holds the windows w = 16 t + k, k = 0 .. 9; the first 8 carry A's station
    delays, the next 2 B's.  Window w of station s = simulate_delayed_fm(8192, d_s, 300 + w, 1000 (s + 1) + w, 1.0, 0.5)
    -> [stack][k][s] u8 IQ"""
    da, db = emitter_delays(A_CELL), emitter_delays(b_cell)
    assert da == noisy_case()[2]
    return [[[oracle.simulate_delayed_fm(8192, (da if k < N_A else db)[s], 300 + 16 * t + k, 1000 * (s + 1) + 16 * t + k, 1.0, NOISE)
              for s in range(4)] for k in range(N_A + N_B)] for t in range(N_STACKS)]


def claim_counts(Q, table, ml, b_cell, round2):
    """Q [12][6][2 ml - 1]; round2(t) -> stack t's cell of round 1 of (K 2, guard 2, min_separation 2) or None -> (stacks whose best
    cell is A, whose plain runner-up is near B, whose round 2 is near B)"""
    from tdoa_amd import locate, locate_multi
    a_ok = runner_near = round2_near = 0
    for t in range(len(Q)):
        rec = locate.locate(Q[t], table, 64, ml, 2, N_A + N_B)[0]
        a_ok += int(rec["cell"]) == A_CELL
        runner_near += rec["runner_q"] > 0 and locate_multi.near(rec["runner_cell"], b_cell, 64)
        cell = round2(t)
        round2_near += cell is not None and locate_multi.near(cell, b_cell, 64)
    return int(a_ok), int(runner_near), int(round2_near)


@pytest.mark.parametrize("b_cell", B_CELLS, ids=["B (30, 50)", "B (34, 14)"])
def test_the_runner_up_is_no_second_emitter_and_round_two_is(oracle, b_cell):
    """Four stations, windows of 8 192, max_lag 128, noise 0.5, stacks of 8 windows of A and 2 of B, guard 2, min_separation 2.
    Measured with the float64 pipeline: B (30, 50): A is the best cell in 12 of 12 stacks, the runner-up is near B in 0, round
    2 is near B in 12; B (34, 14): 12, 0 and 10."""
    from tdoa_amd import locate_multi, stacking
    ml = 128
    table = noisy_case()[0]
    Q = []
    for stack in two_emitter_windows(oracle, b_cell):
        total = np.zeros((6, 2 * ml - 1), dtype=np.int64)
        for x in stack:
            sig = [oracle.b_preprocess(s)[0] for s in x]
            total += np.array([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ml)) for i, j in PAIRS4])
        Q.append(total)

    def round2(t):
        recs = locate_multi.locate_multi(Q[t], table, 64, ml, 2, 2, 2, N_A + N_B)[0]
        assert recs[0].tobytes() == locate_multi.locate_multi(Q[t], table, 64, ml, 1, 2, 2, N_A + N_B)[0][0].tobytes()
        return int(recs["cell"][1]) if recs["score_q"][1] > 0 else None

    a_ok, runner_near, round2_near = claim_counts(Q, table, ml, b_cell, round2)
    print("B (%d, %d): A is the best cell in %d of 12 stacks, the runner-up is near B in %d, round 2 is near B in %d"
          % (b_cell // 64, b_cell % 64, a_ok, runner_near, round2_near))
    assert a_ok >= 11
    assert runner_near <= 2
    assert round2_near >= ROUND2_AT_LEAST[b_cell]
