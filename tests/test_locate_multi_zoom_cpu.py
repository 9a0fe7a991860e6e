"""CPU: the zoomed rounds (tdoa_process_locate_multi_zoom; include/tdoa_mi355x.h, "zoomed rounds").  The entries and the header's
phrases, the boundary that needs no device, the numpy statement (tdoa_amd.locate_multi_zoom) against an enumeration of every
round, window position and pair in Python integers, the identities that follow from the definition, and the two-emitter case on
the float64 pipeline.  multi_case(), COMBOS, statement() and the two-emitter helpers are shared with
tests/test_gpu_locate_multi_zoom.py, which runs the kernels on the same words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_locate_cpu import FS, PAIRS4, ST4
from test_locate_upsample_cpu import BOUND, ML, POSITIONS, cell_position, coarse_table, metres, position_ecef
from test_locate_zoom_cpu import (COARSE_COLS, COARSE_ROWS, FINE_COLS, FINE_ROWS, SMALL_Z, ZOOM_H, ZOOM_Z, global_fine_table, global_position,
                                  pairs_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdoa_process_locate_multi_zoom", "tdoa_group_process_locate_multi_zoom", "tdoa_debug_locate_multi_zoom_from_q")
KEYS = ("loc", "lags", "corr", "map", "zoom", "zpairs", "zlags", "zcorr", "zmap")


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import locate_multi_zoom
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessLocateMultiZoom(", "C.tdoa_process_locate_multi_zoom(", "func (g *Group) ProcessLocateMultiZoom(",
                 "C.tdoa_group_process_locate_multi_zoom("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for name in ("process_locate_multi_zoom", "locate_multi_zoom_from_q"):
        assert hasattr(capi.Context, name), name
    assert hasattr(capi.Group, "process_locate_multi_zoom")
    s = capi._search("locate_multi_zoom")
    assert tuple(o.key for o in s.outputs) == KEYS == locate_multi_zoom.NAMES
    assert s.ints == ("n_emitters", "guard", "min_separation", "Z", "H", "fine_separation")
    assert all(o.shape[0] == "K" for o in s.outputs) and [o.poison for o in s.outputs] == [False] * 4 + [True] * 5
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("The coarse stage is tdoa_process_locate_multi(windows_per_stack, n_emitters, guard, min_separation) unchanged",
                   "the first four outputs are its bytes", "The zoom's maps are not judged",
                   "The window of round r of stack s is the zoom locate's window of (2H + 1)^2 positions around Z x that round's coarse cell",
                   "with the zoom's geometry and competing rule",
                   "The mask is M_p^r, the one round r's coarse scores ran under",
                   "a pair whose lag lies within guard of a centre left by rounds 0 .. r - 1 counts 0",
                   "The centres stay the coarse cells' lags: a round's fine cell adds nothing to E",
                   "everything runs on Q_U, U x the fine table, U x the clocks and U x guard, as the rounds do",
                   "pairs_in counts the pairs inside the range and not excluded at the fine cell",
                   "n_best, the box and the runner-up are taken on the round's masked window scores",
                   "zpairs: (pairs_in, reserved), reserved the pairs inside the range but excluded at the fine cell",
                   "a pair outside the range reports 0 and 0.0, an excluded pair reports its lag and 0.0 (all bytes zero), so tdoa_solve_surface gives it no weight",
                   "zmap: the window's masked scores, -1 where a position does not compete",
                   "a round with the zero coarse record gets the zero tdoa_zoom, zero zpairs, zero lags and correlations and a zmap of -1 throughout",
                   "A window with no competing position, or whose largest masked score is 0, also gets the zero record",
                   "its zmap still holds its scores",
                   "n_emitters = 1 returns tdoa_process_locate_zoom's eight outputs and zpairs = (pairs_in, 0)",
                   "every round's fine cell, score_q, pairs_in, reserved, lags and correlations are that round's coarse record's",
                   "the track rounds (tdoa_process_locate_track_multi) are not zoomed",
                   "the masks come from the coarse cells, never from the fine ones", "there is no stop rule",
                   "Two kernels behind the rounds' launches for any n_emitters, the round a grid dimension",
                   "The graph's key is the rounds' words plus (Z, H, fine_separation, n_cells_f, n_cols_f) under a kind of its own",
                   "the window maps [n_emitters][n_stacks_total][(2H+1)^2] do not fit",
                   "The rounds have tdoa_process_locate_multi_zoom",
                   "Scope: the rounds (tdoa_process_locate_multi) and the cell tracks are not zoomed"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def _outputs(capi, n_sets, p, n_cells, H, K):
    s = capi._search("locate_multi_zoom")
    out = capi._search_outputs(s, capi._shape_numbers({"H": H, "n_emitters": K}, n_sets, 0, n_cells, P=p), {"want_map": True, "want_zmap": True})
    return out, tuple(capi._search_ptrs(s, out))


def test_null_handles_and_bad_arguments_need_no_device(capi):
    lib = capi.load()
    i64 = C.POINTER(C.c_int64)
    q = np.zeros((1, 3, 7), dtype=np.int64)
    out, ptrs = _outputs(capi, 1, 3, 4, 1, 2)
    assert out["zoom"].shape == (2, 1) and out["zpairs"].shape == (2, 1, 2) and out["zmap"].shape == (2, 1, 9)
    before = {k: v.tobytes() for k, v in out.items()}
    for K, guard, sep, Z, H, fsep in ((2, 1, 1, 1, 1, 1), (8, 0, 1, 64, 64, 2), (0, 0, 1, 1, 1, 1), (9, 0, 1, 1, 1, 1), (2, -1, 1, 1, 1, 1),
                                      (2, 0, 0, 1, 1, 1), (2, 0, 1, 0, 1, 1), (2, 0, 1, 65, 1, 1), (2, 0, 1, 1, -1, 1), (2, 0, 1, 1, 65, 1),
                                      (2, 0, 1, 1, 1, 0)):
        assert lib.tdoa_process_locate_multi_zoom(None, 0, K, guard, sep, Z, H, fsep, *ptrs) == 1
        assert lib.tdoa_group_process_locate_multi_zoom(None, 0, K, guard, sep, Z, H, fsep, *ptrs) == 1
        assert lib.tdoa_debug_locate_multi_zoom_from_q(None, q.ctypes.data_as(i64), 1, 3, 1, K, guard, sep, Z, H, fsep, *ptrs) == 1
    assert lib.tdoa_process_locate_multi_zoom(None, 0, 2, 0, 1, 1, 1, 1, *([None] * 9)) == 1
    assert {k: v.tobytes() for k, v in out.items()} == before            # nothing was written
    case = multi_case(3, 4, 1)
    for kw in (dict(K=0), dict(K=9), dict(guard=-1), dict(Z=0), dict(H=65), dict(fsep=0)):      # the numpy statement refuses the same ranges
        with pytest.raises(ValueError):
            statement(case, **dict(dict(H=1, K=2, guard=0), **kw))


# ---- small cases ----------------------------------------------------------------------------------------------------------
# the coarse cells of every set's planted emitters, strongest first: the four corners (whose windows cross the fine table's edge)
# and cells inside; no cell serves two sets, since a cell's delays carry its set's clocks
EMITTERS = ((0, 17, 30), (6, 22), (28, 11, 19), (34, 8), (16, 3, 32))
BLIND = 22                                               # this emitter's own fine cell sees no pair: a window of H = 0 scores 0
# (H, fine_separation, K, guard; guard None: 2 max_lag, every lag of a found pair) -- every H, K and guard of the request
COMBOS = ((0, 1, 1, 0), (0, 1, 3, 1), (1, 1, 2, 1), (1, 2, 3, None), (2, 1, 3, 0), (2, 1, 8, 1), (5, 2, 2, None), (5, 1, 8, 0), (0, 1, 8, None))


def multi_case(S, ml, seed, clocked=False, short=False):
    """small_case of tests/test_locate_zoom_cpu.py with several emitters per set: a coarse 5 x 7 table, Z = 3 and a 13 x 19 fine
    table with fine (3 r, 3 c) = coarse (r, c) (short: the last fine row holds 11 cells), and six sets of n_w = 2 windows.  Set
    k < 5 has, for emitter e of EMITTERS[k], a word of magnitude 2^(44 - 2 e) planted at every pair's lag of that coarse cell --
    whose delays (plus the set's clocks) are whole samples, pair (0, 1)'s lag two apart from emitter to emitter, the other stations'
    within one sample, so that later emitters share lags with earlier ones; set 5 is all zero.  Every other coarse cell has pair
    (0, 1) outside the range, the other fine cells have random delays up to max_lag + 2 samples, the fine cells above and below an
    emitter's (where they exist) repeat its delays -- a plateau -- and the fine cell of coarse cell BLIND itself has every pair
    outside the range.  -> dict(q [6][P][2 ml - 1], table, n_cols, fine, n_cols_f, clock or None, ml, n_w, S, Z)"""
    rng = np.random.default_rng(seed)
    pairs = pairs_of(S)
    P, n = len(pairs), 2 * ml - 1
    fine = rng.integers(-8 * (ml + 2), 8 * (ml + 2) + 1, size=(FINE_ROWS, FINE_COLS, S)).astype(np.int64)
    fine[::SMALL_Z, ::SMALL_Z, 1] = fine[::SMALL_Z, ::SMALL_Z, 0] + 16 * (ml + 1) * rng.choice([-1, 1], size=(COARSE_ROWS, COARSE_COLS))
    clock = np.zeros((6, S), dtype=np.int64)
    if clocked:                                           # whole samples; the difference of stations 0 and 1 is the same in every set
        clock = 16 * rng.integers(-1, 2, size=(6, S))
        clock[:, 1] = clock[:, 0] + 16
    q = rng.integers(-2 ** 30, 2 ** 30, size=(6, P, n), dtype=np.int64)
    for k, cells in enumerate(EMITTERS):
        for e, t in reversed(list(enumerate(cells))):     # (the strongest emitter's words are written last)
            tau = rng.integers(-1, 2, size=S)            # the emitter's delays plus set k's clocks, in samples
            tau[0] = 0
            tau[1] = 2 * (e - 1)                          # pair (0, 1) tells a set's emitters apart, more than a guard of 1
            r, c = SMALL_Z * (t // COARSE_COLS), SMALL_Z * (t % COARSE_COLS)
            for rr in (r - 1, r, r + 1):
                if 0 <= rr < FINE_ROWS:
                    fine[rr, c] = 16 * tau - clock[k]
            for p, (i, j) in enumerate(pairs):
                lag = int(tau[j] - tau[i])
                assert abs(lag) < ml
                q[k, p, lag + ml - 1] = 2 ** (44 - 2 * e) * (-1 if (p + k + e) % 2 else 1)
    q[5] = 0
    table = fine[::SMALL_Z, ::SMALL_Z].reshape(-1, S).astype(np.int32)
    fine[SMALL_Z * (BLIND // COARSE_COLS), SMALL_Z * (BLIND % COARSE_COLS)] = 16 * (ml + 20) * np.arange(S)
    fine = fine.reshape(-1, S).astype(np.int32)
    if short:
        fine = fine[:len(fine) - 8]
    return dict(q=q, table=table, n_cols=COARSE_COLS, fine=fine, n_cols_f=FINE_COLS, clock=clock.astype(np.int32) if clocked else None,
                ml=ml, n_w=2, S=S, Z=SMALL_Z)


def statement(case, H, K, guard, U=1, sep=1, fsep=1, Z=None, fine=None, n_cols_f=None):
    """the numpy statement on a case; guard None: 2 max_lag"""
    from tdoa_amd import locate_multi_zoom
    return locate_multi_zoom.multi_zoom_upsampled(case["q"], case["table"], case["n_cols"], case["fine"] if fine is None else fine,
                                                  case["n_cols_f"] if n_cols_f is None else n_cols_f, case["ml"], case["Z"] if Z is None else Z,
                                                  H, U, K, 2 * case["ml"] if guard is None else guard, sep, fsep, case["n_w"], case["clock"])


def _cell_lags(row, clock, U, ml):
    """one cell's delays -> per pair its lag in 1/U sample, None outside the range; by the definition, in Python integers"""
    hi = (ml - 1) * U
    out = []
    for i, j in pairs_of(len(row)):
        d = int(row[j]) - int(row[i]) + (int(clock[j]) - int(clock[i]) if clock is not None else 0)
        a = (2 * abs(d) * U + 16) // 32
        lag = -a if d < 0 else a
        out.append(lag if -hi <= lag <= hi else None)
    return out


def _enumerate_rounds(case, k, H, U, sep, fsep, K, guard):
    """set k by the definition -> per round dict(scores [coarse cell], best or None, zmap, rec or None, zpairs, zlags, words), the
    words None for a pair outside the range and 0 for an excluded one"""
    from tdoa_amd import upsample
    ml, Z, n_cols, n_cols_f, n_cells_f = case["ml"], case["Z"], case["n_cols"], case["n_cols_f"], len(case["fine"])
    fine_q = [upsample.upsample_exact(row, U) for row in case["q"][k]]
    clock = None if case["clock"] is None else case["clock"][k]
    lo, g = -(ml - 1) * U, guard * U
    coarse_lags = [_cell_lags(row, clock, U, ml) for row in case["table"]]
    fine_lags = {}
    centres = [[] for _ in fine_q]                        # E_p as its intervals' centres
    side = 2 * H + 1

    def word(p, lag):                                     # the pair's word under the mask: None outside, 0 excluded
        if lag is None:
            return None
        return 0 if any(abs(lag - c) <= g for c in centres[p]) else fine_q[p][lag - lo]

    def score(lags):
        return sum(abs(word(p, l) or 0) for p, l in enumerate(lags))

    rounds = []
    for _ in range(K):
        scores = [score(l) for l in coarse_lags]
        out = dict(scores=scores, best=None, zmap=[-1] * (side * side), rec=None, zpairs=[0, 0], zlags=None, words=None)
        rounds.append(out)
        if max(scores) <= 0:
            continue
        best = out["best"] = scores.index(max(scores))
        cand = []
        for wa in range(side):
            for wb in range(side):
                row, col = Z * (best // n_cols) - H + wa, Z * (best % n_cols) - H + wb
                if row < 0 or not 0 <= col < n_cols_f or row * n_cols_f + col >= n_cells_f:
                    continue
                cell = row * n_cols_f + col
                if cell not in fine_lags:
                    fine_lags[cell] = _cell_lags(case["fine"][cell], clock, U, ml)
                s = out["zmap"][wa * side + wb] = score(fine_lags[cell])
                cand.append((s, cell, row, col))
        if cand and max(c[0] for c in cand) > 0:
            top = max(c[0] for c in cand)
            tops = [c for c in cand if c[0] == top]
            win = min(tops, key=lambda c: c[1])
            far = [c for c in cand if max(abs(c[2] - win[2]), abs(c[3] - win[3])) > fsep]
            lags = fine_lags[win[1]]
            words = [word(p, l) for p, l in enumerate(lags)]
            excluded = [l is not None and any(abs(l - c) <= g for c in centres[p]) for p, l in enumerate(lags)]
            inside = sum(l is not None for l in lags)
            rec = dict(cell=win[1], pairs_in=inside - sum(excluded), n_best=len(tops), row_lo=min(c[2] for c in tops),
                       row_hi=max(c[2] for c in tops), col_lo=min(c[3] for c in tops), col_hi=max(c[3] for c in tops), score_q=top,
                       runner_cell=0, runner_q=0)
            if far:
                best_far = max(c[0] for c in far)
                rec["runner_q"], rec["runner_cell"] = best_far, min(c[1] for c in far if c[0] == best_far)
            out.update(rec=rec, zpairs=[rec["pairs_in"], sum(excluded)], zlags=[l or 0 for l in lags],
                       words=[0 if e else w for w, e in zip(words, excluded)])
        for p, l in enumerate(coarse_lags[best]):         # the centres stay the coarse cell's lags
            if l is not None:
                centres[p].append(l)
    return rounds


CASES = [(3, 4, False, False), (4, 9, True, False), (4, 9, False, True), (3, 4, True, True)]


def _case(S, ml, clocked, short):
    return multi_case(S, ml, 140 + 7 * S + ml, clocked, short)


@pytest.mark.parametrize("U", (1, 4, 16))
@pytest.mark.parametrize("S, ml, clocked, short", CASES)
def test_the_statement_against_an_enumeration(S, ml, clocked, short, U):
    from tdoa_amd import stacking
    case = _case(S, ml, clocked, short)
    for H, fsep, K, guard in COMBOS:
        g = 2 * ml if guard is None else guard
        loc, lags, corr, cmap, zoom, zpairs, zlags, zcorr, zmap = statement(case, H, K, guard, U, 1, fsep)
        assert zoom.shape == (K, 6) and zoom.dtype.itemsize == 64 and zpairs.shape == (K, 6, 2) and zpairs.dtype == np.int32
        assert zmap.shape == (K, 6, (2 * H + 1) ** 2) and zmap.dtype == np.int64 and zlags.dtype == np.int32 and zcorr.dtype == np.float64
        for k in range(6):
            for r, want in enumerate(_enumerate_rounds(case, k, H, U, 1, fsep, K, g)):
                at = (H, K, guard, k, r)
                assert cmap[r, k].tolist() == want["scores"], at
                assert zmap[r, k].tolist() == want["zmap"], at
                assert zpairs[r, k].tolist() == want["zpairs"], at
                if want["best"] is None:
                    assert loc[r, k].tobytes() == bytes(48) and (zmap[r, k] == -1).all()
                else:
                    assert int(loc[r, k]["cell"]) == want["best"] and int(loc[r, k]["score_q"]) == want["scores"][want["best"]], at
                if want["rec"] is None:
                    assert zoom[r, k].tobytes() == bytes(64) and not zlags[r, k].any() and zcorr[r, k].tobytes() == bytes(8 * zcorr.shape[2]), at
                    continue
                for name, value in want["rec"].items():
                    assert int(zoom[r, k][name]) == value, at + (name,)
                assert zlags[r, k].tolist() == want["zlags"], at
                assert zcorr[r, k].tobytes() == np.array([0.0 if not w else float(stacking.from_fixed(np.int64(w), case["n_w"]))
                                                          for w in want["words"]]).tobytes(), at
                assert float(zoom[r, k]["score"]) == float(stacking.from_fixed(np.int64(want["rec"]["score_q"]), case["n_w"]))
                assert float(zoom[r, k]["runner_up"]) == float(stacking.from_fixed(np.int64(want["rec"]["runner_q"]), case["n_w"]))


def test_every_kind_of_case_occurs():
    """over the cases above, counted on the statement that test holds to the enumeration: a later round's fine cell with an excluded pair, a window crossing the fine table's edge, a later
    round's plateau, a zero round with its zero zoom record, a window whose masked maximum is 0 behind a coarse cell"""
    total = dict(reserved=0, edge=0, plateau=0, zero=0, blank=0)
    for S, ml, clocked, short in CASES:
        case = _case(S, ml, clocked, short)
        for U in (1, 4, 16):
            for H, fsep, K, guard in COMBOS:
                loc, _, _, _, zoom, zpairs, _, _, zmap = statement(case, H, K, guard, U, 1, fsep)
                found, later = loc["score_q"] > 0, np.arange(K)[:, None] > 0
                total["reserved"] += int((later & (zoom["score_q"] > 0) & (zpairs[..., 1] > 0)).sum())
                total["edge"] += int((found & (zmap == -1).any(axis=2)).sum())
                total["plateau"] += int((later & (zoom["n_best"] >= 2)).sum())
                total["zero"] += int((later & ~found & (zoom["score_q"] == 0) & (zmap == -1).all(axis=2)).sum())
                total["blank"] += int((found & (zmap.max(axis=2) == 0) & (zoom["score_q"] == 0)).sum())
    print(total)
    assert all(n >= 5 for n in total.values()), total


@pytest.mark.parametrize("U", (1, 4))
def test_identities_on_the_statement(U):
    """K = 1 is the zoom locate; round 0 of every K is K = 1; the coarse four are locate_multi's; the table as the fine table with
    Z = 1 returns every round's coarse record"""
    from tdoa_amd import locate_multi, locate_zoom, upsample
    case = multi_case(4, 9, 91, clocked=True)
    args = (case["q"], case["table"], case["n_cols"], case["fine"], case["n_cols_f"], case["ml"], case["Z"])
    for H, guard in ((2, 1), (5, 0)):
        one = statement(case, H, 1, guard, U, 2, 2)
        zoom = locate_zoom.zoom_upsampled(*args, H, U, 2, 2, case["n_w"], case["clock"])
        for a, b in zip(one[:5] + one[6:], zoom):
            assert a.shape == (1,) + b.shape and a.dtype == b.dtype and a[0].tobytes() == b.tobytes()
        assert one[5][0, :, 0].tolist() == zoom[4]["pairs_in"].tolist() and not one[5][0, :, 1].any()
        for K in (2, 3, 8):
            out = statement(case, H, K, guard, U, 2, 2)
            assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(out, one)), K
            t, k, g, ml_u = upsample.scaled_args(case["table"], case["clock"], guard, case["ml"], U)
            rounds = locate_multi.locate_multi_stacks(upsample.upsample(case["q"], U), t, case["n_cols"], ml_u, K, g, 2, case["n_w"], k)
            assert all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(out[:4], rounds)), K
    loc, lags, corr, _, zoom, zpairs, zlags, zcorr, _ = statement(case, 2, 3, 1, U, Z=1, fine=case["table"], n_cols_f=case["n_cols"])
    assert (loc["score_q"][1] > 0).sum() >= 3 and (loc["reserved"] > 0).any()
    for name in ("cell", "score_q", "pairs_in", "score"):
        assert zoom[name].tolist() == loc[name].tolist(), name
    assert zpairs[..., 0].tolist() == loc["pairs_in"].tolist() and zpairs[..., 1].tolist() == loc["reserved"].tolist()
    assert zlags.tobytes() == lags.tobytes() and zcorr.tobytes() == corr.tobytes()


# ---- the two-emitter case -------------------------------------------------------------------------------------------------
N_A, N_B, N_STACKS, NOISE = 8, 2, 12, 0.3
CLAIM = dict(K=2, guard=2, sep=2, fsep=1, U=16)
A_WITHIN_150_AT_LEAST, B_WITHIN_150_AT_LEAST = 10, 9      # measured 12 and 11 of 12: a margin of two stacks


def B_OF(t):
    """stack t: A at POSITIONS[t], B at POSITIONS[(t + 5) % 12]"""
    return (t + 5) % 12


def emitter_window_iq(oracle, pos, w, noise=NOISE):
    """window w of an emitter at POSITIONS[pos], u8 IQ per station: test_locate_upsample_cpu.window_iq's quarter-sample delays,
    with the seeds 300 + w and 1000 (s + 1) + w"""
    from tdoa_amd import locate
    dist = np.linalg.norm(locate.ecef(*np.array(ST4).T) - position_ecef(*POSITIONS[pos]), axis=1)
    d4 = np.rint(4 * FS * dist / locate.SPEED_OF_LIGHT).astype(np.int64)
    d4 -= d4.min()
    return [np.ascontiguousarray(oracle.simulate_delayed_fm(4 * 8192, int(d4[s]), 300 + w, 1000 * (s + 1) + w, 1.0, noise)
                                 .reshape(-1, 2)[::4]).reshape(-1) for s in range(4)]


def two_emitter_windows(oracle):
    """stack t = 0 .. 11 holds the windows w = 16 t + k, k = 0 .. 9: 8 of A, then 2 of B -> [stack][k][station] u8 IQ"""
    return [[emitter_window_iq(oracle, t if k < N_A else B_OF(t), 16 * t + k) for k in range(N_A + N_B)] for t in range(N_STACKS)]


def claim_figures(loc, zoom):
    """loc, zoom [2][12] -> per emitter (A, B): (median distance of the coarse cell's centre, of the zoomed fix, fixes within 100 m,
    within 150 m); a round without a cell counts as infinitely far"""
    n_cols_f = global_fine_table()[1]
    out = []
    for r, where in ((0, lambda t: POSITIONS[t]), (1, lambda t: POSITIONS[B_OF(t)])):
        coarse = np.array([metres(where(t), cell_position(int(loc[r, t]["cell"]))) if loc[r, t]["score_q"] > 0 else np.inf for t in range(12)])
        fix = np.array([metres(where(t), global_position(*divmod(int(zoom[r, t]["cell"]), n_cols_f))) if zoom[r, t]["score_q"] > 0 else np.inf
                        for t in range(12)])
        out.append((float(np.median(coarse)), float(np.median(fix)), int((fix <= 100).sum()), int((fix <= 150).sum())))
    return out


def check_claim(figures, what):
    (a_coarse, a_fix, a100, a150), (b_coarse, b_fix, b100, b150) = figures
    print("%s: A (round 0): coarse cell centre %.1f m, zoomed fix %.1f m, within 100 m %d of 12, within 150 m %d of 12; "
          "B (round 1): coarse cell centre %.1f m, zoomed fix %.1f m (ratio %.2f), within 100 m %d of 12, within 150 m %d of 12"
          % (what, a_coarse, a_fix, a100, a150, b_coarse, b_fix, b_fix / b_coarse, b100, b150))
    assert a150 >= A_WITHIN_150_AT_LEAST
    assert b150 >= B_WITHIN_150_AT_LEAST
    assert b_fix <= BOUND * b_coarse


def test_the_weak_emitter_gets_a_sub_cell_fix(oracle):
    """Four stations, the 48 x 64 grid, the global 377 x 505 fine table (Z = 8, H = 16), max_lag 128, noise 0.3, twelve stacks of 8
    windows of A and 2 of B, K = 2, guard 2, min_separation 2, fine_separation 1, U = 16.  Measured with the float64 pipeline and
    this statement: A (round 0): coarse cell centre 137.5 m, zoomed fix 31.6 m, within 100 m 12 of 12, within 150 m 12 of 12;
    B (round 1): coarse cell centre 137.5 m, zoomed fix 38.2 m (ratio 0.28), within 100 m 10 of 12, within 150 m 11 of 12."""
    from tdoa_amd import locate_multi_zoom, stacking
    table = coarse_table()
    fine, n_cols_f = global_fine_table()
    Q = []
    for stack in two_emitter_windows(oracle):
        total = np.zeros((6, 2 * ML - 1), dtype=np.int64)
        for x in stack:
            sig = [oracle.b_preprocess(s)[0] for s in x]
            total += np.array([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ML)) for i, j in PAIRS4])
        Q.append(total)
    out = locate_multi_zoom.multi_zoom_upsampled(np.stack(Q), table, 64, fine, n_cols_f, ML, ZOOM_Z, ZOOM_H, CLAIM["U"], CLAIM["K"], CLAIM["guard"],
                                                 CLAIM["sep"], CLAIM["fsep"], N_A + N_B)
    check_claim(claim_figures(out[0], out[4]), "float64 pipeline")
