"""CPU: the numpy statement of the fine clock search (tdoa_amd.sync_fine; include/tdoa_mi355x.h, "fine clock search") on
hand-worked cases, against an independent enumeration in Python integers, its properties, and on the measured case the feature
exists for; and the boundary of the entry points that needs no device.  hand_cases(), few_valued_case() and the measured case's
functions are shared with tests/test_gpu_sync_fine.py, which runs the kernels on the same words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_locate_cpu import FS, GRID, PAIRS4, ST4
from test_locate_upsample_cpu import (FINE_SIDE, ML, POSITIONS, cell_position, coarse_table, fine_position, fine_table, metres,
                                      position_ecef)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 2 ** 32
NAMES = ("tdoa_process_sync_fine", "tdoa_group_process_sync_fine", "tdoa_debug_sync_fine_from_q")
FACTORS = (2, 4, 8, 16)
FINE_KEYS = ("sync", "clock", "lags", "corr", "fine", "clock16", "fine_lags", "fine_corr")


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import sync_fine
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessSyncFine(", "C.tdoa_process_sync_fine(", "func (g *Group) ProcessSyncFine(",
                 "C.tdoa_group_process_sync_fine("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_sync_fine", "sync_fine_from_q"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.Group, "process_sync_fine")
    for name in ("refine", "sync_fine", "sync_fine_stacks", "midpoint_clock16"):
        assert callable(getattr(sync_fine, name)), name
    # the definition is in the header in the words the tests hold the library to
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("Exactly tdoa_process_sync(windows_per_stack, gate, rounds, ref_delay, centre, ...)",
                   "A fine lag lam, in 1/U sample, is inside when |lam| <= (max_lag - 1) U.",
                   "Q_U[lam + (max_lag - 1) U] of the pair's row, Q_U exactly as tdoa_locate_set_upsample defines it",
                   "An outside lag adds 0 and is not counted.",
                   "e^U_ij = sgn(d) * ((2|d| U + 16) div 32) with d = ref_delay[j] - ref_delay[i], taken in 64 bits",
                   "kappa_s = U k_s + y_s in 1/U sample, |y_s| <= U, y_0 = 0.",
                   "F_U(kappa) = sum over i < j of M_ij(e^U_ij + kappa_j - kappa_i).",
                   "start_q = F_U(U k).",
                   "rank(y) = 2|y| - (y > 0); the first of equal maxima wins.",
                   "The window stays centred on U k_s in every sweep",
                   "clock16_host[s] = kappa_s * (16 / U): the row tdoa_locate_set_clock takes.",
                   "If the coarse record is the zero record, or the final F_U is 0, every fine output is zero.",
                   "With Rf = 0, clock16 = 16 * clock.",
                   "The call does not read the context's tdoa_locate_set_upsample setting",
                   "|centre[s]| + gate + 1 >= 2^27"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handle_is_invalid_without_a_device(capi):
    lib = capi.load()
    rec, fine = np.zeros(4, dtype=capi.SYNC_DTYPE), np.zeros(4, dtype=capi.SYNC_DTYPE)
    q = np.zeros(3 * 7, dtype=np.int64)
    ref = (C.c_int32 * 3)(0, 16, 32)
    pr, pf, pq = rec.ctypes.data_as(C.c_void_p), fine.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_int64))
    for U, Rf in ((16, 2), (2, 0), (0, 1), (1, 1), (3, 1), (5, 1), (6, 1), (12, 1), (32, 1), (-2, 1), (16, -1), (16, 17)):
        assert lib.tdoa_process_sync_fine(None, 0, 1, 1, U, Rf, ref, None, pr, None, None, None, pf, None, None, None) == 1
        assert lib.tdoa_group_process_sync_fine(None, 0, 1, 1, U, Rf, ref, None, pr, None, None, None, pf, None, None, None) == 1
        assert lib.tdoa_debug_sync_fine_from_q(None, pq, 1, 3, 1, 1, 1, U, Rf, ref, None, pr, None, None, None, pf, None, None, None) == 1
    assert lib.tdoa_process_sync_fine(None, 0, 1, 1, 16, 2, None, None, None, None, None, None, None, None, None, None) == 1


# ---- hand-worked cases: pairs i < j in the library's order, lag l at index l + max_lag - 1 ---------------------------------
def _pair(i, j, S):
    return i * S - i * (i + 1) // 2 + (j - i - 1)


def _q(S, ml, *peaks):
    """P rows of 2 ml - 1 zeros with (i, j, lag, value in units of 2^32) set"""
    q = np.zeros((S * (S - 1) // 2, 2 * ml - 1), dtype=np.int64)
    for i, j, lag, value in peaks:
        q[_pair(i, j, S), lag + ml - 1] = value * ONE
    return q


def hand_cases():
    """[(name, dict(q, ml, ref, centre, G, R, U, Rf, n_w), expected or None for all zeros)]; expected: clock (the coarse stage's,
    samples), clock16, fine lags (0 for a pair outside), inside, moved, pairs_in.  Two equal words v side by side interpolate to
    2 x 20639 / 32768 v = 1.26 v half-way between them and to less everywhere else; v and -v side by side to 0 half-way."""
    # words 8, 8 at lags 2 and 3, the row's last lags (taps beyond the row count 0).  The coarse search takes lag 2 (x = +2
    # comes before +3).  kappa = 2 k + y: fine lag 5 = 2.5 samples is the largest, y = +1
    between = dict(q=_q(2, 4, (0, 1, 2, 8), (0, 1, 3, 8)), ml=4, ref=(0, 0), centre=None, G=3, R=1, U=2, n_w=1)
    # three stations, e_02 = e_12 = 6 samples: outside |l| < 5, and 24 +- 4 fine lags outside |lam| <= 16
    outside = dict(q=_q(3, 5, (0, 1, 0, 5), (0, 1, 1, 5), (0, 2, 4, 9), (1, 2, 4, 9)), ml=5, ref=(0, 0, 96), centre=None, G=0, R=0, n_w=2)
    return [
        ("a peak between two lags, which y moves onto", dict(Rf=1, **between),
         dict(clock=(0, 2), clock16=(0, 40), lags=(5,), inside=(1,), moved=1, pairs_in=1)),
        ("the second fine sweep moves nothing", dict(Rf=2, **between),
         dict(clock=(0, 2), clock16=(0, 40), lags=(5,), inside=(1,), moved=0, pairs_in=1)),
        ("no fine sweep: 16 x the coarse clock", dict(Rf=0, **between),
         dict(clock=(0, 2), clock16=(0, 32), lags=(4,), inside=(1,), moved=0, pairs_in=1)),
        # 7, 1, 7 at lags -1, 0, 1 and k = 0: the word is 7 at y = +-4 (phase 0) and smaller between (5.8 at +-3): the positive y
        # wins in the first sweep, the second moves nothing
        ("equal maxima: the positive y",
         dict(q=_q(2, 6, (0, 1, -1, 7), (0, 1, 0, 1), (0, 1, 1, 7)), ml=6, ref=(0, 0), centre=None, G=0, R=0, U=4, Rf=2, n_w=1),
         dict(clock=(0, 0), clock16=(0, 16), lags=(4,), inside=(1,), moved=0, pairs_in=1)),
        # -7, 7, -7 at lags -1, 0, 1: |word| is 7 at y = 0, +8 and -8 and smaller between (6.6 at +-1, the neighbours' signs
        # cancel): the smaller |y| wins
        ("equal maxima: the smaller |y|",
         dict(q=_q(2, 7, (0, 1, -1, -7), (0, 1, 0, 7), (0, 1, 1, -7)), ml=7, ref=(0, 0), centre=None, G=0, R=0, U=8, Rf=1, n_w=3),
         dict(clock=(0, 0), clock16=(0, 0), lags=(0,), inside=(1,), moved=0, pairs_in=1)),
        # pair 01's peak lies between lags 0 and 1: y_1 = +2 of U = 4; station 2's candidates all add 0: y_2 = 0, the first
        ("a fine lag outside the range adds 0 and is not counted", dict(U=4, Rf=1, **outside),
         dict(clock=(0, 0, 0), clock16=(0, 8, 0), lags=(2, 0, 0), inside=(1, 0, 0), moved=1, pairs_in=1)),
        # e^U_01 = 16 x 23 / 16 = 23 fine lags of 1/16 sample; the coarse stage has e_01 = 1 and the centre puts k_1 = 3: lag 4.
        # The word at lag 5 is the only one: coarse x = +1 -> k_1 = 4 at lag 5 = fine lag 80 = 23 + 16 * 4 - 7: y = -7
        ("e^U from the delays on the fine grid; the centre moves the window",
         dict(q=_q(2, 8, (0, 1, 5, 6)), ml=8, ref=(0, 23), centre=(0, 3), G=1, R=0, U=16, Rf=1, n_w=1),
         dict(clock=(0, 4), clock16=(0, 57), lags=(80,), inside=(1,), moved=1, pairs_in=1)),
        ("all zeros", dict(q=_q(4, 5), ml=5, ref=(0, 16, 32, 48), centre=(0, 1, -1, 2), G=2, R=1, U=16, Rf=2, n_w=1), None),
        ("two stations", dict(q=_q(2, 4, (0, 1, -2, -5), (0, 1, -3, -5)), ml=4, ref=(0, -16), centre=None, G=3, R=1, U=16, Rf=1, n_w=1),
         dict(clock=(0, -1), clock16=(0, -24), lags=(-40,), inside=(1,), moved=1, pairs_in=1)),
    ]


def _exact_word(row, ml, U, lam):
    from tdoa_amd import upsample
    return upsample.upsample_exact(row, U)[lam + (ml - 1) * U]


def _check_hand_case(out, arg, want):
    """out: sync_fine's dict of one stack"""
    from tdoa_amd import sync
    S, P = len(arg["ref"]), len(arg["q"])
    assert out["clock16"].dtype == np.int32 and out["fine_lags"].dtype == np.int32 and out["fine_corr"].dtype == np.float64
    assert out["clock16"].shape == (S,) and out["fine_lags"].shape == out["fine_corr"].shape == (P,)
    coarse = sync.sync(arg["q"], arg["ref"], arg["ml"], arg["G"], arg["R"], arg["centre"], arg["n_w"])
    for key, w in zip(("sync", "clock", "lags", "corr"), coarse):
        assert out[key].tobytes() == w.tobytes(), key
    if want is None:
        assert out["fine"].tobytes() == bytes(sync.SYNC_DTYPE.itemsize)
        assert not out["clock16"].any() and not out["fine_lags"].any() and out["fine_corr"].tobytes() == bytes(out["fine_corr"].nbytes)
        return
    rec, ml, U = out["fine"], arg["ml"], arg["U"]
    root = np.sqrt(np.float64(arg["n_w"]))
    assert out["clock"].tolist() == list(want["clock"])
    assert out["clock16"].tolist() == list(want["clock16"]) and out["fine_lags"].tolist() == list(want["lags"])
    assert (int(rec["moved"]), int(rec["pairs_in"])) == (want["moved"], want["pairs_in"])
    words = [_exact_word(arg["q"][p], ml, U, lam) if inside else 0 for p, (lam, inside) in enumerate(zip(want["lags"], want["inside"]))]
    assert int(rec["score_q"]) == sum(abs(w) for w in words)
    e = [(lambda d: (1 if d >= 0 else -1) * ((2 * abs(d) * U + 16) // 32))(arg["ref"][j] - arg["ref"][i])
         for i in range(S) for j in range(i + 1, S)]
    pairs = [(i, j) for i in range(S) for j in range(i + 1, S)]
    at_start = [e[p] + U * (want["clock"][j] - want["clock"][i]) for p, (i, j) in enumerate(pairs)]
    assert int(rec["start_q"]) == sum(abs(_exact_word(arg["q"][p], ml, U, lam)) for p, lam in enumerate(at_start) if abs(lam) <= (ml - 1) * U)
    assert float(rec["score"]) == float(int(rec["score_q"])) / ONE / root
    assert out["fine_corr"].tolist() == [float(w) / ONE / root for w in words]
    if arg["Rf"] == 0:
        assert out["clock16"].tolist() == [16 * k for k in want["clock"]]


def model(arg):
    from tdoa_amd import sync_fine
    return sync_fine.sync_fine(arg["q"], arg["ref"], arg["ml"], arg["G"], arg["R"], arg["U"], arg["Rf"], arg["centre"], arg["n_w"])


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_worked_cases(name, arg, want):
    _check_hand_case(model(arg), arg, want)


def test_model_arguments_and_the_midpoint():
    from tdoa_amd import sync_fine
    q = _q(3, 4, (0, 1, 0, 1))
    for U, Rf in ((1, 1), (3, 1), (32, 1), (0, 1), (16, -1), (16, 17)):
        with pytest.raises(ValueError):
            sync_fine.refine(q, (0, 0, 0), (0, 0, 0), 4, U, Rf)
        with pytest.raises(ValueError):
            sync_fine.sync_fine(q, (0, 0, 0), 4, 1, 1, U, Rf)
    with pytest.raises(ValueError):
        sync_fine.refine(q, (0, 0, 0), (0, 0), 4, 16, 1)
    with pytest.raises(ValueError):
        sync_fine.refine(q[:2], (0, 0, 0), (0, 0, 0), 4, 16, 1)
    # the nearest integer to (a + b) / 2, halves away from zero
    mid = sync_fine.midpoint_clock16([[0, 1, -1, 3, -3, 7, -2 ** 30]], [[0, 2, -2, 0, 0, 7, -2 ** 30]])
    assert mid.dtype == np.int32 and mid.tolist() == [[0, 2, -2, 2, -2, 7, -2 ** 30]]
    with pytest.raises(ValueError):
        sync_fine.midpoint_clock16([0, 1], [0, 1, 2])


# ---- the statement against an enumeration in Python integers, one candidate at a time --------------------------------------
def _rank(y):
    return 2 * abs(y) - (y > 0)


def _enumerate(q, ref, k, ml, U, Rf):
    """-> (start_q, score_q, moved, kappa, pairs_in, F after every sweep, candidates that tied for a step's maximum)"""
    from tdoa_amd import upsample
    S = len(ref)
    rows = [upsample.upsample_exact(r, U) for r in q]
    half = (ml - 1) * U
    pairs = [(i, j) for i in range(S) for j in range(i + 1, S)]
    e = []
    for i, j in pairs:
        d = int(ref[j]) - int(ref[i])
        e.append((1 if d >= 0 else -1) * ((2 * abs(d) * U + 16) // 32))

    def m(p, lam):
        return abs(rows[p][lam + half]) if abs(lam) <= half else 0

    def f(kap, only=None):
        return sum(m(p, e[p] + kap[j] - kap[i]) for p, (i, j) in enumerate(pairs) if only is None or only in (i, j))

    kap = [U * int(x) for x in k]
    start, moved, after, ties = f(kap), 0, [], 0
    for _ in range(Rf):
        moved = 0
        for s in range(1, S):
            best = None
            for y in sorted(range(-U, U + 1), key=_rank):
                trial = list(kap)
                trial[s] = U * int(k[s]) + y
                v = f(trial, s)
                if best is None or v > best[0]:
                    best, n_best = (v, trial[s]), 1
                elif v == best[0]:
                    n_best += 1
            ties += n_best > 1
            moved += best[1] != kap[s]
            kap[s] = best[1]
        after.append(f(kap))
    inside = sum(abs(e[p] + kap[j] - kap[i]) <= half for p, (i, j) in enumerate(pairs))
    return start, f(kap), moved, kap, inside, after, ties


def few_valued_case(S, ml, seed, n_sets=1):
    """words -3 .. 3 (x 2^32) with many zeros, delays within +-4 samples, centres within +-2: ties are common"""
    rng = np.random.default_rng(seed)
    P = S * (S - 1) // 2
    q = rng.integers(-3, 4, size=(n_sets, P, 2 * ml - 1), dtype=np.int64) * (rng.random((n_sets, P, 2 * ml - 1)) < 0.6) * ONE
    ref = rng.integers(-64, 65, size=S).astype(np.int32)
    centre = rng.integers(-2, 3, size=S).astype(np.int32)
    return q, ref, centre


def test_model_against_the_sweeps_enumerated():
    from tdoa_amd import sync_fine
    seen = dict(ties=0, outside=0, zero=0, moved=0, still=0, second_sweep_moved=0, negative_y=0, positive_y=0, full_y=0)
    for S in (2, 3, 4, 5):
        for U in FACTORS:
            for Rf in (0, 1, 3):
                for trial in range(3):
                    ml = 4 + (S + U + Rf + trial) % 5
                    q, ref, centre = few_valued_case(S, ml, 1000 * S + 10 * U + Rf + 100 * trial)
                    G = (0, 1, 3)[trial]
                    if trial == 2 and U == 16:
                        q[0, :, :] = 0 if Rf == 1 else q[0]
                    out = sync_fine.sync_fine(q[0], ref, ml, G, 1, U, Rf, centre, 2)
                    if int(out["sync"]["score_q"]) == 0:
                        assert out["fine"].tobytes() == bytes(32) and not out["clock16"].any() and not out["fine_lags"].any()
                        seen["zero"] += 1
                        continue
                    start, score, moved, kap, inside, after, ties = _enumerate(q[0], ref, out["clock"], ml, U, Rf)
                    rec = out["fine"]
                    if score == 0:
                        assert rec.tobytes() == bytes(32) and not out["clock16"].any()
                        seen["zero"] += 1
                        continue
                    assert (int(rec["start_q"]), int(rec["score_q"]), int(rec["moved"]), int(rec["pairs_in"])) == (start, score, moved, inside)
                    assert out["clock16"].tolist() == [x * (16 // U) for x in kap], (S, U, Rf, trial)
                    y = np.array(kap) - U * out["clock"].astype(np.int64)
                    assert y[0] == 0 and (np.abs(y) <= U).all()
                    if Rf == 0:
                        assert out["clock16"].tolist() == (16 * out["clock"]).tolist() and moved == 0 and start == score
                    seen["ties"] += ties
                    seen["outside"] += inside < len(q[0])
                    seen["moved" if moved else "still"] += 1
                    seen["second_sweep_moved"] += Rf == 3 and len(set(after)) > 1
                    seen["negative_y"] += int((y < 0).any())
                    seen["positive_y"] += int((y > 0).any())
                    seen["full_y"] += int((np.abs(y) == U).any())
    print("kinds of case seen:", seen)
    assert all(v > 0 for v in seen.values()), seen


def test_properties_of_the_refinement():
    """score_q >= start_q; F_U never decreases over a sweep; a result with moved == 0 is a fixed point of one more sweep"""
    from tdoa_amd import sync, sync_fine, upsample
    n_fixed = 0
    for S in (2, 3, 4, 5):
        for U in FACTORS:
            ml = 5 + S % 4
            q, ref, centre = few_valued_case(S, ml, 77 * S + U)
            k = sync.sync(q[0], ref, ml, 2, 1, centre)[1].astype(np.int64)
            qu, ml_u = upsample.upsample(q[0], U), (ml - 1) * U + 1
            i, j = np.triu_indices(S, 1)
            e = upsample.fine_lags(ref[j].astype(np.int64) - ref[i], U)
            kap, f = U * k, []
            f.append(sync.objective(qu, e, kap, ml_u)[0])
            for _ in range(4):
                moved = sync_fine.sweep(qu, e, kap, U * k, ml_u, U)
                f.append(sync.objective(qu, e, kap, ml_u)[0])
                assert f[-1] >= f[-2] and (moved or f[-1] == f[-2])
            assert f == sorted(f)
            for Rf in (0, 1, 2, 3):
                rec, c16, _, _ = sync_fine.refine(q[0], ref, k, ml, U, Rf, 1)
                assert int(rec["score_q"]) >= int(rec["start_q"])
                if Rf and int(rec["moved"]) == 0 and int(rec["score_q"]) > 0:
                    more = sync_fine.refine(q[0], ref, k, ml, U, Rf + 1, 1)
                    assert more[1].tobytes() == c16.tobytes() and int(more[0]["score_q"]) == int(rec["score_q"]) and int(more[0]["moved"]) == 0
                    n_fixed += 1
    assert n_fixed >= 8


# ---- the measured case ----------------------------------------------------------------------------------------------------
# Four stations ST4, the 48 x 64 GRID, FS, one window of 8 192 per stack, max_lag 128, G 120, R 2, U 16, Rf 2, noise 0.3,
# k = 0 .. 11.  Everything in quarter samples is realised by simulating at 4 FS and keeping every 4th IQ sample.
WL = 8192
GATE, ROUNDS, UP, FINE_ROUNDS, NOISE = 120, 2, 16, 2, 0.3
CLOCK4 = np.array([0, 149, -210, 75], dtype=np.int64)        # the station clocks in quarter samples
REF_EMITTER = (GRID["lat0"] + 40.3 * GRID["dlat"], GRID["lon0"] + 10.6 * GRID["dlon"])
TRUTH16 = (0, 597, -841, 299)


def _quarter_delays(lat, lon):
    """delta = 4 FS dist / c minus its minimum, in quarter samples, float64 [4]"""
    from tdoa_amd import locate
    dist = np.linalg.norm(locate.ecef(*np.array(ST4).T) - position_ecef(lat, lon), axis=1)
    delta = 4 * FS * dist / locate.SPEED_OF_LIGHT
    return delta - delta.min()


def measured_case():
    """-> (ref_delay [4] int32 in 1/16 sample, d4 [4] the realised delays in quarter samples, truth [4] in 1/16 sample)"""
    delta = _quarter_delays(*REF_EMITTER)
    ref_delay, d4 = np.rint(4 * delta).astype(np.int64), np.rint(delta).astype(np.int64)
    truth = 4 * CLOCK4 + 4 * d4 - ref_delay
    return ref_delay.astype(np.int32), d4, truth - truth[0]


def _quarter_window(oracle, delay4, seed, station_seed):
    return [np.ascontiguousarray(oracle.simulate_delayed_fm(4 * WL, int(delay4[s]), seed, station_seed + 1000 * s, 1.0, NOISE)
                                 .reshape(-1, 2)[::4]).reshape(-1) for s in range(4)]


def reference_window_iq(oracle, k):
    d4 = measured_case()[1]
    return _quarter_window(oracle, d4 + CLOCK4 + 400, 300 + k, 1300 + k)


def target_window_iq(oracle, k):
    """position k of tests/test_locate_upsample_cpu.py with that file's quarter-sample delays, plus the clocks"""
    from tdoa_amd import locate
    dist = np.linalg.norm(locate.ecef(*np.array(ST4).T) - position_ecef(*POSITIONS[k]), axis=1)
    d4 = np.rint(4 * FS * dist / locate.SPEED_OF_LIGHT).astype(np.int64)
    d4 -= d4.min()
    return _quarter_window(oracle, d4 + CLOCK4 + 400, 700 + k, 1700 + k)


def _float64_q(oracle, iq):
    from tdoa_amd import stacking
    sig = [oracle.b_preprocess(s)[0] for s in iq]
    return np.array([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ML)) for i, j in PAIRS4])


def fix_metres(q, k, clock16, tables={}):
    """the target window's fix under a clock row in 1/16 sample: the coarse cell under the row, then the 33 x 33 fine grid of
    tests/test_locate_upsample_cpu.py on Q x 16 under 16 x the row -> metres to the planted position"""
    from tdoa_amd import locate, upsample
    if "coarse" not in tables:
        tables["coarse"] = coarse_table()
    cell = int(locate.locate(q, tables["coarse"], 64, ML, 1, 1, clock16)[0]["cell"])
    t, kk, _, ml = upsample.scaled_args(fine_table(cell), clock16, 0, ML, UP)
    f = int(locate.locate(upsample.upsample(q, UP), t, FINE_SIDE, ml, 1, 1, kk)[0]["cell"])
    return metres(POSITIONS[k], fine_position(cell, f))


def measure(q_ref, q_tgt, outs):
    """q_ref, q_tgt [12][6][255]; outs: sync_fine's outputs per reference window -> (fix medians under the whole-lag, refined
    and true clocks, clock-error medians whole-lag and refined in 1/16 sample, windows whose coarse clocks are all within one
    sample); prints every figure"""
    truth = measured_case()[2]
    d, err, near = np.zeros((12, 3)), np.zeros((12, 2)), 0
    for k in range(12):
        whole, fine = 16 * outs[k]["clock"].astype(np.int64), outs[k]["clock16"].astype(np.int64)
        err[k] = np.abs(whole - truth).max(), np.abs(fine - truth).max()
        near += bool((np.abs(whole - truth) <= 16).all())
        for n, row in enumerate((whole, fine, truth)):
            d[k, n] = fix_metres(q_tgt[k], k, row)
        print("window %2d: clocks whole-lag %s refined %s; worst error %d/16 and %d/16; fix %.0f m, %.0f m, true clocks %.0f m"
              % (k, whole.tolist(), fine.tolist(), err[k, 0], err[k, 1], d[k, 0], d[k, 1], d[k, 2]))
    med, med_err = np.median(d, axis=0), np.median(err, axis=0)
    print("medians: fix under whole-lag clocks %.1f m, refined %.1f m, true %.1f m (ratios %.2f and %.2f); worst clock error "
          "whole-lag %.1f/16, refined %.1f/16; coarse clocks within one sample in %d of 12 windows"
          % (med[0], med[1], med[2], med[1] / med[0], med[1] / med[2], med_err[0], med_err[1], near))
    return med, med_err, near


def assert_measured(med, med_err):
    assert med[1] <= 0.5 * med[0]            # 1. the refined fix against the whole-lag-clock fix
    assert med[1] <= 1.25 * med[2]           # 2. ... against the true-clock fix
    assert med_err[1] <= 0.5 * med_err[0]    # 3. the refined clock error against the whole-lag one


def test_refined_clocks_give_the_sub_sample_locate_its_resolution(oracle):
    """The measured case on the float64 pipeline's words.  The request measured: worst station clock error, median over the
    twelve windows, 11/16 sample with whole-lag clocks and 2/16 refined; median distance of the fix 290.4 m under whole-lag
    clocks, 66.1 m under refined ones, 64.1 m under the true ones (ratios 0.23 and 1.03); the coarse search within one sample in
    12 of 12 windows.  This rebuild gives the same figures; they are printed."""
    from tdoa_amd import sync_fine
    ref_delay, _, truth = measured_case()
    assert tuple(truth.tolist()) == TRUTH16
    q_ref = [_float64_q(oracle, reference_window_iq(oracle, k)) for k in range(12)]
    q_tgt = [_float64_q(oracle, target_window_iq(oracle, k)) for k in range(12)]
    outs = [sync_fine.sync_fine(q_ref[k], ref_delay, ML, GATE, ROUNDS, UP, FINE_ROUNDS) for k in range(12)]
    med, med_err, _ = measure(q_ref, q_tgt, outs)
    assert_measured(med, med_err)
