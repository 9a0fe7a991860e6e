"""CPU: the numpy statement of the closure search (tdoa_amd.closure; include/tdoa_mi355x.h, "closure search") on hand-worked
cases, against an enumeration of every cell, and on the noisy case the feature exists for; and the boundary of the four
entry points that needs no device.  hand_cases() is shared with tests/test_gpu_closure.py, which runs the kernels on the
same words."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 2 ** 32
NAMES = ("tdoa_num_triples", "tdoa_process_closure", "tdoa_group_process_closure", "tdoa_debug_closure_from_q")


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import closure
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert "func (g *gpuCorrelator) ProcessClosure(" in go and "C.tdoa_process_closure(" in go
    assert "func (g *Group) ProcessClosure(" in go and "C.tdoa_group_process_closure(" in go
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("num_triples", "process_closure", "closure_from_q"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.Group, "process_closure")
    # the record: the fields of the header in their order, no padding
    assert capi.CLOSURE_DTYPE == closure.CLOSURE_DTYPE and capi.CLOSURE_DTYPE.itemsize == 80
    assert capi.CLOSURE_DTYPE.names == ("lag_ij", "lag_ik", "lag_jk", "residual", "score_q", "own_q", "runner_q", "corr_ij",
                                        "corr_ik", "corr_jk", "score", "runner_up")
    m = re.search(r"typedef struct \{([^}]*)\} tdoa_closure;", hdr)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+([^;]+);", m.group(1))
    assert [(t, [n.strip() for n in names.split(",")]) for t, names in fields] == [
        ("int32_t", ["lag_ij", "lag_ik", "lag_jk", "residual"]), ("int64_t", ["score_q", "own_q", "runner_q"]),
        ("double", ["corr_ij", "corr_ik", "corr_jk"]), ("double", ["score", "runner_up"])]
    # the definition is in the header in the words the tests hold the library to
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("Pairs are i < j in the library's order, p(i,j) = i*S - i(i+1)/2 + (j-i-1).",
                   "Triples are i < j < k in lexicographic order. There are T = S(S-1)(S-2)/6 of them, returned by tdoa_num_triples.",
                   "M_p[l] = |Q_p[l]|, an int64.",
                   "The centre of a pair is c_p(i,j) = centre[j] - centre[i], so centres close by construction.",
                   "G = gate, 0 <= G <= 1023.",
                   "A cell (u, v) of triple (i,j,k) has |u| <= G, |v| <= G and |v-u| <= G.",
                   "Its lags are a = c_ij + u, b = c_ik + v and e = b - a = c_jk + (v-u).",
                   "a cell with a lag outside does not exist.",
                   "score_q(u,v) = M_ij[a] + M_ik[b] + M_jk[e].",
                   "Among equal maxima the smaller |u| wins, then the positive u, then the smaller |v|, then the positive v.",
                   "The zero record (all bytes 0) is returned when no cell exists or the maximum is 0.",
                   "Equal maxima go to the smaller |x|, then the positive x.",
                   "residual = (c_ij+x*_ij) + (c_jk+x*_jk) - (c_ik+x*_ik).",
                   "So score_q <= own_q, and residual == 0 implies score_q == own_q.",
                   "runner_q is the largest score_q over the cells with max(|u-u*|, |v-v*|) > min_separation"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handle_is_invalid_without_a_device(capi):
    lib = capi.load()
    out = np.zeros(8, dtype=capi.CLOSURE_DTYPE)
    q = np.zeros(3 * 7, dtype=np.int64)
    centre = (C.c_int32 * 3)(0, 1, 2)
    po, pq = out.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_int64))
    assert lib.tdoa_num_triples(None) == 0
    for m, G, sep in [(0, 40, 1), (2, 0, 3), (0, 1023, 1), (-1, 40, 1), (0, -1, 1), (0, 1024, 1), (0, 40, 0)]:
        for c in (None, centre):
            assert lib.tdoa_process_closure(None, m, G, sep, c, po) == 1
            assert lib.tdoa_group_process_closure(None, m, G, sep, c, po) == 1
            assert lib.tdoa_debug_closure_from_q(None, pq, 1, 3, 1, G, sep, c, po) == 1
    assert lib.tdoa_process_closure(None, 0, 40, 1, None, None) == 1
    assert lib.tdoa_group_process_closure(None, 0, 40, 1, None, None) == 1
    assert lib.tdoa_debug_closure_from_q(None, None, 0, 2, 0, 40, 1, None, None) == 1


# ---- hand-worked cases: three stations, max_lag 4 (7 lags, lag l at index l + 3), rows ij, ik, jk ------------------------
def _q(ml, *peaks):
    """three rows of 2 ml - 1 zeros with (row, lag, value in units of 2^32) set"""
    q = np.zeros((3, 2 * ml - 1), dtype=np.int64)
    for row, lag, value in peaks:
        q[row, lag + ml - 1] = value * ONE
    return q


def hand_cases():
    """[(name, dict(q, ml, G, sep, centre, n_w), expected fields or None for the zero record)]; lags and integer fields in
    units of 2^32 where they are sums"""
    A = _q(4, (0, 1, 3), (1, -1, 3), (2, -2, 3))                      # 1 + (-2) = -1: the three argmaxes close
    cases = [
        ("the three argmaxes close", dict(q=A, ml=4, G=3, sep=1, centre=None, n_w=1),
         dict(lags=(1, -1, -2), residual=0, score=9, own=9, runner=3)),
        # pair jk's argmax is an outlier at lag 3 (4 > 3): the independent lags give 1 + 3 - (-1) = 5; jointly the cells with
        # e = 3 reach 4 only (u = 1 would need v = 4 > G), the closing set keeps 9
        ("an outlier in one pair is repaired", dict(q=_q(4, (0, 1, 3), (1, -1, 3), (2, -2, 3), (2, 3, 4)), ml=4, G=3, sep=1,
                                                    centre=None, n_w=1),
         dict(lags=(1, -1, -2), residual=5, score=9, own=10, runner=4)),
        ("negative Q counts by its magnitude", dict(q=_q(4, (0, 1, -3), (1, -1, 3), (2, -2, -3)), ml=4, G=3, sep=1, centre=None,
                                                    n_w=4),
         dict(lags=(1, -1, -2), residual=0, score=9, own=9, runner=3, signs=(-1, 1, -1))),
        ("all zeros", dict(q=_q(4), ml=4, G=3, sep=1, centre=None, n_w=1), None),
        # only M_ij is not zero, at u = +1 and -1: the positive u, then the smallest |v|.  (The flat pairs' own peaks are at x = 0
        # by the same rule, so the residual is x*_ij + x*_jk - x*_ik with one term only; score_q = own_q all the same.)
        ("equal maxima: the positive u, the smaller |v|", dict(q=_q(4, (0, 1, 1), (0, -1, 1)), ml=4, G=3, sep=1, centre=None, n_w=1),
         dict(lags=(1, 0, -1), residual=1, score=1, own=1, runner=1)),
        # ... at u = -1 and +2: the smaller |u| before the positive one
        ("equal maxima: the smaller |u|", dict(q=_q(4, (0, -1, 1), (0, 2, 1)), ml=4, G=3, sep=1, centre=None, n_w=1),
         dict(lags=(-1, 0, 1), residual=-1, score=1, own=1, runner=1)),
        # only M_ik is not zero, at v = +2 and -2: u = 0, then the positive v
        ("equal maxima: the positive v", dict(q=_q(4, (1, 2, 1), (1, -2, 1)), ml=4, G=3, sep=1, centre=None, n_w=1),
         dict(lags=(0, 2, 2), residual=-2, score=1, own=1, runner=1)),
        ("equal maxima: the smaller |v|", dict(q=_q(4, (1, -1, 1), (1, 2, 1)), ml=4, G=3, sep=1, centre=None, n_w=1),
         dict(lags=(0, -1, -1), residual=1, score=1, own=1, runner=1)),
        # centre (0, 2, 0): c_ij = 2, c_ik = 0, c_jk = -2; pair ij's window 2 + x is clipped to the lags -1 .. 3 (x <= 1), the
        # 9 at lag -3 lies outside it; u = 1, v = 1, e = -2 + 0
        ("a centre clips a window on one side", dict(q=_q(4, (0, 3, 3), (0, -3, 9), (1, 1, 3), (2, -2, 3)), ml=4, G=3, sep=1,
                                                     centre=(0, 2, 0), n_w=1),
         dict(lags=(3, 1, -2), residual=0, score=9, own=9, runner=3)),
        ("a centre removes a window", dict(q=A, ml=4, G=3, sep=1, centre=(0, 10, 0), n_w=1), None),
        ("one cell: no runner-up", dict(q=_q(4, (0, 0, 2), (1, 0, 2), (2, 0, 1), (0, 1, 7)), ml=4, G=0, sep=1, centre=None, n_w=1),
         dict(lags=(0, 0, 0), residual=0, score=5, own=5, runner=0)),
        ("every other cell within min_separation: no runner-up", dict(q=A, ml=4, G=3, sep=6, centre=None, n_w=1),
         dict(lags=(1, -1, -2), residual=0, score=9, own=9, runner=0)),
    ]
    return cases


def _check_hand_case(rec, arg, want):
    from tdoa_amd import closure
    if want is None:
        assert rec.tobytes() == bytes(closure.CLOSURE_DTYPE.itemsize)
        return
    root = np.sqrt(np.float64(arg["n_w"]))
    assert (int(rec["lag_ij"]), int(rec["lag_ik"]), int(rec["lag_jk"])) == want["lags"]
    assert int(rec["lag_ij"]) + int(rec["lag_jk"]) == int(rec["lag_ik"])
    assert int(rec["residual"]) == want["residual"]
    assert (int(rec["score_q"]), int(rec["own_q"]), int(rec["runner_q"])) == (want["score"] * ONE, want["own"] * ONE, want["runner"] * ONE)
    assert float(rec["score"]) == want["score"] / root and float(rec["runner_up"]) == want["runner"] / root
    corr = [float(rec[n]) for n in ("corr_ij", "corr_ik", "corr_jk")]
    ml = arg["ml"]
    assert corr == [float(arg["q"][r, lag + ml - 1]) / ONE / root for r, lag in enumerate(want["lags"])]
    if "signs" in want:
        assert tuple(np.sign(corr)) == want["signs"]
    assert abs(corr[0]) + abs(corr[1]) + abs(corr[2]) == pytest.approx(float(rec["score"]), rel=1e-15)


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_worked_cases(name, arg, want):
    from tdoa_amd import closure
    rec = closure.closure(arg["q"], 3, arg["ml"], arg["G"], arg["sep"], arg["centre"], arg["n_w"])
    assert rec.shape == (1,)
    _check_hand_case(rec[0], arg, want)
    if want is not None and want["residual"] == 0:
        assert rec[0]["score_q"] == rec[0]["own_q"]


def test_model_arguments():
    from tdoa_amd import closure
    assert closure.triples(4) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)] and closure.num_triples(16) == 560
    assert [closure.pair_index(i, j, 4) for i in range(4) for j in range(i + 1, 4)] == list(range(6))
    q = np.zeros((3, 7), dtype=np.int64)
    for kw in (dict(gate=-1), dict(gate=1024), dict(min_separation=0), dict(centre=(0, 1))):
        with pytest.raises(ValueError):
            closure.closure(q, 3, 4, **{"gate": 3, **kw})
    with pytest.raises(ValueError):
        closure.closure(q[:, :6], 3, 4, 3)
    with pytest.raises(ValueError):
        closure.closure(q[:1], 2, 4, 3)


def _brute(q, S, ml, G, sep, centre):
    """every cell of every triple by enumeration -> [(best cell or None, own_q, residual, runner_q)]"""
    out = []
    inside = lambda l: -ml < l < ml
    M = lambda p, l: abs(int(q[p, l + ml - 1]))
    order = lambda x: (abs(x), x < 0)
    for i, j, k in itertools.combinations(range(S), 3):
        pid = lambda a, b: a * S - a * (a + 1) // 2 + (b - a - 1)
        c_ij, c_ik, c_jk = centre[j] - centre[i], centre[k] - centre[i], centre[k] - centre[j]
        cells = {}
        for u in range(-G, G + 1):
            for v in range(-G, G + 1):
                a, b = c_ij + u, c_ik + v
                e = b - a
                if abs(v - u) <= G and inside(a) and inside(b) and inside(e):
                    assert e == c_jk + (v - u)
                    cells[(u, v)] = M(pid(i, j), a) + M(pid(i, k), b) + M(pid(j, k), e)
        if not cells or max(cells.values()) == 0:
            out.append(None)
            continue
        top = max(cells.values())
        us, vs = min((c for c in cells if cells[c] == top), key=lambda c: order(c[0]) + order(c[1]))
        own, x_own = 0, []
        for (a, b), c in (((i, j), c_ij), ((i, k), c_ik), ((j, k), c_jk)):
            window = [x for x in range(-G, G + 1) if inside(c + x)]
            best = max(M(pid(a, b), c + x) for x in window)
            x_own.append(min((x for x in window if M(pid(a, b), c + x) == best), key=order))
            own += best
        far = [s for (u, v), s in cells.items() if max(abs(u - us), abs(v - vs)) > sep]
        out.append(((c_ij + us, c_ik + vs, c_jk + vs - us), top, own, x_own[0] + x_own[2] - x_own[1], max(far) if far else 0))
    return out


def test_model_against_every_cell_enumerated():
    """small random Q with few distinct values, so equal maxima are common; centres that move windows partly and wholly out
    of the range"""
    from tdoa_amd import closure
    rng = np.random.default_rng(17)
    zero = bytes(closure.CLOSURE_DTYPE.itemsize)
    n_zero = n_ties = n = 0
    for S, ml in itertools.product((3, 4, 5), (2, 4, 9)):
        for G in (0, 1, 3, 2 * ml):
            for centre, sep in ((None, 1), (rng.integers(-ml, ml + 1, size=S), 1), (rng.integers(-3 * ml, 3 * ml + 1, size=S), 2)):
                q = rng.integers(-2, 3, size=(S * (S - 1) // 2, 2 * ml - 1), dtype=np.int64)
                got = closure.closure(q, S, ml, G, sep, centre, n_w=2)
                want = _brute(q, S, ml, G, sep, [0] * S if centre is None else [int(x) for x in centre])
                assert len(got) == len(want) == closure.num_triples(S)
                for rec, w in zip(got, want):
                    n += 1
                    if w is None:
                        n_zero += 1
                        assert rec.tobytes() == zero
                        continue
                    lags, top, own, residual, runner = w
                    assert (int(rec["lag_ij"]), int(rec["lag_ik"]), int(rec["lag_jk"])) == lags, (S, ml, G)
                    assert (int(rec["score_q"]), int(rec["own_q"]), int(rec["residual"]), int(rec["runner_q"])) == (top, own, residual, runner)
                    assert top <= own and (residual != 0 or top == own) and runner <= top
                    n_ties += runner == top
                    assert float(rec["score"]) == float(top) / ONE / np.sqrt(2.0)
    print("%d triples: %d zero records, %d with a runner-up as large as the joint cell" % (n, n_zero, n_ties))
    assert n_zero > 10 and n_ties > 50


def noisy_windows(oracle, n_windows=12):
    """the issue's case: 3 stations with the delays (0, 5, -9), windows of 8192 samples, modulation index 1, noise 0.6;
    window w of station s = simulate_delayed_fm(8192, d[s], 100 + 50 w, 1000 (s + 1) + 50 w, 1.0, 0.6) -> [w][s] u8 IQ"""
    d = (0, 5, -9)
    return [[oracle.simulate_delayed_fm(8192, d[s], 100 + 50 * w, 1000 * (s + 1) + 50 * w, 1.0, 0.6) for s in range(3)]
            for w in range(n_windows)]


def test_the_joint_search_repairs_what_three_argmaxes_miss(oracle):
    """One window per stack, max_lag 64, G 40, twelve windows.  Measured with the float64 pipeline: the three independent
    argmaxes are (5, -9, -14) in 3 of 12 windows, the joint search in 11 of 12."""
    from tdoa_amd import closure, stacking
    ml, G, planted = 64, 40, (5, -9, -14)
    own_ok = joint_ok = 0
    for w, x in enumerate(noisy_windows(oracle)):
        sig = [oracle.b_preprocess(s)[0] for s in x]
        q = np.array([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ml)) for i, j in ((0, 1), (0, 2), (1, 2))])
        rec = closure.closure(q, 3, ml, G, 1)[0]
        own = tuple(int(l) for l in closure.independent_lags(q, 3, ml, G)[0])
        joint = (int(rec["lag_ij"]), int(rec["lag_ik"]), int(rec["lag_jk"]))
        assert int(rec["residual"]) == own[0] + own[2] - own[1] and rec["score_q"] <= rec["own_q"]
        own_ok += own == planted
        joint_ok += joint == planted
        if int(rec["residual"]) == 0 and joint == planted:
            assert rec["score_q"] == rec["own_q"]
        print("window %2d: own %s residual %d, joint %s score %.3f runner-up %.3f" % (w, own, rec["residual"], joint, rec["score"],
                                                                                      rec["runner_up"]))
    print("independent lags right in %d of 12 windows, joint lags in %d" % (own_ok, joint_ok))
    assert own_ok <= 5
    assert joint_ok >= 9
