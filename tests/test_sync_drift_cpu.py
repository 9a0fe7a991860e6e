"""CPU: the numpy statement of the clock-line search (tdoa_amd.sync_drift; include/tdoa_mi355x.h, "clock lines") on
hand-worked cases, against an independent enumeration one candidate at a time, its properties, and the noisy case the feature
exists for; and the boundary of the entry points that needs no device.  hand_cases(), check_hand_case(), random_lines() and
the noisy case's helpers are shared with tests/test_gpu_sync_drift.py, which runs the kernels on the same words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_locate_cpu import PAIRS4
from test_sync_cpu import CLOCKS, noisy_sync_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 2 ** 32
NAMES = ("tdoa_process_sync_drift", "tdoa_debug_sync_drift_from_q", "tdoa_group_process_sync_drift", "tdoa_sync_line_clock")
RATES = (0, 3, -5, 2)             # the noisy case's clock rates in quarter lags per window
NOISY = dict(ml=256, G=120, H=8, D=4, R=2, M=12, noise=0.70)


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import sync_drift
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessSyncDrift(", "C.tdoa_process_sync_drift(", "func (g *Group) ProcessSyncDrift(",
                 "C.tdoa_group_process_sync_drift(", "func SyncLineClock(", "C.tdoa_sync_line_clock("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_sync_drift", "sync_drift_from_q"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.Group, "process_sync_drift") and callable(capi.sync_line_clock)
    for name in ("sync_line", "sync_lines", "line_clock"):
        assert callable(getattr(sync_drift, name)), name
    # the record: the fields of the header in their order, 40 bytes, no padding
    assert capi.SYNC_LINE_DTYPE == sync_drift.SYNC_LINE_DTYPE and capi.SYNC_LINE_DTYPE.itemsize == 40
    assert capi.SYNC_LINE_DTYPE.names == ("moved", "terms_in", "positions", "reserved", "score_q", "start_q", "score")
    m = re.search(r"typedef struct \{([^}]*)\} tdoa_sync_line;", hdr)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+([^;]+);", m.group(1))
    assert [(t, [n.strip() for n in names.split(",")]) for t, names in fields] == [
        ("int32_t", ["moved", "terms_in", "positions", "reserved"]), ("int64_t", ["score_q", "start_q"]), ("double", ["score"])]
    # the definition is in the header in the words the tests hold the library to
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("A line is one block. Its positions are j = 0 .. L-1, the block's stacks in order (L = stacks_per_block).",
                   "N_w is the number of windows of the whole line.",
                   "Per station s: k_s = centre[s] + x_s, |x_s| <= G (0 <= G <= 1023).",
                   "Per station s: a slope h_s, |h_s| <= H (0 <= H <= 512), of h_s / D lags per position (D >= 1).",
                   "Station 0 is the gauge: x_0 = 0, h_0 = 0.",
                   "k_s(j) = k_s + shift(h_s, j), with shift(h, j) = sgn(h) * ((2|h|j + D) div (2D))",
                   "A_ij = sum over j of Q_{j,ij}[e_ij + k_j(j) - k_i(j)], the signed words summed along the line.",
                   "A term outside -max_lag < lag < max_lag adds 0 and is not counted in terms_in.",
                   "F = sum over i < j of |A_ij|.",
                   "The candidates of a station are the (h, x) pairs in the order r = rank(h) * (2G+1) + rank(x).",
                   "smaller |h|, then the positive h, then smaller |x|, then the positive x.",
                   "(x_s, h_s) is the largest sum over i < s of |A_is|, with the earlier stations where they were put.",
                   "(x_s, h_s) is the largest sum over i != s of |A_pair(i,s)|",
                   "start_q is F after placing, and score_q is F at the end, so score_q >= start_q.",
                   "moved counts the stations whose (k, h) the last sweep changed.",
                   "If F = 0 at the end, every output of the line is zero.",
                   "P * N_w > 2^17 returns TDOA_ERR_UNSUPPORTED.",
                   "precondition is |q| <= 2^62 div (P * L).",
                   "16 * k_s + r(16 * h_s * j, D)"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handle_and_the_host_helper_need_no_device(capi):
    from tdoa_amd import sync_drift
    lib = capi.load()
    rec = np.zeros(3, dtype=capi.SYNC_LINE_DTYPE)
    q = np.zeros(3 * 7, dtype=np.int64)
    ref = (C.c_int32 * 3)(0, 16, 32)
    pr, pq = rec.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_int64))
    for m, G, H, D, R in ((0, 1, 1, 1, 1), (2, 0, 0, 1, 0), (-1, 1, 1, 1, 1), (0, -1, 0, 1, 0), (0, 1024, 0, 1, 0), (0, 1, 513, 1, 0),
                          (0, 1, -1, 1, 0), (0, 1, 1, 0, 0), (0, 1, 1, 1, 17)):
        assert lib.tdoa_process_sync_drift(None, m, G, H, D, R, ref, None, pr, None, None, None, None, None) == 1
        assert lib.tdoa_group_process_sync_drift(None, m, G, H, D, R, ref, None, pr, None, None, None, None, None) == 1
        assert lib.tdoa_debug_sync_drift_from_q(None, pq, 1, 1, 3, 1, G, H, D, R, ref, None, pr, None, None, None, None, None) == 1
    # the helper: position 0 is 16 k; r rounds halves away from zero; the model's values
    assert capi.sync_line_clock((0, 37, -52, 18), RATES, 4, 0, 1).tolist() == [[0, 592, -832, 288]]
    assert capi.sync_line_clock((0, 1, -1), (0, 1, -1), 32, 1, 3).tolist() == [[0, 17, -17], [0, 17, -17], [0, 18, -18]]      # 0.5, 1, 1.5
    rng = np.random.default_rng(5)
    for D in (1, 3, 4, 7, 32):
        k, h = rng.integers(-300, 301, size=5), rng.integers(-20, 21, size=5)
        got = capi.sync_line_clock(k, h, D, 9, 40)
        assert got.dtype == np.int32 and got.tobytes() == sync_drift.line_clock(k, h, D, 9, 40).tobytes()
        exact = [[16 * int(k[s]) + 16 * int(h[s]) * j / D for s in range(5)] for j in range(9, 49)]
        assert np.abs(got - np.array(exact)).max() <= 0.5
    i32 = C.POINTER(C.c_int32)
    out = np.zeros(3, dtype=np.int32)
    for args in ((None, ref, 3, 1, 0, 1, out.ctypes.data_as(i32)), (ref, None, 3, 1, 0, 1, out.ctypes.data_as(i32)),
                 (ref, ref, 3, 1, 0, 1, None), (ref, ref, 0, 1, 0, 1, out.ctypes.data_as(i32)),
                 (ref, ref, 3, 0, 0, 1, out.ctypes.data_as(i32)), (ref, ref, 3, 1, -1, 1, out.ctypes.data_as(i32)),
                 (ref, ref, 3, 1, 0, 0, out.ctypes.data_as(i32))):
        assert lib.tdoa_sync_line_clock(*args) == 1


# ---- hand-worked cases: position j, pairs i < j in the library's order, lag l at index l + max_lag - 1 ---------------------
def _pair(i, j, S):
    return i * S - i * (i + 1) // 2 + (j - i - 1)


def _q(S, ml, L, *peaks):
    """[L][P] rows of 2 ml - 1 zeros with (position, i, j, lag, value in units of 2^32) set"""
    q = np.zeros((L, S * (S - 1) // 2, 2 * ml - 1), dtype=np.int64)
    for pos, i, j, lag, value in peaks:
        q[pos, _pair(i, j, S), lag + ml - 1] = value * ONE
    return q


def hand_cases():
    """[(name, dict(q, ml, ref, centre, G, H, D, R, n_w), expected or None for all zeros)]; expected: clock, rate, lags [L][P]
    (0 for a term outside), inside [L][P], moved, terms_in, and score and start in units of 2^32"""
    return [
        # lags (x, x + h).  (h, x) = (0, +1) reads 3 + 4 and so does (+1, 0); every other candidate reads 3 or nothing.  r = 1
        # and r = 3: the smaller |h| wins although its |x| is the larger
        ("equal maxima: |h| before x",
         dict(q=_q(2, 6, 2, (0, 0, 1, 0, 3), (0, 0, 1, 1, 3), (1, 0, 1, 1, 4)), ml=6, ref=(0, 0), centre=None, G=1, H=1, D=1, R=0, n_w=1),
         dict(clock=(0, 1), rate=(0, 0), lags=((1,), (1,)), inside=((1,), (1,)), moved=0, terms_in=2, score=7, start=7)),
        # lags (0, h): h = +1 sums -1 - 5, h = -1 sums -1 + 7 -- signed words, equal magnitudes 6, and h = 0 reads the -1 alone
        ("equal maxima: the positive h",
         dict(q=_q(2, 4, 2, (0, 0, 1, 0, -1), (1, 0, 1, 1, -5), (1, 0, 1, -1, 7)), ml=4, ref=(0, 0), centre=None, G=0, H=1, D=1, R=1, n_w=1),
         dict(clock=(0, 0), rate=(0, 1), lags=((0,), (1,)), inside=((1,), (1,)), moved=0, terms_in=2, score=6, start=6)),
        # one position: every slope is the same line, so h = 0; x = -1 (rank 2) before x = +2 (rank 3)
        ("equal maxima: the smaller |x|; one position has no slope",
         dict(q=_q(2, 4, 1, (0, 0, 1, 2, 5), (0, 0, 1, -1, -5)), ml=4, ref=(0, 0), centre=None, G=2, H=3, D=1, R=1, n_w=4),
         dict(clock=(0, -1), rate=(0, 0), lags=((-1,),), inside=((1,),), moved=0, terms_in=1, score=5, start=5)),
        # k_1 = 2, lags 2 + h j in |l| < 3.  h = 0 sums 4 - 4 - 1, h = -1 reads the 4 alone, and so does h = +1, whose positions 1
        # and 2 are at lags 3 and 4, outside: the positive one of the two wins, and one term is counted
        ("terms outside the range add 0 and are not counted",
         dict(q=_q(2, 3, 3, (0, 0, 1, 2, 4), (1, 0, 1, 2, -4), (2, 0, 1, 2, -1)), ml=3, ref=(0, 0), centre=(0, 2), G=0, H=1, D=1, R=0, n_w=1),
         dict(clock=(0, 2), rate=(0, 1), lags=((2,), (0,), (0,)), inside=((1,), (0,), (0,)), moved=0, terms_in=1, score=4, start=4)),
        # e = (1, 1, 0) from delays (0, 16, 23); D = 2: shift(+-1, 1) = +-1, the half away from zero.  Station 1: window 4 +- 1,
        # pair 01 has 2 at lag 6 of position 0 and 3 at lag 7 of position 1: x = +1, h = +1 (5).  Station 2: window -2 +- 1, pair
        # 02 has 7 at lag -1 of position 0 and 1 at lag -2 of position 1, pair 12 has -1 at lag -7 of position 0: x = 0 with
        # h = -1 reads 8 + 1 (its pair 12 at position 1 is at lag -9, outside), h = 0 reads 7 + 1.  The sweep moves nothing
        ("three stations: the centres move the windows, e from the delays, halves in shift",
         dict(q=_q(3, 8, 2, (0, 0, 1, 6, 2), (1, 0, 1, 7, 3), (0, 0, 2, -1, 7), (1, 0, 2, -2, 1), (0, 1, 2, -7, -1)), ml=8,
              ref=(0, 16, 23), centre=(0, 4, -2), G=1, H=1, D=2, R=1, n_w=2),
         dict(clock=(0, 5, -2), rate=(0, 1, -1), lags=((6, -1, -7), (7, -2, 0)), inside=((1, 1, 1), (1, 1, 0)), moved=0, terms_in=5,
              score=14, start=14)),
        # placing puts station 1 at h = 0 on pair 01's 4 + 4 (8 against 4); station 2 at h = +1 on pair 02's 6 + 6 and the 5 of
        # pair 12's position 0 (17; h = 0 reads 6 + 10): F = 8 + 12 + 5.  The sweep moves station 1 to h = +1: pair 01 keeps the 4
        # of position 0, and pair 12 now reads its 5 + 5 at lag 0 (14 against 13); station 2 stays (22 against 11)
        ("a sweep moves a station's slope",
         dict(q=_q(3, 5, 2, (0, 0, 1, 0, 4), (1, 0, 1, 0, 4), (0, 0, 2, 0, 6), (1, 0, 2, 1, 6), (0, 1, 2, 0, 5), (1, 1, 2, 0, 5)), ml=5,
              ref=(0, 0, 0), centre=None, G=0, H=1, D=1, R=1, n_w=1),
         dict(clock=(0, 0, 0), rate=(0, 1, 1), lags=((0, 0, 0), (1, 1, 0)), inside=((1,) * 3,) * 2, moved=1, terms_in=6, score=26, start=25)),
        ("all zeros", dict(q=_q(3, 5, 3), ml=5, ref=(0, 16, 32), centre=(0, 1, -1), G=2, H=2, D=3, R=1, n_w=1), None),
    ]


def check_hand_case(got, arg, want):
    """got: (record, clock [S], rate [S], rows [L][S], lags [L][P], corr [L][P])"""
    from tdoa_amd import sync_drift
    rec, clock, rate, rows, lags, corr = got
    q, ml, D = arg["q"], arg["ml"], arg["D"]
    L, P, S = q.shape[0], q.shape[1], len(arg["ref"])
    assert clock.dtype == rate.dtype == rows.dtype == lags.dtype == np.int32 and corr.dtype == np.float64
    assert clock.shape == rate.shape == (S,) and rows.shape == (L, S) and lags.shape == corr.shape == (L, P)
    if want is None:
        assert rec.tobytes() == bytes(sync_drift.SYNC_LINE_DTYPE.itemsize)
        assert not clock.any() and not rate.any() and not rows.any() and not lags.any() and corr.tobytes() == bytes(corr.nbytes)
        return
    assert clock.tolist() == list(want["clock"]) and rate.tolist() == list(want["rate"])
    assert lags.tolist() == [list(r) for r in want["lags"]]
    assert (int(rec["moved"]), int(rec["terms_in"]), int(rec["positions"]), int(rec["reserved"])) == (want["moved"], want["terms_in"], L, 0)
    assert (int(rec["score_q"]), int(rec["start_q"])) == (want["score"] * ONE, want["start"] * ONE)
    assert float(rec["score"]) == want["score"] / np.sqrt(np.float64(L * arg["n_w"]))
    for j in range(L):
        for s in range(S):
            h, k = want["rate"][s], want["clock"][s]
            assert rows[j, s] == 16 * (k + (1 if h > 0 else -1) * ((2 * abs(h) * j + D) // (2 * D)))
        assert corr[j].tolist() == [float(q[j, p, lag + ml - 1]) / ONE / np.sqrt(np.float64(arg["n_w"])) if inside else 0.0
                                    for p, (lag, inside) in enumerate(zip(want["lags"][j], want["inside"][j]))]


def run_model(arg):
    from tdoa_amd import sync_drift
    return sync_drift.sync_line(arg["q"], arg["ref"], arg["ml"], arg["G"], arg["H"], arg["D"], arg["R"], arg["centre"], arg["n_w"])


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_worked_cases(name, arg, want):
    check_hand_case(run_model(arg), arg, want)


def test_model_arguments():
    from tdoa_amd import sync_drift
    assert sync_drift.shift(np.array([0, 1, -1, 3, -3, 5]), 3, 4).tolist() == [0, 1, -1, 2, -2, 4]      # 0.75, 2.25, 3.75
    assert sync_drift.shift(1, np.arange(4), 2).tolist() == [0, 1, 1, 2]                                  # halves away from zero
    q = np.zeros((2, 3, 7), dtype=np.int64)
    good = dict(q=q, ref_delay=(0, 0, 0), max_lag=4, gate=1, max_drift=1, drift_den=1, rounds=1)
    for kw in (dict(gate=-1), dict(gate=1024), dict(rounds=-1), dict(rounds=17), dict(max_drift=-1), dict(max_drift=513),
               dict(drift_den=0), dict(ref_delay=(0,)), dict(ref_delay=(0, 0)), dict(q=q[:, :, :6]), dict(q=q[0]), dict(centre=(0, 0))):
        with pytest.raises(ValueError):
            sync_drift.sync_line(**{**good, **kw})
    with pytest.raises(ValueError):
        sync_drift.sync_lines(np.zeros((3, 3, 7), dtype=np.int64), 2, (0, 0, 0), 4)
    for kw in (dict(drift_den=0), dict(first_position=-1), dict(n_positions=0), dict(rate=(0, 0))):
        with pytest.raises(ValueError):
            sync_drift.line_clock(**{**dict(clock=(0, 1, 2), rate=(0, 1, 2), drift_den=1, first_position=0, n_positions=1), **kw})


# ---- an independent statement: plain integers, one candidate at a time ------------------------------------------------------
def _enumerate(q, ref, ml, G, H, D, R, centre):
    """-> (k, h, start F, final F, terms inside, lags [L][P] (None outside), moved, F after every sweep, the kinds of tie seen:
    "h" two slopes of different |h|, "sign_h" +h and -h, "x" two offsets of different |x|, "sign_x" +x and -x)"""
    L, S = len(q), len(ref)
    rank = lambda v: 2 * abs(v) - (v > 0)
    cands = sorted(((h, x) for h in range(-H, H + 1) for x in range(-G, G + 1)), key=lambda c: (rank(c[0]), rank(c[1])))
    ties = set()

    def shift(h, j):
        a = (2 * abs(h) * j + D) // (2 * D)
        return -a if h < 0 else a

    def e(i, j):
        d = int(ref[j]) - int(ref[i])
        a = (2 * abs(d) + 16) // 32
        return -a if d < 0 else a

    def a_pair(i, j, ki, hi, kj, hj):
        """(A_ij, its terms inside, the lags) with station i on (ki, hi) and j on (kj, hj)"""
        total, inside, lags = 0, 0, []
        for pos in range(L):
            lag = e(i, j) + (kj + shift(hj, pos)) - (ki + shift(hi, pos))
            if -ml < lag < ml:
                total += int(q[pos][_pair(i, j, S)][lag + ml - 1])
                inside += 1
                lags.append(lag)
            else:
                lags.append(None)
        return total, inside, lags

    def place(s, partners):
        values = []
        for hc, x in cands:
            ks = centre[s] + x
            values.append(sum(abs(a_pair(i, s, k[i], h[i], ks, hc)[0]) if i < s else abs(a_pair(s, i, ks, hc, k[i], h[i])[0])
                              for i in partners))
        top = max(values)
        first = values.index(top)
        for r, v in enumerate(values):
            if v == top and r != first:
                (h0, x0), (h1, x1) = cands[first], cands[r]
                ties.add("h" if abs(h0) != abs(h1) else "sign_h" if h0 != h1 else "x" if abs(x0) != abs(x1) else "sign_x")
        return centre[s] + cands[first][1], cands[first][0]

    def objective():
        total, inside, lags = 0, 0, [[None] * (S * (S - 1) // 2) for _ in range(L)]
        for i in range(S):
            for j in range(i + 1, S):
                a, n, ls = a_pair(i, j, k[i], h[i], k[j], h[j])
                total += abs(a)
                inside += n
                for pos in range(L):
                    lags[pos][_pair(i, j, S)] = ls[pos]
        return total, inside, lags

    k, h = [int(c) for c in centre], [0] * S
    for s in range(1, S):
        k[s], h[s] = place(s, range(s))
    start = objective()[0]
    moved, per_sweep = 0, []
    for _ in range(R):
        moved = 0
        for s in range(1, S):
            new = place(s, [i for i in range(S) if i != s])
            moved += new != (k[s], h[s])
            k[s], h[s] = new
        per_sweep.append(objective()[0])
    final, inside, lags = objective()
    return k, h, start, final, inside, lags, moved, per_sweep, ties


def test_model_against_the_candidates_enumerated():
    """small random Q with few distinct values, so equal maxima are common; delays and centres that put terms outside"""
    from tdoa_amd import sync_drift
    rng = np.random.default_rng(41)
    n = n_zero = n_out = n_moved = n_sloped = 0
    kinds = {"h": 0, "sign_h": 0, "x": 0, "sign_x": 0}
    for S, ml in ((2, 3), (2, 6), (3, 4), (3, 7), (4, 5), (4, 8)):
        P = S * (S - 1) // 2
        for G in (0, 1, 2, 3):
            for H in (0, 1, 2):
                for D, L, R in ((1, 1, 0), (1, 2, 1), (3, 3, 2), (1, 4, 3), (3, 4, 1), (3, 2, 3)):
                    span = 8 if rng.random() < 0.5 else 16 * ml
                    q = rng.integers(-2, 3, size=(L, P, 2 * ml - 1), dtype=np.int64) * (rng.random() < 0.9)
                    q *= rng.random(q.shape) < 0.6
                    ref = rng.integers(-span, span + 1, size=S, dtype=np.int32)
                    centre = rng.integers(-ml // 2, ml // 2 + 1, size=S, dtype=np.int32) if rng.random() < 0.7 else None
                    rec, clock, rate, rows, lags, corr = sync_drift.sync_line(q, ref, ml, G, H, D, R, centre, n_w=2)
                    k, h, start, final, inside, want_lags, moved, per_sweep, ties = _enumerate(
                        q.tolist(), ref, ml, G, H, D, R, [0] * S if centre is None else centre.tolist())
                    n += 1
                    for kind in ties:
                        kinds[kind] += 1
                    assert all(b >= a for a, b in zip([start] + per_sweep, per_sweep))            # F never falls over a sweep
                    if final == 0:
                        n_zero += 1
                        assert rec.tobytes() == bytes(40) and not (clock.any() or rate.any() or rows.any() or lags.any() or corr.any())
                        continue
                    assert clock.tolist() == k and rate.tolist() == h
                    assert (int(rec["start_q"]), int(rec["score_q"])) == (start, final) and final >= start
                    assert (int(rec["moved"]), int(rec["terms_in"]), int(rec["positions"])) == (moved, inside, L)
                    assert lags.tolist() == [[l or 0 for l in row] for row in want_lags]
                    assert corr.tolist() == [[0.0 if l is None else float(q[j][p][l + ml - 1]) / ONE / np.sqrt(2.0) for p, l in enumerate(row)]
                                             for j, row in enumerate(want_lags)]
                    assert float(rec["score"]) == float(final) / ONE / np.sqrt(2.0 * L)
                    if L == 1:
                        assert not rate.any()
                    n_out += inside < L * P
                    n_moved += moved > 0
                    n_sloped += bool(rate.any())
    print("%d searches: %d all zero, %d with terms outside, %d whose last sweep moved a station, %d with a slope; equal maxima "
          "between |h| in %d, +-h in %d, |x| in %d, +-x in %d" % (n, n_zero, n_out, n_moved, n_sloped, kinds["h"], kinds["sign_h"],
                                                                  kinds["x"], kinds["sign_x"]))
    assert n_zero >= 2 and n_out >= 5 and n_moved >= 2 and n_sloped >= 20 and min(kinds.values()) >= 5     # each kind of case occurs


def random_lines(rng, S, ml, n_lines, L, span=None, zero_line=None, ref_span=None):
    """few-valued words [n_lines L][P][2 ml - 1], delays [S] and centres [S] that put some windows partly or wholly outside;
    zero_line: a line of zeros"""
    P = S * (S - 1) // 2
    q = rng.integers(-3, 4, size=(n_lines * L, P, 2 * ml - 1), dtype=np.int64) * ONE
    q *= rng.random(q.shape) < 0.5
    if zero_line is not None:
        q[zero_line * L:(zero_line + 1) * L] = 0
    r = 16 * ml if ref_span is None else ref_span
    ref = rng.integers(-r, r + 1, size=S, dtype=np.int32)
    c = ml + 6 if span is None else span
    centre = rng.integers(-c, c + 1, size=S, dtype=np.int32)
    return q, ref, centre


def test_properties_of_the_search():
    """score_q >= start_q and F never falls from one more sweep; one position has no slope; H = 0 on L one-window positions is
    H = 0 on the one summed stack; line_clock agrees with the rows wherever 16 h j / D is whole"""
    from tdoa_amd import sync_drift
    rng = np.random.default_rng(43)
    n_whole = 0
    for S, ml, G, H, D, L in ((2, 12, 4, 2, 1, 3), (3, 16, 5, 3, 4, 5), (4, 16, 3, 2, 2, 4), (5, 10, 2, 1, 3, 6)):
        for trial in range(4):
            q, ref, centre = random_lines(rng, S, ml, 1, L, span=2, ref_span=48)
            last = None
            for R in range(4):
                rec, clock, rate, rows, lags, corr = sync_drift.sync_line(q, ref, ml, G, H, D, R, centre)
                assert rec["score_q"] >= rec["start_q"] > 0
                assert last is None or (rec["score_q"] >= last["score_q"] and rec["start_q"] == last["start_q"])
                last = rec
            assert rows[0].tolist() == (16 * clock).tolist()
            cont = sync_drift.line_clock(clock, rate, D, 0, L)
            assert cont[0].tolist() == (16 * clock).tolist()
            for j in range(L):
                for s in range(S):
                    if (16 * int(rate[s]) * j) % D == 0:
                        n_whole += 1
                        assert cont[j, s] == 16 * int(clock[s]) + 16 * int(rate[s]) * j // D
                        if (int(rate[s]) * j) % D == 0:
                            assert cont[j, s] == rows[j, s]
            one = sync_drift.sync_line(q[:1], ref, ml, G, H, D, 2, centre)
            assert not one[2].any() and one[0]["positions"] == 1
            flat = sync_drift.sync_line(q, ref, ml, G, 0, D, 2, centre)
            summed = sync_drift.sync_line(q.sum(axis=0)[None], ref, ml, G, 0, D, 2, centre, n_w=L)
            assert flat[1].tolist() == summed[1].tolist() and flat[0]["score_q"] == summed[0]["score_q"]
            assert flat[0]["score"] == summed[0]["score"] and not flat[2].any()
    assert n_whole >= 100
    lines = sync_drift.sync_lines(np.concatenate([q, q[::-1]]), L, ref, ml, G, H, D, 1, centre)
    both = [sync_drift.sync_line(x, ref, ml, G, H, D, 1, centre) for x in (q, q[::-1])]
    for i in range(3):
        assert lines[i].tobytes() == np.stack([b[i] for b in both]).tobytes()
    for i in range(3, 6):
        assert lines[i].tobytes() == np.concatenate([b[i] for b in both]).tobytes()


# ---- the noisy case --------------------------------------------------------------------------------------------------------
def shift1(h, j, D):
    a = (2 * abs(h) * j + D) // (2 * D)
    return -a if h < 0 else a


def noisy_drift_windows(oracle, d, block, first, seed, noise=NOISY["noise"], M=NOISY["M"], D=NOISY["D"]):
    """[w][s] u8 IQ windows of 8192 of block `block`: station s starts d[s] + CLOCKS[s] + shift(RATES[s], first + w) samples
    late -- the clocks slide by RATES quarter lags per window; seed 300 for a reference block, 700 for a target block"""
    return [[oracle.simulate_delayed_fm(8192, d[s] + CLOCKS[s] + shift1(RATES[s], first + w, D) + 100, seed + 50 * block + w,
                                        seed + 1000 + 1000 * s + 50 * block + w, 1.0, noise) for s in range(4)] for w in range(M)]


def oracle_words(oracle, wins, ml):
    from tdoa_amd import stacking
    out = []
    for x in wins:
        sig = [oracle.b_preprocess(s)[0] for s in x]
        out.append([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ml)) for i, j in PAIRS4])
    return np.array(out)


def true_clocks(first, M=NOISY["M"], D=NOISY["D"]):
    return [[CLOCKS[s] + shift1(RATES[s], first + w, D) for s in range(4)] for w in range(M)]


def test_the_line_finds_sliding_clocks_where_the_clock_search_cannot(oracle):
    """Twelve one-window positions of 8 192 per block, max_lag 256, G 120, H 8, D 4, R 2, noise 0.70, clocks (0, 37, -52, 18)
    sliding by (0, 3, -5, 2) quarter lags per window.  Measured with the float64 pipeline: the line has all offsets and rates
    exact in 12 of 12 blocks; the clock search on one-window stacks has all clocks of a window right in 1 of 36 windows (blocks
    0 .. 2), on the whole-block stack the clocks at the first window in 0 of 12 blocks; the J = 0 cell track of the target block
    under the line continued over positions 12 .. 23 (line_clock) is on the planted cell in 5 of 6 blocks, under the whole-block
    clocks in 0 of 6."""
    from tdoa_amd import locate_track, sync, sync_drift
    ml, G, H, D, R, M = (NOISY[k] for k in ("ml", "G", "H", "D", "R", "M"))
    table, ref_delay, d_ref, planted_cell, d_tgt = noisy_sync_case()
    line_ok = whole_ok = per_ok = track_line = track_whole = 0
    for b in range(12):
        q = oracle_words(oracle, noisy_drift_windows(oracle, d_ref, b, 0, 300), ml)
        rec, clock, rate, rows, lags, corr = sync_drift.sync_line(q, ref_delay, ml, G, H, D, R)
        assert rec["score_q"] >= rec["start_q"] > 0 and rec["terms_in"] == 6 * M and rec["positions"] == M
        exact = clock.tolist() == list(CLOCKS) and rate.tolist() == list(RATES)
        assert not exact or rows.tolist() == (16 * np.array(true_clocks(0))).tolist()
        whole = sync.sync(q.sum(axis=0), ref_delay, ml, G, R, None, M)[1]
        line_ok += exact
        whole_ok += whole.tolist() == list(CLOCKS)
        print("block %2d: clock %s rate %s moved %d score %.3f; whole-block clock search %s" % (b, clock.tolist(), rate.tolist(), rec["moved"],
                                                                                            rec["score"], whole.tolist()))
        if b < 3:
            per = sync.sync_stacks(q, ref_delay, ml, G, R)[1]
            per_ok += sum(per[w].tolist() == true_clocks(0)[w] for w in range(M))
        if b < 6:
            qt = oracle_words(oracle, noisy_drift_windows(oracle, d_tgt, b, M, 700), ml)
            cont = sync_drift.line_clock(clock, rate, D, M, M)
            track_line += int(locate_track.track_stacks(qt, table, 64, ml, M, 0, 1, 1, cont)[0]["cell"][0] == planted_cell)
            flat = np.tile(16 * whole.astype(np.int32), (M, 1))
            track_whole += int(locate_track.track_stacks(qt, table, 64, ml, M, 0, 1, 1, flat)[0]["cell"][0] == planted_cell)
    print("offsets and rates exact in %d of 12 blocks; the clock search right in %d of 36 one-window stacks and at %d of 12 whole-block "
          "stacks; the target block's track on the planted cell in %d of 6 with the line's clocks, %d with the whole block's"
          % (line_ok, per_ok, whole_ok, track_line, track_whole))
    assert line_ok >= 10
    assert per_ok <= 6
    assert whole_ok <= 1
    assert track_line >= 5
    assert track_whole <= 1
