"""CPU: the numpy statement of the clock search (tdoa_amd.sync; include/tdoa_mi355x.h, "clock search") on hand-worked cases,
against an independent enumeration of the three phases, and on the noisy case the feature exists for; the delay-table
search's model with station clocks; and the boundary of the entry points that needs no device.  hand_cases(),
noisy_sync_case() and noisy_sync_windows() are shared with tests/test_gpu_sync.py, which runs the kernels on the same
words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_locate_cpu import FS, GRID, PAIRS4, ST4, _brute, noisy_case, own_lags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 2 ** 32
NAMES = ("tdoa_process_sync", "tdoa_debug_sync_from_q", "tdoa_group_process_sync", "tdoa_locate_set_clock",
         "tdoa_group_locate_set_clock")
CLOCKS = (0, 37, -52, 18)         # the noisy case's station clocks in samples


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import sync
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessSync(", "C.tdoa_process_sync(", "func (g *gpuCorrelator) LocateSetClock(",
                 "C.tdoa_locate_set_clock(", "func (g *Group) ProcessSync(", "C.tdoa_group_process_sync(",
                 "func (g *Group) LocateSetClock(", "C.tdoa_group_locate_set_clock("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_sync", "sync_from_q", "locate_set_clock"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.Group, "process_sync") and hasattr(capi.Group, "locate_set_clock")
    for name in ("sync", "sync_stacks", "midpoint_clock"):
        assert callable(getattr(sync, name)), name
    # the record: the fields of the header in their order, 32 bytes, no padding
    assert capi.SYNC_DTYPE == sync.SYNC_DTYPE and capi.SYNC_DTYPE.itemsize == 32
    assert capi.SYNC_DTYPE.names == ("moved", "pairs_in", "score_q", "start_q", "score")
    m = re.search(r"typedef struct \{([^}]*)\} tdoa_sync;", hdr)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+([^;]+);", m.group(1))
    assert [(t, [n.strip() for n in names.split(",")]) for t, names in fields] == [
        ("int32_t", ["moved", "pairs_in"]), ("int64_t", ["score_q", "start_q"]), ("double", ["score"])]
    # the definition is in the header in the words the tests hold the library to
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("e_ij = sgn(d) * ((2|d| + 16) div 32) with d = ref_delay[j] - ref_delay[i], taken in 64 bits",
                   "k_s = centre[s] + x_s with |x_s| <= G, in samples. x_0 = 0: station 0 is the gauge.",
                   "F(k) = sum over i < j of M_ij[e_ij + k_j - k_i].",
                   "adds 0 to F and is not counted in pairs_in.",
                   "rank(x) = 2|x| - (x > 0)",
                   "Among equal maxima the smaller rank(x_1) wins, then the smaller rank(x_2).",
                   "x_s is the largest sum over i < s of M_is[e_is + (centre[s] + x) - k_i].",
                   "e_si + k_i - (centre[s] + x) for a partner i > s.",
                   "If F at the final k is 0, the record, the clocks, the lags and the correlations are all zero.",
                   "d = (t[c][j] - t[c][i]) + (clock[sid][j] - clock[sid][i]), taken in 64 bits",
                   "Without a clock table, and with an all-zero one, every output is byte-identical."):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handle_is_invalid_without_a_device(capi):
    lib = capi.load()
    rec = np.zeros(4, dtype=capi.SYNC_DTYPE)
    q = np.zeros(3 * 7, dtype=np.int64)
    ref = (C.c_int32 * 3)(0, 16, 32)
    clock = (C.c_int32 * 6)(0, 16, 32, 0, 0, 0)
    pr, pq = rec.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_int64))
    for args in ((clock, 2, 3), (None, 0, 0), (clock, -1, 3), (clock, 2, 1), (clock, 2, 65)):
        assert lib.tdoa_locate_set_clock(None, *args) == 1
        assert lib.tdoa_group_locate_set_clock(None, *args) == 1
    for m, gate, rounds in ((0, 1, 1), (2, 0, 0), (-1, 1, 1), (0, -1, 0), (0, 1024, 0), (0, 1, 17)):
        assert lib.tdoa_process_sync(None, m, gate, rounds, ref, None, pr, None, None, None) == 1
        assert lib.tdoa_group_process_sync(None, m, gate, rounds, ref, None, pr, None, None, None) == 1
        assert lib.tdoa_debug_sync_from_q(None, pq, 1, 3, 1, gate, rounds, ref, None, pr, None, None, None) == 1
    assert lib.tdoa_process_sync(None, 0, 1, 1, None, None, None, None, None, None) == 1
    assert lib.tdoa_debug_sync_from_q(None, None, 0, 1, 0, 1, 1, None, None, None, None, None, None) == 1


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
    """[(name, dict(q, ml, ref, centre, G, R, n_w), expected or None for all zeros)]; expected: clock, lags (0 for a pair
    outside), inside, moved, pairs_in, and score and start in units of 2^32"""
    # four stations.  The start sees pairs 01, 02, 12 only: x_1 = x_2 = 0 (4 + 4).  Station 3 is placed at x = 1 (the 6 of
    # pair 03; x = 2 would get the 5 of M_13[2], x = 0 the 5 of M_13[0]): F = 14.  Sweep, station 1: x = +1 gets M_13[0] = 5,
    # x = -1 gets M_13[2] = 5, x = 0 gets M_01[0] = 4 -- equal maxima, the positive one wins, F = 15.  Stations 2 and 3 stay.
    q4 = _q(4, 6, (0, 1, 0, 4), (0, 2, 0, 4), (0, 3, 1, 6), (1, 3, 2, 5), (1, 3, 0, 5))
    four = dict(q=q4, ml=6, ref=(0, 0, 0, 0), centre=None, G=2, n_w=1)
    return [
        # M_01 is 3 at both +-1, M_02 is 5 at both +-2, M_12 nothing: four cells score 8, (+1, +2) comes first in rank order
        ("equal maxima at the start: the positive x in both coordinates",
         dict(q=_q(3, 4, (0, 1, 1, 3), (0, 1, -1, -3), (0, 2, 2, 5), (0, 2, -2, 5)), ml=4, ref=(0, 0, 0), centre=None, G=2, R=0, n_w=1),
         dict(clock=(0, 1, 2), lags=(1, 2, 1), inside=(1, 1, 1), moved=0, pairs_in=3, score=8, start=8)),
        # ... and the smaller |x_1| before the larger: M_01 is 3 at 0 and at +1 as well
        ("equal maxima at the start: the smaller |x| first",
         dict(q=_q(3, 4, (0, 1, 1, 3), (0, 1, 0, 3), (0, 2, 2, 5), (0, 2, -1, 5)), ml=4, ref=(0, 0, 0), centre=None, G=2, R=1, n_w=4),
         dict(clock=(0, 0, -1), lags=(0, -1, -1), inside=(1, 1, 1), moved=0, pairs_in=3, score=8, start=8)),
        ("equal maxima in a sweep: the positive x", dict(R=1, **four),
         dict(clock=(0, 1, 0, 1), lags=(1, 0, 1, -1, 0, 1), inside=(1,) * 6, moved=1, pairs_in=6, score=15, start=14)),
        ("the second sweep moves nothing", dict(R=2, **four),
         dict(clock=(0, 1, 0, 1), lags=(1, 0, 1, -1, 0, 1), inside=(1,) * 6, moved=0, pairs_in=6, score=15, start=14)),
        ("no sweep: moved 0 and the score of the start", dict(R=0, **four),
         dict(clock=(0, 0, 0, 1), lags=(0, 0, 1, 0, 1, 1), inside=(1,) * 6, moved=0, pairs_in=6, score=14, start=14)),
        # e_02 = e_12 = 5: with |x| <= 1 pair 02's lag is 4 .. 6, outside |l| < 4, and pair 12's 5 + x_2 - x_1 is 3 .. 7: the 9s
        # at lags 3 and 2 are out of reach, x_2 = 0 is the first of equal candidates and puts pair 12 at lag 4, outside too
        ("lags outside the range add 0 and are not counted",
         dict(q=_q(3, 4, (0, 1, 1, 3), (0, 2, 3, 9), (1, 2, 2, 9)), ml=4, ref=(0, 0, 80), centre=None, G=1, R=1, n_w=1),
         dict(clock=(0, 1, 0), lags=(1, 0, 0), inside=(1, 0, 0), moved=0, pairs_in=1, score=3, start=3)),
        # e = (1, 1, 0) from delays (0, 16, 23): 23 / 16 rounds to 1, 7 / 16 to 0.  The windows are 4 +- 1 and -2 +- 1
        ("the centres move the windows; e from the delays",
         dict(q=_q(3, 8, (0, 1, 6, 2), (0, 1, 1, 9), (0, 2, -1, 7), (0, 2, 1, 9), (1, 2, -7, -1)), ml=8, ref=(0, 16, 23),
              centre=(0, 4, -2), G=1, R=2, n_w=2),
         dict(clock=(0, 5, -2), lags=(6, -1, -7), inside=(1, 1, 1), moved=0, pairs_in=3, score=10, start=10)),
        ("all zeros", dict(q=_q(4, 5), ml=5, ref=(0, 16, 32, 48), centre=(0, 1, -1, 2), G=2, R=1, n_w=1), None),
        # e_01 = -1; M_01 is 5 at lags +2 and -3, x = +3 and -2: the smaller |x| wins
        ("two stations", dict(q=_q(2, 4, (0, 1, 2, 5), (0, 1, -3, -5)), ml=4, ref=(0, -16), centre=None, G=3, R=1, n_w=1),
         dict(clock=(0, -2), lags=(-3,), inside=(1,), moved=0, pairs_in=1, score=5, start=5)),
    ]


def _check_hand_case(got, arg, want):
    """got: (record, clock [S], lags [P], corr [P])"""
    from tdoa_amd import sync
    rec, clock, lags, corr = got
    assert clock.dtype == np.int32 and lags.dtype == np.int32 and corr.dtype == np.float64
    assert clock.shape == (len(arg["ref"]),) and lags.shape == corr.shape == (len(arg["q"]),)
    if want is None:
        assert rec.tobytes() == bytes(sync.SYNC_DTYPE.itemsize)
        assert not clock.any() and not lags.any() and corr.tobytes() == bytes(corr.nbytes)
        return
    root = np.sqrt(np.float64(arg["n_w"]))
    assert clock.tolist() == list(want["clock"]) and lags.tolist() == list(want["lags"])
    assert (int(rec["moved"]), int(rec["pairs_in"])) == (want["moved"], want["pairs_in"])
    assert (int(rec["score_q"]), int(rec["start_q"])) == (want["score"] * ONE, want["start"] * ONE)
    assert float(rec["score"]) == want["score"] / root
    ml = arg["ml"]
    assert corr.tolist() == [float(arg["q"][p, lag + ml - 1]) / ONE / root if inside else 0.0
                             for p, (lag, inside) in enumerate(zip(want["lags"], want["inside"]))]
    assert np.abs(corr).sum() == pytest.approx(float(rec["score"]), rel=1e-15)


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_worked_cases(name, arg, want):
    from tdoa_amd import sync
    got = sync.sync(arg["q"], arg["ref"], arg["ml"], arg["G"], arg["R"], arg["centre"], arg["n_w"])
    _check_hand_case(got, arg, want)


def test_model_arguments_and_candidate_order():
    from tdoa_amd import sync
    assert sync.candidates(3).tolist() == [0, 1, -1, 2, -2, 3, -3] and sync.candidates(0).tolist() == [0]
    q = np.zeros((3, 7), dtype=np.int64)
    good = dict(q_pairs=q, ref_delay=(0, 0, 0), max_lag=4, gate=1, rounds=1)
    for kw in (dict(gate=-1), dict(gate=1024), dict(rounds=-1), dict(rounds=17), dict(ref_delay=(0,)), dict(ref_delay=(0, 0)),
               dict(q_pairs=q[:, :6]), dict(centre=(0, 0))):
        with pytest.raises(ValueError):
            sync.sync(**{**good, **kw})
    a, b = np.array([[0, 37, -52, 18]]), np.array([[0, 38, -52, 21]])
    mid = sync.midpoint_clock(a, b)
    assert mid.dtype == np.int32 and mid.tolist() == [[0, 600, -832, 312]]          # 37.5, -52 and 19.5 samples in 1/16
    with pytest.raises(ValueError):
        sync.midpoint_clock(a, b[:, :3])


# ---- an independent statement of the three phases: plain integers, one candidate at a time --------------------------------
def _enumerate(q, ref, ml, G, R, centre):
    """-> (k, start F, final F, pairs inside, lags or None per pair, moved, {"start", "place", "sweep"} where more than one
    candidate had the largest value)"""
    S = len(ref)
    order = sorted(range(-G, G + 1), key=lambda x: 2 * abs(x) - (x > 0))
    ties = set()

    def e(i, j):
        d = int(ref[j]) - int(ref[i])
        a = (2 * abs(d) + 16) // 32
        return -a if d < 0 else a

    def m(i, j, lag):
        return abs(int(q[_pair(i, j, S)][lag + ml - 1])) if -ml < lag < ml else 0

    def best(values, kind):
        top = max(values)
        if values.count(top) > 1:
            ties.add(kind)
        return values.index(top)

    def place(s, partners, kind):
        values = []
        for x in order:
            ks = centre[s] + x
            values.append(sum(m(i, s, e(i, s) + ks - k[i]) if i < s else m(s, i, e(s, i) + k[i] - ks) for i in partners))
        return centre[s] + order[best(values, kind)]

    def objective():
        total, lags = 0, []
        for i in range(S):
            for j in range(i + 1, S):
                lag = e(i, j) + k[j] - k[i]
                total += m(i, j, lag)
                lags.append(lag if -ml < lag < ml else None)
        return total, lags

    k = [int(c) for c in centre]
    if S == 2:
        k[1] = place(1, [0], "start")
    else:
        cells = [(x1, x2) for x1 in order for x2 in order]
        values = [m(0, 1, e(0, 1) + centre[1] + x1 - k[0]) + m(0, 2, e(0, 2) + centre[2] + x2 - k[0]) +
                  m(1, 2, e(1, 2) + (centre[2] + x2) - (centre[1] + x1)) for x1, x2 in cells]
        x1, x2 = cells[best(values, "start")]
        k[1], k[2] = centre[1] + x1, centre[2] + x2
        for s in range(3, S):
            k[s] = place(s, range(s), "place")
    start = objective()[0]
    moved = 0
    for _ in range(R):
        moved = 0
        for s in range(1, S):
            new = place(s, [i for i in range(S) if i != s], "sweep")
            moved += new != k[s]
            k[s] = new
    final, lags = objective()
    return k, start, final, sum(l is not None for l in lags), lags, moved, ties


def test_model_against_the_phases_enumerated():
    """small random Q with few distinct values, so equal maxima are common; delays and centres that put pairs outside"""
    from tdoa_amd import sync
    rng = np.random.default_rng(29)
    n = n_zero = n_out = n_moved = 0
    kinds = {"start": 0, "place": 0, "sweep": 0}
    for S, ml in ((2, 3), (3, 4), (3, 7), (4, 5), (4, 9), (4, 6), (4, 7), (4, 8)):
        P = S * (S - 1) // 2
        for G in (0, 1, 2, 3):
            for R in (0, 1, 1, 3):
                for span in (8, 16 * ml):
                    q = rng.integers(-2, 3, size=(P, 2 * ml - 1), dtype=np.int64) * (rng.random() < 0.9)
                    q *= rng.random(q.shape) < 0.6
                    ref = rng.integers(-span, span + 1, size=S, dtype=np.int32)
                    centre = rng.integers(-ml // 2, ml // 2 + 1, size=S, dtype=np.int32) if rng.random() < 0.7 else None
                    rec, clock, lags, corr = sync.sync(q, ref, ml, G, R, centre, n_w=2)
                    k, start, final, pairs_in, want_lags, moved, ties = _enumerate(q, ref, ml, G, R, [0] * S if centre is None else centre.tolist())
                    n += 1
                    for kind in ties:
                        kinds[kind] += 1
                    if final == 0:
                        n_zero += 1
                        assert rec.tobytes() == bytes(32) and not clock.any() and not lags.any() and not corr.any()
                        continue
                    assert clock.tolist() == k and (int(rec["start_q"]), int(rec["score_q"])) == (start, final)
                    assert (int(rec["moved"]), int(rec["pairs_in"])) == (moved, pairs_in)
                    assert lags.tolist() == [l or 0 for l in want_lags]
                    assert corr.tolist() == [0.0 if l is None else float(q[p][l + ml - 1]) / ONE / np.sqrt(2.0) for p, l in enumerate(want_lags)]
                    assert float(rec["score"]) == float(final) / ONE / np.sqrt(2.0)
                    n_out += pairs_in < P
                    n_moved += moved > 0
    print("%d searches: %d all zero, %d with pairs outside, %d whose last sweep moved a station; equal maxima at the start in "
          "%d, in a placing in %d, in a sweep in %d" % (n, n_zero, n_out, n_moved, kinds["start"], kinds["place"], kinds["sweep"]))
    assert n_zero >= 2 and n_out >= 5 and n_moved >= 2 and min(kinds.values()) >= 5         # each kind of case occurs


def test_properties_of_the_search():
    """score_q >= start_q; a result whose last sweep moved nothing is a fixed point of one more sweep; with G = 0 the clocks are
    the centres"""
    from tdoa_amd import sync
    rng = np.random.default_rng(31)
    n_fixed = 0
    for S, ml, G in ((3, 12, 4), (4, 16, 5), (5, 16, 7), (6, 10, 3)):
        P = S * (S - 1) // 2
        for trial in range(6):
            q = rng.integers(0, 4, size=(P, 2 * ml - 1), dtype=np.int64) * ONE
            ref = rng.integers(-48, 49, size=S, dtype=np.int32)
            centre = rng.integers(-2, 3, size=S, dtype=np.int32)
            last = None
            for R in range(5):
                rec, clock, lags, corr = sync.sync(q, ref, ml, G, R, centre)
                assert rec["score_q"] >= rec["start_q"] > 0
                assert last is None or rec["score_q"] >= last[0]["score_q"]              # F never decreases over a sweep
                if last is not None and R >= 2 and last[0]["moved"] == 0:
                    n_fixed += 1
                    assert rec["moved"] == 0 and clock.tolist() == last[1].tolist() and rec["score_q"] == last[0]["score_q"]
                last = (rec, clock)
            rec, clock, lags, corr = sync.sync(q, ref, ml, 0, 3, centre)
            assert clock.tolist() == centre.tolist() and rec["moved"] == 0 and rec["score_q"] == rec["start_q"]
    assert n_fixed >= 10


# ---- the delay-table search's model with station clocks -------------------------------------------------------------------
def test_locate_model_with_clocks():
    from tdoa_amd import locate
    rng = np.random.default_rng(37)
    n_half = 0
    for S, ml in ((2, 5), (3, 6), (4, 9)):
        P = S * (S - 1) // 2
        for n_cells, n_cols in ((9, 3), (31, 7)):
            q = rng.integers(-3, 4, size=(P, 2 * ml - 1), dtype=np.int64)
            table = rng.integers(-16 * ml, 16 * ml + 1, size=(n_cells, S), dtype=np.int32)
            plain = locate.locate(q, table, n_cols, ml, 1, 2)
            zero = locate.locate(q, table, n_cols, ml, 1, 2, clock=np.zeros(S, dtype=np.int32))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, zero))          # a zero clock: the same bytes
            k = rng.integers(-ml, ml + 1, size=S)
            whole = locate.locate(q, table, n_cols, ml, 1, 2, clock=16 * k)
            moved = locate.locate(q, table + (16 * k)[None, :].astype(np.int32), n_cols, ml, 1, 2)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, moved))         # 16 k: the table's columns moved by k samples
            half = 16 * k + 8 * rng.integers(-1, 2, size=S)                              # half-way clocks: every cell and pair enumerated
            rec, lags, corr, score_map = locate.locate(q, table, n_cols, ml, 2, 2, clock=half)
            scores, best, pairs_in, want_lags, runner = _brute(q, (table.astype(np.int64) + half[None, :]).tolist(), n_cols, ml, 2)
            assert score_map.tolist() == scores and best is not None
            assert (int(rec["cell"]), int(rec["pairs_in"]), int(rec["score_q"])) == (best, pairs_in, scores[best])
            assert lags.tolist() == [l or 0 for l in want_lags]
            assert (int(rec["runner_cell"]), int(rec["runner_q"])) == ((0, 0) if runner is None else (runner, scores[runner]))
            n_half += int((half % 16 == 8).any())
    assert n_half >= 4
    big = locate.pair_lags(np.array([[-2 ** 31, 2 ** 31 - 1]], dtype=np.int32), np.array([-2 ** 31, 2 ** 31 - 1], dtype=np.int32))
    assert big.tolist() == [[(2 * (2 ** 33 - 2) + 16) // 32]]                            # the sum is taken in 64 bits
    q, t = np.zeros((3, 7), dtype=np.int64), np.zeros((2, 3), dtype=np.int32)
    with pytest.raises(ValueError):
        locate.locate(q, t, 2, 4, clock=(0, 0))
    with pytest.raises(ValueError):
        locate.locate_stacks(q[None], t, 2, 4, clock=np.zeros((2, 3), dtype=np.int32))


# ---- the noisy case ------------------------------------------------------------------------------------------------------
def noisy_sync_case():
    """(table [48 * 64][4], ref_delay [4] = the table's row of the known emitter's cell (40, 10), its station delays in samples,
    the target's planted cell (12, 36), its station delays): delays rint(fs dist / c) minus their minimum"""
    from tdoa_amd import locate
    table, planted_cell, d_tgt, _ = noisy_case()
    cell = 40 * 64 + 10
    tx = locate.ecef(GRID["lat0"] + 40 * GRID["dlat"], GRID["lon0"] + 10 * GRID["dlon"], GRID["height_m"])
    dist = np.linalg.norm(locate.ecef(*np.array(ST4).T) - tx, axis=1)
    d = np.rint(FS * dist / locate.SPEED_OF_LIGHT).astype(np.int64)
    d -= d.min()
    return table, table[cell].copy(), [int(x) for x in d], planted_cell, d_tgt


def noisy_sync_windows(oracle, d_ref, d_tgt, n_windows=12):
    """(reference windows, target windows), each [w][s] u8 IQ: station s starts CLOCKS[s] samples late in both"""
    ref = [[oracle.simulate_delayed_fm(8192, d_ref[s] + CLOCKS[s] + 100, 300 + w, 1300 + 1000 * s + w, 1.0, 0.6) for s in range(4)]
           for w in range(n_windows)]
    tgt = [[oracle.simulate_delayed_fm(8192, d_tgt[s] + CLOCKS[s] + 100, 700 + w, 1700 + 1000 * s + w, 1.0, 0.6) for s in range(4)]
           for w in range(n_windows)]
    return ref, tgt


def argmax_clocks(q, e, max_lag):
    """the clocks the independent argmaxes of pairs (0, s) give: lag - e_0s"""
    own = own_lags(q, max_lag)
    return (0,) + tuple(own[s - 1] - int(e[s - 1]) for s in range(1, 4))


def count_noisy_case(q_ref, q_tgt, sync_out, loc_clocked, loc_plain, e, planted_cell, max_lag):
    """the four counts of the issue's table over the windows: q_* [w][6][L]; sync_out (records, clocks); loc_*: records"""
    n = len(q_ref)
    own_ok = sum(argmax_clocks(q_ref[w], e, max_lag) == CLOCKS for w in range(n))
    sync_ok = sum(tuple(sync_out[1][w].tolist()) == CLOCKS for w in range(n))
    with_ok = int((loc_clocked["cell"] == planted_cell).sum())
    without_ok = int((loc_plain["cell"] == planted_cell).sum())
    print("all three clocks right in %d of %d windows by the argmaxes of pairs (0, s), in %d by the clock search; the planted cell "
          "found in %d with the found clocks, in %d without clocks" % (own_ok, n, sync_ok, with_ok, without_ok))
    return own_ok, sync_ok, with_ok, without_ok


def test_the_clock_search_finds_the_clocks_and_the_cell(oracle):
    """One window per stack, max_lag 256, G 120, R 2, twelve windows, noise 0.6.  Measured with the float64 pipeline: the
    argmaxes of pairs (0, s) give all three clocks in 2 of 12 windows, the clock search in 10; locating the target window with
    the found clocks hits the planted cell in 10, without clocks in 0."""
    from tdoa_amd import locate, stacking, sync
    ml, G, R = 256, 120, 2
    table, ref_delay, d_ref, planted_cell, d_tgt = noisy_sync_case()
    e = locate.pair_lags(ref_delay[None, :])[0]
    wins_ref, wins_tgt = noisy_sync_windows(oracle, d_ref, d_tgt)

    def words(wins):
        out = []
        for x in wins:
            sig = [oracle.b_preprocess(s)[0] for s in x]
            out.append([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ml)) for i, j in PAIRS4])
        return np.array(out)

    q_ref, q_tgt = words(wins_ref), words(wins_tgt)
    found = sync.sync_stacks(q_ref, ref_delay, ml, G, R)
    for w in range(12):
        rec = found[0][w]
        assert rec["score_q"] >= rec["start_q"] > 0 and rec["pairs_in"] == 6
        print("window %2d: argmaxes %s, clock search %s moved %d score %.3f" % (w, argmax_clocks(q_ref[w], e, ml), found[1][w].tolist(),
                                                                                  rec["moved"], rec["score"]))
    clocked = locate.locate_stacks(q_tgt, table, 64, ml, 1, 1, clock=16 * found[1])[0]
    plain = locate.locate_stacks(q_tgt, table, 64, ml, 1, 1)[0]
    own_ok, sync_ok, with_ok, without_ok = count_noisy_case(q_ref, q_tgt, found, clocked, plain, e, planted_cell, ml)
    assert own_ok <= 4
    assert sync_ok >= 9
    assert with_ok >= 9
    assert without_ok <= 1
