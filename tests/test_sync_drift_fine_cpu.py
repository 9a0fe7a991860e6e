"""CPU: the numpy statement of the fine clock lines (tdoa_amd.sync_drift_fine; include/tdoa_mi355x.h, "fine clock lines") on
hand-worked cases, against an independent enumeration in Python integers, its properties, and on the measured case the feature
exists for; and the boundary of the entry points that needs no device.  hand_cases(), check_hand_case(), few_valued_lines() and
the measured case's functions are shared with tests/test_gpu_sync_drift_fine.py, which runs the kernels on the same words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_locate_cpu import FS, PAIRS4, ST4
from test_locate_upsample_cpu import FINE_SIDE, ML, POSITIONS, coarse_table, fine_position, fine_table, metres, position_ecef
from test_sync_fine_cpu import CLOCK4, NOISE as _NOISE_STILL, WL, measured_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 2 ** 32
NAMES = ("tdoa_process_sync_drift_fine", "tdoa_group_process_sync_drift_fine", "tdoa_debug_sync_drift_fine_from_q",
         "tdoa_sync_line_clock16")
FACTORS = (2, 4, 8, 16)
COARSE_KEYS = ("line", "clock", "rate", "rows", "lags", "corr")
FINE_KEYS = ("fine", "clock16", "fine_rate", "fine_rows", "fine_lags", "fine_corr")
KEYS = COARSE_KEYS + FINE_KEYS


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


# ---- 1. the entry points ---------------------------------------------------------------------------------------------------
def _prototypes():
    """{function: [(C type, parameter name)]} of every prototype in the header"""
    text = open(os.path.join(ROOT, "include", "tdoa_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for name, params in re.findall(r"\b(tdoa_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        plist = []
        for p in (x.strip() for x in params.split(",")):
            if p in ("", "void"):
                continue
            m = re.fullmatch(r"(.*?)(\w+)\s*(\[\w*\])?", p, flags=re.S)
            plist.append((" ".join((m.group(1) + ("*" if m.group(3) else "")).replace("const", " ").replace("*", " * ").split()), m.group(2)))
        out[name] = plist
    return out


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import sync_drift_fine
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessSyncDriftFine(", "C.tdoa_process_sync_drift_fine(", "func (g *Group) ProcessSyncDriftFine(",
                 "C.tdoa_group_process_sync_drift_fine("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_sync_drift_fine", "sync_drift_fine_from_q"):
        assert hasattr(capi.Context, method) and getattr(capi.Context, method).__doc__, method
    assert hasattr(capi.Group, "process_sync_drift_fine") and callable(capi.sync_line_clock16)
    for name in ("refine_line", "sync_line_fine", "sync_lines_fine", "line_clock16"):
        assert callable(getattr(sync_drift_fine, name)), name
    assert len(capi.SEARCHES) == 9 and "sync_drift_fine" not in capi.SEARCHES and list(capi.LATER_SEARCHES) == ["sync_drift_fine"]
    # the definition is in the header in the words the tests hold the library to
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("U is one of 2, 4, 8, 16. 0 <= Rf <= 16.",
                   "The call does not read the context's tdoa_locate_set_upsample setting.",
                   "Exactly tdoa_process_sync_drift(windows_per_stack, gate, max_drift, drift_den, rounds, ref_delay, centre, ...).",
                   "The first six outputs are that call's bytes.",
                   "A fine lag lam is inside when |lam| <= (max_lag - 1) U.",
                   "Q_U[lam + (max_lag - 1) U] of that (position, pair) row, with Q_U exactly as tdoa_locate_set_upsample defines it.",
                   "An outside term adds 0 and is not counted.", "No Q_U is materialised.",
                   "e^U_ij = sgn(d) * ((2|d| U + 16) div 32) with d = ref_delay[j] - ref_delay[i], taken in 64 bits.",
                   "kappa_s = U k_s + y_s in 1/U sample, |y_s| <= U", "eta_s = U h_s + g_s, |g_s| <= U, in units of 1/(U D) lag per position.",
                   "Station 0 is the gauge: y_0 = g_0 = 0.",
                   "kappa_s(x) = kappa_s + shift(eta_s, x), in 1/U sample.",
                   "shift(h, x) = sgn(h) * ((2|h|x + D) div (2D)) is the slope search's rule with the same D.",
                   "A^U_ij = sum over x of Q_U,x,ij[e^U_ij + kappa_j(x) - kappa_i(x)]", "F_U = sum over i < j of |A^U_ij|.",
                   "start_q = F_U at y = g = 0.", "this is not the coarse line's F.",
                   "There is no placing.", "r = rank(g) * (2U + 1) + rank(y), with rank(x) = 2|x| - (x > 0).",
                   "The first of equal maxima wins.", "The window stays centred on (U k_s, U h_s) in every sweep.",
                   "F_U never decreases.", "clock16[S] = kappa_s * (16 / U).", "fine_rate[S] = eta_s.",
                   "fine_rows[S] = kappa_s(x) * (16 / U), the row tdoa_locate_set_clock takes.",
                   "If the coarse record is the zero record or the final F_U is 0, every fine output of that line is zero.",
                   "With Rf = 0: clock16 = 16 * clock and fine_rate = U * rate.",
                   "|centre[s]| + G + 2 + ((H + 1)(L - 1)) div D >= 2^27", "4 * P * N_w > 2^17", "4 * P * track_len * n_w > 2^17",
                   "|q| <= 2^60 div (P * L)", "out[x - first_position][s] = clock16[s] + r(16 * eta_s * x, U * D)"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_the_later_table_states_the_headers_order_and_types(capi):
    """capi.LATER_SEARCHES against the parsed header, as tests/test_capi_bindings_cpu.py holds the nine"""
    lib, protos = capi.load(), _prototypes()
    c_types = {"int": C.c_int, "int32_t *": C.POINTER(C.c_int32), "double *": C.POINTER(C.c_double), "int64_t *": C.POINTER(C.c_int64)}
    scalars = {"int32_t *": np.int32, "double *": np.float64}
    s = capi.LATER_SEARCHES["sync_drift_fine"]
    assert type(s) is type(capi.SEARCHES["sync_drift"]) and s.track_len and not s.bare and s.stats is None
    assert s.entries == {"own": NAMES[0], "group": NAMES[1], "q": NAMES[2]}
    assert s.ints == ("gate", "max_drift", "drift_den", "rounds", "U", "fine_rounds") and s.inputs == ("ref_delay", "centre")
    assert [o.key for o in s.outputs] == list(KEYS)
    for route, entry in s.entries.items():
        names = ["ctx", "q", "n_sets", "track_len", "n_stations", "n_w"] if route == "q" else ["ctx" if route == "own" else "g", "windows_per_stack"]
        names += list(s.ints) + list(s.inputs) + [o.key if route == "q" else o.key + "_host" for o in s.outputs]
        assert [n for _, n in protos[entry]] == names, entry
        argtypes = getattr(lib, entry).argtypes
        assert len(argtypes) == len(names), entry
        first_out = len(names) - len(s.outputs)
        for k, ((ctype, name), argtype) in enumerate(zip(protos[entry], argtypes)):
            if k == 0:
                assert ctype == ("tdoa_group *" if route == "group" else "tdoa_ctx *") and argtype is C.c_void_p
            elif ctype in c_types:
                assert argtype is c_types[ctype], (entry, name)
            else:
                assert ctype == "tdoa_sync_line *" and argtype is C.c_void_p, (entry, name)
            if k >= first_out:
                dtype = np.dtype(s.outputs[k - first_out].dtype)
                assert dtype == (capi.SYNC_LINE_DTYPE if ctype == "tdoa_sync_line *" else np.dtype(scalars[ctype])), (entry, name)
            elif k >= first_out - 2:
                assert ctype == "int32_t *", (entry, name)
            elif name != "q" and k > 0:
                assert ctype == "int", (entry, name)
    assert [n for _, n in protos[NAMES[3]]] == ["clock16", "fine_rate", "n_stations", "U", "drift_den", "first_position", "n_positions", "out"]
    assert len(lib.tdoa_sync_line_clock16.argtypes) == 8


# ---- 2. what needs no device -------------------------------------------------------------------------------------------------
def test_null_handle_and_the_host_helper_need_no_device(capi):
    from tdoa_amd import sync_drift_fine
    lib = capi.load()
    rec, fine = np.zeros(3, dtype=capi.SYNC_LINE_DTYPE), np.zeros(3, dtype=capi.SYNC_LINE_DTYPE)
    q = np.zeros(3 * 9, dtype=np.int64)
    ref = (C.c_int32 * 3)(0, 16, 32)
    pr, pf, pq = rec.ctypes.data_as(C.c_void_p), fine.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_int64))
    n5 = (None,) * 5
    for U, Rf in ((16, 2), (2, 0), (0, 1), (1, 1), (3, 1), (5, 1), (6, 1), (12, 1), (32, 1), (-2, 1), (16, -1), (16, 17)):
        assert lib.tdoa_process_sync_drift_fine(None, 0, 1, 1, 1, 1, U, Rf, ref, None, pr, *n5, pf, *n5) == 1
        assert lib.tdoa_group_process_sync_drift_fine(None, 0, 1, 1, 1, 1, U, Rf, ref, None, pr, *n5, pf, *n5) == 1
        assert lib.tdoa_debug_sync_drift_fine_from_q(None, pq, 1, 1, 3, 1, 1, 1, 1, 1, U, Rf, ref, None, pr, *n5, pf, *n5) == 1
    assert lib.tdoa_process_sync_drift_fine(None, 0, 1, 1, 1, 1, 16, 2, None, None, None, *n5, None, *n5) == 1
    # the helper: position 0 is clock16; r rounds halves away from zero
    assert capi.sync_line_clock16((0, 592, -832, 288), (0, 52, -88, 36), 16, 4, 0, 1).tolist() == [[0, 592, -832, 288]]
    # 16 eta x / (U D) = eta x / 8 at U = 16, D = 8: +-4 is a half at x = 1, +-12 at x = 1 is 1.5
    assert capi.sync_line_clock16((0, 1, -1, 5, -5), (0, 4, -4, 12, -12), 16, 8, 1, 2).tolist() == [[0, 2, -2, 7, -7], [0, 2, -2, 8, -8]]
    rng = np.random.default_rng(5)
    n_half = 0
    for U in FACTORS:
        for D in (1, 3, 4, 7, 32):
            k, h = rng.integers(-5000, 5001, size=6), rng.integers(-300, 301, size=6)
            got = capi.sync_line_clock16(k, h, U, D, 9, 40)
            assert got.dtype == np.int32 and got.tobytes() == sync_drift_fine.line_clock16(k, h, U, D, 9, 40).tobytes()
            exact = np.array([[int(k[s]) + 16 * int(h[s]) * x / (U * D) for s in range(6)] for x in range(9, 49)])
            assert np.abs(got - exact).max() <= 0.5
            halves = np.abs(np.abs(got - exact) - 0.5) < 1e-9
            n_half += int(halves.sum())
            assert (np.abs(got - k[None, :])[halves] > np.abs(exact - k[None, :])[halves]).all()      # away from zero, either sign
    assert n_half >= 20
    i32 = C.POINTER(C.c_int32)
    out = np.zeros(3, dtype=np.int32)
    po = out.ctypes.data_as(i32)
    for args in ((None, ref, 3, 16, 1, 0, 1, po), (ref, None, 3, 16, 1, 0, 1, po), (ref, ref, 3, 16, 1, 0, 1, None), (ref, ref, 0, 16, 1, 0, 1, po),
                 (ref, ref, 3, 1, 1, 0, 1, po), (ref, ref, 3, 3, 1, 0, 1, po), (ref, ref, 3, 32, 1, 0, 1, po), (ref, ref, 3, 0, 1, 0, 1, po),
                 (ref, ref, 3, 16, 0, 0, 1, po), (ref, ref, 3, 16, 1, -1, 1, po), (ref, ref, 3, 16, 1, 0, 0, po)):
        assert lib.tdoa_sync_line_clock16(*args) == 1, args[2:7]
    assert lib.tdoa_sync_line_clock16(ref, ref, 3, 2, 1, 0, 1, po) == 0
    for bad in (dict(U=1), dict(U=3), dict(drift_den=0), dict(first_position=-1), dict(n_positions=0)):
        with pytest.raises(ValueError):
            sync_drift_fine.line_clock16((0, 1), (0, 1), **{**dict(U=16, drift_den=1, first_position=0, n_positions=1), **bad})


# ---- 3. hand-worked cases: position x, pairs i < j in the library's order, lag l at index l + max_lag - 1 ------------------
def _pair(i, j, S):
    return i * S - i * (i + 1) // 2 + (j - i - 1)


def _q(S, ml, L, *peaks):
    """[L][P] rows of 2 ml - 1 zeros with (position, i, j, lag, value in units of 2^32) set"""
    q = np.zeros((L, S * (S - 1) // 2, 2 * ml - 1), dtype=np.int64)
    for pos, i, j, lag, value in peaks:
        q[pos, _pair(i, j, S), lag + ml - 1] = value * ONE
    return q


def hand_cases():
    """[(name, dict(q, ml, ref, centre, G, H, D, R, U, Rf, n_w), expected or None for all zeros)]; expected: the coarse clock and
    rate, kappa and eta, the fine lags [L][P] (0 for a term outside), inside [L][P], moved.  Two equal words v side by side
    interpolate to 2 x 20639 / 32768 v = 1.26 v half-way between them and to less everywhere else; a lone word v to 0.63 v
    half a lag away and to less than v anywhere off its lag."""
    # one position, words 8, 8 at lags 2 and 3.  The coarse search takes lag 2 (x = +2 comes before +3).  kappa = 2 k + y: fine
    # lag 5 = 2.5 samples is the largest, y = +1.  One position: every g is the same line, rank 0 wins, g = 0
    between = dict(q=_q(2, 5, 1, (0, 0, 1, 2, 8), (0, 0, 1, 3, 8)), ml=5, ref=(0, 0), centre=None, G=3, H=1, D=1, R=1, U=2, n_w=1)
    # three positions whose peak slides by half a lag per position: at lag 0; between lags 0 and 1; at lag 1.  The coarse search
    # (G = 0, H = 1, D = 1) reads 8 + 8 with h = 0 and 8 + 8 with h = +1: h = 0 first.  eta = g in half lags per position: g = +1
    # reads 8 + 1.26 x 8 + 8 at fine lags 0, 1, 2; g = 0 and g = +2 read 16; with y = +-1 two of the three are half a lag off
    sliding = dict(q=_q(2, 6, 3, (0, 0, 1, 0, 8), (1, 0, 1, 0, 8), (1, 0, 1, 1, 8), (2, 0, 1, 1, 8)), ml=6, ref=(0, 0), centre=None,
                   G=0, H=1, D=1, R=1, U=2, n_w=2)
    # pair 01 has 5, 5 at lags 0 and 1 of both positions: y_1 = +2 of U = 4 (0.5 sample), and with D = 4 shift(+-1, 1) = 0 on the
    # grid of 1/16 lag per position, so g = +-1 tie with g = 0, which is first.  e_02 = e_12 = 8 samples = 32 fine lags, and
    # 32 less every offset and shift there is stays outside |lam| <= 20: station 2's candidates all add 0 -- (g, y) = (0, 0),
    # the first -- and four of the six terms are not counted
    outside = dict(q=_q(3, 6, 2, (0, 0, 1, 0, 5), (0, 0, 1, 1, 5), (1, 0, 1, 0, 5), (1, 0, 1, 1, 5), (0, 0, 2, 5, 9), (1, 1, 2, 5, 9)), ml=6,
                   ref=(0, 0, 128), centre=None, G=0, H=0, D=4, R=0, U=4, n_w=1)
    return [
        ("a peak between two lags, which only a fine offset finds", dict(Rf=1, **between),
         dict(clock=(0, 2), rate=(0, 0), kappa=(0, 5), eta=(0, 0), lags=((5,),), inside=((1,),), moved=1)),
        ("the second fine sweep moves nothing", dict(Rf=2, **between),
         dict(clock=(0, 2), rate=(0, 0), kappa=(0, 5), eta=(0, 0), lags=((5,),), inside=((1,),), moved=0)),
        ("no fine sweep: 16 x the coarse clock, U x the coarse rate", dict(Rf=0, **between),
         dict(clock=(0, 2), rate=(0, 0), kappa=(0, 4), eta=(0, 0), lags=((4,),), inside=((1,),), moved=0)),
        ("a slope between two coarse slopes, which only a fine rate finds", dict(Rf=1, **sliding),
         dict(clock=(0, 0), rate=(0, 0), kappa=(0, 0), eta=(0, 1), lags=((0,), (1,), (2,)), inside=((1,),) * 3, moved=1)),
        # position 0 has 4 at lag 0, position 1 has 7, 1, 7 at lags -1, 0, 1.  g = +-2 of U = 2 (one lag per position) read
        # 4 + 7 = 11, g = 0 reads 5, g = +-1 reads 4 and less than 7 half-way between the 1 and a 7; y = +-2 reads a 7 alone.
        # Of the equal maxima the positive g has the smaller rank
        ("equal maxima: the smaller rank, the positive g",
         dict(q=_q(2, 7, 2, (0, 0, 1, 0, 4), (1, 0, 1, -1, 7), (1, 0, 1, 0, 1), (1, 0, 1, 1, 7)), ml=7, ref=(0, 0), centre=None, G=0, H=0, D=1,
              R=0, U=2, Rf=2, n_w=1),
         dict(clock=(0, 0), rate=(0, 0), kappa=(0, 0), eta=(0, 2), lags=((0,), (2,)), inside=((1,),) * 2, moved=0)),
        ("terms outside the range add 0 and are not counted; g = 0 before its equals", dict(Rf=1, **outside),
         dict(clock=(0, 0, 0), rate=(0, 0, 0), kappa=(0, 2, 0), eta=(0, 0, 0), lags=((2, 0, 0), (2, 0, 0)), inside=((1, 0, 0), (1, 0, 0)),
              moved=1)),
        # e^U_01 = 23 fine lags of 1/16 sample from the delays; the coarse stage has e_01 = 1, the centre puts its window at 3 +- 1,
        # and the words 6 at lag 5 of position 0 and lag 6 of position 1 give k_1 = 4, h_1 = +1 (D = 1).  Fine: kappa_1 = 64 + y,
        # eta_1 = 16 + g, the words at fine lags 80 and 96 = 23 + 64 + y + shift(16 + g, x): y = -7, g = 0
        ("e^U from the delays on the fine grid; the centre moves the window; the coarse slope stays",
         dict(q=_q(2, 9, 2, (0, 0, 1, 5, 6), (1, 0, 1, 6, 6)), ml=9, ref=(0, 23), centre=(0, 3), G=1, H=1, D=1, R=0, U=16, Rf=1, n_w=1),
         dict(clock=(0, 4), rate=(0, 1), kappa=(0, 57), eta=(0, 16), lags=((80,), (96,)), inside=((1,),) * 2, moved=1)),
        ("all zeros", dict(q=_q(3, 5, 3), ml=5, ref=(0, 16, 32), centre=(0, 1, -1), G=2, H=2, D=3, R=1, U=16, Rf=2, n_w=1), None),
    ]


def _shift(h, x, D):
    a = (2 * abs(h) * x + D) // (2 * D)
    return -a if h < 0 else a


def _fine_e(ref, U):
    S = len(ref)
    return [(lambda d: (1 if d >= 0 else -1) * ((2 * abs(d) * U + 16) // 32))(int(ref[j]) - int(ref[i])) for i in range(S) for j in range(i + 1, S)]


def _exact_rows(q, U):
    from tdoa_amd import upsample
    return [[upsample.upsample_exact(row, U) for row in pos] for pos in q]


def _f_exact(rows, e, kappa, eta, D, half, only=None):
    """(F_U or the sum over station `only`'s pairs, terms inside, lags [L][P], inside [L][P], words [L][P]) in Python integers"""
    S, L = len(kappa), len(rows)
    pairs = [(i, j) for i in range(S) for j in range(i + 1, S)]
    f = n_in = 0
    lags, ins, words = [[0] * len(pairs) for _ in range(L)], [[0] * len(pairs) for _ in range(L)], [[0] * len(pairs) for _ in range(L)]
    for p, (i, j) in enumerate(pairs):
        if only is not None and only not in (i, j):
            continue
        a = 0
        for x in range(L):
            lam = e[p] + kappa[j] + _shift(eta[j], x, D) - kappa[i] - _shift(eta[i], x, D)
            if abs(lam) <= half:
                lags[x][p], ins[x][p], words[x][p] = lam, 1, rows[x][p][lam + half]
                a += words[x][p]
                n_in += 1
        f += abs(a)
    return f, n_in, lags, ins, words


def check_hand_case(out, arg, want):
    """out: sync_line_fine's dict of one line"""
    from tdoa_amd import sync_drift
    q, ml, D, U = arg["q"], arg["ml"], arg["D"], arg["U"]
    L, P, S = q.shape[0], q.shape[1], len(arg["ref"])
    coarse = sync_drift.sync_line(q, arg["ref"], ml, arg["G"], arg["H"], D, arg["R"], arg["centre"], arg["n_w"])
    for key, w in zip(COARSE_KEYS, coarse):
        assert out[key].tobytes() == w.tobytes(), key
    assert out["clock16"].dtype == out["fine_rate"].dtype == out["fine_rows"].dtype == out["fine_lags"].dtype == np.int32
    assert out["fine_corr"].dtype == np.float64 and out["fine"].dtype == sync_drift.SYNC_LINE_DTYPE
    assert out["clock16"].shape == out["fine_rate"].shape == (S,) and out["fine_rows"].shape == (L, S)
    assert out["fine_lags"].shape == out["fine_corr"].shape == (L, P)
    if want is None:
        assert out["fine"].tobytes() == bytes(40)
        assert not any(out[k].any() for k in FINE_KEYS[1:5]) and out["fine_corr"].tobytes() == bytes(out["fine_corr"].nbytes)
        return
    rec = out["fine"]
    assert out["clock"].tolist() == list(want["clock"]) and out["rate"].tolist() == list(want["rate"])
    assert out["clock16"].tolist() == [k * (16 // U) for k in want["kappa"]] and out["fine_rate"].tolist() == list(want["eta"])
    assert out["fine_lags"].tolist() == [list(r) for r in want["lags"]]
    rows, e, half = _exact_rows(q, U), _fine_e(arg["ref"], U), (ml - 1) * U
    score, n_in, lags, ins, words = _f_exact(rows, e, want["kappa"], want["eta"], D, half)
    assert lags == [list(r) for r in want["lags"]] and ins == [list(r) for r in want["inside"]]
    start = _f_exact(rows, e, [U * k for k in want["clock"]], [U * h for h in want["rate"]], D, half)[0]
    assert (int(rec["moved"]), int(rec["terms_in"]), int(rec["positions"]), int(rec["reserved"])) == (want["moved"], n_in, L, 0)
    assert (int(rec["score_q"]), int(rec["start_q"])) == (score, start) and score >= start > 0
    assert float(rec["score"]) == float(score) / ONE / np.sqrt(np.float64(L * arg["n_w"]))
    root = np.sqrt(np.float64(arg["n_w"]))
    for x in range(L):
        assert out["fine_rows"][x].tolist() == [(want["kappa"][s] + _shift(want["eta"][s], x, D)) * (16 // U) for s in range(S)]
        assert out["fine_corr"][x].tolist() == [float(w) / ONE / root for w in words[x]]
    if arg["Rf"] == 0:
        assert out["clock16"].tolist() == [16 * k for k in want["clock"]] and out["fine_rate"].tolist() == [U * h for h in want["rate"]]
        assert score == start


def model(arg):
    from tdoa_amd import sync_drift_fine
    return sync_drift_fine.sync_line_fine(arg["q"], arg["ref"], arg["ml"], arg["G"], arg["H"], arg["D"], arg["R"], arg["U"], arg["Rf"],
                                          arg["centre"], arg["n_w"])


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_worked_cases(name, arg, want):
    check_hand_case(model(arg), arg, want)


def test_model_arguments():
    from tdoa_amd import sync_drift_fine
    q = _q(3, 5, 2, (0, 0, 1, 0, 1))
    for U, Rf in ((1, 1), (3, 1), (32, 1), (0, 1), (16, -1), (16, 17)):
        with pytest.raises(ValueError):
            sync_drift_fine.refine_line(q, (0, 0, 0), (0, 0, 0), (0, 0, 0), 5, 1, U, Rf)
        with pytest.raises(ValueError):
            sync_drift_fine.sync_line_fine(q, (0, 0, 0), 5, 1, 1, 1, 1, U, Rf)
    with pytest.raises(ValueError):
        sync_drift_fine.refine_line(q, (0, 0, 0), (0, 0), (0, 0, 0), 5, 1, 16, 1)
    with pytest.raises(ValueError):
        sync_drift_fine.refine_line(q, (0, 0, 0), (0, 0, 0), (0, 0, 0), 5, 0, 16, 1)
    with pytest.raises(ValueError):
        sync_drift_fine.sync_lines_fine(q, 3, (0, 0, 0), 5)


# ---- 4. the statement against an enumeration in Python integers, one candidate at a time -----------------------------------
def _rank(y):
    return 2 * abs(y) - (y > 0)


def _enumerate(q, ref, k, h, ml, D, U, Rf):
    """-> (start_q, score_q, moved, kappa, eta, terms_in, steps at which candidates tied for the maximum)"""
    S = len(ref)
    rows, e, half = _exact_rows(q, U), _fine_e(ref, U), (ml - 1) * U
    mid_k, mid_h = [U * int(x) for x in k], [U * int(x) for x in h]
    kap, eta = list(mid_k), list(mid_h)
    start, moved, ties = _f_exact(rows, e, kap, eta, D, half)[0], 0, 0
    order = sorted(range(-U, U + 1), key=_rank)
    for _ in range(Rf):
        moved = 0
        for s in range(1, S):
            best, n_best = None, 0
            for g in order:
                for y in order:
                    tk, te = list(kap), list(eta)
                    tk[s], te[s] = mid_k[s] + y, mid_h[s] + g
                    v = _f_exact(rows, e, tk, te, D, half, only=s)[0]
                    if best is None or v > best[0]:
                        best, n_best = (v, tk[s], te[s]), 1
                    elif v == best[0]:
                        n_best += 1
            ties += n_best > 1
            moved += (best[1], best[2]) != (kap[s], eta[s])
            kap[s], eta[s] = best[1], best[2]
    score, n_in = _f_exact(rows, e, kap, eta, D, half)[:2]
    return start, score, moved, kap, eta, n_in, ties


def few_valued_lines(S, ml, L, seed, n_lines=1, zero_line=None):
    """words -3 .. 3 (x 2^32) with many zeros [n_lines L][P][2 ml - 1], delays within +-4 samples, centres within +-2: ties are
    common and windows reach outside the range"""
    rng = np.random.default_rng(seed)
    P = S * (S - 1) // 2
    shape = (n_lines * L, P, 2 * ml - 1)
    q = rng.integers(-3, 4, size=shape, dtype=np.int64) * (rng.random(shape) < 0.6) * ONE
    if zero_line is not None:
        q[zero_line * L:(zero_line + 1) * L] = 0
    return q, rng.integers(-64, 65, size=S).astype(np.int32), rng.integers(-2, 3, size=S).astype(np.int32)


def test_model_against_the_steps_enumerated():
    from tdoa_amd import sync_drift_fine
    seen = dict(ties=0, outside=0, zero=0, moved=0, still=0, fine_rate=0, fine_offset=0, full=0)
    for S in (2, 3, 4):
        for U in (2, 4):
            for D in (1, 2, 4):
                for trial, (L, Rf, G, H) in enumerate(((1, 1, 1, 1), (2, 2, 0, 1), (3, 1, 2, 0), (3, 0, 1, 2))):
                    ml = 5 + (S + U + D + trial) % 5
                    q, ref, centre = few_valued_lines(S, ml, L, 1000 * S + 100 * U + 10 * D + trial)
                    if (S, U, trial) == (3, 4, 2):
                        q[:] = 0
                    out = sync_drift_fine.sync_line_fine(q, ref, ml, G, H, D, 1, U, Rf, centre, 2)
                    if int(out["line"]["score_q"]) == 0:
                        assert all(out[k].tobytes() == bytes(out[k].nbytes) for k in FINE_KEYS)
                        seen["zero"] += 1
                        continue
                    start, score, moved, kap, eta, n_in, ties = _enumerate(q, ref, out["clock"], out["rate"], ml, D, U, Rf)
                    rec = out["fine"]
                    if score == 0:
                        assert all(out[k].tobytes() == bytes(out[k].nbytes) for k in FINE_KEYS)
                        seen["zero"] += 1
                        continue
                    assert (int(rec["start_q"]), int(rec["score_q"]), int(rec["moved"]), int(rec["terms_in"])) == (start, score, moved, n_in), \
                        (S, U, D, trial)
                    assert out["clock16"].tolist() == [x * (16 // U) for x in kap] and out["fine_rate"].tolist() == eta, (S, U, D, trial)
                    y = np.array(kap) - U * out["clock"].astype(np.int64)
                    g = np.array(eta) - U * out["rate"].astype(np.int64)
                    assert y[0] == g[0] == 0 and (np.abs(y) <= U).all() and (np.abs(g) <= U).all() and score >= start
                    if L == 1:
                        assert not g.any()
                    seen["ties"] += ties
                    seen["outside"] += n_in < L * len(q[0])
                    seen["moved" if moved else "still"] += 1
                    seen["fine_rate"] += int(g.any())
                    seen["fine_offset"] += int(y.any())
                    seen["full"] += int((np.abs(y) == U).any() or (np.abs(g) == U).any())
    print("kinds of case seen:", seen)
    assert all(v > 0 for v in seen.values()), seen


# ---- 5. properties -------------------------------------------------------------------------------------------------------------
def test_properties_of_the_refinement():
    """score_q >= start_q and F_U never falls from one more sweep; Rf = 0 returns the coarse line on the fine grid; one position:
    no fine rate, and the fine clock search's outputs on the same words and coarse clocks; a zero line gives zero outputs"""
    from tdoa_amd import sync_drift, sync_drift_fine, sync_fine
    n_one = 0
    for S in (2, 3, 4, 5):
        for U in FACTORS:
            ml, D, L = 5 + S % 4, (1, 2, 4, 3)[S - 2], 1 + (S + U) % 3
            q, ref, centre = few_valued_lines(S, ml, L, 77 * S + U)
            last = None
            if int(sync_drift.sync_line(q, ref, ml, 2, 1, D, 1, centre, 3)[0]["score_q"]) == 0:          # every window outside
                out = sync_drift_fine.sync_line_fine(q, ref, ml, 2, 1, D, 1, U, 2, centre, 3)
                assert all(out[k].tobytes() == bytes(out[k].nbytes) for k in KEYS)
                continue
            for Rf in (0, 1, 2, 3):
                out = sync_drift_fine.sync_line_fine(q, ref, ml, 2, 1, D, 1, U, Rf, centre, 3)
                rec = out["fine"]
                assert int(rec["score_q"]) >= int(rec["start_q"]) > 0 and int(rec["positions"]) == L
                assert last is None or (int(rec["score_q"]) >= int(last["score_q"]) and int(rec["start_q"]) == int(last["start_q"]))
                last = rec
                if Rf == 0:
                    assert out["clock16"].tolist() == (16 * out["clock"]).tolist() and out["fine_rate"].tolist() == (U * out["rate"]).tolist()
                    assert int(rec["moved"]) == 0 and int(rec["score_q"]) == int(rec["start_q"])
                assert out["fine_rows"][0].tolist() == out["clock16"].tolist()
                cont = sync_drift_fine.line_clock16(out["clock16"], out["fine_rate"], U, D, 0, L)
                for x in range(L):
                    for s in range(S):
                        if (int(out["fine_rate"][s]) * x) % D == 0:          # shift is exact there: the helper continues the rows
                            assert cont[x, s] == out["fine_rows"][x, s]
            # one position: every g ties and rank 0 wins; the rest is the fine clock search on the same words and coarse clocks
            one = sync_drift_fine.sync_line_fine(q[:1], ref, ml, 2, 1, D, 1, U, 2, centre, 3)
            assert one["fine_rate"].tolist() == (U * one["rate"]).tolist() and not one["rate"].any()
            still = sync_fine.refine(q[0], ref, one["clock"], ml, U, 2, 3)
            assert one["clock16"].tobytes() == still[1].tobytes() and one["fine_lags"][0].tobytes() == still[2].tobytes()
            assert one["fine_corr"][0].tobytes() == still[3].tobytes() and one["fine_rows"][0].tobytes() == still[1].tobytes()
            for key in ("score_q", "start_q", "moved", "score"):
                assert one["fine"][key] == still[0][key], key
            assert int(one["fine"]["terms_in"]) == int(still[0]["pairs_in"])
            n_one += 1
    assert n_one >= 12
    zero = sync_drift_fine.sync_line_fine(np.zeros_like(q), ref, ml, 2, 1, D, 1, 16, 2, centre)
    assert all(zero[k].tobytes() == bytes(zero[k].nbytes) for k in KEYS)
    both = sync_drift_fine.sync_lines_fine(np.concatenate([q, q[::-1]]), L, ref, ml, 2, 1, D, 1, 8, 1, centre)
    for n, x in enumerate((q, q[::-1])):
        single = sync_drift_fine.sync_line_fine(x, ref, ml, 2, 1, D, 1, 8, 1, centre)
        for key in KEYS:
            part = both[key][n] if key in ("line", "clock", "rate", "fine", "clock16", "fine_rate") else both[key][n * L:(n + 1) * L]
            assert part.tobytes() == single[key].tobytes(), key


# ---- 6. the measured case --------------------------------------------------------------------------------------------------------
# Four stations ST4, the 48 x 64 GRID, FS, twelve blocks of twelve one-window reference positions (w = 0 .. 11) and twelve target
# positions (w = 12 .. 23) of 8 192 samples, max_lag 128, noise 0.5.  The clocks are CLOCK4 quarter samples and slide by RATE16
# sixteenths of a lag per window; everything in quarter samples is realised by simulating at 4 FS and keeping every 4th IQ sample.
M_POS = 12
LINE = dict(G=120, H=8, D=4, R=2, U=16, Rf=2)
NOISE = 0.5
RATE16 = np.array([0, 13, -22, 9], dtype=np.int64)
FINE_RATES = (0, 52, -88, 36)                                 # RATE16 on the fine grid of 1/(U D) lag per position
TRUE_FIX_RATIO_SIX = 2.16                                     # the same over blocks 0 .. 5 alone: 94.7 m / 43.8 m
TRUE_FIX_RATIO = 1.41                                         # median refined fix / median true-clock fix, measured (see the test)


def _r(a, b):
    """the nearest integer to a / b, halves away from zero"""
    a = np.asarray(a, dtype=np.int64)
    return np.sign(a) * ((2 * np.abs(a) + b) // (2 * b))


def slide4(w):
    """the clocks' slide at window w in quarter samples [4]"""
    return _r(RATE16 * int(w), 4)


def true_rows16(first, n):
    """the true clock rows of positions first .. first + n - 1 in 1/16 sample [n][4], station 0 the gauge"""
    ref_delay, d4, _ = measured_case()
    rows = np.array([4 * (CLOCK4 + slide4(w) + d4) - ref_delay for w in range(first, first + n)], dtype=np.int64)
    return rows - rows[:, :1]


def _quarter_window(oracle, delay4, seed, station_seed):
    return [np.ascontiguousarray(oracle.simulate_delayed_fm(4 * WL, int(delay4[s]), seed, station_seed + 1000 * s, 1.0, NOISE)
                                 .reshape(-1, 2)[::4]).reshape(-1) for s in range(4)]


def reference_windows_iq(oracle, b):
    """[w][s] u8 IQ of block b's reference windows w = 0 .. 11"""
    d4 = measured_case()[1]
    return [_quarter_window(oracle, d4 + CLOCK4 + slide4(w) + 400, 300 + 50 * b + w, 1300 + 50 * b + w) for w in range(M_POS)]


def target_windows_iq(oracle, b):
    """[w - 12][s] u8 IQ of block b's target windows w = 12 .. 23: the emitter at POSITIONS[b], the clocks sliding on"""
    from tdoa_amd import locate
    dist = np.linalg.norm(locate.ecef(*np.array(ST4).T) - position_ecef(*POSITIONS[b]), axis=1)
    d4 = np.rint(4 * FS * dist / locate.SPEED_OF_LIGHT).astype(np.int64)
    d4 -= d4.min()
    return [_quarter_window(oracle, d4 + CLOCK4 + slide4(w) + 400, 700 + 50 * b + w, 1700 + 50 * b + w) for w in range(M_POS, 2 * M_POS)]


def float64_words(oracle, windows):
    """[w][6][255] int64: the float64 pipeline's words of every window and pair"""
    from tdoa_amd import stacking
    out = []
    for iq in windows:
        sig = [oracle.b_preprocess(s)[0] for s in iq]
        out.append([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ML)) for i, j in PAIRS4])
    return np.array(out)


def block_fix_metres(q_tgt, b, rows16, tables={}):
    """the target block's fix under clock rows [12][4] in 1/16 sample: the J = 0 cell track (the sum of the twelve maps) on the
    coarse 48 x 64 table, then the same track on Q x 16 on the 33 x 33 fine grid around that cell -> metres to POSITIONS[b]"""
    from tdoa_amd import locate_track, upsample
    if "coarse" not in tables:
        tables["coarse"] = coarse_table()
    rows16 = np.asarray(rows16, dtype=np.int64)
    cell = int(locate_track.track_stacks(q_tgt, tables["coarse"], 64, ML, M_POS, 0, 1, 1, rows16)[0]["cell"][0])
    t, kk, _, ml = upsample.scaled_args(fine_table(cell), rows16, 0, ML, LINE["U"])
    f = int(locate_track.track_stacks(upsample.upsample(q_tgt, LINE["U"]), t, FINE_SIDE, ml, M_POS, 0, 1, 1, kk)[0]["cell"][0])
    return metres(POSITIONS[b], fine_position(cell, f))


def measure_block(b, q_tgt, out):
    """out: the line's outputs of block b's reference windows (one line) -> (fix under the coarse line continued, the fine line
    continued and the true rows in metres; the worst row error over positions 12 .. 23 coarse and fine in 1/16 sample); prints"""
    from tdoa_amd import sync_drift, sync_drift_fine
    truth = true_rows16(M_POS, M_POS)
    coarse = sync_drift.line_clock(out["clock"], out["rate"], LINE["D"], M_POS, M_POS).astype(np.int64)
    fine = sync_drift_fine.line_clock16(out["clock16"], out["fine_rate"], LINE["U"], LINE["D"], M_POS, M_POS).astype(np.int64)
    err = (int(np.abs(coarse - truth).max()), int(np.abs(fine - truth).max()))
    d = tuple(block_fix_metres(q_tgt, b, rows) for rows in (coarse, fine, truth))
    print("block %2d: coarse line k %s h %s; fine line clock16 %s rate %s moved %d; worst row error %d/16 -> %d/16; fix %.0f m -> %.0f m, "
          "true clocks %.0f m" % (b, out["clock"].tolist(), out["rate"].tolist(), out["clock16"].tolist(), out["fine_rate"].tolist(),
                                  int(out["fine"]["moved"]), err[0], err[1], d[0], d[1], d[2]))
    return d, err


def summarise(d, err):
    d, err = np.array(d, dtype=np.float64), np.array(err, dtype=np.float64)
    med, med_err = np.median(d, axis=0), np.median(err, axis=0)
    print("medians over %d blocks: fix under the coarse line %.1f m, the fine line %.1f m, the true clocks %.1f m (ratios %.2f and %.2f); "
          "worst row error coarse %.1f/16, fine %.1f/16 (ratio %.2f)" % (len(d), med[0], med[1], med[2], med[1] / med[0], med[1] / med[2],
                                                                         med_err[0], med_err[1], med_err[1] / med_err[0]))
    return med, med_err


def assert_measured_lines(med, med_err, true_fix_ratio=TRUE_FIX_RATIO):
    assert med[1] <= 0.5 * med[0]                              # 1. the refined fix against the coarse-line fix
    assert med_err[1] <= 0.5 * med_err[0]                      # 2. the refined worst row error against the coarse one
    assert med[1] <= 1.25 * true_fix_ratio * med[2]            # 3. ... against the true-clock fix: 25 % over the measured ratio


def test_fine_lines_keep_the_sub_sample_locate_its_resolution_past_the_block(oracle):
    """The measured case on the float64 pipeline's words, noise 0.5.  Measured with the numpy statement: the coarse line is
    (k, h) = (37, -52, 19), (3, -6, 2) in every block and the fine rates are (51, -90, 36), a few blocks one step off (true: 52,
    -88, 36); the worst row error over positions 12 .. 23, median over the twelve blocks, falls from 35/16 to 9/16 sample (ratio
    0.26) and the median fix of the target block from 516.6 m under the coarse line continued to 81.6 m under the fine line
    continued (ratio 0.16), 57.7 m under the true rows: TRUE_FIX_RATIO = 81.6 / 57.7 = 1.41, held with the project's 25 % margin.
    Every block's figures are printed."""
    from tdoa_amd import sync_drift_fine
    ref_delay = measured_case()[0]
    d, err = [], []
    for b in range(12):
        q_ref = float64_words(oracle, reference_windows_iq(oracle, b))
        q_tgt = float64_words(oracle, target_windows_iq(oracle, b))
        out = sync_drift_fine.sync_line_fine(q_ref, ref_delay, ML, LINE["G"], LINE["H"], LINE["D"], LINE["R"], LINE["U"], LINE["Rf"])
        assert int(out["fine"]["score_q"]) >= int(out["fine"]["start_q"]) > 0
        one = measure_block(b, q_tgt, out)
        d.append(one[0])
        err.append(one[1])
    assert_measured_lines(*summarise(d, err))
    # blocks 0 .. 5 alone, the blocks tests/test_gpu_sync_drift_fine.py runs as captures: their own measured ratio
    assert_measured_lines(*summarise(d[:6], err[:6]), true_fix_ratio=TRUE_FIX_RATIO_SIX)
