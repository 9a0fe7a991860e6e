"""CPU: the zoomed cell tracks (tdoa_process_locate_track_zoom; include/tdoa_mi355x.h, "zoomed cell tracks").  The entries and
the header's phrases, the boundary that needs no device, the binding's record against the parsed header, the numpy statement
(tdoa_amd.locate_track_zoom) against an enumeration of every fine path in Python integers, hand-worked cases, the five identities
of the header on random integers, and the two demonstrations: the fine clock lines' block fix (tests/test_sync_drift_fine_cpu.py)
in one statement, exactly, and the moving emitter of tests/test_locate_track_cpu.py against the brute force on the whole fine table.
statement(), random_case() and the demonstrations' helpers are shared with tests/test_gpu_locate_track_zoom.py, which runs the
kernels on the same words."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from test_locate_zoom_cpu import FINE_COLS, FINE_ROWS, _enumerate_cell, global_fine_table, pairs_of, small_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdoa_process_locate_track_zoom", "tdoa_group_process_locate_track_zoom", "tdoa_debug_locate_track_zoom_from_q")
COARSE_KEYS = ("track", "cells", "own", "lags", "corr", "total")
Z_KEYS = ("ztrack", "zcells", "zown", "zlags", "zcorr", "zmap", "ztotal")
KEYS = COARSE_KEYS + Z_KEYS
INTS = ("max_step", "min_separation", "Z", "H", "fine_step", "fine_separation")


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


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


# ---- the entries --------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import locate_track, locate_track_zoom
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessLocateTrackZoom(", "C.tdoa_process_locate_track_zoom(", "func (g *Group) ProcessLocateTrackZoom(",
                 "C.tdoa_group_process_locate_track_zoom("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_locate_track_zoom", "locate_track_zoom_from_q"):
        assert hasattr(capi.Context, method) and getattr(capi.Context, method).__doc__, method
    assert hasattr(capi.Group, "process_locate_track_zoom")
    assert locate_track_zoom.NAMES == KEYS and capi.CELL_TRACK_DTYPE == locate_track.CELL_TRACK_DTYPE
    for name in ("track_zoom_stacks", "track_zoom_upsampled", "backward", "window_scores"):
        assert callable(getattr(locate_track_zoom, name)), name
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("The coarse stage is tdoa_process_locate_track(windows_per_stack, max_step, min_separation) unchanged",
                   "The first six outputs are that call's bytes", "The fine planes are not judged",
                   "position j of track t is stack sid = t L + j", "w_j is zmap",
                   "F_{L-1}[pos] = w_{L-1}[pos]. F_j[pos] = -1 where w_j[pos] = -1.",
                   "it must lie inside that window (0 <= wa', wb' <= 2H), and a -1 there does not count",
                   "F_j[pos] = w_j[pos] + m. If no such position exists, F_j[pos] = -1: no continuation",
                   "ties go to the smaller rank(dr), then the smaller rank(dc)",
                   "Consecutive windows are offset by Z (C_{j+1} - C_j). With Z J > 2H + Jf they need not touch",
                   "f_0 is the position with the largest F_0, equal maxima: the smaller fine cell. f_{j+1} = f_j + E_j[f_j]",
                   "ztotal is F_0 in the coordinates of window 0",
                   "steps = the number of j with f_{j+1} != f_j", "score and runner_up are on the coarse track's scale, 2^-32 / sqrt(N_w)",
                   "F_0 >= 0 over positions with max(|row - row_0|, |col - col_0|) > fine_separation",
                   "its zmap and ztotal are -1 throughout", "A track whose largest F_0 is <= 0 gets the same zeros; its zmap and ztotal keep their words",
                   "1. L = 1: ztrack's cell, runner_cell, score_q, runner_q, score and runner_up are tdoa_process_locate_zoom's tdoa_zoom fields",
                   "2. J = 0 and Jf = 0: all windows of a track coincide and ztotal = the sum over j of zmap_j word for word",
                   "3. score_q = ztotal[pos(f_0)] = the sum over j of zown[j]; consecutive zcells are at most Jf fine rows and columns apart",
                   "4. With the fine table equal to the table, Z = 1 and Jf = J, ztrack.score_q = track.score_q for any H",
                   "5. ztrack.score_q is at most the score of tdoa_process_locate_track with the fine table as the table and max_step = Jf",
                   "equals it whenever that brute-force track lies inside the windows",
                   "The graph's key is the tracks' words plus (Z, H, fine_step, fine_separation, n_cells_f, n_cols_f)",
                   "fine_step outside 0 .. 16, fine_separation < 1, a NULL ztrack_host",
                   "the steps E (2 bytes per stack and position) or ztotal do not fit",
                   "All argument checks happen before anything needs a device"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_the_later_table_states_the_headers_order_and_types(capi):
    """the binding's record of the search against the parsed header, as tests/test_capi_bindings_cpu.py holds the nine"""
    lib, protos = capi.load(), _prototypes()
    c_types = {"int": C.c_int, "int32_t *": C.POINTER(C.c_int32), "double *": C.POINTER(C.c_double), "int64_t *": C.POINTER(C.c_int64)}
    scalars = {"int32_t *": np.int32, "double *": np.float64, "int64_t *": np.int64}
    s = capi._search("locate_track_zoom")
    assert "locate_track_zoom" not in capi.SEARCHES and type(s) is type(capi.SEARCHES["locate_track"])
    assert s.track_len and not s.bare and s.stats == "track" and s.inputs == ()
    assert s.entries == {"own": NAMES[0], "group": NAMES[1], "q": NAMES[2]}
    assert s.ints == INTS and [o.key for o in s.outputs] == list(KEYS)
    assert [o.poison for o in s.outputs] == [False] * 6 + [True] * 7
    assert [o.want for o in s.outputs] == [None] * 5 + ["want_total"] + [None] * 5 + ["want_zmap", "want_ztotal"]
    for route, entry in s.entries.items():
        names = ["ctx", "q", "n_sets", "track_len", "n_stations", "n_w"] if route == "q" else ["ctx" if route == "own" else "g", "windows_per_stack"]
        names += list(s.ints) + [o.key if route == "q" else o.key + "_host" for o in s.outputs]
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
                assert ctype == "tdoa_cell_track *" and argtype is C.c_void_p, (entry, name)
            if k >= first_out:
                dtype = np.dtype(s.outputs[k - first_out].dtype)
                assert dtype == (capi.CELL_TRACK_DTYPE if ctype == "tdoa_cell_track *" else np.dtype(scalars[ctype])), (entry, name)
            elif name != "q" and k > 0:
                assert ctype == "int", (entry, name)
    # the flags' defaults: want_total follows the tracks' (off on the own and group routes, on from Q), the z planes are on
    import inspect
    for cls, method, total in ((capi.Context, "process_locate_track_zoom", False), (capi.Context, "locate_track_zoom_from_q", True),
                               (capi.Group, "process_locate_track_zoom", False)):
        p = inspect.signature(getattr(cls, method)).parameters
        assert (p["want_total"].default, p["want_zmap"].default, p["want_ztotal"].default) == (total, True, True), method


def _outputs(capi, n_sets, L, P, n_cells, H):
    s = capi._search("locate_track_zoom")
    out = capi._search_outputs(s, capi._shape_numbers({"H": H}, n_sets, 0, n_cells, L, P=P), dict(want_total=True, want_zmap=True, want_ztotal=True))
    return out, capi._search_ptrs(s, out)


def test_null_handles_and_bad_arguments_need_no_device(capi):
    lib = capi.load()
    q = np.zeros((2, 3, 7), dtype=np.int64)
    out, ptrs = _outputs(capi, 2, 2, 3, 4, 1)
    assert [out[k].shape for k in KEYS] == [(1,), (1, 2), (1, 2), (2, 3), (2, 3), (1, 4), (1,), (1, 2), (1, 2), (2, 3), (2, 3), (2, 9), (1, 9)]
    before = {k: v.tobytes() for k, v in out.items()}
    assert all(set(before[k]) == {0xA5} for k in Z_KEYS)
    pq = q.ctypes.data_as(C.POINTER(C.c_int64))
    for J, sep, Z, H, Jf, fsep in ((0, 1, 1, 1, 0, 1), (16, 2, 64, 64, 16, 3), (-1, 1, 1, 1, 0, 1), (17, 1, 1, 1, 0, 1), (0, 0, 1, 1, 0, 1), (0, 1, 0, 1, 0, 1),
                                   (0, 1, 65, 1, 0, 1), (0, 1, 1, -1, 0, 1), (0, 1, 1, 65, 0, 1), (0, 1, 1, 1, -1, 1), (0, 1, 1, 1, 17, 1), (0, 1, 1, 1, 0, 0)):
        assert lib.tdoa_process_locate_track_zoom(None, 0, J, sep, Z, H, Jf, fsep, *ptrs) == 1
        assert lib.tdoa_group_process_locate_track_zoom(None, 0, J, sep, Z, H, Jf, fsep, *ptrs) == 1
        assert lib.tdoa_debug_locate_track_zoom_from_q(None, pq, 2, 2, 3, 1, J, sep, Z, H, Jf, fsep, *ptrs) == 1
    assert lib.tdoa_process_locate_track_zoom(None, 0, 0, 1, 1, 1, 0, 1, *([None] * 13)) == 1
    assert {k: v.tobytes() for k, v in out.items()} == before            # nothing was written
    case = small_case(3, 4, 1)
    for kw in (dict(Z=0), dict(Z=65), dict(H=-1), dict(H=65), dict(Jf=-1), dict(Jf=17), dict(fsep=0), dict(J=17), dict(sep=0), dict(L=4)):
        with pytest.raises(ValueError):                                  # the numpy statement refuses the same ranges
            statement(case, **dict(dict(L=3, J=0, H=1, Jf=0), **kw))


# ---- the statement ------------------------------------------------------------------------------------------------------------
def statement(case, L, J, H, Jf, U=1, sep=1, fsep=1, Z=None, fine=None, n_cols_f=None, q=None, clock="case", n_w=None):
    """tdoa_amd.locate_track_zoom on a case of small_case()'s form -> the thirteen outputs"""
    from tdoa_amd import locate_track_zoom
    return locate_track_zoom.track_zoom_upsampled(
        case["q"] if q is None else q, case["table"], case["n_cols"], case["fine"] if fine is None else fine,
        case["n_cols_f"] if n_cols_f is None else n_cols_f, case["ml"], L, J, case["Z"] if Z is None else Z, H, Jf, U, sep, fsep,
        case["n_w"] if n_w is None else n_w, case["clock"] if isinstance(clock, str) else clock)


def _rank(x):
    return 2 * abs(x) - (x > 0)


def _enumerate_track(case, fine_qs, t, L, coarse_cells, H, Jf, U, fsep):
    """track t by the definition, in Python integers: every window position's score, then every path through the windows;
    fine_qs[set][pair] = upsample.upsample_exact of the set's rows ->
    (zmap [L][n_pos], ztotal [n_pos], record as a dict or None, fine cells, own scores, lags [L][P], words [L][P])"""
    ml, Z, n_cols, n_cols_f, n_cells_f = case["ml"], case["Z"], case["n_cols"], case["n_cols_f"], len(case["fine"])
    side = 2 * H + 1
    n_pos = side * side
    w, where, detail = [], [], []
    for j in range(L):
        sid = t * L + j
        fine_q = fine_qs[sid]
        clock = None if case["clock"] is None else case["clock"][sid]
        c = int(coarse_cells[j])
        w.append([-1] * n_pos)
        where.append([None] * n_pos)
        detail.append([None] * n_pos)
        for pos in range(n_pos):
            row, col = Z * (c // n_cols) - H + pos // side, Z * (c % n_cols) - H + pos % side
            where[j][pos] = (row, col)
            if row < 0 or not 0 <= col < n_cols_f or row * n_cols_f + col >= n_cells_f:
                continue
            s = _enumerate_cell(case["fine"][row * n_cols_f + col], clock, fine_q, U, ml)
            w[j][pos], detail[j][pos] = s[0], s
    at = [{rc: pos for pos, rc in enumerate(where[j])} for j in range(L)]
    paths = {}                                                           # start position -> [(total, tie key, path)]
    for p0 in range(n_pos):
        if w[0][p0] < 0:
            continue
        stack = [(w[0][p0], (), (p0,))]
        while stack:
            total, key, path = stack.pop()
            j = len(path)
            if j == L:
                paths.setdefault(p0, []).append((total, key, path))
                continue
            row, col = where[j - 1][path[-1]]
            for dr, dc in itertools.product(range(-Jf, Jf + 1), repeat=2):
                nxt = at[j].get((row + dr, col + dc))
                if nxt is not None and w[j][nxt] >= 0:
                    stack.append((total + w[j][nxt], key + ((_rank(dr), _rank(dc)),), path + (nxt,)))
    ztotal = [max(x[0] for x in paths[p]) if p in paths else -1 for p in range(n_pos)]
    top = max(ztotal)
    if top <= 0:
        return w, ztotal, None, None, None, None, None
    cell_of = lambda j, pos: where[j][pos][0] * n_cols_f + where[j][pos][1]      # noqa: E731
    f0 = min((p for p in range(n_pos) if ztotal[p] == top), key=lambda p: cell_of(0, p))
    best = min((x for x in paths[f0] if x[0] == top), key=lambda x: x[1])[2]      # the first in the order (rank(dr), rank(dc)), step by step
    cells = [cell_of(j, pos) for j, pos in enumerate(best)]
    far = [p for p in range(n_pos) if ztotal[p] >= 0 and max(abs(where[0][p][0] - where[0][f0][0]), abs(where[0][p][1] - where[0][f0][1])) > fsep]
    rec = dict(cell=cells[0], positions=L, steps=sum(a != b for a, b in zip(cells, cells[1:])), score_q=top, runner_cell=0, runner_q=0)
    if far:
        rq = max(ztotal[p] for p in far)
        rec["runner_q"], rec["runner_cell"] = rq, min(cell_of(0, p) for p in far if ztotal[p] == rq)
    return (w, ztotal, rec, cells, [w[j][pos] for j, pos in enumerate(best)], [detail[j][pos][2] for j, pos in enumerate(best)],
            [detail[j][pos][3] for j, pos in enumerate(best)])


@pytest.mark.parametrize("U", (1, 4))
@pytest.mark.parametrize("S, ml, clocked, short", [(3, 4, False, False), (4, 9, True, False), (4, 9, False, True), (3, 4, True, True)])
def test_the_statement_against_an_enumeration_of_every_fine_path(S, ml, clocked, short, U):
    """six sets as two tracks of three on the 5 x 7 table and the 13 x 19 fine table, Z = 3; the coarse tracks are the cell tracks'
    statement's (tests/test_locate_track_cpu.py holds it).  J = 0 stands still, J = 1 moves by up to three fine cells a stack, and
    with J = 16 the first track jumps between the planted corners: windows that do not touch"""
    from tdoa_amd import stacking, upsample
    planted = small_case(S, ml, 60 + 7 * S + ml, clocked, short)
    # the planted words hold a track to its plateau; the same tables under random words alone let it wander
    wander = dict(planted, q=np.random.default_rng(ml + S).integers(-2 ** 40, 2 ** 40, size=planted["q"].shape, dtype=np.int64))
    seen = dict(found=0, moved=0, apart=0, dead=0, runner=0, outside=0)
    for case, configs in ((planted, ((0, 0, 0, 1), (0, 2, 0, 1), (0, 1, 2, 1), (1, 2, 1, 2), (1, 0, 2, 1), (16, 2, 2, 1), (16, 1, 0, 1))),
                          (wander, ((1, 1, 1, 1), (1, 2, 2, 1), (2, 2, 1, 2), (0, 1, 2, 1)))):
        fine_qs = [[upsample.upsample_exact(row, U) for row in rows] for rows in case["q"]]
        for J, H, Jf, fsep in configs:
            out = dict(zip(KEYS, statement(case, 3, J, H, Jf, U, 1, fsep)))
            assert out["zmap"].shape == (6, (2 * H + 1) ** 2) and out["ztotal"].shape == (2, (2 * H + 1) ** 2) and out["ztrack"].dtype.itemsize == 48
            n_all = 3 * case["n_w"]
            for t in range(2):
                assert int(out["track"][t]["score_q"]) > 0
                zmap, ztotal, rec, cells, own, lags, words = _enumerate_track(case, fine_qs, t, 3, out["cells"][t], H, Jf, U, fsep)
                assert out["zmap"][3 * t:3 * t + 3].tolist() == zmap and out["ztotal"][t].tolist() == ztotal, (J, H, Jf, t)
                seen["dead"] += any(-1 in row for row in zmap)
                if rec is None:
                    seen["apart"] += max(ztotal) == -1
                    assert out["ztrack"][t].tobytes() == bytes(48) and not out["zcells"][t].any() and not out["zown"][t].any()
                    assert not out["zlags"][3 * t:3 * t + 3].any() and not out["zcorr"][3 * t:3 * t + 3].any()
                    continue
                for name, value in rec.items():
                    assert int(out["ztrack"][t][name]) == value, (J, H, Jf, t, name)
                assert out["zcells"][t].tolist() == cells and out["zown"][t].tolist() == own
                assert out["zlags"][3 * t:3 * t + 3].tolist() == lags
                for j in range(3):
                    assert out["zcorr"][3 * t + j].tolist() == [0.0 if x is None else float(stacking.from_fixed(np.int64(x), case["n_w"])) for x in words[j]]
                assert float(out["ztrack"][t]["score"]) == float(stacking.from_fixed(np.int64(rec["score_q"]), n_all))
                assert float(out["ztrack"][t]["runner_up"]) == float(stacking.from_fixed(np.int64(rec["runner_q"]), n_all))
                seen["found"] += 1
                seen["moved"] += rec["steps"] > 0
                seen["runner"] += rec["runner_q"] > 0
                seen["outside"] += any(x is None for row in words for x in row)
    print(seen)
    assert seen["found"] >= 8 and seen["moved"] > 0 and seen["apart"] > 0 and seen["dead"] > 0 and seen["runner"] > 0, seen


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------------
def _two_station_case(lags_f, rows_f, q_rows, Z, n_w=1):
    """two stations, max_lag 4: the fine table's cells have the lags lags_f (row-major, rows_f rows), the table is every Z-th fine
    cell; q_rows [n_sets][7] words in units of 2^32 at the lags -3 .. 3 -> a case of small_case()'s form"""
    f = np.asarray(lags_f, dtype=np.int64).reshape(rows_f, -1)
    fine = np.stack([np.zeros(f.size, dtype=np.int64), 16 * f.reshape(-1)], axis=1).astype(np.int32)
    coarse = f[::Z, ::Z]
    table = np.stack([np.zeros(coarse.size, dtype=np.int64), 16 * coarse.reshape(-1)], axis=1).astype(np.int32)
    return dict(q=(np.asarray(q_rows, dtype=np.int64) << 32)[:, None, :], table=table, n_cols=coarse.shape[1], fine=fine, n_cols_f=f.shape[1],
                clock=None, ml=4, n_w=n_w, S=2, Z=Z)


def test_hand_worked_cases():
    one = 1 << 32
    # (a) a window hanging over the table's corner.  The 3 x 3 fine table has the lags [[0, 1, 2], [-1, 0, 1], [-2, 3, -3]], Z = 2,
    # the 2 x 2 table the lags [[0, 2], [-2, -3]].  One stack with the words 1 .. 7 at the lags -3 .. 3: the coarse scores are 4, 6,
    # 2, 1, the coarse cell is 1 = (0, 1), the window's origin the fine (-1, 1): its first row and its last column hang over
    case = _two_station_case([0, 1, 2, -1, 0, 1, -2, 3, -3], 3, [[1, 2, 3, 4, 5, 6, 7]], 2)
    out = dict(zip(KEYS, statement(case, 1, 0, 1, 0)))
    assert out["cells"].tolist() == [[1]] and out["zmap"].tolist() == [[-1, -1, -1, 5 * one, 6 * one, -1, 4 * one, 5 * one, -1]]
    assert out["ztotal"].tolist() == out["zmap"].tolist() and out["zcells"].tolist() == [[2]] and out["zown"].tolist() == [[6 * one]]
    rec = out["ztrack"][0]
    assert (int(rec["cell"]), int(rec["positions"]), int(rec["steps"]), int(rec["score_q"])) == (2, 1, 0, 6 * one)
    assert (int(rec["runner_cell"]), int(rec["runner_q"])) == (0, 0)     # every competing position is within one of (0, 2)
    assert out["zlags"].tolist() == [[2]] and out["zcorr"].tolist() == [[6.0]] and float(rec["score"]) == 6.0
    # (b) two windows that do not touch.  A 1 x 7 fine table with the lags 0, 1, 2, 3, 2, 1, 0 and Z = 3: the table's cells are the
    # fine cells 0, 3, 6 with the lags 0, 3, 0.  Stack 0 has its word at the lag 0 (coarse cells 0 and 2 tie: the smaller, 0),
    # stack 1 at the lag 3 (coarse cell 1).  J = 1: the coarse track is 0 -> 1, and with H = 0 the windows are the fine cells 0 and 3,
    # three apart: with Jf = 2 there is no continuation -- all of F_0 is -1 and the record is zero, zmap keeps its words; Jf = 3 joins
    case = _two_station_case([0, 1, 2, 3, 2, 1, 0], 1, [[0, 0, 0, 9, 0, 0, 0], [0, 0, 0, 0, 0, 0, 5]], 3)
    out = dict(zip(KEYS, statement(case, 2, 1, 0, 2)))
    assert out["cells"].tolist() == [[0, 1]] and int(out["track"][0]["score_q"]) == 14 * one
    assert out["zmap"].tolist() == [[9 * one], [5 * one]] and out["ztotal"].tolist() == [[-1]]
    assert out["ztrack"].tobytes() == bytes(48) and not out["zcells"].any() and not out["zown"].any() and not out["zlags"].any() and not out["zcorr"].any()
    out = dict(zip(KEYS, statement(case, 2, 1, 0, 3)))
    assert out["ztotal"].tolist() == [[14 * one]] and out["zcells"].tolist() == [[0, 3]] and int(out["ztrack"][0]["steps"]) == 1
    # ... and with H = 1 and Jf = 1 the windows are the fine cells (-1) 0 1 and 2 3 4: 1 -> 2 joins them.  w_0 = -1, 9, 0 and
    # w_1 = 0, 5, 0 (the lags 2, 3, 2): F_0 = -1 (dead), -1 (no position of window 1 within one of the fine cell 0), 0 + 0
    out = dict(zip(KEYS, statement(case, 2, 1, 1, 1)))
    assert out["zmap"].tolist() == [[-1, -1, -1, -1, 9 * one, 0, -1, -1, -1], [-1, -1, -1, 0, 5 * one, 0, -1, -1, -1]]
    assert out["ztotal"].tolist() == [[-1, -1, -1, -1, -1, 0, -1, -1, -1]]
    assert out["ztrack"].tobytes() == bytes(48) and not out["zcells"].any()      # the largest F_0 is 0: the zero record, the planes keep their words
    # (c) a window with some dead positions, L = 2, J = 0, Jf = 1: case (a)'s tables, both stacks with the words 1 .. 7.  The windows
    # coincide; F_1 = w, F_0[pos] = w[pos] + the largest w within one: 6 everywhere (the window is 2 x 2 competing cells)
    case = _two_station_case([0, 1, 2, -1, 0, 1, -2, 3, -3], 3, [[1, 2, 3, 4, 5, 6, 7]] * 2, 2)
    out = dict(zip(KEYS, statement(case, 2, 0, 1, 1)))
    assert out["cells"].tolist() == [[1, 1]]
    assert out["ztotal"].tolist() == [[-1, -1, -1, 11 * one, 12 * one, -1, 10 * one, 11 * one, -1]]
    assert out["zcells"].tolist() == [[2, 2]] and out["zown"].tolist() == [[6 * one, 6 * one]] and int(out["ztrack"][0]["steps"]) == 0
    assert int(out["ztrack"][0]["score_q"]) == 12 * one and float(out["ztrack"][0]["score"]) == 12.0 / np.sqrt(2.0)
    # (d) a tie decided by rank(dr) before rank(dc), on the recurrence itself: one 3 x 3 window twice, Jf = 1.  F_1 has the value 5 at
    # (2, 0) and at (0, 1): from the centre these are (dr, dc) = (+1, -1), ranks (1, 2), and (-1, 0), ranks (2, 0) -- the first wins
    from tdoa_amd import locate_track_zoom
    w = np.zeros((2, 9), dtype=np.int64)
    w[1, 6] = w[1, 1] = 5
    F, E = locate_track_zoom.backward(w, [(0, 0), (0, 0)], 1, 1)
    assert E[0, 4].tolist() == [1, -1] and F[0].tolist() == [5, 5, 5, 5, 5, 5, 5, 5, 0]
    assert E[0, 0].tolist() == [0, 1] and E[0, 3].tolist() == [1, 0] and E[0, 8].tolist() == [0, 0] and F[0][8] == 0 + 0
    # ... the same plane one row and two columns on: window 1's origin is (1, 2), so its 5s lie at the fine (3, 2) and (1, 3) and its
    # zeros on the fine rows 1 .. 3, columns 2 .. 4.  Window 0's column 0 reaches none of them; (2, 2) reaches both 5s, as (+1, 0) and
    # (-1, +1): the first; the centre reaches zeros only, the first of them (0, +1)
    F, E = locate_track_zoom.backward(w, [(0, 0), (1, 2)], 1, 1)
    assert F[0].tolist() == [-1, 0, 5, -1, 0, 5, -1, 5, 5] and E[0, 8].tolist() == [1, 0] and E[0, 4].tolist() == [0, 1] and E[0, 0].tolist() == [0, 0]


# ---- the identities of the header -----------------------------------------------------------------------------------------------
IDENTITY_CASES = (((3, 4, 4, 5, 3, 21), {}), ((4, 9, 3, 6, 2, 22), dict(clocked=False, short=4)))      # random_case's arguments


def random_case(S, ml, rows, cols, Z, seed, n_sets=6, clocked=True, short=0, n_w=None):
    """a random table of rows x cols cells and a fine table at Z cells per cell, fine (Z r, Z c) = coarse (r, c), short: cells cut
    from the fine table's last row; random words, clocks and windows per set (n_w: the same number in every set) -> a case of
    small_case()'s form"""
    rng = np.random.default_rng(seed)
    rows_f, cols_f = (rows - 1) * Z + 1, (cols - 1) * Z + 1
    fine = rng.integers(-16 * ml, 16 * ml + 1, size=(rows_f, cols_f, S)).astype(np.int32)
    table = np.ascontiguousarray(fine[::Z, ::Z].reshape(-1, S))
    fine = fine.reshape(-1, S)[:rows_f * cols_f - short]
    P = S * (S - 1) // 2
    return dict(q=rng.integers(-2 ** 40, 2 ** 40, size=(n_sets, P, 2 * ml - 1), dtype=np.int64), table=table, n_cols=cols,
                fine=np.ascontiguousarray(fine), n_cols_f=cols_f, clock=rng.integers(-40, 41, size=(n_sets, S)).astype(np.int32) if clocked else None,
                ml=ml, n_w=rng.integers(1, 4, size=n_sets) if n_w is None else n_w, S=S, Z=Z)


def check_identities(case, run, run_zoom, run_track, U):
    """identities 1 - 5 of the header on any implementation: run(case, L, J, H, Jf, U, **kw) -> the thirteen outputs by name,
    run_zoom(case, H, U) -> the zoom locate's eight by name, run_track(case, table, n_cols, L, J, U) -> the cell tracks' six by name"""
    Z, n_cols_f = case["Z"], case["n_cols_f"]
    n_sets = len(case["q"])
    # 1. L = 1: the zoom locate
    for H in (0, 2):
        out, zoom = run(case, 1, 3, H, 2, U, fsep=2), run_zoom(case, H, U, fsep=2)
        for name in ("cell", "runner_cell", "score_q", "runner_q", "score", "runner_up"):
            assert out["ztrack"][name].tobytes() == zoom["zoom"][name].tobytes(), name
        assert out["zlags"].tobytes() == zoom["zlags"].tobytes() and out["zcorr"].tobytes() == zoom["zcorr"].tobytes()
        assert out["zmap"].tobytes() == zoom["zmap"].tobytes() == out["ztotal"].tobytes()
    for L in (2, 3):
        n_tracks = n_sets // L
        # 2. J = 0 and Jf = 0: the sum of the windows' maps
        out = run(case, L, 0, 2, 0, U)
        zmap = out["zmap"].reshape(n_tracks, L, -1)
        assert (out["cells"] == out["cells"][:, :1]).all() and ((zmap == -1) == (zmap[:, :1] == -1)).all()
        assert (out["ztotal"] == np.where(zmap[:, 0] == -1, -1, zmap.sum(axis=1))).all()
        assert (out["ztrack"]["steps"] == 0).all() and (out["zcells"] == out["zcells"][:, :1]).all()
        # 3. the record, the walk and the planes agree (windows two coarse cells apart need not touch: a zero record is all zeros)
        n_found = 0
        for J, H, Jf in ((1, 3, 2), (2, 2, 1), (1, 4, 16)):
            out = run(case, L, J, H, Jf, U)
            found = out["ztrack"]["score_q"] > 0
            n_found += int(found.sum())
            r, c = np.divmod(out["zcells"], n_cols_f)
            assert (np.abs(np.diff(r, axis=1)) <= Jf).all() and (np.abs(np.diff(c, axis=1)) <= Jf).all()
            assert (out["ztrack"]["score_q"] == out["zown"].sum(axis=1)).all() and (out["ztrack"]["steps"] == (np.diff(out["zcells"], axis=1) != 0).sum(axis=1)).all()
            assert (out["ztrack"]["score_q"][found] == out["ztotal"].max(axis=1)[found]).all() and (out["ztrack"]["positions"][found] == L).all()
            for t in np.flatnonzero(found):
                r0, c0 = Z * (out["cells"][t, 0] // case["n_cols"]) - H, Z * (out["cells"][t, 0] % case["n_cols"]) - H
                pos = (r[t, 0] - r0) * (2 * H + 1) + (c[t, 0] - c0)
                assert out["ztotal"][t, pos] == out["ztrack"]["score_q"][t]
        assert n_found >= n_tracks
        # 4. the fine table equal to the table, Z = 1, Jf = J: the coarse track's score for any H
        flat = dict(case, fine=case["table"], n_cols_f=case["n_cols"], Z=1)
        for J, H in ((1, 0), (2, 1), (2, 5)):
            out = run(flat, L, J, H, J, U)
            assert (out["ztrack"]["score_q"] == out["track"]["score_q"]).all(), (L, J, H)
            assert (out["ztrack"]["score"] == out["track"]["score"]).all()
        # 5. never more than the brute force on the whole fine table, and equal whenever its track lies inside the windows
        inside = 0
        for J, H, Jf in ((1, 2, 1), (1, 4, 2), (2, 64, 3)):
            out, brute = run(case, L, J, H, Jf, U), run_track(case, case["fine"], n_cols_f, L, Jf, U)
            assert (out["ztrack"]["score_q"] <= brute["track"]["score_q"]).all()
            br, bc = np.divmod(brute["cells"], n_cols_f)
            cr, cc = np.divmod(out["cells"], case["n_cols"])
            for t in range(n_tracks):
                if (np.maximum(np.abs(br[t] - Z * cr[t]), np.abs(bc[t] - Z * cc[t])) <= H).all() and int(out["track"]["score_q"][t]) > 0:
                    inside += 1
                    assert int(out["ztrack"]["score_q"][t]) == int(brute["track"]["score_q"][t])
                    if H == 64:                                          # the windows hold the whole fine table: the same track, cell for cell
                        assert out["zcells"][t].tolist() == brute["cells"][t].tolist() and out["zown"][t].tolist() == brute["own"][t].tolist()
        assert inside >= n_tracks                                        # (H = 64 holds the whole fine table)


@pytest.mark.parametrize("U", (1, 4))
def test_identities_on_random_integers(U):
    from tdoa_amd import locate_track, locate_zoom, upsample

    def run(case, L, J, H, Jf, U, fsep=1):
        return dict(zip(KEYS, statement(case, L, J, H, Jf, U, 1, fsep)))

    def run_zoom(case, H, U, fsep=1):
        return dict(zip(locate_zoom.NAMES, locate_zoom.zoom_upsampled(case["q"], case["table"], case["n_cols"], case["fine"], case["n_cols_f"],
                                                                      case["ml"], case["Z"], H, U, 1, fsep, case["n_w"], case["clock"])))

    def run_track(case, table, n_cols, L, J, U):
        t, k, _, ml_u = upsample.scaled_args(table, case["clock"], 0, case["ml"], U)
        return dict(zip(COARSE_KEYS, locate_track.track_stacks(upsample.upsample(case["q"], U), t, n_cols, ml_u, L, J, 1, case["n_w"], k)))

    for args, kw in IDENTITY_CASES:
        check_identities(random_case(*args, **kw), run, run_zoom, run_track, U)


# ---- the demonstrations -----------------------------------------------------------------------------------------------------------
DEMO = dict(Z=8, H=16, U=16, J=0, Jf=0)                   # the block fix of tests/test_sync_drift_fine_cpu.py in one statement


def block_fix_two_steps(q_tgt, rows16, coarse):
    """block_fix_metres of tests/test_sync_drift_fine_cpu.py with its steps kept: (coarse cell of the J = 0 track on whole lags, the
    second step's position on the host-built 33 x 33 grid around it)"""
    from tdoa_amd import locate_track, upsample
    from test_locate_upsample_cpu import FINE_SIDE, ML, fine_table
    from test_sync_drift_fine_cpu import LINE, M_POS
    rows16 = np.asarray(rows16, dtype=np.int64)
    cell = int(locate_track.track_stacks(q_tgt, coarse, 64, ML, M_POS, 0, 1, 1, rows16)[0]["cell"][0])
    t, kk, _, ml = upsample.scaled_args(fine_table(cell), rows16, 0, ML, LINE["U"])
    return cell, int(locate_track.track_stacks(upsample.upsample(q_tgt, LINE["U"]), t, FINE_SIDE, ml, M_POS, 0, 1, 1, kk)[0]["cell"][0])


def compare_block_fix(b, q_tgt, rows16, out, coarse, fine, n_cols_f):
    """One block under one set of clock rows: out, the thirteen outputs by name of the call with DEMO's arguments on that block as one
    track, against the two-step fix.  -> (covered: the coarse cells agree and the global fine table's delays over the window equal
    the host-built grid's; the call's fix in metres; the two-step fix in metres).  Where covered, the positions must be equal"""
    from test_locate_upsample_cpu import FINE, FINE_SIDE, POSITIONS, fine_position, fine_table, metres
    from test_locate_zoom_cpu import global_position
    cell, f = block_fix_two_steps(q_tgt, rows16, coarse)
    zc = int(out["ztrack"]["cell"][0])
    row, col = divmod(zc, n_cols_f)
    d_call, d_two = metres(POSITIONS[b], global_position(row, col)), metres(POSITIONS[b], fine_position(cell, f))
    r0, c0 = FINE * (cell // 64) - DEMO["H"], FINE * (cell % 64) - DEMO["H"]
    covered = int(out["cells"][0, 0]) == cell and r0 >= 0 and c0 >= 0 and r0 + FINE_SIDE <= len(fine) // n_cols_f and c0 + FINE_SIDE <= n_cols_f
    if covered:
        window = fine.reshape(-1, n_cols_f, 4)[r0:r0 + FINE_SIDE, c0:c0 + FINE_SIDE].reshape(-1, 4)
        covered = bool((window == fine_table(cell)).all())
    if covered:
        assert (row - r0, col - c0) == divmod(f, FINE_SIDE), (b, divmod(zc, n_cols_f), cell, f)
        assert int(out["ztrack"]["steps"][0]) == 0 and (out["zcells"][0] == zc).all()
    return covered, d_call, d_two


def test_the_block_fix_in_one_statement(oracle):
    """Blocks 0 .. 5 of the measured case of tests/test_sync_drift_fine_cpu.py, the target block as one track of twelve one-window
    stacks under the coarse line continued, the fine line continued and the true rows: J = 0 and Jf = 0 on the 48 x 64 table and the
    global 377 x 505 fine table, Z = 8, H = 16, U = 16.  Wherever the coarse stage on the upsampled words picks the cell the two-step
    fix picks on whole lags and the global table's delays over the window are the host-built grid's, f_0 is the two-step fix's
    position: an identity.  Measured: 10 of the 18 (block, rows) pairs are covered -- in seven the global table, laid from the
    area's corner, differs from the grid laid from the cell's centre by one sixteenth in some delay, and under block 1's coarse line
    the upsampled coarse stage picks another cell (3 962 m against 485 m) -- and the fix is the same to the metre in 17 of 18.  The
    medians over the six blocks under the fine line and the true rows are that test's 94.7 m and 43.8 m from either; under the
    coarse line 944.3 m from the call, 674.0 m from the two steps."""
    from tdoa_amd import sync_drift, sync_drift_fine
    from test_locate_upsample_cpu import ML, coarse_table
    from test_sync_drift_fine_cpu import (LINE, M_POS, float64_words, measured_case, reference_windows_iq, target_windows_iq, true_rows16)
    ref_delay = measured_case()[0]
    coarse = coarse_table()
    fine, n_cols_f = global_fine_table()
    covered, d_call, d_two = 0, [], []
    for b in range(6):
        q_ref = float64_words(oracle, reference_windows_iq(oracle, b))
        q_tgt = float64_words(oracle, target_windows_iq(oracle, b))
        line = sync_drift_fine.sync_line_fine(q_ref, ref_delay, ML, LINE["G"], LINE["H"], LINE["D"], LINE["R"], LINE["U"], LINE["Rf"])
        rows = (sync_drift.line_clock(line["clock"], line["rate"], LINE["D"], M_POS, M_POS).astype(np.int64),
                sync_drift_fine.line_clock16(line["clock16"], line["fine_rate"], LINE["U"], LINE["D"], M_POS, M_POS).astype(np.int64),
                true_rows16(M_POS, M_POS))
        a, c = [], []
        for rows16 in rows:
            case = dict(q=q_tgt, table=coarse, n_cols=64, fine=fine, n_cols_f=n_cols_f, ml=ML, n_w=1, Z=DEMO["Z"], clock=rows16)
            out = dict(zip(KEYS, statement(case, M_POS, DEMO["J"], DEMO["H"], DEMO["Jf"], DEMO["U"])))
            one = compare_block_fix(b, q_tgt, rows16, out, coarse, fine, n_cols_f)
            covered += one[0]
            a.append(one[1])
            c.append(one[2])
        print("block %d: the call's fix under the coarse line %.0f m, the fine line %.0f m, the true rows %.0f m; the two-step fix %.0f m, %.0f m, %.0f m"
              % ((b,) + tuple(a) + tuple(c)))
        d_call.append(a)
        d_two.append(c)
    med_call, med_two = np.median(np.array(d_call), axis=0), np.median(np.array(d_two), axis=0)
    print("covered %d of 18; medians over six blocks: the call %.1f m, %.1f m, %.1f m; the two-step fix %.1f m, %.1f m, %.1f m"
          % ((covered,) + tuple(med_call) + tuple(med_two)))
    same = sum(abs(x - y) < 0.5 for a, c in zip(d_call, d_two) for x, y in zip(a, c))       # (the two grids' latitudes differ in the last bits)
    print("the same fix to the metre in %d of 18" % same)
    assert covered == COVERED and same >= covered                        # (a covered pair has the same position: compare_block_fix)
    assert [round(x, 1) for x in med_call[1:]] == [round(x, 1) for x in med_two[1:]] == [94.7, 43.8]      # that test's numbers over six blocks


COVERED = 10                                              # measured (printed above); the equality holds wherever a pair is covered


def near_path(cells, n_cols_f, path, Z):
    """the stacks whose fine cell lies within Z / 2 fine rows and columns of Z x the planted coarse cell"""
    r, c = np.divmod(np.asarray(cells, dtype=np.int64), n_cols_f)
    want = Z * np.asarray(path, dtype=np.int64)
    return int((np.maximum(np.abs(r - want[:, 0]), np.abs(c - want[:, 1])) <= Z // 2).sum())


MOVING_ZOOM = dict(J=1, Z=8, H=16, Jf=8)
MOVING_NEAR = (11, 6)                                     # (the call, the brute force) stacks near the planted path, measured


def test_a_moving_emitter_followed_on_the_fine_table(oracle, U=1):
    """The MOVING case of tests/test_locate_track_cpu.py (one coarse row and column per stack, noise 0.7, twelve one-window stacks,
    whole lags) with J = 1, the global 377 x 505 fine table, Z = 8, H = 16 and Jf = 8: identity 5 against the brute force, the cell
    tracks' statement on the whole fine table with max_step 8.  Measured: the brute-force track leaves the windows and scores 0.5 %
    more (539 800 943 098 against 536 937 884 427) -- on noise: 6 of its 12 fine cells lie within 4 fine cells of the planted path,
    11 of 12 of the call's, as 11 of 12 of the coarse track's cells are the planted ones.  (Run once with U = 16, where the coarse
    track has 7 of 12: the call 5 of 12, the brute force 0 of 12.)"""
    from tdoa_amd import locate_track, upsample
    from test_locate_track_cpu import MOVING, _float64_q, track_windows
    from test_locate_upsample_cpu import ML, coarse_table
    q = _float64_q(oracle, track_windows(oracle, **MOVING))
    fine, n_cols_f = global_fine_table()
    a = MOVING_ZOOM
    case = dict(q=q, table=coarse_table(), n_cols=64, fine=fine, n_cols_f=n_cols_f, ml=ML, n_w=1, Z=a["Z"], clock=None)
    out = dict(zip(KEYS, statement(case, 12, a["J"], a["H"], a["Jf"], U)))
    t, _, _, ml_u = upsample.scaled_args(fine, None, 0, ML, U)
    brute = dict(zip(COARSE_KEYS, locate_track.track_stacks(upsample.upsample(q, U), t, n_cols_f, ml_u, 12, a["Jf"], 1, 1)))
    assert int(out["ztrack"]["score_q"][0]) <= int(brute["track"]["score_q"][0])
    br, bc = np.divmod(brute["cells"][0], n_cols_f)
    cr, cc = np.divmod(out["cells"][0], 64)
    inside = bool((np.maximum(np.abs(br - a["Z"] * cr), np.abs(bc - a["Z"] * cc)) <= a["H"]).all())
    near = near_path(out["zcells"][0], n_cols_f, MOVING["path"], a["Z"]), near_path(brute["cells"][0], n_cols_f, MOVING["path"], a["Z"])
    print("U = %d: the brute-force track inside the windows: %s; score %d against %d; near the planted path: the call %d of 12, the brute "
          "force %d of 12, the coarse track's cells %d of 12; steps %d against %d"
          % (U, inside, out["ztrack"]["score_q"][0], brute["track"]["score_q"][0], near[0], near[1],
             int((out["cells"][0] == np.array([r * 64 + c for r, c in MOVING["path"]])).sum()), out["ztrack"]["steps"][0], brute["track"]["steps"][0]))
    if inside:
        assert int(out["ztrack"]["score_q"][0]) == int(brute["track"]["score_q"][0])
    if out["zcells"][0].tolist() == brute["cells"][0].tolist():          # where the paths agree the count is no lower than the brute force's
        assert near[0] >= near[1]
    assert near == MOVING_NEAR
