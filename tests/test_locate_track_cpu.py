"""CPU: the numpy statement of the cell tracks (tdoa_amd.locate_track; include/tdoa_mi355x.h, "cell tracks") against an
enumeration of every path on tiny grids, on hand-worked tie cases, on the identities the header states, and on the two noisy
cases the feature exists for; sync.ramp_clock against exact fractions; and the boundary of the entry points that needs no
device.  hand_cases(), track_windows(), STILL and MOVING are shared with tests/test_gpu_locate_track.py, which runs the
kernels on the same words."""
import ctypes as C
import itertools
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from test_locate_cpu import FS, GRID, PAIRS4, ST4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdoa_process_locate_track", "tdoa_debug_locate_track_from_q", "tdoa_group_process_locate_track")


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import locate_track
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_locate_track", "locate_track_from_q"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.Group, "process_locate_track")
    # the record: the fields of the header in their order, 48 bytes, no padding
    assert capi.CELL_TRACK_DTYPE == locate_track.CELL_TRACK_DTYPE and capi.CELL_TRACK_DTYPE.itemsize == 48
    m = re.search(r"typedef struct \{([^}]*)\} tdoa_cell_track;", hdr)
    fields = re.findall(r"\b(int32_t|int64_t|double)\s+([^;]+);", m.group(1))
    assert [n.strip() for _, names in fields for n in names.split(",")] == list(capi.CELL_TRACK_DTYPE.names)
    assert [t for t, _ in fields] == ["int32_t", "int32_t", "int64_t", "double"]
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("T_{L-1}[c] = s_{L-1}[c]", "Ties in D_j: the smaller rank(dr), then the smaller rank(dc)",
                   "L_{j+1} = L_j + D_j[L_j].", "If max T_0 = 0, the zero record is returned and every per-position output is 0.",
                   "TDOA_ERR_UNSUPPORTED when P * windows_per_block > 2^17",
                   "J = 0: total = the sum over j of the stacks' maps, word for word.",
                   "score_q = total[cell] = the sum over j of own[j]."):
        assert phrase in flat, phrase


def test_null_handle_is_invalid_without_a_device(capi):
    lib = capi.load()
    rec = np.zeros(3, dtype=capi.CELL_TRACK_DTYPE)
    q = np.zeros(2 * 3 * 7, dtype=np.int64)
    pr, pq = rec.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.POINTER(C.c_int64))
    for m, J, sep in ((0, 0, 1), (1, 16, 3), (-1, 0, 1), (0, 17, 1), (0, -1, 1), (0, 0, 0)):
        assert lib.tdoa_process_locate_track(None, m, J, sep, pr, None, None, None, None, None) == 1
        assert lib.tdoa_group_process_locate_track(None, m, J, sep, pr, None, None, None, None, None) == 1
        assert lib.tdoa_debug_locate_track_from_q(None, pq, 2, 2, 3, 1, J, sep, pr, None, None, None, None, None) == 1
    assert lib.tdoa_process_locate_track(None, 0, 0, 1, None, None, None, None, None, None) == 1


# ---- every path enumerated ------------------------------------------------------------------------------------------------
def _rank_order(J):
    return [0] + [x for k in range(1, J + 1) for x in (k, -k)]


def _exists(r, c, n_cols, n_cells):
    return r >= 0 and 0 <= c < n_cols and r * n_cols + c < n_cells


def _brute(maps, n_cols, J):
    """for every start cell: (the largest sum over every path of existing cells, the first such path in the lexicographic
    order of (rank(dr_0), rank(dc_0), rank(dr_1), ...))"""
    L, n_cells = maps.shape
    moves = [(dr, dc) for dr in _rank_order(J) for dc in _rank_order(J)]          # rank order, dr first
    out = []
    for c0 in range(n_cells):
        best = None
        for seq in itertools.product(moves, repeat=L - 1):                        # lexicographic in that order
            r, c, path, total = c0 // n_cols, c0 % n_cols, [c0], int(maps[0, c0])
            for j, (dr, dc) in enumerate(seq):
                r, c = r + dr, c + dc
                if not _exists(r, c, n_cols, n_cells):
                    break
                path.append(r * n_cols + c)
                total += int(maps[j + 1, path[-1]])
            else:
                if best is None or total > best[0]:                               # strict: the first maximum
                    best = (total, path)
        out.append(best)
    return out


def _walk(D, n_cols, c):
    path = [c]
    for j in range(D.shape[0] - 1):
        c += int(D[j, c, 0]) * n_cols + int(D[j, c, 1])
        path.append(c)
    return path


@pytest.mark.parametrize("n_cells, n_cols", [(12, 4), (10, 4), (7, 7), (5, 1)], ids=["3x4", "short last row", "list", "column"])
def test_model_against_every_path_enumerated(n_cells, n_cols):
    """three positions, J 0 .. 2, few distinct values so that equal maxima are common"""
    from tdoa_amd import locate_track
    rng = np.random.default_rng(101 + n_cells)
    n_tied = 0
    for J in (0, 1, 2):
        for trial in range(3):
            maps = rng.integers(0, 3, size=(3, n_cells), dtype=np.int64)
            T, D = locate_track.backward(maps, n_cols, J)
            want = _brute(maps, n_cols, J)
            assert T[0].tolist() == [w[0] for w in want], (J, trial)
            for c in range(n_cells):
                assert _walk(D, n_cols, c) == want[c][1], (J, trial, c)
            rec, cells, own, total = locate_track.track(maps, n_cols, J, 1, 3)
            top = max(w[0] for w in want)
            first = [w[0] for w in want].index(top)
            n_tied += [w[0] for w in want].count(top) > 1
            if top == 0:
                assert rec.tobytes() == bytes(48) and not cells.any() and not own.any()
                continue
            assert (int(rec["cell"]), int(rec["score_q"]), cells.tolist()) == (first, top, want[first][1])
            assert int(rec["steps"]) == sum(a != b for a, b in zip(want[first][1], want[first][1][1:])) and int(rec["positions"]) == 3
    assert n_tied >= 2                                                            # equal maxima of T_0 occur


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------
def hand_cases():
    """[(name, dict(maps [L][n_cells], n_cols, J, sep), expected or None for the zero record)]; expected: cells, total (T_0),
    runner_cell, runner_q, and D of position 0 where the case is about it"""
    z = lambda n, **kw: [kw.get(str(i), kw.get("c%d" % i, 0)) for i in range(n)]
    # 3 x 4 cells all 5: every (dr, dc) ties, (0, 0) is first; every T_0 = 15, the smallest cell wins; the runner-up is the
    # smallest cell more than one row or column away: cell 2
    equal = np.full((3, 12), 5, dtype=np.int64)
    # a list of 7: position 1 has equal maxima one to the right and one to the left of cell 3: +1 is first
    lr = np.array([z(7, c3=1), z(7, c2=4, c4=4)], dtype=np.int64)
    # 3 x 3: position 1 has equal maxima below (dr = +1) and above (dr = -1) cell 4, and an equal one to its left
    # (dr = 0, dc = -1): rank(dr) = 0 comes first whatever dc is
    ud = np.array([z(9, c4=1), z(9, c1=6, c7=6, c3=6)], dtype=np.int64)
    ud2 = np.array([z(9, c4=1), z(9, c1=6, c7=6)], dtype=np.int64)             # without the left one: dr = +1 before -1
    # rows of 4, 10 cells: the last row holds cells 8 and 9 only.  Position 0 starts at cell 7 = (1, 3); position 2 pays at
    # cell 9 = (2, 1).  The short way leads over (2, 2), which does not exist: the track goes (1, 3) -> (1, 2) -> (2, 1), and
    # position 1 pays nothing anywhere, so the first step is the first in rank order from which cell 9 is still in reach:
    # (0, -1).  Cell 3 = (0, 3) must not reach cell 4 = (1, 0), where position 1 is worth 9, through its index: its best is
    # 8 at (1, 2), and T_0[3] = 1 + 8.
    short = np.array([z(10, c7=2, c3=1), z(10), z(10, c9=8, c4=9)], dtype=np.int64)
    return [
        ("an all-equal map: every step (0, 0), the smallest cell", dict(maps=equal, n_cols=4, J=2, sep=1),
         dict(cells=[0, 0, 0], total=[15] * 12, runner_cell=2, runner_q=15, d0=[(0, 0)] * 12)),
        ("equal maxima at +1 and -1 along a list: +1", dict(maps=lr, n_cols=7, J=1, sep=1),
         dict(cells=[3, 4], total=[0, 4, 4, 5, 4, 4, 0], runner_cell=1, runner_q=4, d0={3: (0, 1), 1: (0, 1), 5: (0, -1), 2: (0, 0)})),
        ("equal maxima in the row, below and above: the row", dict(maps=ud, n_cols=3, J=1, sep=1),
         dict(cells=[4, 3], total=[6, 6, 6, 6, 7, 6, 6, 6, 6], runner_cell=0, runner_q=0, d0={4: (0, -1)}, no_runner=True)),
        ("equal maxima below and above: below", dict(maps=ud2, n_cols=3, J=1, sep=1),
         dict(cells=[4, 7], total=[6, 6, 6, 6, 7, 6, 6, 6, 6], runner_cell=0, runner_q=0, d0={4: (1, 0)}, no_runner=True)),
        ("the short last row's missing cell is no stepping stone", dict(maps=short, n_cols=4, J=1, sep=1),
         dict(cells=[7, 6, 9], total=[9, 9, 9, 9, 9, 9, 9, 10, 9, 9], runner_cell=0, runner_q=9, d0={7: (0, -1), 3: (1, -1)})),
        ("all zeros: the zero record", dict(maps=np.zeros((4, 10), dtype=np.int64), n_cols=4, J=3, sep=1), None),
    ]


def _check_hand_case(got, arg, want):
    """got: (record, cells, own, total) of one track"""
    rec, cells, own, total = got
    maps = arg["maps"]
    if want is None:
        assert rec.tobytes() == bytes(48) and not cells.any() and not own.any() and not total.any()
        return
    assert cells.tolist() == want["cells"] and total.tolist() == want["total"]
    assert own.tolist() == [int(maps[j, c]) for j, c in enumerate(want["cells"])]
    assert (int(rec["cell"]), int(rec["positions"])) == (want["cells"][0], len(maps))
    assert int(rec["steps"]) == sum(a != b for a, b in zip(want["cells"], want["cells"][1:]))
    assert int(rec["score_q"]) == want["total"][want["cells"][0]] == int(own.sum())
    assert (int(rec["runner_cell"]), int(rec["runner_q"])) == (want["runner_cell"], want["runner_q"])
    n_w = len(maps)
    assert float(rec["score"]) == float(rec["score_q"]) / 2 ** 32 / np.sqrt(float(n_w))
    assert float(rec["runner_up"]) == float(rec["runner_q"]) / 2 ** 32 / np.sqrt(float(n_w))


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_worked_cases(name, arg, want):
    from tdoa_amd import locate_track
    got = locate_track.track(arg["maps"], arg["n_cols"], arg["J"], arg["sep"], len(arg["maps"]))
    _check_hand_case(got, arg, want)
    if want is not None:
        D = locate_track.backward(arg["maps"], arg["n_cols"], arg["J"])[1]
        d0 = want["d0"]
        for c, d in (enumerate(d0) if isinstance(d0, list) else d0.items()):
            assert tuple(D[0, c]) == d, (c, D[0, c])


# ---- the identities of the header -------------------------------------------------------------------------------------------
def test_identities_on_random_integers():
    from tdoa_amd import locate, locate_track
    rng = np.random.default_rng(7)
    for S, ml, n_cells, n_cols, L, J in ((3, 6, 40, 7, 4, 2), (4, 9, 33, 33, 3, 1), (2, 5, 50, 8, 5, 16), (4, 7, 29, 5, 1, 3)):
        P = S * (S - 1) // 2
        q = rng.integers(-50, 51, size=(2 * L, P, 2 * ml - 1), dtype=np.int64)
        table = rng.integers(-16 * ml, 16 * ml + 1, size=(n_cells, S), dtype=np.int32)
        clock = rng.integers(-40, 41, size=(2 * L, S), dtype=np.int32)
        n_w = rng.integers(1, 4, size=2 * L)
        for sep in (1, 2):
            loc = locate.locate_stacks(q, table, n_cols, ml, sep, n_w, clock)
            rec, cells, own, lags, corr, total = locate_track.track_stacks(q, table, n_cols, ml, L, J, sep, n_w, clock)
            zero = locate_track.track_stacks(q, table, n_cols, ml, L, 0, sep, n_w, clock)
            assert (zero[5] == loc[3].reshape(2, L, n_cells).sum(axis=1)).all()              # J = 0: the sum of the maps
            assert (zero[1] == zero[1][:, :1]).all() and (zero[0]["steps"] == 0).all()
            assert (rec["score_q"] == total[np.arange(2), rec["cell"]]).all() and (rec["score_q"] == own.sum(axis=1)).all()
            assert (rec["score_q"] >= zero[0]["score_q"]).all()                               # a larger J never loses
            r, c = np.divmod(cells, n_cols)
            assert (np.abs(np.diff(r, axis=1)) <= J).all() and (np.abs(np.diff(c, axis=1)) <= J).all()
            assert (rec["steps"] == (np.diff(cells, axis=1) != 0).sum(axis=1)).all() and (rec["positions"] == L).all()
            assert (own == loc[3].reshape(2, L, n_cells)[np.arange(2)[:, None], np.arange(L)[None, :], cells]).all()
            for sid in range(2 * L):                                                          # the position's row is locate's for that cell
                want = locate_track.cell_lags(q[sid], table, cells[sid // L, sid % L], ml, int(n_w[sid]), clock[sid])
                assert (lags[sid] == want[0]).all() and (corr[sid] == want[1]).all()
            if L == 1:                                                                        # one stack: the location's bytes
                for a, b in (("cell", "cell"), ("runner_cell", "runner_cell"), ("score_q", "score_q"), ("runner_q", "runner_q"),
                             ("score", "score"), ("runner_up", "runner_up")):
                    assert rec[a].tobytes() == loc[0][b].tobytes()
                assert lags.tobytes() == loc[1].tobytes() and corr.tobytes() == loc[2].tobytes() and total.tobytes() == loc[3].tobytes()


# ---- ramp_clock -------------------------------------------------------------------------------------------------------------
def test_ramp_clock_against_exact_fractions():
    from tdoa_amd import sync
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 5, 12, 33):
        a = rng.integers(-2000, 2001, size=6)
        b = a + rng.integers(-70, 71, size=6)
        got = sync.ramp_clock(a, b, n)
        assert got.shape == (n, 6) and got.dtype == np.int32
        for j in range(n):
            for s in range(6):
                x = Fraction(16 * int(b[s] - a[s]) * (n + 2 * j + 1), 4 * n)
                r = int(abs(x) + Fraction(1, 2)) * (1 if x >= 0 else -1)                     # halves away from zero
                assert int(got[j, s]) == 16 * int(a[s]) + r, (n, j, s)
        mid = sync.midpoint_clock(a, b)
        assert (np.abs(got.astype(np.float64).mean(axis=0) - mid) <= 0.5).all()              # each term is rounded by at most 1/2
    # halves: n = 1, j = 0: 16 d / 2 = 8 d exactly; n = 2: 16 d 3 / 8 = 6 d and 16 d 5 / 8 = 10 d; n = 4, d = 1: 5, 7, 9, 11
    assert sync.ramp_clock([0], [1], 4)[:, 0].tolist() == [5, 7, 9, 11]
    assert sync.ramp_clock([3], [2], 4)[:, 0].tolist() == [43, 41, 39, 37]
    # 16 d (n + 2 j + 1) / (4 n) with n = 32, d = 1: (33 + 2 j) / 8; j = 0: 4.125 -> 4; j = 2: 4.625 -> 5; halves: n = 8, d = 1,
    # (9 + 2 j) / 2 = 4.5, 5.5 .. -> 5, 6 and for d = -1 -> -5, -6
    assert sync.ramp_clock([0], [1], 8)[:2, 0].tolist() == [5, 6] and sync.ramp_clock([0], [-1], 8)[:2, 0].tolist() == [-5, -6]
    with pytest.raises(ValueError):
        sync.ramp_clock([0, 1], [0], 3)
    with pytest.raises(ValueError):
        sync.ramp_clock([0], [0], 0)


# ---- the noisy cases --------------------------------------------------------------------------------------------------------
STILL = dict(path=[(12, 36)] * 12, noise=0.75)                         # the planted cell of tests/test_locate_cpu.py
MOVING = dict(path=[(12 + w, 30 + w) for w in range(12)], noise=0.7)   # one row and one column per stack


def cell_delays(row, col):
    """station delays in samples of a transmitter in cell (row, col) of the 48 x 64 grid: rint(fs dist / c) minus their minimum,
    as tests/test_locate_cpu.py's noisy_case() has them for (12, 36)"""
    from tdoa_amd import locate
    tx = locate.ecef(GRID["lat0"] + row * GRID["dlat"], GRID["lon0"] + col * GRID["dlon"], GRID["height_m"])
    d = np.rint(FS * np.linalg.norm(locate.ecef(*np.array(ST4).T) - tx, axis=1) / locate.SPEED_OF_LIGHT).astype(np.int64)
    return [int(x) for x in d - d.min()]


def track_windows(oracle, path, noise):
    """window w of station s = simulate_delayed_fm(8192, d_s(path[w]), 300 + w, 1000 (s + 1) + w, 1.0, noise) -> [w][s] u8 IQ:
    noisy_windows() of tests/test_locate_cpu.py with the noise and the cell free"""
    return [[oracle.simulate_delayed_fm(8192, cell_delays(*rc)[s], 300 + w, 1000 * (s + 1) + w, 1.0, noise) for s in range(4)]
            for w, rc in enumerate(path)]


def noisy_counts(q, table, path, J):
    """q [12][6][255] of twelve one-window stacks -> (stacks the delay-table search alone gets right, stacks the track gets
    right, the track's outputs)"""
    from tdoa_amd import locate, locate_track
    want = np.array([r * 64 + c for r, c in path])
    loc = locate.locate_stacks(q, table, 64, 128, 1, 1)
    out = locate_track.track_stacks(q, table, 64, 128, 12, J, 1, 1)
    return int((loc[0]["cell"] == want).sum()), int((out[1][0] == want).sum()), out


def _float64_q(oracle, wins):
    from tdoa_amd import stacking
    out = []
    for x in wins:
        sig = [oracle.b_preprocess(s)[0] for s in x]
        out.append([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], 128)) for i, j in PAIRS4])
    return np.array(out)


def test_a_stationary_emitter_the_stacks_alone_miss(oracle):
    """Twelve one-window stacks as one track, noise 0.75.  Measured with the float64 pipeline: the delay-table search alone
    finds the planted cell in 0 of 12 stacks; the sum of the twelve maps (J = 0) has it on top, 1.25 times the runner-up."""
    from tdoa_amd import locate
    table = locate.grid_table(ST4, sample_rate=FS, **GRID)
    alone, along, out = noisy_counts(_float64_q(oracle, track_windows(oracle, **STILL)), table, STILL["path"], 0)
    rec = out[0][0]
    print("alone %d of 12, the track's cell (%d, %d), score / runner-up %.3f" % (alone, rec["cell"] // 64, rec["cell"] % 64,
                                                                               rec["score"] / rec["runner_up"]))
    assert alone == 0 and alone < 6
    assert int(rec["cell"]) == 12 * 64 + 36 and along == 12 and int(rec["steps"]) == 0


def test_a_moving_emitter_the_track_follows(oracle):
    """The planted cell moves one row and one column per stack, noise 0.7.  Measured with the float64 pipeline: the
    delay-table search alone is right on 2 of 12 stacks, the J = 1 track on 11."""
    from tdoa_amd import locate
    table = locate.grid_table(ST4, sample_rate=FS, **GRID)
    alone, along, out = noisy_counts(_float64_q(oracle, track_windows(oracle, **MOVING)), table, MOVING["path"], 1)
    print("alone %d of 12, along the track %d of 12, steps %d, cells %s" % (alone, along, out[0][0]["steps"],
                                                                           [divmod(int(c), 64) for c in out[1][0]]))
    assert (alone, along) == (2, 11)
    assert along > alone and 12 - alone >= 4                               # the case shows something
