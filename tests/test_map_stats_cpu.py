"""CPU: the numpy statement of the map statistics (tdoa_amd.map_stats; include/tdoa_mi355x.h, "map statistics") against a
plain-Python sort on hand cases, on the noisy case the setting exists for (tests/test_locate_cpu.py: does the best cell stand
out of its own map?), and on the rounds of the two-emitter case of tests/test_locate_multi_cpu.py; and the boundary of the
entry points that needs no device.  tests/test_gpu_map_stats.py holds the kernels to the same model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_locate_cpu import PAIRS4, noisy_case
from test_locate_multi_cpu import B_CELLS, N_A, N_B, two_emitter_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdoa_locate_set_stats", "tdoa_locate_last_stats", "tdoa_group_locate_set_stats", "tdoa_group_locate_last_stats")
RANKS = (32768, 64880)
FOOT = 49152
THRESHOLD = 2.0


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def test_entry_points_declared_bound_and_exported(capi):
    from tdoa_amd import map_stats
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) LocateSetStats(", "C.tdoa_locate_set_stats(", "func (g *gpuCorrelator) LocateLastStats(",
                 "C.tdoa_locate_last_stats(", "func (g *Group) LocateSetStats(", "C.tdoa_group_locate_set_stats(",
                 "func (g *Group) LocateLastStats(", "C.tdoa_group_locate_last_stats("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for owner in (capi.Context, capi.Group):
        assert hasattr(owner, "locate_set_stats") and hasattr(owner, "locate_last_stats")
    assert re.search(r"#define TDOA_MAP_STATS_MAX_RANKS 8\b", hdr) and map_stats.MAX_RANKS == capi.MAP_STATS_MAX_RANKS == 8
    # the record's layout: declared in the header, mirrored as a numpy dtype (twice: the binding's and the model's)
    body = re.search(r"typedef struct \{([^}]*)\} tdoa_map_stats;", hdr).group(1)
    fields = [f.strip().split("[")[0] for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert tuple(fields) == capi.MAP_STATS_DTYPE.names == map_stats.MAP_STATS_DTYPE.names
    assert capi.MAP_STATS_DTYPE == map_stats.MAP_STATS_DTYPE and capi.MAP_STATS_DTYPE.itemsize == 168
    assert [capi.MAP_STATS_DTYPE.fields[n][1] for n in ("quantile_q", "quantile", "level_q", "n_live", "reserved")] == [0, 64, 128, 136, 164]
    flat = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("n_live = #{c : v[c] > 0}.", "(ranks[i] * (n_live - 1)) div 65535", "rank 0 is the smallest live word, rank 65535 is best",
                   "level_q = q0 + (d >> 16) * foot + (((d & 0xffff) * foot) >> 16)", "foot == 0 leaves level_q and the footprint's fields 0.",
                   "A zero record (score_q == 0) gives the all-zero statistics.", "The call's own outputs keep their bytes.",
                   "n_ranks outside 0 .. 8, foot outside 0 .. 65535"):
        assert phrase in flat, phrase
    # no profiling scope was added
    assert [lib.tdoa_kernel_name(k).decode() for k in range(len(capi.KERNELS))][-2:] == ["k_track_step", "k_track_finish"]


def test_null_handle_and_argument_errors_need_no_device(capi):
    lib = capi.load()
    ranks = (C.c_uint16 * 9)(*range(0, 9000, 1000))
    out = np.zeros(4, dtype=capi.MAP_STATS_DTYPE)
    n = C.c_int(-7)
    for n_ranks, foot in ((2, 0), (0, 0), (9, 0), (2, -1), (2, 65536)):
        assert lib.tdoa_locate_set_stats(None, ranks, n_ranks, foot) == 1
        assert lib.tdoa_group_locate_set_stats(None, ranks, n_ranks, foot) == 1
    assert lib.tdoa_locate_last_stats(None, out.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == 1
    assert lib.tdoa_group_locate_last_stats(None, out.ctypes.data_as(C.c_void_p), 4, C.byref(n)) == 1 and n.value == -7


def test_model_argument_errors():
    from tdoa_amd import map_stats
    v = np.arange(6, dtype=np.int64)
    for kw in (dict(ranks=()), dict(ranks=range(9)), dict(ranks=(-1,)), dict(ranks=(65536,)), dict(foot=-1), dict(foot=65536)):
        with pytest.raises(ValueError):
            map_stats.plane_stats(**{"v": v, "n_cols": 3, "ranks": (0,), **kw})
    with pytest.raises(ValueError):
        map_stats.stats(np.zeros((2, 6), dtype=np.int64), np.zeros(3, dtype=[("score_q", np.int64), ("cell", np.int32)]), 3, (0,))


# ---- hand cases against a plain-Python sort -----------------------------------------------------------------------------------
def _plain(v, n_cols, ranks, foot, sep):
    """the definition, cell by cell, in Python integers: (n_live, words, level, foot_cells, foot_near, box)"""
    v = [int(x) for x in v]
    best = max(v)
    if best <= 0:
        return 0, [0] * len(ranks), 0, 0, 0, (0, 0, 0, 0)
    b = v.index(best)
    live = sorted(x for x in v if x > 0)
    words = [live[(r * (len(live) - 1)) // 65535] for r in ranks]
    if foot == 0:
        return len(live), words, 0, 0, 0, (0, 0, 0, 0)
    lv = words[0] + ((best - words[0]) * foot) // 65536
    cells = [c for c, x in enumerate(v) if x > 0 and x >= lv]
    rows, cols = [c // n_cols for c in cells], [c % n_cols for c in cells]
    near = sum(abs(r - b // n_cols) <= sep and abs(c - b % n_cols) <= sep for r, c in zip(rows, cols))
    return len(live), words, lv, len(cells), near, (min(rows), max(rows), min(cols), max(cols))


def _agrees(v, n_cols, ranks, foot, sep):
    from tdoa_amd import map_stats
    s = map_stats.plane_stats(v, n_cols, ranks, foot, min_separation=sep)
    n_live, words, lv, cells, near, box = _plain(v, n_cols, ranks, foot, sep)
    assert int(s["n_live"]) == n_live and s["quantile_q"][:len(ranks)].tolist() == words and not s["quantile_q"][len(ranks):].any()
    assert (int(s["level_q"]), int(s["foot_cells"]), int(s["foot_near"])) == (lv, cells, near)
    assert tuple(int(s[k]) for k in ("row_lo", "row_hi", "col_lo", "col_hi")) == box
    assert s["quantile"][:len(ranks)].tolist() == [w / 2.0 ** 32 for w in words] and int(s["reserved"]) == 0
    return s


def test_hand_cases_against_a_plain_sort():
    from tdoa_amd import map_stats
    every = (0, 65535, 65535, 1, 32768, 0)                               # ranks 0 and 65535, duplicates
    none = _agrees([0] * 10, 4, every, FOOT, 1)                          # no live cell: the zero record's statistics
    assert not none.tobytes().strip(b"\0")
    one = _agrees([0, 0, 0, 0, 0, 0, 41, 0, 0, 0], 4, every, FOOT, 1)    # one live cell: every word, the level and the box are its
    assert one["quantile_q"][:6].tolist() == [41] * 6 and (int(one["level_q"]), int(one["foot_cells"]), int(one["foot_near"])) == (41, 1, 1)
    assert tuple(int(one[k]) for k in ("row_lo", "row_hi", "col_lo", "col_hi")) == (1, 1, 2, 2)
    same = _agrees([9] * 11, 4, every, FOOT, 1)                          # all words equal: the footprint is the plane
    assert same["quantile_q"][:6].tolist() == [9] * 6 and int(same["foot_cells"]) == 11 and int(same["foot_near"]) == 4
    assert tuple(int(same[k]) for k in ("row_lo", "row_hi", "col_lo", "col_hi")) == (0, 2, 0, 3)       # (a short last row)
    v = [5, 0, 3, 9, 1, 0, 7, 7, 2, 8, 6]                                # live sorted: 1 2 3 5 6 7 7 8 9
    s = _agrees(v, 4, every, FOOT, 1)
    assert s["quantile_q"][:6].tolist() == [1, 9, 9, 1, 6, 1] and int(s["n_live"]) == 9
    assert _agrees(v, 4, (65534,), 0, 1)["quantile_q"][0] == 8           # (65534 * 8) div 65535 = 7: the word before the best
    assert _agrees(v, 4, (8192,), 0, 1)["quantile_q"][0] == 2            # (8192 * 8) div 65535 = 1
    # the level rule near 2^62: the product (best - q0) foot does not fit 64 bits, the two halves do
    big = 2 ** 62
    for q0, best, foot in ((1, big, 65535), (3, big - 1, FOOT), (big - 70000, big, 1), (big // 3, big, 12345), (7, 7, 65535)):
        assert map_stats.level(q0, best, foot) == q0 + ((best - q0) * foot) // 65536
    _agrees([1, big, 3, big - 1, big // 2, 0, big // 2 + 1], 3, (0, 32768, 65535), FOOT, 1)
    _agrees([1, big, 3, big - 1, big // 2, 0, big // 2 + 1], 3, (32768, 0), 65535, 1)
    # box and foot_near at the grid's edges, with a short last row: the best cell in a corner, in the last row, at a row's end
    rng = np.random.default_rng(401)
    for n_cells, n_cols, best_at in ((23, 5, 0), (23, 5, 22), (23, 5, 4), (23, 5, 20), (17, 17, 16), (17, 1, 0), (64, 8, 63)):
        v = rng.integers(0, 50, size=n_cells)
        v[best_at] = 100
        for sep in (1, 2, 30):
            for foot in (1, 20000, 65535):
                s = _agrees(v, n_cols, (0, 32768), foot, sep)
                assert int(s["foot_near"]) >= 1


def test_stats_over_planes_and_contrast():
    from tdoa_amd import map_stats
    planes = np.array([[[1, 2, 3, 4, 5, 6, 7, 8, 9, 109], [0] * 10], [[5, 5, 5, 5, 5, 5, 5, 5, 5, 5], [0, 1, 2, 3, 0, 0, 0, 0, 0, 30]]],
                      dtype=np.int64)
    rec = np.zeros((2, 2), dtype=[("cell", np.int32), ("score_q", np.int64)])
    rec["score_q"], rec["cell"] = planes.max(axis=2), planes.argmax(axis=2)
    s = map_stats.stats(planes, rec, 5, (32768, 57343, 65535), FOOT, 1, [[1, 4], [4, 1]])
    assert s.shape == (2, 2) and s["n_live"].tolist() == [[10, 0], [10, 4]]
    assert s["quantile_q"][0, 0, :3].tolist() == [5, 8, 109] and s["quantile"][1, 0, 0] == 5 / 2.0 ** 32 / 2.0
    # (109 - 5) / (8 - 5); the zero record and the plane of equal words have no contrast; (30 - 2) / (3 - 2)
    assert map_stats.contrast(s).tolist() == [[104 / 3, 0.0], [0.0, 28.0]]
    assert map_stats.contrast(s, best=rec["score_q"]).tolist() == map_stats.contrast(s).tolist()
    assert map_stats.contrast(s, floor=1, ref=2, best=rec["score_q"])[0, 0] == 1.0


# ---- the claim: two order statistics and a count tell when to believe the best cell ---------------------------------------------
def _window_stats(oracle, x, table, ml=128, sep=2):
    """one window's stations -> (the location's record, the statistics of its map) with the float64 oracle"""
    from tdoa_amd import locate, map_stats, stacking
    sig = [oracle.b_preprocess(s)[0] for s in x]
    q = np.array([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ml)) for i, j in PAIRS4])
    rec, _, _, score_map = locate.locate(q, table, 64, ml, sep)
    return rec, map_stats.plane_stats(score_map, 64, RANKS, FOOT, rec["score_q"], rec["cell"], sep)


def test_contrast_and_footprint_tell_an_emitter_from_noise(oracle):
    """The case of tests/test_locate_cpu.py: four stations, the 48 x 64 grid, max_lag 128, one window of 8 192 per stack,
    min_separation 2, ranks (32768, 64880), foot 49152, threshold 2.0.  Measured with the float64 pipeline: the contrast is at
    least 2.0 in 11 of the 12 emitter windows, in 0 of the 12 windows with no common signal and in 0 of the 12 at noise 0.75 (where
    the locate is wrong in all 12); one cell reaches 3/4 of the way from the median to the best in 11 of the emitter windows"""
    from tdoa_amd import map_stats
    table, planted_cell, delays, _ = noisy_case()
    kinds = {"emitter": lambda w, s: (delays[s], 300 + w, 0.6), "noise only": lambda w, s: (delays[s], 300 + w + 50 * s + 7, 0.6),
             "noise 0.75": lambda w, s: (delays[s], 300 + w, 0.75)}
    over, single, right = {}, {}, {}
    for name, arg in kinds.items():
        over[name] = single[name] = right[name] = 0
        for w in range(12):
            x = [oracle.simulate_delayed_fm(8192, arg(w, s)[0], arg(w, s)[1], 1000 * (s + 1) + w, 1.0, arg(w, s)[2]) for s in range(4)]
            rec, s = _window_stats(oracle, x, table)
            c = float(map_stats.contrast(s, best=rec["score_q"]))
            over[name] += c >= THRESHOLD
            single[name] += int(s["foot_cells"]) == 1
            right[name] += int(rec["cell"]) == planted_cell
            print("%s window %2d: contrast %.2f foot_cells %d near %d box rows %d..%d cols %d..%d cell (%d, %d)"
                  % (name, w, c, s["foot_cells"], s["foot_near"], s["row_lo"], s["row_hi"], s["col_lo"], s["col_hi"],
                     rec["cell"] // 64, rec["cell"] % 64))
    print("contrast >= %.1f: %s; foot_cells == 1: %s; the planted cell: %s" % (THRESHOLD, over, single, right))
    assert over["emitter"] >= 10
    assert over["noise only"] <= 1
    assert over["noise 0.75"] <= 1
    assert single["emitter"] >= 10


# stacks of 12 in which the contrasts of rounds 0 and 1 must both exceed round 2's: the float64 model shows it in 12 and in 11,
# that is for all stacks but at most 2, so it is asserted, with the margin the request names
ROUNDS_ABOVE = {B_CELLS[0]: 10, B_CELLS[1]: 10}


@pytest.mark.parametrize("b_cell", B_CELLS, ids=["B (30, 50)", "B (34, 14)"])
def test_contrasts_of_the_rounds_of_the_two_emitter_case(oracle, b_cell):
    """The two-emitter case of tests/test_locate_multi_cpu.py with K = 3 (guard 2, min_separation 2): rounds 0 and 1 find A and
    B, round 2 has no third emitter to find.  The contrasts of the three rounds' maps are printed and recorded in DESIGN.md
    section 3.  Measured with the float64 pipeline: medians 4.77, 3.05 and 1.59 for B (30, 50), where rounds 0 and 1 both exceed
    round 2 in 12 of 12 stacks; 4.80, 2.12 and 1.46 for B (34, 14), in 11 of 12 (stack 0: 1.68 against 1.75)."""
    from tdoa_amd import locate_multi, map_stats, stacking
    ml = 128
    table = noisy_case()[0]
    c = np.zeros((12, 3))
    for t, stack in enumerate(two_emitter_windows(oracle, b_cell)):
        total = np.zeros((6, 2 * ml - 1), dtype=np.int64)
        for x in stack:
            sig = [oracle.b_preprocess(s)[0] for s in x]
            total += np.array([stacking.to_fixed(oracle.b_xcorr_all_lags(sig[i], sig[j], ml)) for i, j in PAIRS4])
        recs, _, _, maps = locate_multi.locate_multi(total, table, 64, ml, 3, 2, 2, N_A + N_B)
        s = map_stats.stats(maps, recs, 64, RANKS, FOOT, 2, N_A + N_B)
        c[t] = map_stats.contrast(s, best=recs["score_q"])
        print("B (%d, %d) stack %2d: contrast of rounds 0, 1, 2: %.2f %.2f %.2f; foot_cells %s"
              % (b_cell // 64, b_cell % 64, t, c[t, 0], c[t, 1], c[t, 2], s["foot_cells"].tolist()))
    above = int((c[:, :2].min(axis=1) > c[:, 2]).sum())
    print("B (%d, %d): rounds 0 and 1 both exceed round 2 in %d of 12 stacks; medians %.2f %.2f %.2f"
          % (b_cell // 64, b_cell % 64, above, *np.median(c, axis=0)))
    assert above >= ROUNDS_ABOVE[b_cell]
