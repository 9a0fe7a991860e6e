"""CPU: the clock mix of tdoa_process_sync_locate (include/tdoa_mi355x.h, "clocks to fix in one call").

1. clock_mix.mix_rows against fractions.Fraction, halves away from zero, on a few thousand random (a16, b16, wa, wb) and the
   corners: negative sums, exact halves of both signs, wb = 0, wa = 0, den = 65536, clocks at +-(2^31 - 16);
2. the (1, 1) mix is sync_fine.midpoint_clock16, word for word;
3. tdoa_clock_mix_rows (host only) returns mix_rows' bytes and refuses what the header says;
4. midpoint_mix(spb) reproduces the clock table tests/test_gpu_sync_fine.py's CLI test builds by hand;
5. the chain's statement (tdoa_amd.sync_locate) on a measured window of tests/test_sync_fine_cpu.py is the three statements
   called one after another;
6. the entries are declared, bound and exported.
corner_cases() is shared with tests/test_gpu_sync_locate.py, which runs the kernel on the same words."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from test_locate_cpu import FS, GRID, ST4
from test_locate_upsample_cpu import ML, coarse_table
from test_sync_fine_cpu import (FINE_KEYS, FINE_ROUNDS, GATE, ROUNDS, UP, _float64_q, measured_case, reference_window_iq,
                                target_window_iq)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 2 ** 31 - 16              # the largest clock the fine clock search can return: 16 (2^27 - 1)
NAMES = ("tdoa_process_sync_locate", "tdoa_group_process_sync_locate", "tdoa_debug_sync_locate_from_q", "tdoa_clock_mix_rows",
         "tdoa_debug_clock_mix")


@pytest.fixture(scope="module")
def capi():
    import tdoa_amd
    tdoa_amd.build.build()
    return tdoa_amd.capi


def exact_row(a16, b16, wa, wb):
    """the nearest integer to (wa a16 + wb b16) / (wa + wb), halves away from zero, in rationals"""
    x = Fraction(int(wa) * int(a16) + int(wb) * int(b16), int(wa) + int(wb))
    n = abs(x) + Fraction(1, 2)
    r = n.numerator // n.denominator
    return -r if x < 0 else r


def corner_cases():
    """-> (clock16 [n][1] int32, mix [m][4] int32): every corner as one (stack a, stack b, wa, wb) on one-station stacks"""
    cases = []
    for a, b in ((3, 4), (-3, -4), (3, -4), (-3, 4), (1, 0), (-1, 0), (0, 0), (7, 7), (-7, -7), (5, -5), (1, -2), (-1, 2)):
        cases += [(a, b, 1, 1), (a, b, 1, 0), (a, b, 0, 1), (a, b, 3, 1), (a, b, 1, 3), (a, b, 4, 4)]      # exact halves of both signs
    for den in (2, 8, 65536):                                                # exact halves and their neighbours at every den
        for t in (den // 2, -(den // 2), den // 2 + 1, -(den // 2) - 1, den // 2 - 1, -(den // 2) + 1, 3 * den // 2, -3 * den // 2):
            cases += [(t, 0, 1, den - 1), (0, t, den - 1, 1)]
    for a, b in ((TOP, TOP), (-TOP, -TOP), (TOP, -TOP), (-TOP, TOP), (TOP, TOP - 1), (-TOP, -TOP + 1), (TOP, 0), (0, -TOP)):
        cases += [(a, b, 1, 1), (a, b, 65535, 1), (a, b, 1, 65535), (a, b, 32768, 32768), (a, b, 65536, 0), (a, b, 0, 65536), (a, b, 5, 3)]
    clock16 = np.array([[v] for c in cases for v in c[:2]], dtype=np.int32)
    mix = np.array([[2 * k, 2 * k + 1, c[2], c[3]] for k, c in enumerate(cases)], dtype=np.int32)
    return clock16, mix


def random_cases(seed, n):
    """n random mixes over 64 three-station stacks; every fourth row small numbers with a small den (many exact halves)"""
    rng = np.random.default_rng(seed)
    clock16 = rng.integers(-TOP, TOP + 1, size=(64, 3)).astype(np.int32)
    clock16[::4] = rng.integers(-9, 10, size=(16, 3))
    den = np.where(rng.random(n) < 0.5, rng.integers(1, 9, size=n), rng.integers(1, 65537, size=n))
    wa = (rng.random(n) * (den + 1)).astype(np.int64).clip(0, den)
    mix = np.stack([rng.integers(0, 64, size=n), rng.integers(0, 64, size=n), wa, den - wa], axis=1).astype(np.int32)
    mix[::3, :2] = 4 * rng.integers(0, 16, size=(len(mix[::3]), 2))           # the small rows among themselves
    return clock16, mix


def _exact(clock16, mix):
    return np.array([[exact_row(clock16[a][s], clock16[b][s], wa, wb) for s in range(clock16.shape[1])] for a, b, wa, wb in mix.tolist()],
                    dtype=np.int64)


def test_mix_rows_against_fractions():
    from tdoa_amd import clock_mix
    clock16, mix = corner_cases()
    got = clock_mix.mix_rows(clock16, mix)
    assert got.dtype == np.int32 and (got == _exact(clock16, mix)).all()
    den = mix[:, 2].astype(np.int64) + mix[:, 3]
    t = mix[:, 2].astype(np.int64) * clock16[mix[:, 0], 0] + mix[:, 3].astype(np.int64) * clock16[mix[:, 1], 0]
    half = (2 * np.abs(t)) % (2 * den) == den
    assert (half & (t > 0)).sum() >= 10 and (half & (t < 0)).sum() >= 10 and (t < 0).sum() >= 40          # the corners are there
    assert (den == 65536).sum() >= 40 and (mix[:, 2] == 0).sum() >= 10 and (mix[:, 3] == 0).sum() >= 10
    assert (np.abs(got[half, 0].astype(np.int64)) * 2 * den[half] ==2 * np.abs(t[half]) + den[half]).all()                  # away from zero
    n_half = 0
    for seed in (1, 2, 3):
        clock16, mix = random_cases(seed, 1500)
        got = clock_mix.mix_rows(clock16, mix)
        want = _exact(clock16, mix)
        assert (got == want).all()
        d = (mix[:, 2].astype(np.int64) + mix[:, 3])[:, None]
        tt = mix[:, 2, None].astype(np.int64) * clock16[mix[:, 0]] + mix[:, 3, None].astype(np.int64) * clock16[mix[:, 1]]
        n_half += int(((2 * np.abs(tt)) % (2 * d) == d).sum())
        assert (np.abs(got) <= np.maximum(np.abs(clock16[mix[:, 0]].astype(np.int64)), np.abs(clock16[mix[:, 1]].astype(np.int64)))).all()
    assert n_half >= 50
    for bad in ([[0, 64, 1, 1]], [[-1, 0, 1, 1]], [[0, 0, -1, 2]], [[0, 0, 0, 0]], [[0, 0, 65536, 1]], [[0, 0, 1]], []):
        with pytest.raises(ValueError):
            clock_mix.mix_rows(clock16, bad)


def test_the_equal_mix_is_the_midpoint_and_the_own_mix_the_clock():
    from tdoa_amd import clock_mix, sync_fine
    rng = np.random.default_rng(11)
    rows = rng.integers(-TOP, TOP + 1, size=(40, 5)).astype(np.int32)
    rows[:12] = rng.integers(-6, 7, size=(12, 5))                            # exact halves of both signs
    rows[12] = TOP
    rows[13] = -TOP
    a, b = np.divmod(np.arange(40 * 40), 40)
    mix = np.stack([a, b, np.ones_like(a), np.ones_like(a)], axis=1)
    got = clock_mix.mix_rows(rows, mix)
    want = sync_fine.midpoint_clock16(rows[a], rows[b])
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    odd = (rows[a].astype(np.int64) + rows[b]) % 2 == 1
    assert (odd & (want > 0)).any() and (odd & (want < 0)).any()
    assert clock_mix.mix_rows(rows, clock_mix.own_mix(40)).tobytes() == rows.tobytes()
    same = np.stack([a, b, 7 * np.ones_like(a), 7 * np.ones_like(a)], axis=1)       # equal weights of any size: the same rule
    assert clock_mix.mix_rows(rows, same).tobytes() == want.tobytes()


def test_clock_mix_rows_in_c_returns_the_statements_bytes_and_refuses(capi):
    from tdoa_amd import clock_mix
    for clock16, mix in (corner_cases(), random_cases(5, 2000)):
        got = capi.clock_mix_rows(clock16, mix)
        want = clock_mix.mix_rows(clock16, mix)
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    lib = capi.load()
    i32p = C.POINTER(C.c_int32)
    c16 = np.arange(12, dtype=np.int32).reshape(4, 3)
    rows = np.zeros((2, 3), dtype=np.int32)
    pc, pr = c16.ctypes.data_as(i32p), rows.ctypes.data_as(i32p)

    def call(mix, pc=pc, pr=pr, n=4, S=3, m=2, null_mix=False):
        mm = np.array(mix, dtype=np.int32)
        return lib.tdoa_clock_mix_rows(pc, n, S, None if null_mix else mm.ctypes.data_as(i32p), m, pr)

    ok = [[0, 3, 1, 1], [2, 2, 65536, 0]]
    assert call(ok) == 0 and rows.tolist() == [[5, 6, 7], [6, 7, 8]]            # (9 + 1) div 2, (11 + 1) div 2, (13 + 1) div 2
    for bad in ([0, 4, 1, 1], [4, 0, 1, 1], [-1, 0, 1, 1], [0, -1, 1, 1], [0, 0, -1, 2], [0, 0, 2, -1], [0, 0, 0, 0], [0, 0, 65536, 1],
                [0, 0, 1, 65536], [0, 0, 2 ** 31 - 1, 2 ** 31 - 1]):
        assert call([ok[0], bad]) == 1, bad
    assert call(ok, pc=None) == 1 and call(ok, pr=None) == 1 and call(ok, null_mix=True) == 1
    assert call(ok, n=0) == 1 and call(ok, S=0) == 1 and call(ok, m=0) == 1
    with pytest.raises(capi.TdoaError) as e:
        capi.clock_mix_rows(c16, [[0, 9, 1, 1]])
    assert e.value.status == 1


@pytest.mark.parametrize("spb", [1, 3])
def test_midpoint_mix_reproduces_the_hand_built_clock_table(spb):
    """tests/test_gpu_sync_fine.py::test_cli_sync_fine_prints_the_library_result: np.stack([c[0], midpoint_clock16(c[0], c[2]),
    c[2]]) on whole-block stacks; with spb stacks per block the same, stack by stack"""
    from tdoa_amd import clock_mix, sync_fine
    rng = np.random.default_rng(20 + spb)
    c16 = rng.integers(-40, 41, size=(3 * spb, 3)).astype(np.int32)
    mix = clock_mix.midpoint_mix(spb)
    assert mix.shape == (3 * spb, 4) and mix.dtype == np.int32
    by_hand = np.concatenate([c16[:spb], sync_fine.midpoint_clock16(c16[:spb], c16[2 * spb:]), c16[2 * spb:]])
    assert clock_mix.mix_rows(c16, mix).tobytes() == by_hand.tobytes()
    if spb == 1:
        assert by_hand.tobytes() == np.stack([c16[0], sync_fine.midpoint_clock16(c16[0], c16[2]), c16[2]]).tobytes()
        assert mix.tolist() == [[0, 0, 1, 0], [0, 2, 1, 1], [2, 2, 1, 0]]
    assert (clock_mix.own_mix(4) == [[0, 0, 1, 0], [1, 1, 1, 0], [2, 2, 1, 0], [3, 3, 1, 0]]).all()
    d = clock_mix.pair_differences(np.array([[1, 4, 9]]))
    assert d.tolist() == [[3, 8, 5]]                                          # pairs (0,1), (0,2), (1,2)


def test_the_chains_statement_is_the_three_statements_one_after_another(oracle):
    """[reference | target | reference] = windows 3, 3 and 4 of the measured case as three one-window stacks: sync_locate under
    midpoint_mix(1) returns what sync_fine_stacks, mix_rows and zoom_stacks / zoom_upsampled return when the caller chains them,
    and the target's fix moves when the clocks are dropped"""
    from tdoa_amd import clock_mix, locate, locate_zoom, sync_fine, sync_locate
    ref_delay = measured_case()[0]
    q = np.stack([_float64_q(oracle, reference_window_iq(oracle, 3)), _float64_q(oracle, target_window_iq(oracle, 3)),
                  _float64_q(oracle, reference_window_iq(oracle, 4))])
    Z, H = 2, 3
    table = coarse_table()
    grid = dict(GRID, dlat=GRID["dlat"] / Z, dlon=GRID["dlon"] / Z, rows=(GRID["rows"] - 1) * Z + 1, cols=(GRID["cols"] - 1) * Z + 1)
    fine = locate.grid_table(ST4, sample_rate=FS, **grid)
    mix = clock_mix.midpoint_mix(1)
    for U_loc in (1, 4):
        got = sync_locate.sync_locate(q, ref_delay, table, 64, fine, grid["cols"], ML, Z, H, mix, GATE, ROUNDS, UP, FINE_ROUNDS, None, 1, 1, 1, U_loc)
        found = sync_fine.sync_fine_stacks(q, ref_delay, ML, GATE, ROUNDS, UP, FINE_ROUNDS)
        rows = np.stack([found["clock16"][0], sync_fine.midpoint_clock16(found["clock16"][0], found["clock16"][2]), found["clock16"][2]])
        if U_loc == 1:
            z = locate_zoom.zoom_stacks(q, table, 64, fine, grid["cols"], ML, Z, H, 1, 1, 1, rows)
            bare = locate_zoom.zoom_stacks(q, table, 64, fine, grid["cols"], ML, Z, H, 1, 1, 1, None)
        else:
            z = locate_zoom.zoom_upsampled(q, table, 64, fine, grid["cols"], ML, Z, H, U_loc, 1, 1, 1, rows)
            bare = locate_zoom.zoom_upsampled(q, table, 64, fine, grid["cols"], ML, Z, H, U_loc, 1, 1, 1, None)
        assert set(got) == set(FINE_KEYS) | {"rows"} | set(sync_locate.ZOOM_KEYS)
        for k in FINE_KEYS:
            assert got[k].dtype == found[k].dtype and got[k].tobytes() == found[k].tobytes(), k
        assert got["rows"].tobytes() == rows.tobytes() and got["rows"].any()
        for k, want in zip(sync_locate.ZOOM_KEYS, z):
            assert got[k].dtype == want.dtype and got[k].tobytes() == want.tobytes(), (U_loc, k)
        assert (got["zoom"]["score_q"] > 0).all()
        assert (got["zoom"]["cell"] != bare[4]["cell"]).any()                   # a dropped clock would show
    own = sync_locate.sync_locate(q, ref_delay, table, 64, fine, grid["cols"], ML, Z, H, None, GATE, ROUNDS, UP, FINE_ROUNDS)
    assert own["rows"].tobytes() == own["clock16"].tobytes()


def test_entry_points_declared_bound_and_exported(capi):
    hdr = open(os.path.join(ROOT, "include", "tdoa_mi355x.h"), encoding="utf-8").read()
    go = open(os.path.join(ROOT, "go", "tdoa_cgo.go"), encoding="utf-8").read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for text in ("func (g *gpuCorrelator) ProcessSyncLocate(", "C.tdoa_process_sync_locate(", "func (g *Group) ProcessSyncLocate(",
                 "C.tdoa_group_process_sync_locate(", "func ClockMixRows(", "C.tdoa_clock_mix_rows("):
        assert text in go, text
    assert lib.tdoa_abi_version() == 4                    # additions only
    for method in ("process_sync_locate", "sync_locate_from_q", "debug_clock_mix"):
        assert hasattr(capi.Context, method), method
    assert hasattr(capi.Group, "process_sync_locate") and callable(capi.clock_mix_rows)
    s = capi._search("sync_locate")
    assert s.ints == ("gate", "rounds", "U", "fine_rounds") and s.inputs == ("ref_delay", "centre", "mix")
    assert s.late_ints == ("min_separation", "Z", "H", "fine_separation") and s.stats == "loc"
    keys = [o.key for o in s.outputs]
    assert keys == list(FINE_KEYS) + ["rows", "loc", "loc_lags", "loc_corr", "map", "zoom", "zlags", "zcorr", "zmap"]
    # the table states the header's order: the names of every prototype's parameters
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for route, lead in (("own", ["ctx", "windows_per_stack"]), ("group", ["g", "windows_per_stack"]),
                        ("q", ["ctx", "q", "n_sets", "n_stations", "n_w"])):
        params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % s.entries[route], flat).group(1)
        names = [re.search(r"(\w+)\s*$", p).group(1) for p in params.split(",")]
        assert names == lead + list(s.ints) + list(s.inputs) + list(s.late_ints) + [k + "_host" for k in keys], route
        assert len(getattr(lib, s.entries[route]).argtypes) == len(names)
    text = " ".join(hdr.replace("\n *", " ").split())
    for phrase in ("row[t][s] = sgn(T) ((2 |T| + den) div (2 den))", "(t, t, 1, 0) is the stack's own clock",
                   "(a, b, 1, 1) is the midpoint of two rows", "is neither read nor changed", "mix == NULL: every stack takes its own clock",
                   "wa + wb outside 1 .. 65536", "16 (|centre| + gate + 1) U_loc >= 2^31"):
        assert phrase in text, phrase


def test_null_handle_is_invalid_without_a_device(capi):
    lib = capi.load()
    s = capi._search("sync_locate")
    n_out = len(s.outputs)
    ref = (C.c_int32 * 3)(0, 16, 32)
    q = np.zeros(3 * 7, dtype=np.int64)
    assert lib.tdoa_process_sync_locate(None, 0, 1, 1, 16, 2, ref, None, None, 1, 2, 2, 1, *[None] * n_out) == 1
    assert lib.tdoa_group_process_sync_locate(None, 0, 1, 1, 16, 2, ref, None, None, 1, 2, 2, 1, *[None] * n_out) == 1
    assert lib.tdoa_debug_sync_locate_from_q(None, q.ctypes.data_as(C.POINTER(C.c_int64)), 1, 3, 1, 1, 1, 16, 2, ref, None, None, 1, 2, 2, 1,
                                             *[None] * n_out) == 1
    assert lib.tdoa_debug_clock_mix(None, ref, 1, 3, None, 1, 1, None, None, None) == 1
