"""GPU: the delay-table search (tdoa_locate_set_table, tdoa_process_locate, tdoa_group_process_locate,
tdoa_debug_locate_from_q; include/tdoa_mi355x.h, "delay-table search").

Every comparison with the numpy model (tdoa_amd.locate) is exact: process_stacked(1, 1, 1, want_partial=True) returns each
window's fixed-point q word for word, their sums are the stacks' Q, the model turns those into records, lags, correlations
and maps.

1. the definition: the outputs are the model's bytes over stacks of 1, 2 and whole blocks, a grid table and a random one with
   a short last row and many pairs outside the range, min_separation 1 and 5;
2. locate_from_q: the hand-worked cases of tests/test_locate_cpu.py, 16 stations on small integers with partial tiles and
   several tiles, 64 stations (the generic station loop), words of magnitude 2^62 div P;
3. the noisy case of tests/test_locate_cpu.py: the six argmaxes miss, the table search finds the planted cell;
4. the step graph replays, a new table of the same shape leaves it as it is, and its neighbours keep their bytes;
5. a group of members on one device returns a single context's bytes;
6. argument and state errors on a live context;
7. tdoa_processor --stack --locate prints what Context.process_locate returns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from stack_helpers import same_bytes as _same_bytes, stacks_q as _stacks_q, windows_q as _windows_q
from test_locate_cpu import FS, GRID, ST4, _check_hand_case, hand_cases, noisy_case, noisy_windows, own_lags

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ST = ST4[:3]
TX = (41.20, -96.00, 400.0)


def _synth(c, n_stations, block):
    for s in range(n_stations):
        c.synth_capture(s, block, ST[s % 3], TX, 0x10CA7E00 + s)


def _same_outputs(got, want):
    """got: process_locate's dict; want: the model's (records, lags, corr, map)"""
    names = ("loc", "lags", "corr", "map")
    return all(_same_bytes(got[k], w) for k, w in zip(names, want) if k in got)


def _model(c, q, m, table, n_cols, sep):
    from tdoa_amd import locate
    Q, n_w = _stacks_q(c, q, m)
    return locate.locate_stacks(Q, table, n_cols, c.params.max_lag, sep, n_w)


def _grid_table(stations, **kw):
    from tdoa_amd import locate
    return locate.grid_table(stations, sample_rate=FS, **{**GRID, **kw})


def _random_table(n_cells, n_stations, span, seed):
    return np.random.default_rng(seed).integers(-span, span + 1, size=(n_cells, n_stations), dtype=np.int32)


TABLES = {"grid": lambda: (_grid_table([ST[s % 3] for s in range(4)]), 64),          # 48 x 64
          "random": lambda: (_random_table(1000, 4, 16 * 900, 41), 37)}              # 27 rows of 37 and one of 1


@pytest.fixture(scope="module")
def four_stations():
    """4 stations (6 pairs), windows of 10 000, 5 per block, 1399 lags"""
    import tdoa_amd
    wl, wpb, ml = 10_000, 5, 700
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        _synth(c, 4, wpb * wl)
        assert c.num_pairs() == 6
        yield c, _windows_q(c)


@pytest.mark.parametrize("name", sorted(TABLES))
@pytest.mark.parametrize("m", [1, 2, 0])
def test_definition_against_the_model(four_stations, m, name):
    from tdoa_amd import locate
    c, q = four_stations
    table, n_cols = TABLES[name]()
    c.locate_set_table(table, n_cols)
    lag = locate.pair_lags(table)
    inside = (lag > -700) & (lag < 700)
    for sep in (1, 5):
        got = c.process_locate(m, sep, want_map=True)
        want = _model(c, q, m, table, n_cols, sep)
        n = c.num_stacks(m)[1]
        assert got["loc"].shape == (n,) and got["lags"].shape == got["corr"].shape == (n, 6) and got["map"].shape == (n, len(table))
        assert _same_outputs(got, want), (m, name, sep, got["loc"][:2], want[0][:2])
        loc = got["loc"]
        assert (loc["score_q"] > 0).all() and (loc["runner_q"] <= loc["score_q"]).all()
        assert (got["map"][np.arange(n), loc["cell"]] == loc["score_q"]).all()
        assert (got["map"][np.arange(n), loc["runner_cell"]] == loc["runner_q"]).all()
        assert (loc["pairs_in"] == inside[loc["cell"]].sum(axis=1)).all()
        assert (got["lags"] == np.where(inside[loc["cell"]], lag[loc["cell"]], 0)).all()
        far = np.maximum(abs(loc["cell"] // n_cols - loc["runner_cell"] // n_cols), abs(loc["cell"] % n_cols - loc["runner_cell"] % n_cols))
        assert (far > sep).all()
        print("m %d %s sep %d: cells %s pairs_in %s, %d of %d cells with a pair outside" % (m, name, sep, loc["cell"][:4].tolist(),
                                                                                          loc["pairs_in"][:4].tolist(), (~inside.all(axis=1)).sum(), len(table)))
    assert _same_bytes(c.process_locate(m, 1)["loc"], _model(c, q, m, table, n_cols, 1)[0])        # without the map


@pytest.fixture(scope="module")
def tiny():
    import tdoa_amd
    with tdoa_amd.Context(max_lag=4, window_len=1024) as c:
        yield c


@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_locate_from_q_hand_worked_cases(tiny, name, arg, want):
    from tdoa_amd import locate
    tiny.locate_set_table(arg["table"], arg["n_cols"])
    got = tiny.locate_from_q(arg["q"], 3, arg["n_w"], arg["sep"])
    assert got["loc"].shape == (1,)
    _check_hand_case((got["loc"][0], got["lags"][0], got["corr"][0], got["map"][0]), arg, want)
    model = locate.locate(arg["q"], arg["table"], arg["n_cols"], arg["ml"], arg["sep"], arg["n_w"])
    assert _same_outputs(got, [x[None] for x in model])


@pytest.mark.parametrize("n_cells, n_cols", [(257, 19), (4099, 64)])
def test_locate_from_q_sixteen_stations_three_sets(n_cells, n_cols):
    """120 pairs, max_lag 24, small integers (equal maxima everywhere), n_sets = 3; 257 cells: a full tile and one cell,
    4099: seventeen tiles; delays up to +-30 samples, so some pairs fall outside"""
    import tdoa_amd
    from tdoa_amd import locate
    rng = np.random.default_rng(43)
    S, ml = 16, 24
    q = rng.integers(-3, 4, size=(3, S * (S - 1) // 2, 2 * ml - 1), dtype=np.int64)
    table = _random_table(n_cells, S, 16 * 15, 47)
    with tdoa_amd.Context(max_lag=ml, window_len=1024) as c:
        c.locate_set_table(table, n_cols)
        for sep, n_w in ((1, 1), (2, 7)):
            got = c.locate_from_q(q, S, n_w, sep)
            assert got["loc"].shape == (3,) and got["map"].shape == (3, n_cells)
            assert _same_outputs(got, locate.locate_stacks(q, table, n_cols, ml, sep, n_w)), (sep, n_w)
            assert (got["loc"]["pairs_in"] <= 120).all() and (got["loc"]["runner_q"] <= got["loc"]["score_q"]).all()
        one = c.locate_from_q(q[1], S, 1, 1)
        assert all(one[k][0].tobytes() == c.locate_from_q(q, S, 1, 1)[k][1].tobytes() for k in one)
        c.locate_set_table(table)                                   # a plain list: columns only
        assert _same_outputs(c.locate_from_q(q, S, 1, 3), locate.locate_stacks(q, table, n_cells, ml, 3, 1))


def test_locate_from_q_sixty_four_stations():
    """2016 pairs: more stations than stay in registers, more pairs than the finishing kernel has threads"""
    import tdoa_amd
    from tdoa_amd import locate
    rng = np.random.default_rng(53)
    S, ml, n_cells, n_cols = 64, 12, 300, 21
    q = rng.integers(-3, 4, size=(2, S * (S - 1) // 2, 2 * ml - 1), dtype=np.int64)
    table = _random_table(n_cells, S, 16 * 8, 59)
    with tdoa_amd.Context(max_lag=ml, window_len=1024) as c:
        c.locate_set_table(table, n_cols)
        got = c.locate_from_q(q, S, 2, 1)
        assert _same_outputs(got, locate.locate_stacks(q, table, n_cols, ml, 1, 2))
        assert (got["loc"]["score_q"] > 0).all() and (got["map"][[0, 1], got["loc"]["cell"]] == got["loc"]["score_q"]).all()
        print("pairs_in %s of 2016" % got["loc"]["pairs_in"].tolist())


def test_locate_from_q_large_words_do_not_overflow():
    """words of magnitude 2^62 div P: a cell with every pair at the largest word scores P (2^62 div P) <= 2^62"""
    import tdoa_amd
    from tdoa_amd import locate
    rng = np.random.default_rng(61)
    S, ml, P = 4, 9, 6
    big = 2 ** 62 // P
    q = rng.choice(np.array([-big, -big + 1, 0, 5, big - 1, big], dtype=np.int64), size=(2, P, 2 * ml - 1))
    q[0, :, ml - 1] = (big, -big, big, -big, big, -big)            # set 0: the cell of equal delays reaches the bound
    table = _random_table(500, S, 16 * 6, 67)
    table[123] = 1000
    with tdoa_amd.Context(max_lag=ml, window_len=1024) as c:
        c.locate_set_table(table, 25)
        got = c.locate_from_q(q, S, 3, 1)
        assert _same_outputs(got, locate.locate_stacks(q, table, 25, ml, 1, 3))
        assert int(got["loc"]["score_q"][0]) == P * big and (got["loc"]["score_q"] > 0).all() and (got["map"] >= 0).all()


def test_the_table_search_finds_the_cell_the_six_argmaxes_miss(oracle):
    """the inputs of tests/test_locate_cpu.py, the 12 windows repeated over the three blocks, one window per stack: the records
    are the model's; per block the six independent argmaxes are all right in at most 2 windows, the best cell is the planted
    one in at least 11"""
    import tdoa_amd
    wl, ml = 8192, 128
    table, planted_cell, delays, planted = noisy_case()
    wins = noisy_windows(oracle, delays)
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        for s in range(4):
            c.capture_upload(s, np.concatenate([w[s] for w in wins] * 3))
        assert c.num_windows() == (12, 36)
        c.locate_set_table(table, 64)
        got = c.process_locate(1, 1, want_map=True)
        q = _windows_q(c)
        assert _same_outputs(got, _model(c, q, 1, table, 64, 1))
        for block in range(3):
            loc = got["loc"][12 * block:12 * (block + 1)]
            own_ok = sum(own_lags(q[12 * block + w], ml) == planted for w in range(12))
            cell_ok = int((loc["cell"] == planted_cell).sum())
            print("block %d: the six argmaxes all right in %d of 12 windows, the best cell the planted one in %d; score / runner-up %s"
                  % (block, own_ok, cell_ok, np.round(loc["score"] / loc["runner_up"], 2).tolist()))
            assert (loc["pairs_in"] == 6).all()
            assert own_ok <= 2
            assert cell_ok >= 11


def test_graph_replays_and_leaves_its_neighbours_alone():
    import tdoa_amd
    wl, wpb, ml = 10_000, 5, 700
    stations = [ST[s % 3] for s in range(4)]
    grid, moved_grid = _grid_table(stations), _grid_table(stations, lat0=GRID["lat0"] + 0.01)
    other, other_cols = TABLES["random"]()
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        _synth(c, 4, wpb * wl)
        q = _windows_q(c)
        base = c.process()
        drift = c.process_stacked_drift(2, 5, 2, 8, 8, want_surface=True, want_partial=True)
        track = c.process_track(2, 1, want_surface=True, want_total=True)
        clos = c.process_closure(2, 37, 1)
        stack = c.process_stacked(2, 8, 8, want_surface=True, want_partial=True)
        stack_nodes = c.graph_info()["nodes"]                    # the step, the stack's accumulation and its four finishing kernels
        c.locate_set_table(grid, 64)
        a = c.process_locate(2, 1, want_map=True)
        first = c.graph_info()                                   # ... and the scores, the runner-up's pass and two finishes
        assert first["memsets"] == 0 and first["roots"] == 1 and first["nodes"] == stack_nodes
        assert _same_outputs(a, _model(c, q, 2, grid, 64, 1))
        c.poison_workspace()
        b = c.process_locate(2, 1, want_map=True)                # the same key: replayed, on poisoned workspace
        assert c.graph_info() == first and all(_same_bytes(a[k], b[k]) for k in a)
        c.locate_set_table(moved_grid, 64)                       # a new table of the same shape: the same graph
        moved = c.process_locate(2, 1, want_map=True)
        assert c.graph_info() == first
        assert _same_outputs(moved, _model(c, q, 2, moved_grid, 64, 1)) and not _same_bytes(moved["map"], a["map"])
        c.locate_set_table(grid, 64)                             # ... and back
        assert all(_same_bytes(c.process_locate(2, 1, want_map=True)[k], a[k]) for k in a)
        assert _same_bytes(c.process(), base)
        mid = c.process_stacked(2, 8, 8, want_surface=True, want_partial=True)
        assert all(_same_bytes(mid[k], stack[k]) for k in stack)
        c.locate_set_table(other, other_cols)                    # another n_cells: another graph of the same shape
        far = c.process_locate(2, 3, want_map=True)
        info = c.graph_info()
        assert info["memsets"] == 0 and info["roots"] == 1 and info["nodes"] == first["nodes"]
        assert _same_outputs(far, _model(c, q, 2, other, other_cols, 3))
        c.locate_set_table(grid, 64)
        assert all(_same_bytes(c.process_locate(2, 1, want_map=True)[k], a[k]) for k in a)
        assert _same_bytes(c.process(), base)
        after = c.process_stacked(2, 8, 8, want_surface=True, want_partial=True)
        assert all(_same_bytes(after[k], stack[k]) for k in stack)
        after = c.process_stacked_drift(2, 5, 2, 8, 8, want_surface=True, want_partial=True)
        assert all(_same_bytes(after[k], drift[k]) for k in drift)
        after = c.process_track(2, 1, want_surface=True, want_total=True)
        assert all(_same_bytes(after[k], track[k]) for k in track)
        assert _same_bytes(c.process_closure(2, 37, 1), clos)
    with tdoa_amd.Context(max_lag=ml, window_len=wl, windows_per_batch=1) as c:     # a stack spans several launch groups
        _synth(c, 4, wpb * wl)
        c.locate_set_table(grid, 64)
        assert all(_same_bytes(c.process_locate(2, 1, want_map=True)[k], a[k]) for k in a)
        c.locate_set_table(other, other_cols)
        assert all(_same_bytes(c.process_locate(2, 3, want_map=True)[k], far[k]) for k in far)


@pytest.mark.parametrize("n_members", [2, 3])
def test_group_returns_a_single_contexts_bytes(n_members):
    import tdoa_amd
    block, wl, ml = 50_000, 10_000, 300
    table, n_cols = _random_table(700, 4, 16 * 350, 71), 29
    with tdoa_amd.Group([0] * n_members, max_lag=ml, window_len=wl) as g, tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        for target in [g.member(k) for k in range(n_members)] + [c]:
            _synth(target, 4, block)
        with pytest.raises(tdoa_amd.TdoaError) as e:                 # no table yet
            g.process_locate(0, 1)
        assert e.value.status == 6
        g.locate_set_table(table, n_cols)
        c.locate_set_table(table, n_cols)
        wants = {}
        for m in (2, 0):
            for sep in (1, 4):
                want = wants[m, sep] = c.process_locate(m, sep, want_map=True)
                got = g.process_locate(m, sep, want_map=True)
                again = g.process_locate(m, sep, want_map=True)      # the members replay their steps
                assert (want["loc"]["score_q"] > 0).all()
                assert all(_same_bytes(got[k], want[k]) and _same_bytes(again[k], want[k]) for k in want), (m, sep)
        with pytest.raises(tdoa_amd.TdoaError) as e:
            g.process_locate(0, 0)
        assert e.value.status == 1
    with tdoa_amd.Group([0], max_lag=ml, window_len=wl) as g:        # a group of one calls the member
        _synth(g.member(0), 4, block)
        g.locate_set_table(table, n_cols)
        got = g.process_locate(2, 4, want_map=True)
        assert all(_same_bytes(got[k], wants[2, 4][k]) for k in got)


def test_argument_and_state_errors():
    import tdoa_amd
    wl, ml = 1024, 64
    table = _random_table(50, 3, 16 * 40, 73)

    def status(fn, *a, **kw):
        with pytest.raises(tdoa_amd.TdoaError) as e:
            fn(*a, **kw)
        return e.value.status

    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:
        c.locate_set_table(table, 10)                                # needs no captures
        assert status(c.process_locate, 0, 1) == 6                   # ... the search does
        _synth(c, 3, 4 * wl)
        assert c.process_locate(0, 1)["loc"].shape == (3,)
        for kw in ({"min_separation": 0}, {"windows_per_stack": -1}):
            assert status(c.process_locate, **kw) == 1, kw
        assert c._L.tdoa_process_locate(c._h, 0, 1, None, None, None, None) == 1
        f = c._L.tdoa_locate_set_table
        pt = table.ctypes.data_as(f.argtypes[1])
        for n_cells, n_cols, S in ((-1, 10, 3), (2 ** 22 + 1, 10, 3), (50, 0, 3), (50, -3, 3), (50, 10, 1), (50, 10, 65)):
            assert f(c._h, pt, n_cells, n_cols, S) == 1, (n_cells, n_cols, S)
        assert c.process_locate(0, 1)["loc"].shape == (3,)           # a refused table leaves the old one
        c.locate_set_table(None)                                     # forgotten
        assert status(c.process_locate, 0, 1) == 6
        assert f(c._h, pt, 0, 10, 3) == 0 and status(c.process_locate, 0, 1) == 6      # n_cells == 0 forgets too
        c.locate_set_table(_random_table(50, 4, 16 * 40, 79), 10)    # a table for four stations
        assert status(c.process_locate, 0, 1) == 6
        # the debug entry
        q = np.zeros((1, 3, 2 * ml - 1), dtype=np.int64)
        assert status(c.locate_from_q, q, 3) == 6                    # the table's n_stations
        c.locate_set_table(None)
        assert status(c.locate_from_q, q, 3) == 6                    # no table
        c.locate_set_table(table, 10)
        loc = np.zeros(1, dtype=tdoa_amd.capi.LOCATION_DTYPE)
        d = c._L.tdoa_debug_locate_from_q
        pq, pl = q.ctypes.data_as(d.argtypes[1]), loc.ctypes.data_as(d.argtypes[6])
        for n_sets, S, n_w, sep in ((0, 3, 1, 1), (65536, 3, 1, 1), (1, 1, 1, 1), (1, 65, 1, 1), (1, 3, 0, 1), (1, 3, 1, 0)):
            assert d(c._h, pq, n_sets, S, n_w, sep, pl, None, None, None) == 1, (n_sets, S, n_w, sep)
        assert d(c._h, None, 1, 3, 1, 1, pl, None, None, None) == 1 and d(c._h, pq, 1, 3, 1, 1, None, None, None, None) == 1
        # the overflow bound: P n_w <= 2^17; 3 * 43 690 = 131 070, 3 * 43 691 = 131 073
        assert d(c._h, pq, 1, 3, 43690, 1, pl, None, None, None) == 0
        assert d(c._h, pq, 1, 3, 43691, 1, pl, None, None, None) == 5
    with tdoa_amd.Context(max_lag=ml, window_len=wl) as c:           # one station: no pair
        _synth(c, 1, 4 * wl)
        loc = np.zeros(3, dtype=tdoa_amd.capi.LOCATION_DTYPE)
        assert c._L.tdoa_process_locate(c._h, 0, 1, loc.ctypes.data_as(C.c_void_p), None, None, None) == 5
    with tdoa_amd.Context(max_lag=ml, window_len=wl, lag_mode=tdoa_amd.capi.LAGS_GO) as c:
        _synth(c, 3, 5 * wl)
        c.locate_set_table(table, 10)
        assert status(c.process_locate, 0, 1) == 5


def test_cli_locate_prints_the_library_result(tmp_path):
    """tdoa_processor --stack --locate=32x32/30 on the golden three-station captures: one LOCATE line per stack with what
    process_locate returns for the same grid; --locate without --stack is refused; without --locate no line changes"""
    import tdoa_amd
    tdoa_amd.build.build()
    cli = tdoa_amd.build.build_cli()
    csv = tmp_path / "lat-lon-table.csv"
    csv.write_text("Name,Latitude,Longitude,Elevation\nKEVO,41.30888549464701,-96.02619229605524,356.0\n"
                   "162400000,41.25703803095629,-95.95512763589404,349.07\nkx0u,41.18660274289527,-95.96064116595667,355.69\n"
                   "n3pay,41.24669616513154,-96.08366304481238,329.0\nkf0mtl,41.32916620016985,-96.03513381562004,373.18\n")
    dats = [os.path.join(GOLD, "sim-%s-1754900000.dat" % n) for n in ("kx0u", "n3pay", "kf0mtl")]
    opts = ["--window", "2000", "--max-lag", "150"]
    tail = ["162400000", "101700000", str(csv)] + dats
    r = subprocess.run([cli, "--stack", "--locate=32x32/30"] + opts + tail, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stderr            # (the 3-station solve may fail on these captures: tests/test_processor_cli.py)
    rows = re.findall(r"^LOCATE block (\d) stack (\d+): cell=(\d+) lat=(-?[\d.]+) lon=(-?[\d.]+) pairs=(\d+) score=([\d.]+) "
                      r"runner=([\d.]+)$", r.stdout, flags=re.M)
    assert len(rows) == 3, r.stdout
    # the tool's grid: 30 km on a side around the stations' centroid at their mean height, 111.32 km per degree of latitude
    lat_c, lon_c, h_c = (sum(s[k] / 3 for s in ST) for k in range(3))
    dlat, dlon = 30.0 / 111.32 / 31, 30.0 / (111.32 * np.cos(lat_c * np.pi / 180)) / 31
    lat0, lon0 = lat_c - dlat * 31 / 2, lon_c - dlon * 31 / 2
    with tdoa_amd.Context(max_lag=150, window_len=2000) as c:
        for s, p in enumerate(dats):
            c.capture_upload_file(s, p)
        assert c.num_stacks(0) == (1, 3)
        c.locate_set_table(tdoa_amd.capi.locate_grid_table(ST, lat0, lon0, dlat, dlon, 32, 32, h_c, c.params.sample_rate), 32)
        out = c.process_locate(0, 1)["loc"]
    for row in rows:
        rec = out[int(row[0]) - 1]
        cell = int(rec["cell"])
        assert int(row[1]) == 0 and int(row[2]) == cell and int(row[5]) == int(rec["pairs_in"]) == 3
        assert abs(float(row[3]) - (lat0 + (cell // 32) * dlat)) <= 5.1e-7 and abs(float(row[4]) - (lon0 + (cell % 32) * dlon)) <= 5.1e-7
        for text, value in ((row[6], float(rec["score"])), (row[7], float(rec["runner_up"]))):
            assert abs(float(text) - value) <= 5.1e-7
    assert sorted(int(row[0]) for row in rows) == [1, 2, 3]
    plain = subprocess.run([cli, "--stack"] + opts + tail, capture_output=True, text=True, timeout=300)
    assert plain.returncode in (0, 3) and "LOCATE" not in plain.stdout
    assert plain.stdout == "".join(l for l in r.stdout.splitlines(True) if not l.startswith("LOCATE "))
    alone = subprocess.run([cli, "--locate=32x32/30"] + opts + tail, capture_output=True, text=True, timeout=300)
    assert alone.returncode == 1 and "--locate needs --stack" in alone.stderr
    huge = subprocess.run([cli, "--stack", "--locate=100000x100000/30"] + opts + tail, capture_output=True, text=True, timeout=300)
    assert huge.returncode == 1 and "2^22" in huge.stderr                # refused where the option is read
