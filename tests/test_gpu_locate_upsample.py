"""GPU: sub-sample locate (tdoa_locate_set_upsample, tdoa_debug_upsample_q and the group form; include/tdoa_mi355x.h,
"sub-sample locate").

Every comparison is exact.  The upsampler's words are tdoa_amd.upsample's; with U > 1 every search of the delay-table family
returns the bytes of its existing numpy statement on upsample(q, U), U table, U clock, U guard and max_lag' = (max_lag - 1) U + 1.

1. upsample_q over rows shorter than the taps, one word past a tile and three tiles, every U, on a poisoned output;
2. the four tdoa_debug_locate*_from_q entries against their statements, with and without clocks; the map statistics;
3. the setting and the step graph: U = 1 set explicitly, U = 1 -> 16 -> 1 -> 16, a new table of the same shape;
4. end to end through captures, a group of one and of two members;
5. what the setting refuses;
6. the noisy case of tests/test_locate_upsample_cpu.py on the library's own words;
7. tdoa_processor --locate-upsample prints what Context.process_locate returns."""
import os
import re
import subprocess

import numpy as np
import pytest

from stack_helpers import same_bytes as _same_bytes, stacks_q as _stacks_q, windows_q as _windows_q
from test_locate_cpu import FS, GRID, ST4, hand_cases
from test_locate_upsample_cpu import FACTORS, FINE_SIDE, ML, coarse_table, edge_rows, fine_cell, fine_table, window_iq

pytestmark = pytest.mark.gpu

RANKS = (32768, 64880)
FOOT = 49152
SEARCH = ("loc", "lags", "corr", "map")
TRACK = ("track", "cells", "own", "lags", "corr", "total")
TRACK_MULTI = ("track", "cells", "own", "pairs", "lags", "corr", "total")


def _same_outputs(got, want, names):
    return all(_same_bytes(got[k], w) for k, w in zip(names, want) if k in got)


def _which(got, want, names):
    return [k for k, w in zip(names, want) if k in got and not _same_bytes(got[k], w)]


def _status(fn, *a, **kw):
    import tdoa_amd
    with pytest.raises(tdoa_amd.TdoaError) as e:
        fn(*a, **kw)
    return e.value.status, str(e.value)


def _statement(kind, q, table, n_cols, ml, U, n_w, clock=None, sep=1, K=1, guard=0, L=1, J=0):
    """the existing numpy function of the search on the scaled arguments"""
    from tdoa_amd import locate, locate_multi, locate_track, locate_track_multi, upsample
    t, k, g, ml_u = upsample.scaled_args(table, clock, guard, ml, U)
    qu = upsample.upsample(q, U)
    if kind == "locate":
        return locate.locate_stacks(qu, t, n_cols, ml_u, sep, n_w, k)
    if kind == "multi":
        return locate_multi.locate_multi_stacks(qu, t, n_cols, ml_u, K, g, sep, n_w, k)
    if kind == "track":
        return locate_track.track_stacks(qu, t, n_cols, ml_u, L, J, sep, n_w, k)
    return locate_track_multi.track_multi_stacks(qu, t, n_cols, ml_u, L, J, K, g, sep, n_w, k)


# ---- 1. the upsampler ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ml", [4, 129, 300])
def test_upsample_q_is_the_numpy_statement(ml):
    """max_lag 4: 7 lags, shorter than the taps' span; 129: 257 lags, one word past a tile of 256; 300: 599 lags, three tiles, the
    last one short.  Rows: random words up to 2^60, rows of +-2^60, and a delta in the first and last lag of every tile"""
    import tdoa_amd
    from tdoa_amd import upsample
    n = 2 * ml - 1
    rows = [edge_rows(n, 300 + ml)]
    for at in sorted({0, min(255, n - 1), min(256, n - 1), min(511, n - 1), min(512, n - 1), n - 1}):
        d = np.zeros((1, n), dtype=np.int64)
        d[0, at] = -(2 ** 60) if at % 2 else 2 ** 60
        rows.append(d)
    q = np.concatenate(rows)
    with tdoa_amd.Context(max_lag=ml, window_len=1024) as c:
        for U in FACTORS:
            got = c.upsample_q(q, U)                                     # (written over a poisoned array)
            want = upsample.upsample(q, U)
            assert got.shape == (len(q), (n - 1) * U + 1)
            assert _same_bytes(got, want), (U, np.argwhere(got != want)[:4].tolist())
            assert (got[:, ::U] == q).all()
        assert _same_bytes(c.upsample_q(q[3], 4), upsample.upsample(q[3], 4))        # one row
        assert _same_bytes(c.upsample_q(q, 1), q)
        assert _status(c.upsample_q, q, 3)[0] == 1


# ---- 2. the four searches on the caller's words -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    import tdoa_amd
    with tdoa_amd.Context(max_lag=4, window_len=1024) as c:
        yield c
        c.locate_set_upsample(1)


@pytest.mark.parametrize("U", [16, 4])
@pytest.mark.parametrize("name, arg, want", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_locate_from_q_hand_cases(tiny, name, arg, want, U):
    tiny.locate_set_clock(None)
    tiny.locate_set_table(arg["table"], arg["n_cols"])
    tiny.locate_set_upsample(U)
    got = tiny.locate_from_q(arg["q"], 3, arg["n_w"], arg["sep"])
    model = _statement("locate", arg["q"][None], arg["table"], arg["n_cols"], arg["ml"], U, arg["n_w"], sep=arg["sep"])
    assert _same_outputs(got, model, SEARCH), _which(got, model, SEARCH)
    if want is None:
        assert got["loc"].tobytes() == bytes(48) and not got["map"].any()


@pytest.fixture(scope="module")
def five():
    """5 stations (10 pairs), max_lag 32 (63 lags), a 12 x 16 table, 8 sets of 3 windows: every other set's rows start 8 bytes off
    a 16-byte line"""
    import tdoa_amd
    rng = np.random.default_rng(83)
    q = rng.integers(-2 ** 44, 2 ** 44, size=(8, 10, 63), dtype=np.int64)
    q[:, :, ::5] *= 8                                                   # a few words stand out
    table = rng.integers(-16 * 30, 16 * 30 + 1, size=(192, 5), dtype=np.int32)
    clock = rng.integers(-16 * 6, 16 * 6 + 1, size=(8, 5), dtype=np.int32)
    with tdoa_amd.Context(max_lag=32, window_len=1024) as c:
        c.locate_set_table(table, 16)
        yield c, q, table, clock
        c.locate_set_upsample(1)


@pytest.mark.parametrize("clocked", [False, True], ids=["no clocks", "clocks"])
@pytest.mark.parametrize("U", [16, 4])
def test_the_four_searches_from_q(five, U, clocked):
    """locate; locate_multi with K = 3, guard 2; locate_track with J = 1, L = 4; locate_track_multi with K = 2"""
    c, q, table, clock = five
    k = clock if clocked else None
    c.locate_set_clock(k)
    c.locate_set_stats(None)
    c.locate_set_upsample(U)
    c.poison_workspace()
    got = c.locate_from_q(q, 5, 3, 2)
    want = _statement("locate", q, table, 16, 32, U, 3, k, sep=2)
    assert _same_outputs(got, want, SEARCH), _which(got, want, SEARCH)
    assert (got["loc"]["score_q"] > 0).all() and (np.abs(got["lags"]) % U != 0).any()          # fine lags between the whole ones
    got = c.locate_multi_from_q(q, 5, 3, 3, 2, 2)
    want = _statement("multi", q, table, 16, 32, U, 3, k, sep=2, K=3, guard=2)
    assert _same_outputs(got, want, SEARCH), _which(got, want, SEARCH)
    assert (got["loc"]["score_q"][1:] > 0).any()
    got = c.locate_track_from_q(q, 5, 4, 3, 1, 2)
    want = _statement("track", q, table, 16, 32, U, 3, k, sep=2, L=4, J=1)
    assert got["track"].shape == (2,) and _same_outputs(got, want, TRACK), _which(got, want, TRACK)
    got = c.locate_track_multi_from_q(q, 5, 4, 3, 1, 2, 2, 2)
    want = _statement("track_multi", q, table, 16, 32, U, 3, k, sep=2, K=2, guard=2, L=4, J=1)
    assert got["track"].shape == (2, 2) and _same_outputs(got, want, TRACK_MULTI), _which(got, want, TRACK_MULTI)
    c.locate_set_clock(None)


def test_map_statistics_on_the_upsampled_planes(five):
    from tdoa_amd import map_stats
    c, q, table, _ = five
    c.locate_set_clock(None)
    c.locate_set_upsample(4)
    plain = c.locate_from_q(q, 5, 3, 2)
    c.locate_set_stats(RANKS, FOOT)
    got = c.locate_from_q(q, 5, 3, 2)
    c.locate_set_stats(None)
    rec, _, _, planes = _statement("locate", q, table, 16, 32, 4, 3, sep=2)
    assert _same_bytes(got["stats"], map_stats.stats(planes, rec, 16, RANKS, FOOT, 2, 3))
    assert all(_same_bytes(got[k], plain[k]) for k in plain) and (got["stats"]["n_live"] > 0).all()


# ---- 3, 4, 6: through captures ------------------------------------------------------------------------------------------
def _noisy_captures(oracle):
    """the twelve windows of tests/test_locate_upsample_cpu.py at noise 0.3, per station: three blocks of 4 windows of 8 192"""
    wins = [window_iq(oracle, k, 0.3) for k in range(12)]
    return [np.concatenate([w[s] for w in wins]) for s in range(4)]


@pytest.fixture(scope="module")
def noisy(oracle):
    import tdoa_amd
    caps = _noisy_captures(oracle)
    with tdoa_amd.Context(max_lag=ML, window_len=8192) as c:
        for s in range(4):
            c.capture_upload(s, caps[s])
        assert c.num_windows() == (4, 12)
        yield c, _windows_q(c), caps
        c.locate_set_upsample(1)


def _process_statement(c, q, m, table, n_cols, U, sep=1):
    Q, n_w = _stacks_q(c, q, m)
    return _statement("locate", Q, table, n_cols, ML, U, n_w, sep=sep)


def test_the_setting_and_the_step_graph(noisy):
    import tdoa_amd
    c, q, caps = noisy
    table = coarse_table()
    with tdoa_amd.Context(max_lag=ML, window_len=8192) as fresh:         # a context that never heard of the setting
        for s in range(4):
            fresh.capture_upload(s, caps[s])
        fresh.locate_set_table(table, 64)
        never = fresh.process_locate(0, 1, want_map=True)
    c.locate_set_clock(None)
    c.locate_set_table(table, 64)
    for U in (1, 16, 1, 16):
        c.locate_set_upsample(U)
        got = c.process_locate(0, 1, want_map=True)
        want = _process_statement(c, q, 0, table, 64, U)
        assert _same_outputs(got, want, SEARCH), (U, _which(got, want, SEARCH))
        if U == 1:
            assert all(_same_bytes(got[k], never[k]) for k in never)
        again = c.process_locate(0, 1, want_map=True)                    # the replay
        assert all(_same_bytes(again[k], got[k]) for k in got), U
    nodes = c.graph_info()["nodes"]
    from tdoa_amd import locate
    other = locate.grid_table(ST4, sample_rate=FS, **{**GRID, "lat0": GRID["lat0"] + 0.0017, "lon0": GRID["lon0"] - 0.0021})
    c.locate_set_table(other, 64)                                        # a new table of the same shape: data of the same graph
    got = c.process_locate(0, 1, want_map=True)
    want = _process_statement(c, q, 0, other, 64, 16)
    assert _same_outputs(got, want, SEARCH), _which(got, want, SEARCH)
    assert c.graph_info()["nodes"] == nodes and not _same_bytes(got["map"], again["map"])
    c.locate_set_upsample(1)
    assert c.graph_info()["nodes"] == nodes                              # (a setting: nothing runs)
    assert c.process_locate(0, 1)["loc"].shape == (3,) and c.graph_info()["nodes"] < nodes


@pytest.mark.parametrize("m", [1, 0], ids=["one-window stacks", "whole blocks"])
def test_end_to_end_through_captures_and_a_group(noisy, m):
    """four stations, windows of 8 192, max_lag 128, three blocks of 4 windows: process_locate with U = 16 is the statement on the
    library's own Q; a group of one member and a group of two (which upsamples the merged sum) return the same bytes"""
    import tdoa_amd
    c, q, caps = noisy
    table = coarse_table()
    c.locate_set_clock(None)
    c.locate_set_table(table, 64)
    c.locate_set_upsample(16)
    got = c.process_locate(m, 2, want_map=True)
    want = _process_statement(c, q, m, table, 64, 16, sep=2)
    assert got["loc"].shape == ({1: 12, 0: 3}[m],) and _same_outputs(got, want, SEARCH), _which(got, want, SEARCH)
    assert (got["loc"]["pairs_in"] == 6).all() and (got["loc"]["score_q"] > 0).all()
    multi = c.process_locate_multi(m, 2, 3, 2, want_map=True)
    Q, n_w = _stacks_q(c, q, m)
    want_multi = _statement("multi", Q, table, 64, ML, 16, n_w, sep=2, K=2, guard=3)
    assert _same_outputs(multi, want_multi, SEARCH), _which(multi, want_multi, SEARCH)
    c.locate_set_upsample(1)
    for n_members in (1, 2):
        with tdoa_amd.Group([0] * n_members, max_lag=ML, window_len=8192) as g:
            for k in range(n_members):
                for s in range(4):
                    g.member(k).capture_upload(s, caps[s])
            g.locate_set_table(table, 64)
            g.locate_set_upsample(16)
            out = g.process_locate(m, 2, want_map=True)
            assert all(_same_bytes(out[k], got[k]) for k in got), (n_members, [k for k in got if not _same_bytes(out[k], got[k])])
            g.locate_set_upsample(1)
            assert not _same_bytes(g.process_locate(m, 2, want_map=True)["lags"], got["lags"])


def test_the_noisy_case_on_the_librarys_words(noisy):
    """per window: the coarse cell, then the fine grid around it with U = 16 -- the cells of the CPU statement on the library's Q"""
    from tdoa_amd import locate
    c, q, _ = noisy
    c.locate_set_clock(None)
    c.locate_set_upsample(1)
    c.locate_set_table(coarse_table(), 64)
    coarse = c.process_locate(1, 1)["loc"]["cell"]
    assert coarse.tolist() == [int(locate.locate(q[k], coarse_table(), 64, ML, 1)[0]["cell"]) for k in range(12)]
    c.locate_set_upsample(16)
    for k in range(12):
        table = fine_table(int(coarse[k]))
        c.locate_set_table(table, FINE_SIDE)
        got = c.process_locate(1, 1)
        assert int(got["loc"]["cell"][k]) == fine_cell(q[k], int(coarse[k]), 16), k
        if k == 0:
            want = _process_statement(c, q, 1, table, FINE_SIDE, 16)
            assert _same_outputs(got, want, SEARCH), _which(got, want, SEARCH)
    c.locate_set_upsample(1)
    print("coarse cells %s" % [(int(x) // 64, int(x) % 64) for x in coarse])


# ---- 5. what the setting refuses ----------------------------------------------------------------------------------------
def test_refusals():
    import tdoa_amd
    with tdoa_amd.Context(max_lag=4, window_len=1024) as c:
        assert _status(c.locate_set_upsample, 3)[0] == 1 and _status(c.locate_set_upsample, 0)[0] == 1
        assert _status(c.locate_set_upsample, 32)[0] == 1
        q = np.ones((1, 1, 7), dtype=np.int64)
        table = np.array([[0, 16], [0, 32]], dtype=np.int32)
        c.locate_set_table(table, 2)
        n_w = 2 ** 15 + 1                                                # P n_w <= 2^17 < 4 P n_w
        assert c.locate_from_q(q, 2, n_w)["loc"]["cell"].shape == (1,)
        for U in FACTORS:
            c.locate_set_upsample(U)
            status, text = _status(c.locate_from_q, q, 2, n_w)
            assert status == 5 and "upsampled" in text
            assert c.locate_from_q(q, 2, 2 ** 15)["loc"]["score_q"][0] > 0          # 4 P n_w = 2^17 exactly
            status, text = _status(c.locate_track_from_q, q.repeat(2, axis=0), 2, 2, 2 ** 14 + 1)
            assert status == 5 and "upsampled" in text                   # 4 P track_len n_w > 2^17
        c.locate_set_table(np.array([[0, 2 ** 27]], dtype=np.int32), 1)  # 16 x 2^27 = 2^31
        c.locate_set_upsample(16)
        status, text = _status(c.locate_from_q, q, 2)
        assert status == 5 and "table entry" in text
        c.locate_set_upsample(8)
        assert c.locate_from_q(q, 2)["loc"].shape == (1,)
        c.locate_set_table(table, 2)
        c.locate_set_upsample(16)
        c.locate_set_clock(np.array([[0, -(2 ** 27)]], dtype=np.int32))
        status, text = _status(c.locate_from_q, q, 2)
        assert status == 5 and "clock table entry" in text
    # the surfaces' size, refused by arithmetic before anything is allocated: 768 one-window stacks x 6 pairs x 33.5 M fine lags
    # are 1.2 TB
    with tdoa_amd.Context(max_lag=2 ** 20, window_len=64) as c:
        for s in range(4):
            c.synth_capture(s, 256 * 64, ST4[s], (41.20, -96.00, 400.0), 0x10CA7E00 + s)
        assert c.num_stacks(1) == (256, 768)
        c.locate_set_table(np.zeros((4, 4), dtype=np.int32), 2)
        c.locate_set_upsample(16)
        status, text = _status(c.process_locate, 1, 1)
        assert status == 4 and "upsampled surfaces [768 stacks][6 pairs]" in text and "do not fit in device memory" in text


# ---- 7. the command-line tool -------------------------------------------------------------------------------------------
def test_cli_locate_upsample_prints_the_library_result(tmp_path):
    """tdoa_processor --stack --locate=32x32/30 --locate-upsample=4 on the golden three-station captures: the LOCATE lines carry
    what Context.process_locate returns with the setting on; a bad U is refused"""
    import tdoa_amd
    tdoa_amd.build.build()
    cli = tdoa_amd.build.build_cli()
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    st = ST4[:3]
    csv = tmp_path / "lat-lon-table.csv"
    csv.write_text("Name,Latitude,Longitude,Elevation\nKEVO,41.30888549464701,-96.02619229605524,356.0\n"
                   "162400000,41.25703803095629,-95.95512763589404,349.07\nkx0u,41.18660274289527,-95.96064116595667,355.69\n"
                   "n3pay,41.24669616513154,-96.08366304481238,329.0\nkf0mtl,41.32916620016985,-96.03513381562004,373.18\n")
    dats = [os.path.join(gold, "sim-%s-1754900000.dat" % n) for n in ("kx0u", "n3pay", "kf0mtl")]
    tail = ["--window", "2000", "--max-lag", "150", "162400000", "101700000", str(csv)] + dats
    r = subprocess.run([cli, "--stack", "--locate=32x32/30", "--locate-upsample=4"] + tail, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stderr            # (the 3-station solve may fail on these captures: tests/test_processor_cli.py)
    rows = [re.match(r"LOCATE block (\d) stack 0: cell=(\d+) .* pairs=(\d+) score=([\d.]+) runner=([\d.]+)$", l) for l in r.stdout.splitlines()
            if l.startswith("LOCATE block")]
    assert len(rows) == 3 and all(rows), r.stdout
    lat_c, lon_c, h_c = (sum(x[k] / 3 for x in st) for k in range(3))
    dlat, dlon = 30.0 / 111.32 / 31, 30.0 / (111.32 * np.cos(lat_c * np.pi / 180)) / 31
    with tdoa_amd.Context(max_lag=150, window_len=2000) as c:
        for s, p in enumerate(dats):
            c.capture_upload_file(s, p)
        c.locate_set_table(tdoa_amd.capi.locate_grid_table(st, lat_c - dlat * 31 / 2, lon_c - dlon * 31 / 2, dlat, dlon, 32, 32, h_c,
                                                           c.params.sample_rate), 32)
        c.locate_set_upsample(4)
        loc = c.process_locate(0, 1)["loc"]
    for m, l in zip(rows, loc):
        assert (int(m.group(2)), int(m.group(3))) == (int(l["cell"]), int(l["pairs_in"]))
        assert abs(float(m.group(4)) - float(l["score"])) <= 5.1e-7 and abs(float(m.group(5)) - float(l["runner_up"])) <= 5.1e-7
    bad = subprocess.run([cli, "--stack", "--locate=32x32/30", "--locate-upsample=3"] + tail, capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "--locate-upsample=U" in bad.stderr
    alone = subprocess.run([cli, "--stack", "--locate-upsample=4"] + tail, capture_output=True, text=True, timeout=300)
    assert alone.returncode == 1 and "--locate-upsample needs --stack --locate" in alone.stderr
