"""GPU: the zoomed cell tracks (tdoa_process_locate_track_zoom, tdoa_debug_locate_track_zoom_from_q and the group form;
include/tdoa_mi355x.h, "zoomed cell tracks").

Every comparison is exact: all thirteen outputs are the bytes of the numpy statement (tdoa_amd.locate_track_zoom), and the seven
the call adds are written over a poison pattern from a poisoned workspace.

1. locate_track_zoom_from_q on the small cases of tests/test_locate_zoom_cpu.py: 2, 3, 4 and 17 stations, max_lag 4 and 20, six
   sets as 1 x 6, 2 x 3 and 6 x 1 tracks, windows of 1, 9, 121, 289 and 16 641 positions, fine steps 0, 1 and 16, coarse steps 0, 1
   and 16 (windows that do not touch), clocks, a short last row, U = 1 and 4;
2. the five identities of the header on the library's outputs;
3. the step graph: a replay, a new fine table and new clocks of the same shape, another Z, H, fine_step and fine_separation, the
   statistics setting;
4. end to end through captures, a group of one and of two members; tdoa_processor --locate-track-zoom;
5. what the call refuses;
6. the fine clock lines' block fix of tests/test_locate_track_zoom_cpu.py on the library's own words."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from stack_helpers import same_bytes as _same_bytes, stacks_q as _stacks_q, windows_q as _windows_q
from test_locate_cpu import ST4
from test_locate_upsample_cpu import ML, coarse_table, window_iq
from test_locate_zoom_cpu import FINE_COLS, ZOOM_H, ZOOM_Z, global_fine_table, small_case
from test_locate_track_zoom_cpu import COARSE_KEYS, IDENTITY_CASES, KEYS, Z_KEYS, check_identities, random_case, statement

pytestmark = pytest.mark.gpu

RANKS = (32768, 64880)
FOOT = 49152


def _which(got, want):
    return [k for k, w in zip(KEYS, want) if k not in got or not _same_bytes(got[k], w)]


def _same_outputs(got, want):
    return not _which(got, want)


def _status(fn, *a, **kw):
    import tdoa_amd
    with pytest.raises(tdoa_amd.TdoaError) as e:
        fn(*a, **kw)
    return e.value.status, str(e.value)


def _set_case(c, case, U=1):
    c.locate_set_stats(None)
    c.locate_set_upsample(U)
    c.locate_set_clock(case["clock"])
    c.locate_set_table(case["table"], case["n_cols"])
    c.locate_set_fine_table(case["fine"], case["n_cols_f"])


@pytest.fixture(scope="module")
def contexts():
    import tdoa_amd
    made = {}

    def get(ml):
        if ml not in made:
            made[ml] = tdoa_amd.Context(max_lag=ml, window_len=1024)
        return made[ml]

    yield get
    for c in made.values():
        c.close()


# ---- 1. on the caller's words -------------------------------------------------------------------------------------------
# (track_len, max_step, H, fine_step, fine_separation): six sets as 1 x 6, 2 x 3 and 6 x 1 tracks; H = 0 is one position, 8 is 289
# -- more than one tile of the scores' kernel --, 64 (16 641 positions, the kernel's largest instantiation) is larger than the
# 13 x 19 fine table; with J = 16 the coarse track jumps between the planted corners and the windows do not touch
SHAPES = ((1, 0, 0, 0, 1), (1, 0, 5, 1, 2), (3, 0, 1, 0, 1), (3, 1, 5, 1, 1), (3, 16, 5, 16, 2), (3, 16, 64, 1, 3), (6, 1, 8, 16, 1), (6, 0, 64, 0, 1),
          (6, 16, 1, 1, 1))
WIDE = (3, 1, 64, 16, 1)                                  # every position's 33 x 33 neighbourhood: once


@pytest.mark.parametrize("S, ml, clocked, short, U", [(2, 4, False, False, 1), (2, 20, True, False, 4), (3, 4, True, True, 4),
                                                      (3, 20, False, False, 1), (4, 20, False, True, 1), (4, 20, True, False, 4),
                                                      (17, 4, True, False, 1), (17, 20, False, True, 4)])
def test_locate_track_zoom_from_q_is_the_numpy_statement(contexts, S, ml, clocked, short, U):
    c = contexts(ml)
    planted = small_case(S, ml, 700 + 31 * S + ml + U, clocked, short)
    # the planted words hold a track to its plateau; the same tables under random words alone let it wander
    wander = dict(planted, q=np.random.default_rng(ml + S).integers(-2 ** 40, 2 ** 40, size=planted["q"].shape, dtype=np.int64))
    _set_case(c, planted, U)
    apart, moved = 0, 0
    for case, shapes in ((planted, SHAPES + ((WIDE,) if (S, ml) == (4, 20) else ())), (wander, SHAPES[2:5] + SHAPES[6:7])):
        for L, J, H, Jf, fsep in shapes:
            c.poison_workspace()
            got = c.locate_track_zoom_from_q(case["q"], S, L, case["Z"], H, case["n_w"], J, 1, Jf, fsep)
            want = statement(case, L, J, H, Jf, U, 1, fsep)
            assert got["zmap"].shape == (6, (2 * H + 1) ** 2) and got["ztotal"].shape == (6 // L, (2 * H + 1) ** 2)
            assert _same_outputs(got, want), (L, J, H, Jf, _which(got, want))
            plain = c.locate_track_from_q(case["q"], S, L, case["n_w"], J, 1)          # the coarse six: tdoa_debug_locate_track_from_q's bytes
            assert all(_same_bytes(got[k], plain[k]) for k in COARSE_KEYS)
            if L == 1 and case is planted:                               # the all-zero set's track: the zero record and -1 maps
                assert got["track"][5].tobytes() == bytes(48) and got["ztrack"][5].tobytes() == bytes(48)
                assert (got["zmap"][5] == -1).all() and (got["ztotal"][5] == -1).all() and not got["zcells"][5].any() and not got["zlags"][5].any()
                assert (got["ztrack"]["score_q"][:5] > 0).all() or short
            apart += int(((got["track"]["score_q"] > 0) & (got["ztotal"].max(axis=1) == -1)).sum())
            moved += int((got["ztrack"]["steps"] > 0).sum())
    assert apart > 0 and moved > 0
    c.locate_set_upsample(1)
    c.locate_set_clock(None)


# ---- 2. the identities --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", (1, 4))
def test_identities_on_the_librarys_outputs(contexts, U):
    def run(case, L, J, H, Jf, U, fsep=1):
        c = contexts(case["ml"])
        _set_case(c, case, U)
        return c.locate_track_zoom_from_q(case["q"], case["S"], L, case["Z"], H, case["n_w"], J, 1, Jf, fsep)

    def run_zoom(case, H, U, fsep=1):
        c = contexts(case["ml"])
        _set_case(c, case, U)
        return c.locate_zoom_from_q(case["q"], case["S"], case["Z"], H, case["n_w"], 1, fsep)

    def run_track(case, table, n_cols, L, J, U):
        c = contexts(case["ml"])
        _set_case(c, case, U)
        c.locate_set_table(table, n_cols)                                # the brute force: the whole fine table as the table
        return c.locate_track_from_q(case["q"], case["S"], L, case["n_w"], J, 1)

    for args, kw in IDENTITY_CASES:
        check_identities(random_case(*args, n_w=2, **kw), run, run_zoom, run_track, U)
    for ml in (4, 9):
        contexts(ml).locate_set_upsample(1)
        contexts(ml).locate_set_clock(None)


# ---- 3, 4: through captures ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy(oracle):
    """the twelve windows of tests/test_locate_upsample_cpu.py at noise 0.3, per station: three blocks of 4 windows of 8 192; the
    48 x 64 table and the global 377 x 505 fine table; clocks of a few sixteenths per stack"""
    import tdoa_amd
    wins = [window_iq(oracle, k, 0.3) for k in range(12)]
    caps = [np.concatenate([w[s] for w in wins]) for s in range(4)]
    fine, n_cols_f = global_fine_table()
    clock = np.random.default_rng(5).integers(-24, 25, size=(12, 4)).astype(np.int32)
    with tdoa_amd.Context(max_lag=ML, window_len=8192) as c:
        for s in range(4):
            c.capture_upload(s, caps[s])
        assert c.num_windows() == (4, 12)
        yield c, _windows_q(c), caps, coarse_table(), fine, n_cols_f, clock
        c.locate_set_upsample(1)


def _model(c, q, m, table, fine, n_cols_f, J, Z, H, Jf, U, sep=1, fsep=1, clock=None):
    from tdoa_amd import locate_track_zoom
    Q, n_w = _stacks_q(c, q, m)
    per_block, _ = c.num_stacks(m)
    return locate_track_zoom.track_zoom_upsampled(Q, table, 64, fine, n_cols_f, ML, per_block, J, Z, H, Jf, U, sep, fsep, n_w, clock)


def test_the_step_graph(noisy):
    from tdoa_amd import map_stats
    c, q, _, table, fine, n_cols_f, clock = noisy
    c.locate_set_stats(None)
    c.locate_set_upsample(4)
    c.locate_set_clock(clock)
    c.locate_set_table(table, 64)
    c.locate_set_fine_table(fine, n_cols_f)
    args = dict(windows_per_stack=1, max_step=1, min_separation=2, fine_step=4, fine_separation=1, want_total=True)
    plain = c.process_locate_track(1, 1, 2, want_total=True)
    a = c.process_locate_track_zoom(ZOOM_Z, ZOOM_H, **args)
    first = c.graph_info()
    assert first["memsets"] == 0 and first["roots"] == 1
    want = _model(c, q, 1, table, fine, n_cols_f, 1, ZOOM_Z, ZOOM_H, 4, 4, 2, 1, clock)
    assert a["ztrack"].shape == (3,) and a["zcells"].shape == (3, 4) and _same_outputs(a, want), _which(a, want)
    assert all(_same_bytes(a[k], plain[k]) for k in COARSE_KEYS)        # the coarse stage: tdoa_process_locate_track's bytes
    assert (a["ztrack"]["score_q"] > 0).all() and (a["ztrack"]["steps"] > 0).any()
    c.poison_workspace()
    again = c.process_locate_track_zoom(ZOOM_Z, ZOOM_H, **args)          # the same key: replayed, on poisoned workspace
    assert c.graph_info() == first and all(_same_bytes(again[k], a[k]) for k in KEYS)
    other, ticks = np.ascontiguousarray(fine[::-1]), np.ascontiguousarray(clock[::-1])      # a new fine table and new clocks of the same
    c.locate_set_fine_table(other, n_cols_f)                                                 # shape: data of the same graph
    c.locate_set_clock(ticks)
    moved = c.process_locate_track_zoom(ZOOM_Z, ZOOM_H, **args)
    want = _model(c, q, 1, table, other, n_cols_f, 1, ZOOM_Z, ZOOM_H, 4, 4, 2, 1, ticks)
    assert c.graph_info() == first and _same_outputs(moved, want), _which(moved, want)
    assert not _same_bytes(moved["zmap"], a["zmap"]) and not _same_bytes(moved["ztrack"], a["ztrack"])
    c.locate_set_fine_table(fine, n_cols_f)
    c.locate_set_clock(clock)
    for Z, H, Jf, fsep in ((4, ZOOM_H, 4, 1), (ZOOM_Z, 5, 4, 1), (ZOOM_Z, ZOOM_H, 0, 1), (ZOOM_Z, ZOOM_H, 4, 6)):      # other keys
        got = c.process_locate_track_zoom(Z, H, **dict(args, fine_step=Jf, fine_separation=fsep))
        want = _model(c, q, 1, table, fine, n_cols_f, 1, Z, H, Jf, 4, 2, fsep, clock)
        assert _same_outputs(got, want), (Z, H, Jf, fsep, _which(got, want))
        assert not _same_bytes(got["ztrack"], a["ztrack"]) or not _same_bytes(got["zmap"], a["zmap"])
    c.locate_set_stats(RANKS, FOOT)                                      # the statistics judge the coarse T_0, as after process_locate_track
    judged = c.process_locate_track_zoom(ZOOM_Z, ZOOM_H, **args)
    stats_plain = c.process_locate_track(1, 1, 2, want_total=True)
    c.locate_set_stats(None)
    assert all(_same_bytes(judged[k], a[k]) for k in KEYS) and _same_bytes(judged["stats"], stats_plain["stats"])
    assert judged["stats"].shape == (3,) and (judged["stats"]["n_live"] > 0).all()
    c.locate_set_upsample(1)
    c.locate_set_clock(None)


@pytest.mark.parametrize("m, U, J, Jf", [(1, 16, 1, 8), (2, 1, 0, 0)], ids=["one-window stacks, U = 16", "two-window stacks, U = 1"])
def test_end_to_end_through_captures_and_a_group(noisy, m, U, J, Jf):
    """four stations, windows of 8 192, max_lag 128, three blocks of 4 windows: process_locate_track_zoom is the statement on the
    library's own Q; a group of one member and a group of two (which search the merged sum) return the same bytes"""
    import tdoa_amd
    c, q, caps, table, fine, n_cols_f, _ = noisy
    c.locate_set_clock(None)
    c.locate_set_stats(None)
    c.locate_set_table(table, 64)
    c.locate_set_fine_table(fine, n_cols_f)
    c.locate_set_upsample(U)
    got = c.process_locate_track_zoom(ZOOM_Z, ZOOM_H, m, J, 1, Jf, 2, want_total=True)
    want = _model(c, q, m, table, fine, n_cols_f, J, ZOOM_Z, ZOOM_H, Jf, U, 1, 2)
    assert got["ztrack"].shape == (3,) and got["zcells"].shape == (3, 4 // m) and _same_outputs(got, want), _which(got, want)
    assert (got["ztrack"]["score_q"] >= got["track"]["score_q"]).all() and (got["ztrack"]["positions"] == 4 // m).all()
    c.locate_set_upsample(1)
    for n_members in (1, 2):
        with tdoa_amd.Group([0] * n_members, max_lag=ML, window_len=8192) as g:
            for k in range(n_members):
                for s in range(4):
                    g.member(k).capture_upload(s, caps[s])
            g.locate_set_table(table, 64)
            g.locate_set_fine_table(fine, n_cols_f)
            g.locate_set_upsample(U)
            out = g.process_locate_track_zoom(ZOOM_Z, ZOOM_H, m, J, 1, Jf, 2, want_total=True)
            assert all(_same_bytes(out[k], got[k]) for k in KEYS), (n_members, [k for k in KEYS if not _same_bytes(out[k], got[k])])


# ---- 5. what the call refuses -------------------------------------------------------------------------------------------
def test_refusals():
    import tdoa_amd
    capi = tdoa_amd.capi
    with tdoa_amd.Context(max_lag=4, window_len=1024) as c:
        case = small_case(3, 4, 5)
        q = case["q"]
        run = c.locate_track_zoom_from_q
        status, text = _status(run, q, 3, 3, 3, 1)
        assert status == 6 and "no delay table" in text                  # the tracks': no table
        c.locate_set_table(case["table"], 7)
        status, text = _status(run, q, 3, 3, 3, 1)
        assert status == 6 and "no fine delay table" in text
        c.locate_set_fine_table(case["fine"][:, :2], FINE_COLS)
        status, text = _status(run, q, 3, 3, 3, 1)
        assert status == 6 and "n_stations differs" in text
        c.locate_set_fine_table(case["fine"], FINE_COLS)
        assert run(q, 3, 3, 3, 1)["ztrack"].shape == (2,)
        for kw, what in ((dict(Z=0), "Z outside 1 .. 64"), (dict(Z=65), "Z outside 1 .. 64"), (dict(H=-1), "H outside 0 .. 64"),
                         (dict(H=65), "H outside 0 .. 64"), (dict(fine_step=-1), "fine_step outside 0 .. 16"),
                         (dict(fine_step=17), "fine_step outside 0 .. 16"), (dict(fine_separation=0), "fine_separation < 1"),
                         (dict(max_step=17), "max_step outside 0 .. 16"), (dict(max_step=-1), "max_step outside 0 .. 16"),
                         (dict(min_separation=0), "min_separation < 1")):
            status, text = _status(run, q, 3, 3, **dict(dict(Z=3, H=1), **kw))
            assert status == 1 and what in text, (kw, text)
        status, text = _status(run, q, 3, 4, 3, 1)
        assert status == 1 and "track_len < 1 or not a divisor of n_sets" in text      # the tracks'
        assert run(q, 3, 6, 64, 64, fine_step=16)["ztotal"].shape == (1, 129 * 129) and run(q, 3, 1, 1, 0)["zmap"].shape == (6, 1)
        s = capi._search("locate_track_zoom")
        out = capi._search_outputs(s, capi._shape_numbers({"H": 1}, 6, 3, 35, 3), dict(want_total=True, want_zmap=True, want_ztotal=True))
        ptrs = capi._search_ptrs(s, out)
        pq = q.ctypes.data_as(C.POINTER(C.c_int64))
        fn = c._L.tdoa_debug_locate_track_zoom_from_q
        assert fn(c._h, pq, 6, 3, 3, 2, 0, 1, 3, 1, 0, 1, *(ptrs[:6] + [None] + ptrs[7:])) == 1
        assert "ztrack_host is NULL" in c._L.tdoa_last_error(c._h).decode()
        assert fn(c._h, pq, 6, 3, 3, 2, 0, 1, 3, 1, 0, 1, *([None] + ptrs[1:])) == 1
        assert "track_host is NULL" in c._L.tdoa_last_error(c._h).decode()                      # the tracks'
        assert fn(c._h, pq, 6, 3, 3, 2, 0, 1, 3, 1, 0, 1, ptrs[0], *([None] * 5), ptrs[6], *([None] * 6)) == 0      # the rest may be NULL
        assert int(out["ztrack"]["positions"][0]) == 3
        assert _status(c.process_locate_track_zoom, 3, 1)[0] == 6                # no captures (tdoa_num_stacks)
        status, text = _status(run, q, 3, 3, 3, 1, n_w=2 ** 15)
        assert status == 5 and "a track's sum could overflow" in text            # the tracks': P track_len n_w > 2^17
        c.locate_set_fine_table(None)                                            # forgotten
        assert _status(run, q, 3, 3, 3, 1)[0] == 6
        big = case["fine"].copy()
        big[7, 2] = 2 ** 27                                                      # 16 x 2^27 = 2^31
        c.locate_set_fine_table(big, FINE_COLS)
        c.locate_set_upsample(16)
        status, text = _status(run, q, 3, 3, 3, 1)
        assert status == 5 and "fine delay table entry" in text
        c.locate_set_upsample(8)
        assert run(q, 3, 3, 3, 1)["ztrack"].shape == (2,)
        c.locate_set_upsample(1)
    # TDOA_ERR_NOMEM reaches the caller through the call: the coarse stage's upsampled surfaces, refused by arithmetic.  The call's own
    # planes are at most 65 535 x 16 641 x 10 bytes, 10.9 GB: no arithmetic refuses them on this device, and their message is not
    # reached here
    with tdoa_amd.Context(max_lag=2 ** 20, window_len=64) as c:
        for s in range(4):
            c.synth_capture(s, 256 * 64, ST4[s], (41.20, -96.00, 400.0), 0x10CA7E00 + s)
        c.locate_set_table(np.zeros((4, 4), dtype=np.int32), 2)
        c.locate_set_fine_table(np.zeros((9, 4), dtype=np.int32), 3)
        for kw in (dict(Z=0), dict(Z=65), dict(H=-1), dict(H=65), dict(fine_step=17), dict(fine_separation=0)):
            assert _status(c.process_locate_track_zoom, **dict(dict(Z=2, H=1, windows_per_stack=1), **kw))[0] == 1, kw
        c.locate_set_fine_table(np.zeros((9, 3), dtype=np.int32), 3)
        assert _status(c.process_locate_track_zoom, 2, 1, 1)[0] == 6             # a fine table of another n_stations
        c.locate_set_fine_table(np.zeros((9, 4), dtype=np.int32), 3)
        c.locate_set_upsample(16)
        status, text = _status(c.process_locate_track_zoom, 2, 1, 1)
        assert status == 4 and "do not fit in device memory" in text


# ---- 4 (continued). the command-line tool -------------------------------------------------------------------------------
def test_cli_locate_track_zoom_prints_the_library_result(tmp_path):
    """tdoa_processor --stack=2 --locate=32x32/30 --locate-upsample=4 --locate-track=1 --locate-track-zoom=4/6/3/2 on the golden
    three-station captures: the LOCATE-TRACK lines are unchanged and the TRACKZOOM lines carry what
    Context.process_locate_track_zoom returns on the 125 x 125 fine grid"""
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
    tail = ["--window", "1000", "--max-lag", "150", "162400000", "101700000", str(csv)] + dats
    head = [cli, "--stack=2", "--locate=32x32/30", "--locate-upsample=4", "--locate-track=1"]
    r = subprocess.run(head + ["--locate-track-zoom=4/6/3/2"] + tail, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stderr            # (the 3-station solve may fail on these captures: tests/test_processor_cli.py)
    base = subprocess.run(head + tail, capture_output=True, text=True, timeout=300)
    tracks = [l for l in base.stdout.splitlines() if l.startswith("LOCATE-TRACK block")]
    assert tracks and [l for l in r.stdout.splitlines() if l.startswith("LOCATE-TRACK block")] == tracks
    rows = [re.match(r"TRACKZOOM block (\d): cell=(-?\d+) lat=([-\d.]+) lon=([-\d.]+) positions=(\d+) steps=(\d+) score=([\d.]+) runner=([\d.]+) "
                     r"runner_cell=(\d+) cells=([\d,]+)$", l) for l in r.stdout.splitlines() if l.startswith("TRACKZOOM block")]
    assert len(rows) == 3 and all(rows), r.stdout
    lat_c, lon_c, h_c = (sum(x[k] / 3 for x in st) for k in range(3))
    dlat, dlon = 30.0 / 111.32 / 31, 30.0 / (111.32 * np.cos(lat_c * np.pi / 180)) / 31
    lat0, lon0 = lat_c - dlat * 31 / 2, lon_c - dlon * 31 / 2
    with tdoa_amd.Context(max_lag=150, window_len=1000) as c:
        for s, p in enumerate(dats):
            c.capture_upload_file(s, p)
        grid = tdoa_amd.capi.locate_grid_table
        c.locate_set_table(grid(st, lat0, lon0, dlat, dlon, 32, 32, h_c, c.params.sample_rate), 32)
        c.locate_set_fine_table(grid(st, lat0, lon0, dlat / 4, dlon / 4, 125, 125, h_c, c.params.sample_rate), 125)
        c.locate_set_upsample(4)
        out = c.process_locate_track_zoom(4, 6, 2, 1, 1, 3, 2)
    assert out["zcells"].shape == (3, 2)                                  # blocks of four windows: two stacks each
    for m, z, cells in zip(rows, out["ztrack"], out["zcells"]):
        assert int(z["score_q"]) > 0
        assert [int(m.group(k)) for k in (2, 5, 6, 9)] == [int(z[n]) for n in ("cell", "positions", "steps", "runner_cell")]
        assert [int(x) for x in m.group(10).split(",")] == cells.tolist()
        assert abs(float(m.group(3)) - (lat0 + (int(z["cell"]) // 125) * dlat / 4)) <= 5.1e-7
        assert abs(float(m.group(4)) - (lon0 + (int(z["cell"]) % 125) * dlon / 4)) <= 5.1e-7
        assert abs(float(m.group(7)) - float(z["score"])) <= 5.1e-7 and abs(float(m.group(8)) - float(z["runner_up"])) <= 5.1e-7
    bad = subprocess.run(head + ["--locate-track-zoom=4/6/17"] + tail, capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "--locate-track-zoom=Z[/H[/JF[/SEP]]]" in bad.stderr
    large = subprocess.run([cli, "--stack", "--locate=600x600/30", "--locate-track=1", "--locate-track-zoom=8"] + tail, capture_output=True, text=True,
                           timeout=300)
    assert large.returncode == 1 and "more than 2^22 cells" in large.stderr
    alone = subprocess.run([cli, "--stack", "--locate=32x32/30", "--locate-track-zoom=4"] + tail, capture_output=True, text=True, timeout=300)
    assert alone.returncode == 1 and "--locate-track-zoom needs --stack --locate --locate-track" in alone.stderr


# ---- 6. the block fix on the library's own words --------------------------------------------------------------------------
def test_the_block_fix_on_the_librarys_own_words(oracle):
    """blocks 0 .. 2 of the measured case of tests/test_sync_drift_fine_cpu.py as captures of [12 reference | 12 target | 12
    reference] windows of 8 192: the clock rows are the library's own fine lines -- the reference blocks under theirs, the target
    block under block 1's continued -- and process_locate_track_zoom on one-window stacks (J = 0, Jf = 0, Z = 8, H = 16, U = 16: one
    captured graph for the three captures) is the statement on the library's own words in all thirteen outputs; the target block's
    fix against the two-step fix of tests/test_locate_track_zoom_cpu.py is printed, and equal wherever that test's conditions hold"""
    import tdoa_amd
    from tdoa_amd import locate_track_zoom, sync_drift_fine
    from test_locate_track_zoom_cpu import DEMO, compare_block_fix
    from test_sync_drift_fine_cpu import LINE, M_POS, reference_windows_iq, target_windows_iq
    from test_sync_fine_cpu import WL, measured_case
    ref_delay = measured_case()[0]
    line_args = tuple(LINE[k] for k in ("G", "H", "D", "R", "U", "Rf"))
    coarse = coarse_table()
    fine, n_cols_f = global_fine_table()
    graphs = []
    with tdoa_amd.Context(max_lag=ML, window_len=WL) as c:
        c.locate_set_table(coarse, 64)
        c.locate_set_fine_table(fine, n_cols_f)
        for b in range(3):
            ref, tgt = reference_windows_iq(oracle, b), target_windows_iq(oracle, b)
            for s in range(4):
                c.capture_upload(s, np.concatenate([w[s] for blk in (ref, tgt, ref) for w in blk]))
            assert c.num_stacks(1) == (M_POS, 3 * M_POS)
            c.locate_set_upsample(1)
            line = c.process_sync_drift_fine(ref_delay, 1, *line_args)
            continued = sync_drift_fine.line_clock16(line["clock16"][0], line["fine_rate"][0], LINE["U"], LINE["D"], M_POS, M_POS)
            clock = np.concatenate([line["fine_rows"][:M_POS], continued, line["fine_rows"][2 * M_POS:]]).astype(np.int32)
            q = _windows_q(c)
            c.locate_set_clock(clock)
            c.locate_set_upsample(DEMO["U"])
            c.poison_workspace()
            got = c.process_locate_track_zoom(DEMO["Z"], DEMO["H"], 1, DEMO["J"], 1, DEMO["Jf"], 1, want_total=True)
            graphs.append(c.graph_info())
            want = locate_track_zoom.track_zoom_upsampled(q, coarse, 64, fine, n_cols_f, ML, M_POS, DEMO["J"], DEMO["Z"], DEMO["H"], DEMO["Jf"],
                                                          DEMO["U"], 1, 1, 1, clock)
            assert _same_outputs(got, want), (b, _which(got, want))
            assert (got["ztrack"]["score_q"] > 0).all() and (got["ztrack"]["steps"] == 0).all()
            target = {k: got[k][1:2] for k in ("track", "cells", "ztrack", "zcells")}
            covered, d_call, d_two = compare_block_fix(b, q[M_POS:2 * M_POS], continued.astype(np.int64), target, coarse, fine, n_cols_f)
            print("block %d: the target block's fix under the library's fine line continued %.0f m, the two-step fix %.0f m (covered: %s)"
                  % (b, d_call, d_two, covered))
            c.locate_set_clock(None)
    assert graphs[1] == graphs[0] and graphs[2] == graphs[0]             # new captures and new clocks are data of the same graph
