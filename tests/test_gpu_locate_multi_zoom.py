"""GPU: the zoomed rounds (tdoa_process_locate_multi_zoom, tdoa_debug_locate_multi_zoom_from_q and the group form;
include/tdoa_mi355x.h, "zoomed rounds").

Every comparison is exact: all nine outputs are the bytes of the numpy statement (tdoa_amd.locate_multi_zoom), and the zoom's five
are written over a poison pattern from a poisoned workspace.

1. locate_multi_zoom_from_q on the small cases of tests/test_locate_multi_zoom_cpu.py: 2, 3, 4, 15, 16 and 17 stations (15 and 16
   straddle the masked register form's limit, 17 re-reads), max_lag 4 and 20, windows of 1, 9, 289 and 16 641 positions, 1, 2, 3
   and 8 rounds, guards 0, 1 and the whole range, clocks, U = 1 and 4, the short last row; a sentinel plane behind every z output;
2. the identities: one round is the zoom locate, the coarse four are the rounds', the table as the fine table;
3. the step graph: replay, new tables and clocks of the same shape, other keys, the statistics setting;
4. end to end through captures, a group of one and of two members;
5. the two-emitter case of tests/test_locate_multi_zoom_cpu.py on the library's own words;
6. what the call refuses;
7. tdoa_processor --zoom-emitters prints what Context.process_locate_multi_zoom returns."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from stack_helpers import same_bytes as _same_bytes, stacks_q as _stacks_q, windows_q as _windows_q
from test_locate_cpu import ST4
from test_locate_multi_zoom_cpu import (CLAIM, KEYS, N_A, N_B, check_claim, claim_figures, multi_case, statement, two_emitter_windows)
from test_locate_upsample_cpu import ML, coarse_table, window_iq
from test_locate_zoom_cpu import FINE_COLS, ZOOM_H, ZOOM_Z, global_fine_table

pytestmark = pytest.mark.gpu

COARSE, Z_KEYS = KEYS[:4], KEYS[4:]
RANKS = (32768, 64880)
FOOT = 49152


def _which(got, want):
    return [k for k, w in zip(KEYS, want) if k in got and not _same_bytes(got[k], w)]


def _same_outputs(got, want):
    return all(k in got for k in KEYS) and not _which(got, want)


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


def _outputs(n_sets, S, n_cells, H, K):
    """the entry's nine arrays with K planes, the z outputs poisoned, and their pointers"""
    from tdoa_amd import capi
    s = capi._search("locate_multi_zoom")
    out = capi._search_outputs(s, capi._shape_numbers({"H": H}, n_sets, S, n_cells, K=K), {"want_map": True, "want_zmap": True})
    return out, capi._search_ptrs(s, out)


def _from_q_with_a_sentinel(c, case, H, K, guard, fsep):
    """tdoa_debug_locate_multi_zoom_from_q into arrays of K + 1 planes: plane K of every z output keeps its poison bytes; -> the K
    planes"""
    q = np.ascontiguousarray(case["q"], dtype=np.int64)
    out, ptrs = _outputs(len(q), case["S"], len(case["table"]), H, K + 1)
    c._chk(c._L.tdoa_debug_locate_multi_zoom_from_q(c._h, q.ctypes.data_as(C.POINTER(C.c_int64)), len(q), case["S"], case["n_w"], K,
                                                    2 * case["ml"] if guard is None else guard, 1, case["Z"], H, fsep, *ptrs))
    for k in Z_KEYS:
        assert (out[k][K].view(np.uint8) == 0xA5).all(), k
    return {k: np.ascontiguousarray(v[:K]) for k, v in out.items()}


# ---- 1. on the caller's words -------------------------------------------------------------------------------------------
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


# (H, fine_separation, K, guard; None: 2 max_lag): 1, 9, 289 (a tile of 256 and 33 more) and 16 641 positions (larger than the 13 x 19
# fine table)
COMBOS = ((0, 1, 1, 0), (1, 1, 2, 1), (8, 1, 3, None), (64, 3, 8, 1), (8, 2, 8, 0), (1, 1, 3, None), (0, 1, 2, 0))


@pytest.mark.parametrize("S, ml, clocked, short, U", [(2, 4, False, False, 1), (2, 20, True, False, 4), (3, 4, True, True, 4),
                                                      (3, 20, False, False, 1), (4, 20, False, True, 1), (4, 20, True, False, 4),
                                                      (15, 4, True, False, 1), (15, 20, False, True, 4), (16, 4, False, False, 4),
                                                      (16, 20, True, True, 1), (17, 4, True, False, 1), (17, 20, False, True, 4)])
def test_locate_multi_zoom_from_q_is_the_numpy_statement(contexts, S, ml, clocked, short, U):
    """six sets in one call, each with two or three planted emitters of decreasing magnitude, the sixth all zero"""
    c = contexts(ml)
    case = multi_case(S, ml, 700 + 31 * S + ml + U, clocked, short)
    _set_case(c, case, U)
    later = 0
    for H, fsep, K, guard in COMBOS:
        c.poison_workspace()
        got = _from_q_with_a_sentinel(c, case, H, K, guard, fsep)
        want = statement(case, H, K, guard, U, 1, fsep)
        assert got["zmap"].shape == (K, 6, (2 * H + 1) ** 2) and got["zpairs"].shape == (K, 6, 2)
        assert _same_outputs(got, want), (H, K, guard, _which(got, want))
        assert (got["loc"]["score_q"][0, :5] > 0).all() and got["loc"][:, 5].tobytes() == bytes(48 * K)
        assert got["zoom"][:, 5].tobytes() == bytes(64 * K) and (got["zmap"][:, 5] == -1).all() and not got["zpairs"][:, 5].any()
        later += int((got["zoom"]["score_q"][1:] > 0).sum())
    assert later >= 5                                                    # later rounds found fine cells
    c.locate_set_upsample(1)
    c.locate_set_clock(None)


# ---- 2. the identities --------------------------------------------------------------------------------------------------
def test_the_identities(contexts):
    c = contexts(9)
    case = multi_case(4, 9, 91, clocked=True)
    _set_case(c, case, 4)
    q, S, Z, n_w = case["q"], 4, case["Z"], case["n_w"]
    one = c.locate_multi_zoom_from_q(q, S, Z, 2, n_w, 1, 1, 2, 2)
    zoom = c.locate_zoom_from_q(q, S, Z, 2, n_w, 2, 2)
    for k in ("loc", "lags", "corr", "map", "zoom", "zlags", "zcorr", "zmap"):               # K = 1: the zoom locate's eight arrays
        assert one[k].shape == (1,) + zoom[k].shape and _same_bytes(one[k][0], zoom[k]), k
    assert one["zpairs"][0, :, 0].tolist() == zoom["zoom"]["pairs_in"].tolist() and not one["zpairs"][0, :, 1].any()
    for K, guard in ((3, 1), (8, 0)):
        got = c.locate_multi_zoom_from_q(q, S, Z, 2, n_w, K, guard, 2, 2)
        rounds = c.locate_multi_from_q(q, S, n_w, K, guard, 2)
        assert all(_same_bytes(got[k], rounds[k]) for k in COARSE), K                      # the coarse four: the rounds' bytes
        assert all(_same_bytes(got[k][0], one[k][0]) for k in KEYS), K                     # round 0 of every K is K = 1
    c.locate_set_fine_table(case["table"], case["n_cols"])                                   # Z = 1 on the table itself
    got = c.locate_multi_zoom_from_q(q, S, 1, 2, n_w, 3, 1)
    assert (got["loc"]["score_q"][1] > 0).sum() >= 3 and (got["loc"]["reserved"] > 0).any()
    for name in ("cell", "score_q", "pairs_in", "score"):
        assert got["zoom"][name].tolist() == got["loc"][name].tolist(), name
    assert got["zpairs"][..., 0].tolist() == got["loc"]["pairs_in"].tolist() and got["zpairs"][..., 1].tolist() == got["loc"]["reserved"].tolist()
    assert _same_bytes(got["zlags"], got["lags"]) and _same_bytes(got["zcorr"], got["corr"])
    c.locate_set_upsample(1)
    c.locate_set_clock(None)


# ---- 3, 4: through captures ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy(oracle):
    """the noisy captures of tests/test_gpu_locate_zoom.py: the twelve windows of tests/test_locate_upsample_cpu.py at noise 0.3,
    per station three blocks of 4 windows of 8 192; the 48 x 64 table and the global 377 x 505 fine table"""
    import tdoa_amd
    wins = [window_iq(oracle, k, 0.3) for k in range(12)]
    caps = [np.concatenate([w[s] for w in wins]) for s in range(4)]
    fine, n_cols_f = global_fine_table()
    with tdoa_amd.Context(max_lag=ML, window_len=8192) as c:
        for s in range(4):
            c.capture_upload(s, caps[s])
        assert c.num_windows() == (4, 12)
        yield c, _windows_q(c), caps, coarse_table(), fine, n_cols_f
        c.locate_set_upsample(1)


def _model(c, q, m, table, fine, n_cols_f, Z, H, U, K, guard, sep=1, fsep=1, clock=None):
    from tdoa_amd import locate_multi_zoom
    Q, n_w = _stacks_q(c, q, m)
    return locate_multi_zoom.multi_zoom_upsampled(Q, table, 64, fine, n_cols_f, ML, Z, H, U, K, guard, sep, fsep, n_w, clock)


def test_the_step_graph(noisy):
    c, q, _, table, fine, n_cols_f = noisy
    rng = np.random.default_rng(5)
    clocks = [np.zeros((12, 4), dtype=np.int32), rng.integers(-40, 41, size=(12, 4)).astype(np.int32)]
    c.locate_set_stats(None)
    c.locate_set_upsample(4)
    c.locate_set_clock(clocks[0])
    c.locate_set_table(table, 64)
    c.locate_set_fine_table(fine, n_cols_f)
    Z, H = ZOOM_Z, 8
    call = lambda K=2, guard=2, Z=Z, H=H, fsep=1: c.process_locate_multi_zoom(Z, H, 1, K, guard, 2, fsep, want_map=True)
    model = lambda K=2, guard=2, Z=Z, H=H, fsep=1, table=table, fine=fine, clock=clocks[0]: \
        _model(c, q, 1, table, fine, n_cols_f, Z, H, 4, K, guard, 2, fsep, clock)
    plain = c.process_locate_multi(1, 2, 2, 2, want_map=True)
    a = call()
    first = c.graph_info()
    assert first["memsets"] == 0 and first["roots"] == 1
    want = model()
    assert _same_outputs(a, want), _which(a, want)
    assert all(_same_bytes(a[k], plain[k]) for k in COARSE)             # the coarse stage: tdoa_process_locate_multi's bytes
    assert (a["zoom"]["score_q"] > 0).all()
    c.poison_workspace()
    again = call()                                                       # the same key: replayed, on poisoned workspace
    assert c.graph_info() == first and all(_same_bytes(again[k], a[k]) for k in KEYS)
    other_fine, other_table = np.ascontiguousarray(fine[::-1]), np.ascontiguousarray(table[::-1])
    c.locate_set_fine_table(other_fine, n_cols_f)                        # new tables and clocks of the same shape: data of the same graph
    got, want = call(), model(fine=other_fine)
    assert c.graph_info() == first and _same_outputs(got, want), _which(got, want)
    assert not _same_bytes(got["zmap"], a["zmap"]) and all(_same_bytes(got[k], a[k]) for k in COARSE)
    c.locate_set_fine_table(fine, n_cols_f)
    c.locate_set_table(other_table, 64)
    got, want = call(), model(table=other_table)
    assert c.graph_info() == first and _same_outputs(got, want), _which(got, want)
    assert not _same_bytes(got["loc"], a["loc"])
    c.locate_set_table(table, 64)
    c.locate_set_clock(clocks[1])
    got, want = call(), model(clock=clocks[1])
    assert c.graph_info() == first and _same_outputs(got, want), _which(got, want)
    assert not _same_bytes(got["zoom"], a["zoom"])
    c.locate_set_clock(clocks[0])
    base = model()
    for kw in (dict(K=3), dict(guard=1), dict(Z=4), dict(H=5), dict(fsep=6)):                # other keys
        # the last graph captured is the base call's: a word missing from the key would replay it with the base call's launch
        # arguments and return the base call's z outputs, which the statement says are not this call's
        assert all(_same_bytes(call()[k], a[k]) for k in KEYS), kw
        got, want = call(**kw), model(**kw)
        assert any(not _same_bytes(w, b) for w, b in zip(want[4:], base[4:])), kw
        assert _same_outputs(got, want), (kw, _which(got, want))
        if "K" in kw:
            assert c.graph_info()["nodes"] > first["nodes"]              # (a round more is more launches; the window's stay two)
    assert not _same_bytes(got["zoom"], a["zoom"])
    c.locate_set_stats(RANKS, FOOT)                                      # the statistics judge the coarse maps, as after the rounds
    judged = call()
    stats_plain = c.process_locate_multi(1, 2, 2, 2, want_map=True)
    c.locate_set_stats(None)
    assert all(_same_bytes(judged[k], a[k]) for k in KEYS) and _same_bytes(judged["stats"], stats_plain["stats"])
    assert judged["stats"].shape == a["loc"].shape
    c.locate_set_clock(None)
    c.locate_set_upsample(1)


@pytest.mark.parametrize("m, U", [(1, 16), (0, 1)], ids=["one-window stacks, U = 16", "whole blocks, U = 1"])
def test_end_to_end_through_captures_and_a_group(noisy, m, U):
    """four stations, windows of 8 192, max_lag 128, three blocks of 4 windows: process_locate_multi_zoom is the statement on the
    library's own Q; a group of one member and a group of two (which search the merged sum) return the same bytes"""
    import tdoa_amd
    c, q, caps, table, fine, n_cols_f = noisy
    c.locate_set_clock(None)
    c.locate_set_stats(None)
    c.locate_set_table(table, 64)
    c.locate_set_fine_table(fine, n_cols_f)
    c.locate_set_upsample(U)
    got = c.process_locate_multi_zoom(ZOOM_Z, ZOOM_H, m, 3, 2, 1, 2, want_map=True)
    want = _model(c, q, m, table, fine, n_cols_f, ZOOM_Z, ZOOM_H, U, 3, 2, 1, 2)
    assert got["zoom"].shape == (3, {1: 12, 0: 3}[m]) and _same_outputs(got, want), _which(got, want)
    assert (got["zoom"]["pairs_in"][0] == 6).all() and (got["zoom"]["score_q"][0] >= got["loc"]["score_q"][0]).all()
    c.locate_set_upsample(1)
    for n_members in (1, 2):
        with tdoa_amd.Group([0] * n_members, max_lag=ML, window_len=8192) as g:
            for k in range(n_members):
                for s in range(4):
                    g.member(k).capture_upload(s, caps[s])
            g.locate_set_table(table, 64)
            g.locate_set_fine_table(fine, n_cols_f)
            g.locate_set_upsample(U)
            out = g.process_locate_multi_zoom(ZOOM_Z, ZOOM_H, m, 3, 2, 1, 2, want_map=True)
            assert all(_same_bytes(out[k], got[k]) for k in KEYS), (n_members, [k for k in KEYS if not _same_bytes(out[k], got[k])])


# ---- 5. the two-emitter case --------------------------------------------------------------------------------------------
def test_the_weak_emitter_gets_a_sub_cell_fix_on_the_librarys_words(oracle):
    """the inputs of tests/test_locate_multi_zoom_cpu.py: three blocks of four stacks of 8 windows of A and 2 of B, captures
    uploaded, one call for the twelve stacks; the outputs are the statement's on the library's own Q, and the CPU test's three
    bounds hold.  Printed on one MI355X: A (round 0): coarse cell centre 137.5 m, zoomed fix 31.6 m, within 100 m 12 of 12, within
    150 m 12 of 12; B (round 1): coarse cell centre 137.5 m, zoomed fix 38.2 m (ratio 0.28), within 100 m 10 of 12, within 150 m
    11 of 12 -- the float64 pipeline's figures"""
    import tdoa_amd
    table = coarse_table()
    fine, n_cols_f = global_fine_table()
    stacks = two_emitter_windows(oracle)
    m = N_A + N_B
    with tdoa_amd.Context(max_lag=ML, window_len=8192) as c:
        for s in range(4):
            c.capture_upload(s, np.concatenate([x[s] for stack in stacks for x in stack]))
        assert c.num_windows() == (4 * m, 12 * m)
        c.locate_set_table(table, 64)
        c.locate_set_fine_table(fine, n_cols_f)
        c.locate_set_upsample(CLAIM["U"])
        got = c.process_locate_multi_zoom(ZOOM_Z, ZOOM_H, m, CLAIM["K"], CLAIM["guard"], CLAIM["sep"], CLAIM["fsep"])
        want = _model(c, _windows_q(c), m, table, fine, n_cols_f, ZOOM_Z, ZOOM_H, CLAIM["U"], CLAIM["K"], CLAIM["guard"], CLAIM["sep"], CLAIM["fsep"])
        assert not _which(got, want), _which(got, want)
    check_claim(claim_figures(got["loc"], got["zoom"]), "the library's words")


# ---- 6. what the call refuses -------------------------------------------------------------------------------------------
def test_refusals():
    import tdoa_amd
    with tdoa_amd.Context(max_lag=4, window_len=1024) as c:
        case = multi_case(3, 4, 5)
        q = case["q"]
        call = c.locate_multi_zoom_from_q
        assert _status(call, q, 3, 3, 1)[0] == 6                                 # the rounds': no table
        c.locate_set_table(case["table"], 7)
        status, text = _status(call, q, 3, 3, 1)
        assert status == 6 and "no fine delay table" in text                     # the zoom's, with its messages
        c.locate_set_fine_table(case["fine"][:, :2], FINE_COLS)
        status, text = _status(call, q, 3, 3, 1)
        assert status == 6 and "n_stations differs" in text
        c.locate_set_fine_table(case["fine"], FINE_COLS)
        assert call(q, 3, 3, 1, n_emitters=2)["zoom"].shape == (2, 6)
        for Z, H, sep in ((0, 1, 1), (65, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 65, 1), (1, 1, 0), (1, 1, -3)):
            status, text = _status(call, q, 3, Z, H, fine_separation=sep)
            assert status == 1 and ("Z outside" in text or "H outside" in text or "fine_separation < 1" in text), (Z, H, sep)
        for kw, text in ((dict(n_emitters=0), "n_emitters outside 1 .. 8"), (dict(n_emitters=9), "n_emitters outside 1 .. 8"),
                         (dict(guard=-1), "guard < 0"), (dict(min_separation=0), "min_separation < 1")):      # the rounds'
            status, got = _status(call, q, 3, 3, 1, **kw)
            assert status == 1 and text in got, kw
        assert call(q, 3, 64, 64, n_emitters=8, guard=10 ** 6)["zmap"].shape == (8, 6, 129 * 129)
        out, ptrs = _outputs(6, 3, 35, 1, 2)
        pq = q.ctypes.data_as(C.POINTER(C.c_int64))
        fn = c._L.tdoa_debug_locate_multi_zoom_from_q
        assert fn(c._h, pq, 6, 3, 2, 2, 0, 1, 3, 1, 1, *(ptrs[:4] + [None] + ptrs[5:])) == 1
        assert "zoom_host is NULL" in c._L.tdoa_last_error(c._h).decode()
        assert fn(c._h, pq, 6, 3, 2, 2, 0, 1, 3, 1, 1, *([None] + ptrs[1:])) == 1
        assert "loc_host is NULL" in c._L.tdoa_last_error(c._h).decode()
        assert fn(c._h, pq, 6, 3, 2, 2, 0, 1, 3, 1, 1, ptrs[0], None, None, None, ptrs[4], None, None, None, None) == 0      # the rest may be NULL
        assert _status(c.process_locate_multi_zoom, 3, 1)[0] == 6                # no captures (tdoa_num_stacks)
        assert _status(call, q, 3, 3, 1, n_w=2 ** 16)[0] == 5                    # the rounds': P n_w > 2^17
        c.locate_set_clock(np.zeros((5, 3), dtype=np.int32))
        status, text = _status(call, q, 3, 3, 1)
        assert status == 6 and "clock table's n_stacks differs" in text
        c.locate_set_clock(None)
        big = case["fine"].copy()
        big[7, 2] = 2 ** 27                                                      # 16 x 2^27 = 2^31
        c.locate_set_fine_table(big, FINE_COLS)
        c.locate_set_upsample(16)
        status, text = _status(call, q, 3, 3, 1)
        assert status == 5 and "fine delay table entry" in text
        c.locate_set_upsample(1)
        c.locate_set_fine_table(None)                                            # forgotten
        assert _status(call, q, 3, 3, 1)[0] == 6
    # TDOA_ERR_NOMEM reaches the caller through the call: the rounds' upsampled surfaces, refused by arithmetic (768 one-window stacks
    # x 6 pairs x 33.5 M fine lags are 1.2 TB).  The window maps are at most 8 x 65 535 x 16 641 words, 70 GB: no arithmetic refuses
    # them on this device, and their message is not reached here
    with tdoa_amd.Context(max_lag=2 ** 20, window_len=64) as c:
        for s in range(4):
            c.synth_capture(s, 256 * 64, ST4[s], (41.20, -96.00, 400.0), 0x10CA7E00 + s)
        c.locate_set_table(np.zeros((4, 4), dtype=np.int32), 2)
        c.locate_set_fine_table(np.zeros((9, 4), dtype=np.int32), 3)
        for kw in (dict(Z=0), dict(Z=65), dict(H=-1), dict(H=65), dict(fine_separation=0), dict(n_emitters=9), dict(guard=-1)):
            assert _status(c.process_locate_multi_zoom, **dict(dict(Z=1, H=1, windows_per_stack=1), **kw))[0] == 1, kw
        c.locate_set_fine_table(np.zeros((9, 3), dtype=np.int32), 3)
        assert _status(c.process_locate_multi_zoom, 2, 1, 1, 2)[0] == 6          # a fine table of another n_stations
        c.locate_set_fine_table(np.zeros((9, 4), dtype=np.int32), 3)
        c.locate_set_upsample(16)
        status, text = _status(c.process_locate_multi_zoom, 2, 1, 1, 2)
        assert status == 4 and "do not fit in device memory" in text


# ---- 7. the command-line tool -------------------------------------------------------------------------------------------
def test_cli_zoom_emitters_prints_the_library_result(tmp_path):
    """tdoa_processor --stack --locate=32x32/30 --locate-upsample=4 --emitters=2/1 --locate-zoom=4/6/2 --zoom-emitters on the golden
    three-station captures: an EMITTER-ZOOM line per stack and round with what Context.process_locate_multi_zoom returns on the
    125 x 125 fine grid; every other line is what the tool prints without the flag, and without it stdout has no such line"""
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
    head = [cli, "--stack", "--locate=32x32/30", "--locate-upsample=4", "--emitters=2/1", "--locate-zoom=4/6/2"]
    r = subprocess.run(head + ["--zoom-emitters"] + tail, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stderr            # (the 3-station solve may fail on these captures: tests/test_processor_cli.py)
    base = subprocess.run(head + tail, capture_output=True, text=True, timeout=300)
    assert base.returncode == r.returncode and "EMITTER-ZOOM" not in base.stdout
    assert [l for l in r.stdout.splitlines() if not l.startswith("EMITTER-ZOOM")] == base.stdout.splitlines()
    rows = [re.match(r"EMITTER-ZOOM block (\d) stack 0 round (\d): cell=(-?\d+) lat=([-\d.]+) lon=([-\d.]+) pairs=(\d+) score=([\d.]+) best=(\d+) "
                     r"rows=(\d+)\.\.(\d+) cols=(\d+)\.\.(\d+) runner=([\d.]+) runner_cell=(\d+) reserved=(\d+)$", l)
            for l in r.stdout.splitlines() if l.startswith("EMITTER-ZOOM")]
    assert len(rows) == 6 and all(rows), r.stdout
    assert [(int(m.group(1)), int(m.group(2))) for m in rows] == [(b, k) for b in (1, 2, 3) for k in (0, 1)]
    lat_c, lon_c, h_c = (sum(x[k] / 3 for x in st) for k in range(3))
    dlat, dlon = 30.0 / 111.32 / 31, 30.0 / (111.32 * np.cos(lat_c * np.pi / 180)) / 31
    lat0, lon0 = lat_c - dlat * 31 / 2, lon_c - dlon * 31 / 2
    with tdoa_amd.Context(max_lag=150, window_len=2000) as c:
        for s, p in enumerate(dats):
            c.capture_upload_file(s, p)
        grid = tdoa_amd.capi.locate_grid_table
        c.locate_set_table(grid(st, lat0, lon0, dlat, dlon, 32, 32, h_c, c.params.sample_rate), 32)
        c.locate_set_fine_table(grid(st, lat0, lon0, dlat / 4, dlon / 4, 125, 125, h_c, c.params.sample_rate), 125)
        c.locate_set_upsample(4)
        out = c.process_locate_multi_zoom(4, 6, 0, 2, 1, 1, 2)
    assert (out["zoom"]["score_q"][0] > 0).all()
    for m in rows:
        b, k = int(m.group(1)) - 1, int(m.group(2))
        z, pairs = out["zoom"][k, b], out["zpairs"][k, b]
        if int(z["score_q"]) == 0:
            assert int(m.group(3)) == -1
            continue
        assert [int(m.group(n)) for n in (3, 6, 8, 9, 10, 11, 12, 14, 15)] == \
               [int(z[n]) for n in ("cell", "pairs_in", "n_best", "row_lo", "row_hi", "col_lo", "col_hi", "runner_cell")] + [int(pairs[1])]
        assert int(pairs[0]) == int(z["pairs_in"])
        assert abs(float(m.group(4)) - (lat0 + (int(z["cell"]) // 125) * dlat / 4)) <= 5.1e-7
        assert abs(float(m.group(5)) - (lon0 + (int(z["cell"]) % 125) * dlon / 4)) <= 5.1e-7
        assert abs(float(m.group(7)) - float(z["score"])) <= 5.1e-7 and abs(float(m.group(13)) - float(z["runner_up"])) <= 5.1e-7
    for flags in (["--stack", "--locate=32x32/30", "--locate-zoom=4", "--zoom-emitters"], ["--stack", "--locate=32x32/30", "--emitters=2", "--zoom-emitters"]):
        bad = subprocess.run([cli] + flags + tail, capture_output=True, text=True, timeout=300)
        assert bad.returncode == 1 and "usage: --zoom-emitters needs" in bad.stderr and bad.stdout == ""
