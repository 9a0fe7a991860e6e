"""GPU: the staged column walk with the neighbour shares settled inside a 64-column block (k_pair_decimate_staged<.., MERGE_>,
csrc/dec_staged.hpp) against the same walk with every column's shares left in X for the small plan's row pass
(TDOA_NO_STG_MERGE=1, read when the context is made).

An output of the decimated pair step near either end of a column is G + one share of the neighbouring column's walk.  The
merged walk makes that one f32 addition itself for 126 of a block's 128 columns and leaves only the block-edge columns' shares
in X; the unmerged walk leaves all of them to k_inv_rows_plain_r8 / k_small_rows_col_peak.  Same two operands, one addition:
every output must carry the SAME BITS.  Held here on
- tdoa_process peak records, byte for byte;
- tdoa_process_lags surfaces over all 39 999 lags as bit patterns -- these lags land in every column of the small plan,
  the block-edge columns and columns 0 / 4095 included;
- tdoa_process_fine records (the refinement reads the peak's neighbours out of V': the two-kernel small plan in the new mode).
The merged calls run on workspace filled with NaN (Context.poison_workspace, after one warm-up call that sizes it): a merged-mode
kernel that still read an X entry nobody wrote would show up as NaN.

The library merges where two workgroups of the merging kernel still share a CU (it runs at two waves per SIMD: workgroups of
at most four waves -- three walks and a loader wave, three stations); larger groups keep full shares, and each case states
which it expects.  TDOA_DEC_STAGED_CW=3 cuts the pairs of more stations into groups of three walks: the merging kernel in a
batch of several groups, next to idle compute waves in the last one, with up to five station slots in the ring.

One window of a case = tdoa_process(rank 1 of 2) on three-window captures, two windows = rank 0 of 2."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ML = 20000
WL_256, WL_512 = 2_000_000, 4_000_000          # 4096 x 256 and 4096 x 512 plans
GATE = 200.0


@functools.lru_cache(maxsize=None)
def _captures(n_stations, wl):
    from oracle import pyoracle
    rng = np.random.default_rng(4000 + n_stations)
    delays = tuple(int(x) for x in rng.integers(0, 300, size=n_stations))
    caps = tuple(pyoracle.simulate_delayed_fm(3 * wl, d, 640 + n_stations, 100 * (s + 1)) for s, d in enumerate(delays))
    for c in caps:
        c.setflags(write=False)
    return caps, delays


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _run(monkeypatch, n_stations, wl, rank, merge, flags=None, fine=False, lags=True, walks=0):
    """a fresh context with or without TDOA_NO_STG_MERGE (walks > 0: at most that many walks per workgroup); warm up, then
    every call under test on poisoned workspace"""
    import tdoa_amd
    caps, _ = _captures(n_stations, wl)
    if walks:
        monkeypatch.setenv("TDOA_DEC_STAGED_CW", str(walks))
    else:
        monkeypatch.delenv("TDOA_DEC_STAGED_CW", raising=False)
    if merge:
        monkeypatch.delenv("TDOA_NO_STG_MERGE", raising=False)
    else:
        monkeypatch.setenv("TDOA_NO_STG_MERGE", "1")
    out = {}
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        for s, cap in enumerate(caps):
            c.capture_upload(s, cap)
        c.debug_flags(**(flags or {}))
        c.process(rank=rank, world=2)
        c.poison_workspace()
        out["peaks"] = c.process(rank=rank, world=2)
        out["route"] = c.last_route()
        if lags:
            c.process_lags(rank=rank, world=2)
            c.poison_workspace()
            out["lags"] = c.process_lags(rank=rank, world=2)
            assert c.last_route()["stg_merged"] == out["route"]["stg_merged"]
        if fine:
            c.process_fine(GATE / 2, rank=rank, world=2)
            c.poison_workspace()
            out["fine"] = c.process_fine(GATE, rank=rank, world=2)
            assert c.last_route()["stg_merged"] == out["route"]["stg_merged"] and not c.last_route()["small_fused"]
        out["plan"] = tuple(c.plan_info())[1:]
    return out


def _own(rank):
    return [0, 2] if rank == 0 else [1]


def _clean_and_right(out, n_stations, wl, rank):
    _, delays = _captures(n_stations, wl)
    want = np.array([delays[j] - delays[i] for i in range(n_stations) for j in range(i + 1, n_stations)])
    own = _own(rank)
    p = out["peaks"][own]
    assert (p["lag"] == want[None, :]).all() and np.isfinite(p["corr"]).all() and (p["abs_corr"] > 100.0).all()
    if "lags" in out:
        assert np.isfinite(out["lags"][own]).all(), "a surface value came from workspace nobody wrote"


# (stations, window length, rank of 2, walks per workgroup (0: the library's), merged expected): 3 x 2 windows -- bench.py's
# geometry, four-wave workgroups; 4 x 1 -- six walks and a loader (seven waves: one merging workgroup per CU, unmerged);
# 5 x 1 -- ten walks; 9 x 1 -- several groups with merged leftovers; 13 x 1 -- the folded form without a loader wave; 3 x 1 on
# the 4096 x 512 plan; then the merging kernel on more stations, three walks per workgroup: 5 x 1 -- four groups, the last
# with one walk and two idle compute waves
CASES = [(3, WL_256, 0, 0, True), (4, WL_256, 1, 0, False), (5, WL_256, 1, 0, False), (9, WL_256, 1, 0, False),
         (13, WL_256, 1, 0, False), (3, WL_512, 1, 0, True), (5, WL_256, 1, 3, True)]


@pytest.mark.parametrize("n_stations,wl,rank,walks,merged", CASES)
def test_merged_shares_give_the_unmerged_bits(monkeypatch, n_stations, wl, rank, walks, merged):
    a = _run(monkeypatch, n_stations, wl, rank, merge=True, walks=walks)
    b = _run(monkeypatch, n_stations, wl, rank, merge=False, walks=walks)
    assert a["plan"] == b["plan"] == ((4096, 256) if wl == WL_256 else (4096, 512))
    for o in (a, b):
        assert (o["route"]["inverse"], o["route"]["pair_step"], o["route"]["stg_blocked"]) == ("decimated", "staged", True)
    assert a["route"]["stg_merged"] == merged and not b["route"]["stg_merged"]
    assert a["route"]["stg_folded"] == (n_stations == 13 and not walks)
    _clean_and_right(a, n_stations, wl, rank)
    assert np.array_equal(_bits(a["peaks"]), _bits(b["peaks"]))
    assert a["lags"].shape[-1] == 2 * ML - 1
    assert np.array_equal(a["lags"].view(np.uint32), b["lags"].view(np.uint32))


@pytest.mark.parametrize("wl", [WL_256, WL_512])
def test_merged_shares_give_the_per_pair_walks_bits(monkeypatch, wl):
    """three stations: k_pair_decimate_cols (TDOA_DEBUG_NO_DEC_STAGED) leaves full shares in memory"""
    a = _run(monkeypatch, 3, wl, 1, merge=True)
    b = _run(monkeypatch, 3, wl, 1, merge=True, flags={"dec_cols_always": True, "no_dec_staged": True})
    assert a["route"]["stg_merged"] and (b["route"]["pair_step"], b["route"]["stg_merged"]) == ("columns", False)
    assert np.array_equal(_bits(a["peaks"]), _bits(b["peaks"]))
    assert np.array_equal(a["lags"].view(np.uint32), b["lags"].view(np.uint32))


def test_merged_shares_in_the_fused_small_plan(monkeypatch):
    """k_small_rows_col_peak reads the block-edge shares the same way (TDOA_DEBUG_SMALL_FUSED_ALWAYS: three pair-windows)"""
    a = _run(monkeypatch, 3, WL_256, 1, merge=True, flags={"small_fused_always": True})
    b = _run(monkeypatch, 3, WL_256, 1, merge=False, flags={"small_fused_always": True})
    assert a["route"]["small_fused"] and b["route"]["small_fused"] and a["route"]["stg_merged"] and not b["route"]["stg_merged"]
    _clean_and_right(a, 3, WL_256, 1)
    assert np.array_equal(_bits(a["peaks"]), _bits(b["peaks"]))
    assert np.array_equal(a["lags"].view(np.uint32), b["lags"].view(np.uint32))


def test_refinement_reads_the_same_neighbours(monkeypatch):
    a = _run(monkeypatch, 3, WL_256, 0, merge=True, fine=True, lags=False)
    b = _run(monkeypatch, 3, WL_256, 0, merge=False, fine=True, lags=False)
    assert a["route"]["stg_merged"] and not b["route"]["stg_merged"]
    (pa, fa), (pb, fb) = a["fine"], b["fine"]
    own = _own(0)
    assert np.isfinite(fa["y"][own]).all() and np.isfinite(fa["frac"][own]).all(), "the refinement read workspace it did not write"
    assert np.array_equal(_bits(pa), _bits(pb)) and np.array_equal(_bits(fa), _bits(fb))
    assert np.array_equal(_bits(pa), _bits(a["peaks"]))
