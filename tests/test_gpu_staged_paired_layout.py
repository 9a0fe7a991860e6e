"""GPU: the staged column walk on the PAIRED block layout of the unpacked spectra (stg_paired_at, csrc/dec_staged.hpp: line
[cb][k2] = a row's 64 columns of block cb, then the partner row's 64 columns of block 63 - cb -- one contiguous KB per LDS-DMA),
written by k_fwd_row4096_unpack and read by both loaders and by the walk's row-0 reads, and its non-temporal loader loads.

The LDS image and every multiply-add are those of the earlier layouts, so every output must carry the SAME BITS as
- TDOA_NO_STG_PAIRED=1: the [column / 64][k2][column % 64] blocks (two 512-byte pieces per LDS-DMA);
- TDOA_NO_STG_BLOCKS=1: row-major spectra, independent of both blocked layouts;
- TDOA_NO_STG_NT=1: the same loads with the default cache policy.
Held on tdoa_process peak records, byte for byte, on tdoa_process_lags surfaces over all 39 999 lags as bit patterns, and on one
tdoa_process_fine call; the lags are the simulated delays.  Each case states the route it expects.

The frame is tests/test_gpu_staged_share_merge.py's: three-window captures, one window = tdoa_process(rank 1 of 2), two = rank 0
of 2; one warm-up call, then every call under test on workspace filled with NaN (Context.poison_workspace)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ML = 20000
WL_256, WL_512 = 2_000_000, 2_200_001          # the smallest window on the 4096 x 256 plan; 4096 x 512, an odd length
GATE = 200.0
SWITCHES = ("TDOA_NO_STG_PAIRED", "TDOA_NO_STG_BLOCKS", "TDOA_NO_STG_NT")


@functools.lru_cache(maxsize=None)
def _captures(n_stations, wl):
    from oracle import pyoracle
    rng = np.random.default_rng(9000 + n_stations)
    delays = tuple(int(x) for x in rng.integers(0, 300, size=n_stations))
    caps = tuple(pyoracle.simulate_delayed_fm(3 * wl, d, 910 + n_stations, 100 * (s + 1)) for s, d in enumerate(delays))
    for c in caps:
        c.setflags(write=False)
    return caps, delays


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def _run(n_stations, wl, rank, off=(), fine=False):
    """a fresh context with the switches in `off` set to 1 (read when the context is made); warm up, then every call under test
    on poisoned workspace.  Cached: a leg that several comparisons need runs once, and nobody writes to its arrays."""
    import tdoa_amd
    caps, _ = _captures(n_stations, wl)
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for name in SWITCHES:
            if name in off:
                mp.setenv(name, "1")
            else:
                mp.delenv(name, raising=False)
        with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
            for s, cap in enumerate(caps):
                c.capture_upload(s, cap)
            c.process(rank=rank, world=2)
            c.poison_workspace()
            out["peaks"] = c.process(rank=rank, world=2)
            out["route"] = c.last_route()
            c.process_lags(rank=rank, world=2)
            c.poison_workspace()
            out["lags"] = c.process_lags(rank=rank, world=2)
            assert {k: v for k, v in c.last_route().items() if k.startswith("stg_")} == {k: v for k, v in out["route"].items() if k.startswith("stg_")}
            if fine:
                c.process_fine(GATE / 2, rank=rank, world=2)
                c.poison_workspace()
                out["fine"] = c.process_fine(GATE, rank=rank, world=2)
                assert c.last_route()["stg_paired"] == out["route"]["stg_paired"]
            out["plan"] = tuple(c.plan_info())[1:]
    for v in out.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def _own(rank):
    return [0, 2] if rank == 0 else [1]


def _clean_and_right(out, n_stations, wl, rank):
    _, delays = _captures(n_stations, wl)
    want = np.array([delays[j] - delays[i] for i in range(n_stations) for j in range(i + 1, n_stations)])
    own = _own(rank)
    p = out["peaks"][own]
    assert (p["lag"] == want[None, :]).all() and np.isfinite(p["corr"]).all() and (p["abs_corr"] > 100.0).all()
    assert out["lags"].shape[-1] == 2 * ML - 1
    assert np.isfinite(out["lags"][own]).all(), "a surface value came from workspace nobody wrote"


def _same_bits(a, b):
    assert np.array_equal(_bits(a["peaks"]), _bits(b["peaks"]))
    assert np.array_equal(a["lags"].view(np.uint32), b["lags"].view(np.uint32))


def _staged(route):
    return (route["inverse"], route["pair_step"]) == ("decimated", "staged")


# (stations, window length, rank of 2, merged, folded, non-temporal): 3 x 2 windows on 4096 x 256 -- bench.py's geometry, the
# merged four-wave kernel, one pair group; 3 x 1 on 4096 x 512; 4 x 1 -- six unmerged walks next to a loader wave, one group; 9 x 1
# -- several groups, default cache policy; 13 x 1 -- the folded form, its waves bring one station each (issue_one)
CASES = [(3, WL_256, 0, True, False, True), (3, WL_512, 1, True, False, True), (4, WL_256, 1, False, False, True),
         (9, WL_256, 1, False, False, False), (13, WL_256, 1, False, True, False)]


@pytest.mark.parametrize("n_stations,wl,rank,merged,folded,nt", CASES)
def test_paired_lines_give_the_bits_of_both_earlier_layouts(n_stations, wl, rank, merged, folded, nt):
    import tdoa_amd
    a = _run(n_stations, wl, rank)
    b = _run(n_stations, wl, rank, off=("TDOA_NO_STG_PAIRED",))
    c = _run(n_stations, wl, rank, off=("TDOA_NO_STG_BLOCKS",))
    assert a["plan"] == b["plan"] == c["plan"] == ((4096, 256) if wl == WL_256 else (4096, 512))
    for o in (a, b, c):
        assert _staged(o["route"])
    ra, rb, rc = a["route"], b["route"], c["route"]
    assert (ra["stg_paired"], ra["stg_blocked"], ra["stg_merged"], ra["stg_folded"], ra["stg_nt"]) == (True, True, merged, folded, nt)
    assert (rb["stg_paired"], rb["stg_blocked"], rb["stg_merged"], rb["stg_folded"], rb["stg_nt"]) == (False, True, merged, folded, False)
    assert (rc["stg_paired"], rc["stg_blocked"], rc["stg_merged"], rc["stg_folded"], rc["stg_nt"]) == (False, False, False, False, False)
    assert ra["row_pass"] == rb["row_pass"] == "unpack_blocks" and rc["row_pass"] == "unpack_in_place"
    # non-temporal loads exactly where a window's pairs are ONE group of a workgroup with a loader wave
    groups = len(tdoa_amd.capi.staged_groups(n_stations, 16 if folded else 15))
    assert nt == (groups == 1 and not folded)
    _clean_and_right(a, n_stations, wl, rank)
    _same_bits(a, b)
    _same_bits(a, c)


def test_non_temporal_loads_change_no_bit():
    a = _run(3, WL_256, 1)
    b = _run(3, WL_256, 1, off=("TDOA_NO_STG_NT",))
    assert _staged(a["route"]) and _staged(b["route"])
    assert a["route"]["stg_nt"] and not b["route"]["stg_nt"] and a["route"]["stg_paired"] and b["route"]["stg_paired"]
    assert {k: v for k, v in a["route"].items() if k != "stg_nt"} == {k: v for k, v in b["route"].items() if k != "stg_nt"}
    _clean_and_right(a, 3, WL_256, 1)
    _same_bits(a, b)


def test_refinement_on_paired_lines():
    a = _run(3, WL_256, 1, fine=True)
    b = _run(3, WL_256, 1, off=("TDOA_NO_STG_PAIRED",), fine=True)
    assert a["route"]["stg_paired"] and not b["route"]["stg_paired"] and b["route"]["stg_blocked"]
    (pa, fa), (pb, fb) = a["fine"], b["fine"]
    own = _own(1)
    assert np.isfinite(fa["y"][own]).all() and np.isfinite(fa["frac"][own]).all(), "the refinement read workspace it did not write"
    assert np.array_equal(_bits(pa), _bits(pb)) and np.array_equal(_bits(fa), _bits(fb))
    assert np.array_equal(_bits(pa), _bits(a["peaks"]))
