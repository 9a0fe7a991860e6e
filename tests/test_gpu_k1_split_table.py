"""GPU: the fused column kernels' split half-plane look-up (k1_split_angle2, csrc/k1_discriminator.hpp: a 96 KB table next
to the whole exchange plane, 160 KB of LDS) against the oracle and against the quadrant route (TDOA_K1_QUAD_TABLE=1, read
when the context is made).  The 4096 x 512 plan's kernel takes the split table under TDOA_K1_SPLIT_512=1 only; its cases set it.

Both look-ups give the same angle of a sample modulo a turn, so every stored code is the same integer and everything
after it -- window statistics, spectra, surfaces, keys, peak records -- must carry the SAME BITS on either route.
Every case asserts which route ran (last_route()["k1_split"], the column pass) and, where it applies, the single-look path.

One window of a case = tdoa_process(rank 1 of 2) on three-window captures, two windows = rank 0 of 2."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ML = 20000
WL_ODD = 1_060_001                     # 4096 x 256: general rows at the window's first row and tail, zero-padded rows
WL_512 = 2_200_001                     # 4096 x 512
WL_2048 = 8_400_000                    # 4096 x 2048: the two-sweep plan (SUB = true)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def _all_pairs_capture(seed, n):
    """n samples: seeded permutations of all 65 536 byte pairs laid end to end, each followed by itself rotated by one sample,
    so that every pair lands in both halves of a dword"""
    rng = np.random.default_rng(seed)
    blocks = []
    while 65536 * len(blocks) < n:
        p = rng.permutation(65536).astype(np.uint16)
        blocks += [p, np.roll(p, 1)]
    out = np.concatenate(blocks)[:n].astype("<u2").view(np.uint8)
    out.setflags(write=False)
    return out


def _stats_tuple(st):
    return (st.s1, st.s2_lo, st.s2_hi, np.float32(st.mean).view(np.uint32), np.float32(st.scale).view(np.uint32))


def test_every_table_entry_against_the_oracle(oracle, monkeypatch):
    import tdoa_amd
    monkeypatch.delenv("TDOA_K1_QUAD_TABLE", raising=False)
    monkeypatch.delenv("TDOA_NO_K1_ONCE", raising=False)
    caps = [_all_pairs_capture(7100 + s, WL_ODD) for s in range(2)]
    for cap in caps:
        words = cap.view("<u2")
        for parity in (0, 1):
            assert np.unique(words[parity::2]).size == 65536
        # the boundary look-up (one sample, k1_split_angle) takes the sample before each 64-column tile of a row, 128 m - 1:
        # 8281 positions of the window, nearly all of them different pairs
        assert np.unique(words[127::128]).size > 7000
    with tdoa_amd.Context(max_lag=ML, window_len=WL_ODD) as c:
        c.fm_xcorr(caps[0], caps[1], ML)
        route = c.last_route()
        assert tuple(c.plan_info())[1:] == (4096, 256)
        assert route["k1_split"] and route["col_pass"] == "k1_256" and route["fused_k1"] and c.last_k1(0)[1]
        got = [_stats_tuple(c.last_k1(s)[0]) for s in range(2)]
    for s, cap in enumerate(caps):
        want = oracle.b_phase_stats(oracle.b_discriminate(cap))
        assert got[s] == _stats_tuple(want), s


@functools.lru_cache(maxsize=None)
def _fm_captures(n_stations, wl):
    """three windows per capture, all with the same content (one window's worth is generated)"""
    from oracle import pyoracle
    delays = (0, 41, -17)[:n_stations]
    caps = tuple(np.tile(pyoracle.simulate_delayed_fm(wl, 300 + d, 77, 100 * (s + 1)), 3) for s, d in enumerate(delays))
    for c in caps:
        c.setflags(write=False)
    return caps, delays


def _run(monkeypatch, n_stations, wl, rank, split, no_once=False, split_512=True):
    import tdoa_amd
    caps, _ = _fm_captures(n_stations, wl)
    # (k_fwd_col512_k1 takes the split table only when asked: TDOA_K1_SPLIT_512=1; the other kernels ignore the switch)
    for name, on in (("TDOA_K1_QUAD_TABLE", not split), ("TDOA_NO_K1_ONCE", no_once), ("TDOA_K1_SPLIT_512", split and split_512)):
        if on:
            monkeypatch.setenv(name, "1")
        else:
            monkeypatch.delenv(name, raising=False)
    out = {}
    with tdoa_amd.Context(max_lag=ML, window_len=wl) as c:
        for s, cap in enumerate(caps):
            c.capture_upload(s, cap)
        out["peaks"] = c.process(rank=rank, world=2)
        out["route"], out["once"] = c.last_route(), c.last_k1(0)[1]
        out["lags"] = c.process_lags(rank=rank, world=2)
        assert [c.last_route()[k] for k in ("k1_split", "col_pass")] == [out["route"][k] for k in ("k1_split", "col_pass")]
        out["plan"] = tuple(c.plan_info())[1:]
    return out


# (stations, window length, rank of 2, TDOA_NO_K1_ONCE, plan, column pass)
CASES = [(3, WL_ODD, 0, False, (4096, 256), "k1_256"), (3, WL_ODD, 0, True, (4096, 256), "k1_256"),
         (2, WL_512, 1, False, (4096, 512), "k1_512"), (2, WL_2048, 1, False, (4096, 2048), "k1_two_sweep")]


@pytest.mark.parametrize("n_stations,wl,rank,no_once,plan,col", CASES)
def test_split_route_gives_the_quadrant_routes_bits(monkeypatch, n_stations, wl, rank, no_once, plan, col):
    a = _run(monkeypatch, n_stations, wl, rank, split=True, no_once=no_once)
    b = _run(monkeypatch, n_stations, wl, rank, split=False, no_once=no_once)
    assert a["plan"] == b["plan"] == plan
    for o in (a, b):
        assert o["route"]["col_pass"] == col and o["route"]["fused_k1"] and o["once"] == (not no_once)
    assert a["route"]["k1_split"] and not b["route"]["k1_split"]
    assert {k: v for k, v in a["route"].items() if k != "k1_split"} == {k: v for k, v in b["route"].items() if k != "k1_split"}
    _, delays = _fm_captures(n_stations, wl)
    want = np.array([delays[j] - delays[i] for i in range(n_stations) for j in range(i + 1, n_stations)])
    own = [0, 2] if rank == 0 else [1]
    assert (a["peaks"][own]["lag"] == want[None, :]).all()
    assert np.array_equal(_bits(a["peaks"]), _bits(b["peaks"]))
    assert a["lags"].shape[-1] == 2 * ML - 1 and np.abs(a["lags"][own]).max() > 0
    assert np.array_equal(a["lags"].view(np.uint32), b["lags"].view(np.uint32))


def test_the_512_plan_keeps_the_quadrant_table_unless_asked(monkeypatch):
    """k_fwd_col512_k1 measured slower with the split table: a default context runs the quadrant route
    there, and gives the bits of the split one"""
    a = _run(monkeypatch, 2, WL_512, 1, split=True, split_512=False)
    b = _run(monkeypatch, 2, WL_512, 1, split=True)
    assert a["plan"] == b["plan"] == (4096, 512) and a["route"]["col_pass"] == b["route"]["col_pass"] == "k1_512"
    assert not a["route"]["k1_split"] and b["route"]["k1_split"] and a["once"] and b["once"]
    assert np.array_equal(_bits(a["peaks"]), _bits(b["peaks"]))
    assert np.array_equal(a["lags"].view(np.uint32), b["lags"].view(np.uint32))
