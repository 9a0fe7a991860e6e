#!/usr/bin/env python3
"""ms per call of tdoa_process, tdoa_process_peaks(k = 1, min_separation = 1) and tdoa_process_stacked(0, 1, 1) on the window
geometry of BASELINE config 2 (synthetic captures on the device, one GPU), in one run.  The three are timed in alternation,
`--rounds` rounds of `--steps` calls each, so that the spread between rounds of the same call stands next to the
differences between the calls: median, and the lowest and highest round.  The graphs replay; host copies are included,
as a caller sees them.  Every `--drift H/D` adds a leg: tdoa_process_stacked_drift(0, H, D, 1, 1) with the profile downloaded
(0/1 is the plain stack with the search's fixed cost; the difference between two legs is the search kernel's time for the
hypotheses between them).  Every `--track J` adds a leg: tdoa_process_track(0, J) with score, lags and values downloaded (one
kernel per window of a block after the surfaces; the difference between two legs is what the wider scan costs).  Every
`--closure G` adds a leg: tdoa_process_closure(0, G, 1) with the records downloaded (the stack's accumulation, then two
launches of the search and two of its finish).  Every `--locate ROWSxCOLS` adds a leg: tdoa_process_locate(0, 1) on a grid of
that many cells over 0.3 x 0.4 degrees around the stations, with the records, lags and correlations downloaded and the map
left on the device (the table is set once per round, outside the timed window).  Every `--sync G[/R]` adds a leg:
tdoa_process_sync(0, G, R) (R defaults to 2) against the delays of a known emitter at TX, with the records, clocks, lags and
correlations downloaded (the stack's accumulation, then the joint start over (2G+1)^2 cells and one workgroup per stack for
the placing and the sweeps).  Every `--locate-track J` adds a leg per `--locate` grid: tdoa_process_locate_track(0, J, 1) on
that grid with the records, cells, own scores, lags and correlations downloaded and T_0 left on the device (the search's
launches, then one launch per stack of a block but the last and four to finish).  Every `--emitters K[/GUARD]` adds a leg
per `--locate` grid: tdoa_process_locate_multi(0, K, GUARD, 1) (GUARD defaults to 2) on that grid with the K planes of records,
lags and correlations downloaded and the maps left on the device (the search's launches, then four per further round;
K = 1 is the locate leg's work through the other entry).  Every `--track-emitters K[/GUARD]` adds a leg per `--locate` grid and
`--locate-track J`: tdoa_process_locate_track_multi(0, J, K, GUARD, 1) (GUARD defaults to 2) with the K planes of records, cells,
own scores, counts, lags and correlations downloaded and every T_0 left on the device (the track's launches and one for the
centres, then per further round the masked scores, the recurrence and four to finish; K = 1 is the locate-track leg's work
through the other entry).  `--stack M` gives the locate, locate-track, emitters and track-emitters legs stacks
of M windows (default 0: whole blocks, one position per track).  `--map-stats R1,R2[/FOOT]` adds, next to each of those four
kinds of leg, the same leg with the map statistics on (tdoa_locate_set_stats with those ranks and FOOT, default 0; name
..._stats_ms): the statistics' kernels and their download come on top, the planes stay on the device.  Every `--sync-drift G/H[/D[/R]]` adds a leg:
tdoa_process_sync_drift(M, G, H, D, R) (D defaults to 1, R to 2; M from `--stack`) against the same delays, with the records,
clocks, rates, rows, lags and correlations downloaded (the stack's accumulation, then two launches per station's step: (2G+1)
(2H+1) candidates in tiles of 256, and the commit; H = 0 is the search's fixed cost).  `--stations S` runs all
legs on S stations (default 3; 8 gives 56 triples).  Every `--locate-upsample U` adds a leg per `--locate` grid:
tdoa_process_locate(M, 1) with tdoa_locate_set_upsample(U) (name ..._upU_ms): the two scalings and the upsampler come in front
of the search's launches, which then gather from surfaces U times as long; every other leg runs with U = 1.  `--max-lag N`
(default 20000) sets the context's search range: one-window stacks (`--stack 1`) at U = 16 want 512.  Every
`--sync-fine G/U[/R[/RF]]` adds a leg: tdoa_process_sync_fine(M, G, R, U, RF) (R and RF default to 2; M from `--stack`) against
the same delays with all eight outputs downloaded -- the clock search's launches and one more kernel, one workgroup per stack --
and, when M is not 0, the leg process_sync_G_R_stackM_ms: tdoa_process_sync(M, G, R), what the fine leg is compared with.
Every `--locate-zoom Z[/H]` (H defaults to 2 Z) adds, per `--locate` grid and for U = 1 and every `--locate-upsample U`, two legs:
tdoa_process_locate_zoom(M, 1, Z, H, 1) with the same grid at Z cells per cell as the fine table (name
process_locate_zoom_RxC_Z_H[_upU]_ms: the locate's launches and two more kernels; records, lags and correlations of both stages
downloaded, the maps left on the device), and tdoa_process_locate(M, 1) with that fine grid as the table (name
process_locate_fine_RxC_Z[_upU]_ms), the brute force the zoom replaces; the second is left out where the fine grid has more than
2^22 cells.  Every `--sync-drift-fine G/H/D/R/U/RF` adds a leg: tdoa_process_sync_drift_fine(M, G, H, D, R, U, RF) against the same
delays with all twelve outputs downloaded -- the clock-line search's launches, then the fine table, two launches per fine step
((2U+1)^2 candidates in tiles of 256, and the commit) and two finishes; give the same G/H/D/R to `--sync-drift` to have the leg
it is compared with in the same process.  Every `--locate-track-zoom Z[/H[/JF]]` (H defaults to 2 Z, JF to Z, at most 16) adds, per
`--locate` grid, per `--locate-track J` and for U = 1 and every `--locate-upsample U`, three legs: tdoa_process_locate_track_zoom(M,
J, 1, Z, H, JF, 1) with the same grid at Z cells per cell as the fine table (name process_locate_track_zoom_RxC_JJ_Z_H_JF[_upU]_ms:
the tracks' launches and four more kernels; records, cells, own scores, lags and correlations of both stages downloaded, the planes
left on the device), tdoa_process_locate_track(M, J, 1) on the coarse table (the `--locate-track` leg, with U > 1 the name
process_locate_track_RxC_JJ_upU_ms) and tdoa_process_locate_track(M, JF, 1) with that fine grid as the table (name
process_locate_track_fine_RxC_JJF_Z[_upU]_ms), the brute force the call replaces; the last is left out, with a message, where its
maps, steps and sums do not fit the device.  `--sync-locate` adds, per `--locate` grid, `--locate-zoom Z[/H]`, `--sync-fine G/U[/R[/RF]]`
and for U_loc = 1 and every `--locate-upsample U`, two legs: tdoa_process_sync_locate(M, G, R, U, RF, midpoint mix, 1, Z, H, 1) with
the seventeen outputs but the maps downloaded (name process_sync_locate_RxC_Z_H_G_U_R_RF[_upU]_ms: the fine clock search's
launches, one kernel for the rows and the zoom locate's launches in one step behind one accumulation), and the chain it
replaces, timed as one unit (name sync_locate_chain_RxC_Z_H_G_U_R_RF[_upU]_ms): tdoa_process_sync_fine, tdoa_clock_mix_rows on
the host, tdoa_locate_set_clock and tdoa_process_locate_zoom.  Give the same options their own legs (they are there already) to
have process_sync_fine and process_locate_zoom in the same process.  `--sync-drift-locate` adds, per `--locate` grid, `--locate-track J`,
`--locate-track-zoom Z[/H[/JF]]`, `--sync-drift-fine G/H/D/R/U/RF` and for U_loc = 1 and every `--locate-upsample U`, two legs:
tdoa_process_sync_drift_locate(M, G, H, D, R, U, RF, forward mix, J, 1, Z, H, JF, 1) with the twenty-six outputs but the planes
downloaded (name process_sync_drift_locate_RxC_JJ_Z_H_JF_G_H_D_R_U_RF[_upU]_ms: the fine lines' launches, one kernel for the rows
and the zoomed tracks' launches in one step behind one accumulation), and the chain it replaces, timed as one unit (name
sync_drift_locate_chain_...): tdoa_process_sync_drift_fine, tdoa_line_mix_rows on the host, tdoa_locate_set_clock and
tdoa_process_locate_track_zoom.  `--emitters-zoom` adds, per `--locate` grid, `--emitters K[/GUARD]`, `--locate-zoom Z[/H]` and for
U = 1 and every `--locate-upsample U`, three legs: tdoa_process_locate_multi_zoom(M, K, GUARD, 1, Z, H, 1) with the same grid at Z
cells per cell as the fine table (name process_locate_multi_zoom_RxC_KK_GG_Z_H[_upU]_ms: the rounds' launches and two more kernels
for any K; records, counts, lags and correlations of both stages downloaded, the maps left on the device),
tdoa_process_locate_multi(M, K, GUARD, 1) on the coarse table (the `--emitters` leg, with U > 1 the name
process_locate_multi_RxC_KK_GG_upU_ms) and tdoa_process_locate_multi(M, K, GUARD, 1) with that fine grid as the table (name
process_locate_multi_fine_RxC_KK_GG_Z[_upU]_ms), the nearest brute force; the last is left out, with a message, where its K
planes of maps do not fit the device.
usage: scripts/time_stacked.py [--steps N] [--rounds R] [--stations S] [--stack M] [--drift H/D]... [--track J]...
[--closure G]... [--locate ROWSxCOLS]... [--locate-track J]... [--emitters K[/GUARD]]... [--track-emitters K[/GUARD]]... [--map-stats R1,R2[/FOOT]] [--sync G[/R]]... [--sync-drift G/H[/D[/R]]]... [--locate-upsample U]... [--sync-fine G/U[/R[/RF]]]... [--locate-zoom Z[/H]]... [--sync-drift-fine G/H/D/R/U/RF]... [--locate-track-zoom Z[/H[/JF]]]... [--sync-locate] [--sync-drift-locate] [--emitters-zoom] [--max-lag N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tdoa-geolocation_amd"))
try:
    import torch          # noqa: F401  before the library: the process keeps torch's HIP runtime (bench.py does the same)
except Exception:         # pragma: no cover
    torch = None
import numpy as np
import tdoa_amd

ST = [(41.18660274289527, -95.96064116595667, 355.69), (41.24669616513154, -96.08366304481238, 329.0),
      (41.32916620016985, -96.03513381562004, 373.18)]
TX = (41.20, -96.00, 400.0)


def timed(fn, steps):
    fn()                  # the call's own graph is captured again after another call's: not part of the timed window
    fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e3


def main(steps, rounds, drifts=(), tracks=(), closures=(), stations=3, locates=(), syncs=(), locate_tracks=(), stack=0, emitters=(),
         track_emitters=(), map_stats=None, sync_drifts=(), upsamples=(), max_lag=20000, sync_fines=(), zooms=(), sync_drift_fines=(), track_zooms=(),
         sync_locate=False, sync_drift_locate=False, emitters_zoom=False):
    c = tdoa_amd.Context(sample_rate=2e6, window_len=2_000_000, max_lag=max_lag)
    for s in range(stations):
        c.synth_capture(s, 66_666_666, ST[s % 3], TX, 0x5D0A0000 + s)
    _, W = c.num_windows()
    P = c.num_pairs()
    _, n_stacks = c.num_stacks(0)
    legs = {"process_ms": lambda: c.process(), "process_peaks_k1_ms": lambda: c.process_peaks(1, 1),
            "process_stacked_ms": lambda: c.process_stacked(0, 1, 1)}
    for H, D in drifts:
        legs["process_stacked_drift_%d_%d_ms" % (H, D)] = lambda H=H, D=D: c.process_stacked_drift(0, H, D, 1, 1)
    for J in tracks:
        legs["process_track_%d_ms" % J] = lambda J=J: c.process_track(0, J)
    for G in closures:
        legs["process_closure_%d_ms" % G] = lambda G=G: c.process_closure(0, G, 1)
    setup = {}
    ref = tdoa_amd.capi.locate_grid_table([ST[s % 3] for s in range(stations)], TX[0], TX[1], 0.0, 0.0, 1, 1, TX[2], 2e6)[0]
    mix = tdoa_amd.clock_mix.midpoint_mix(c.num_stacks(stack)[0])

    def chain(G, R, U, Rf, Z, H):
        """what a caller does without tdoa_process_sync_locate, as one unit"""
        found = c.process_sync_fine(ref, stack, G, R, U, Rf)
        c.locate_set_clock(tdoa_amd.capi.clock_mix_rows(found["clock16"], mix))
        return c.process_locate_zoom(Z, H, stack, 1, 1, want_zmap=False)

    forward = tdoa_amd.line_mix.forward_mix(c.num_stacks(stack)[0])

    def drift_chain(G, Hd, D, R, U, Rf, J, Z, H, Jf):
        """what a caller does without tdoa_process_sync_drift_locate, as one unit"""
        found = c.process_sync_drift_fine(ref, stack, G, Hd, D, R, U, Rf)
        c.locate_set_clock(tdoa_amd.capi.line_mix_rows(found["clock16"], found["fine_rate"], U, D, forward))
        return c.process_locate_track_zoom(Z, H, stack, J, 1, Jf, 1, want_zmap=False, want_ztotal=False)

    def family(name, table, cols, fn, U=1, fine=None, fine_cols=None):
        """a leg of the delay-table family with the statistics off and, with --map-stats, the same leg with them on"""
        def base():
            c.locate_set_clock(None)                                         # (the chain leg of --sync-locate leaves its rows there)
            c.locate_set_table(table, cols)
            if fine is not None:
                c.locate_set_fine_table(fine, fine_cols)
            if upsamples:
                c.locate_set_upsample(U)
        setup[name] = lambda: (base(), c.locate_set_stats(None)) if map_stats else base()
        legs[name] = fn
        if map_stats:
            on = name[:-3] + "_stats_ms"
            setup[on] = lambda: (base(), c.locate_set_stats(*map_stats))
            legs[on] = fn

    for rows, cols in locates:
        table = tdoa_amd.capi.locate_grid_table([ST[s % 3] for s in range(stations)], 41.10, -96.20, 0.3 / max(rows - 1, 1),
                                                0.4 / max(cols - 1, 1), rows, cols, 350.0, 2e6)
        family("process_locate_%dx%d_ms" % (rows, cols), table, cols, lambda: c.process_locate(stack, 1))
        for U in upsamples:
            family("process_locate_%dx%d_up%d_ms" % (rows, cols, U), table, cols, lambda: c.process_locate(stack, 1), U)
        for Z, H in zooms:
            rows_f, cols_f = (rows - 1) * Z + 1, (cols - 1) * Z + 1
            if rows_f * cols_f > 2 ** 22:
                raise SystemExit("--locate-zoom: the fine grid of %d x %d cells has more than 2^22 cells" % (rows_f, cols_f))
            fine = tdoa_amd.capi.locate_grid_table([ST[s % 3] for s in range(stations)], 41.10, -96.20, 0.3 / max(rows - 1, 1) / Z,
                                                   0.4 / max(cols - 1, 1) / Z, rows_f, cols_f, 350.0, 2e6)
            for U in [1] + list(upsamples):
                up = "_up%d" % U if U > 1 else ""
                family("process_locate_zoom_%dx%d_%d_%d%s_ms" % (rows, cols, Z, H, up), table, cols,
                       lambda Z=Z, H=H: c.process_locate_zoom(Z, H, stack, 1, 1, want_zmap=False), U, fine, cols_f)
                family("process_locate_fine_%dx%d_%d%s_ms" % (rows, cols, Z, up), fine, cols_f, lambda: c.process_locate(stack, 1), U)
                for G, Uf, R, Rf in sync_fines if sync_locate else ():
                    tag = "%dx%d_%d_%d_%d_%d_%d_%d%s_ms" % (rows, cols, Z, H, G, Uf, R, Rf, up)
                    family("process_sync_locate_" + tag, table, cols,
                           lambda Z=Z, H=H, G=G, Uf=Uf, R=R, Rf=Rf: c.process_sync_locate(ref, Z, H, stack, G, R, Uf, Rf, None, mix, 1, 1,
                                                                                          want_zmap=False), U, fine, cols_f)
                    family("sync_locate_chain_" + tag, table, cols, lambda Z=Z, H=H, G=G, Uf=Uf, R=R, Rf=Rf: chain(G, R, Uf, Rf, Z, H), U, fine,
                           cols_f)
        for J in locate_tracks:
            family("process_locate_track_%dx%d_J%d_ms" % (rows, cols, J), table, cols, lambda J=J: c.process_locate_track(stack, J, 1))
            for Z, H, Jf in track_zooms:
                rows_f, cols_f = (rows - 1) * Z + 1, (cols - 1) * Z + 1
                if rows_f * cols_f > 2 ** 22:
                    raise SystemExit("--locate-track-zoom: the fine grid of %d x %d cells has more than 2^22 cells" % (rows_f, cols_f))
                fine = tdoa_amd.capi.locate_grid_table([ST[s % 3] for s in range(stations)], 41.10, -96.20, 0.3 / max(rows - 1, 1) / Z,
                                                       0.4 / max(cols - 1, 1) / Z, rows_f, cols_f, 350.0, 2e6)
                for U in [1] + list(upsamples):
                    up = "_up%d" % U if U > 1 else ""
                    family("process_locate_track_zoom_%dx%d_J%d_%d_%d_%d%s_ms" % (rows, cols, J, Z, H, Jf, up), table, cols,
                           lambda J=J, Z=Z, H=H, Jf=Jf: c.process_locate_track_zoom(Z, H, stack, J, 1, Jf, 1, want_zmap=False, want_ztotal=False),
                           U, fine, cols_f)
                    for G, Hd, D, R, Uf, Rf in sync_drift_fines if sync_drift_locate else ():
                        tag = "%dx%d_J%d_%d_%d_%d_%d_%d_%d_%d_%d_%d%s_ms" % (rows, cols, J, Z, H, Jf, G, Hd, D, R, Uf, Rf, up)
                        family("process_sync_drift_locate_" + tag, table, cols,
                               lambda J=J, Z=Z, H=H, Jf=Jf, G=G, Hd=Hd, D=D, R=R, Uf=Uf, Rf=Rf: c.process_sync_drift_locate(
                                   ref, Z, H, stack, G, Hd, D, R, Uf, Rf, None, forward, J, 1, Jf, 1, want_zmap=False, want_ztotal=False),
                               U, fine, cols_f)
                        family("sync_drift_locate_chain_" + tag, table, cols,
                               lambda J=J, Z=Z, H=H, Jf=Jf, G=G, Hd=Hd, D=D, R=R, Uf=Uf, Rf=Rf: drift_chain(G, Hd, D, R, Uf, Rf, J, Z, H, Jf),
                               U, fine, cols_f)
                    if U > 1:
                        family("process_locate_track_%dx%d_J%d%s_ms" % (rows, cols, J, up), table, cols,
                               lambda J=J: c.process_locate_track(stack, J, 1), U)
                    name = "process_locate_track_fine_%dx%d_J%d_%d%s_ms" % (rows, cols, Jf, Z, up)
                    if name not in legs:
                        c.locate_set_table(fine, cols_f)
                        c.locate_set_upsample(U)
                        try:                                             # its maps, steps and sums may not fit the device
                            c.process_locate_track(stack, Jf, 1)
                        except tdoa_amd.TdoaError as e:
                            print("%s: left out: %s" % (name, e), file=sys.stderr)
                        else:
                            family(name, fine, cols_f, lambda Jf=Jf: c.process_locate_track(stack, Jf, 1), U)
                        c.locate_set_upsample(1)
            for K, guard in track_emitters:
                family("process_locate_track_multi_%dx%d_J%d_K%d_G%d_ms" % (rows, cols, J, K, guard), table, cols,
                       lambda J=J, K=K, guard=guard: c.process_locate_track_multi(stack, J, K, guard, 1))
        for K, guard in emitters:
            family("process_locate_multi_%dx%d_K%d_G%d_ms" % (rows, cols, K, guard), table, cols,
                   lambda K=K, guard=guard: c.process_locate_multi(stack, K, guard, 1))
            for Z, H in zooms if emitters_zoom else ():
                rows_f, cols_f = (rows - 1) * Z + 1, (cols - 1) * Z + 1
                if rows_f * cols_f > 2 ** 22:
                    raise SystemExit("--emitters-zoom: the fine grid of %d x %d cells has more than 2^22 cells" % (rows_f, cols_f))
                fine = tdoa_amd.capi.locate_grid_table([ST[s % 3] for s in range(stations)], 41.10, -96.20, 0.3 / max(rows - 1, 1) / Z,
                                                       0.4 / max(cols - 1, 1) / Z, rows_f, cols_f, 350.0, 2e6)
                for U in [1] + list(upsamples):
                    up = "_up%d" % U if U > 1 else ""
                    family("process_locate_multi_zoom_%dx%d_K%d_G%d_%d_%d%s_ms" % (rows, cols, K, guard, Z, H, up), table, cols,
                           lambda K=K, guard=guard, Z=Z, H=H: c.process_locate_multi_zoom(Z, H, stack, K, guard, 1, 1, want_zmap=False),
                           U, fine, cols_f)
                    if U > 1:
                        family("process_locate_multi_%dx%d_K%d_G%d%s_ms" % (rows, cols, K, guard, up), table, cols,
                               lambda K=K, guard=guard: c.process_locate_multi(stack, K, guard, 1), U)
                    name = "process_locate_multi_fine_%dx%d_K%d_G%d_%d%s_ms" % (rows, cols, K, guard, Z, up)
                    c.locate_set_clock(None)
                    c.locate_set_table(fine, cols_f)
                    c.locate_set_upsample(U)
                    try:                                                 # its K planes of maps may not fit the device
                        c.process_locate_multi(stack, K, guard, 1)
                    except tdoa_amd.TdoaError as e:
                        print("%s: left out: %s" % (name, e), file=sys.stderr)
                    else:
                        family(name, fine, cols_f, lambda K=K, guard=guard: c.process_locate_multi(stack, K, guard, 1), U)
                    c.locate_set_upsample(1)
    for G, R in syncs:
        legs["process_sync_%d_%d_ms" % (G, R)] = lambda G=G, R=R: c.process_sync(ref, 0, G, R)
    for G, H, D, R in sync_drifts:
        legs["process_sync_drift_%d_%d_%d_%d_ms" % (G, H, D, R)] = lambda G=G, H=H, D=D, R=R: c.process_sync_drift(ref, stack, G, H, D, R)
    for G, U, R, Rf in sync_fines:
        if stack != 0:
            legs["process_sync_%d_%d_stack%d_ms" % (G, R, stack)] = lambda G=G, R=R: c.process_sync(ref, stack, G, R)
        legs["process_sync_fine_%d_%d_%d_%d_ms" % (G, U, R, Rf)] = lambda G=G, U=U, R=R, Rf=Rf: c.process_sync_fine(ref, stack, G, R, U, Rf)
    for G, H, D, R, U, Rf in sync_drift_fines:
        legs["process_sync_drift_fine_%d_%d_%d_%d_%d_%d_ms" % (G, H, D, R, U, Rf)] = \
            lambda G=G, H=H, D=D, R=R, U=U, Rf=Rf: c.process_sync_drift_fine(ref, stack, G, H, D, R, U, Rf)
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            if name in setup:
                setup[name]()
            times[name].append(timed(fn, steps))
    out = {"config": "cfg2" if stations == 3 else "cfg2 windows, %d stations" % stations, "stations": stations, "pairs": P, "windows": W, "stacks": n_stacks, "locate_stacks": c.num_stacks(stack)[1], "steps": steps, "rounds": rounds,
           "surface_MB": round(W * P * (2 * max_lag - 1) * 4 / 1e6, 1)}
    if max_lag != 20000:
        out["max_lag"] = max_lag
    if map_stats:
        out["map_stats"] = {"ranks": list(map_stats[0]), "foot": map_stats[1]}
    for name, t in times.items():
        out[name] = {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
    print(json.dumps(out), flush=True)
    c.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {"--steps": 20, "--rounds": 5, "--stations": 3, "--stack": 0, "--max-lag": 20000}
    for name in opt:
        if name in args:
            i = args.index(name)
            opt[name] = int(args[i + 1])
            del args[i:i + 2]
    drifts = []
    while "--drift" in args:
        i = args.index("--drift")
        h, _, d = args[i + 1].partition("/")
        drifts.append((int(h), int(d or 1)))
        del args[i:i + 2]
    tracks = []
    while "--track" in args:
        i = args.index("--track")
        tracks.append(int(args[i + 1]))
        del args[i:i + 2]
    closures = []
    while "--closure" in args:
        i = args.index("--closure")
        closures.append(int(args[i + 1]))
        del args[i:i + 2]
    locate_tracks = []
    while "--locate-track" in args:
        i = args.index("--locate-track")
        locate_tracks.append(int(args[i + 1]))
        del args[i:i + 2]
    track_emitters = []
    while "--track-emitters" in args:
        i = args.index("--track-emitters")
        k, _, g = args[i + 1].partition("/")
        track_emitters.append((int(k), int(g or 2)))
        del args[i:i + 2]
    emitters = []
    while "--emitters" in args:
        i = args.index("--emitters")
        k, _, g = args[i + 1].partition("/")
        emitters.append((int(k), int(g or 2)))
        del args[i:i + 2]
    map_stats = None
    if "--map-stats" in args:
        i = args.index("--map-stats")
        r, _, f = args[i + 1].partition("/")
        map_stats = (tuple(int(x) for x in r.split(",")), int(f or 0))
        del args[i:i + 2]
    upsamples = []
    while "--locate-upsample" in args:
        i = args.index("--locate-upsample")
        upsamples.append(int(args[i + 1]))
        del args[i:i + 2]
    locates = []
    while "--locate" in args:
        i = args.index("--locate")
        rows, _, cols = args[i + 1].partition("x")
        locates.append((int(rows), int(cols)))
        del args[i:i + 2]
    zooms = []
    while "--locate-zoom" in args:
        i = args.index("--locate-zoom")
        z, _, h = args[i + 1].partition("/")
        zooms.append((int(z), int(h) if h else 2 * int(z)))
        del args[i:i + 2]
    sync_fines = []
    while "--sync-fine" in args:
        i = args.index("--sync-fine")
        parts = args[i + 1].split("/")
        sync_fines.append((int(parts[0]), int(parts[1]), int(parts[2]) if len(parts) > 2 else 2, int(parts[3]) if len(parts) > 3 else 2))
        del args[i:i + 2]
    sync_drift_fines = []
    while "--sync-drift-fine" in args:
        i = args.index("--sync-drift-fine")
        parts = args[i + 1].split("/")
        if len(parts) != 6:
            raise SystemExit("--sync-drift-fine G/H/D/R/U/RF")
        sync_drift_fines.append(tuple(int(x) for x in parts))
        del args[i:i + 2]
    track_zooms = []
    while "--locate-track-zoom" in args:
        i = args.index("--locate-track-zoom")
        parts = args[i + 1].split("/")
        z = int(parts[0])
        track_zooms.append((z, int(parts[1]) if len(parts) > 1 else min(2 * z, 64), int(parts[2]) if len(parts) > 2 else min(z, 16)))
        del args[i:i + 2]
    sync_locate = "--sync-locate" in args
    if sync_locate:
        args.remove("--sync-locate")
    sync_drift_locate = "--sync-drift-locate" in args
    if sync_drift_locate:
        args.remove("--sync-drift-locate")
    emitters_zoom = "--emitters-zoom" in args
    if emitters_zoom:
        args.remove("--emitters-zoom")
    sync_drifts = []
    while "--sync-drift" in args:
        i = args.index("--sync-drift")
        parts = args[i + 1].split("/")
        sync_drifts.append((int(parts[0]), int(parts[1]), int(parts[2]) if len(parts) > 2 else 1, int(parts[3]) if len(parts) > 3 else 2))
        del args[i:i + 2]
    syncs = []
    while "--sync" in args:
        i = args.index("--sync")
        g, _, r = args[i + 1].partition("/")
        syncs.append((int(g), int(r or 2)))
        del args[i:i + 2]
    main(opt["--steps"], opt["--rounds"], drifts, tracks, closures, opt["--stations"], locates, syncs, locate_tracks, opt["--stack"], emitters,
         track_emitters, map_stats, sync_drifts, upsamples, opt["--max-lag"], sync_fines, zooms, sync_drift_fines, track_zooms, sync_locate,
         sync_drift_locate, emitters_zoom)
