// stack_locate_track_multi.hpp -- tdoa_process_locate_track_multi: several emitters per block, found one after the other as
// cell tracks (include/tdoa_mi355x.h, "several emitters per block").  Round 0 is the delay-table search and the cell track of
// stack_locate.hpp and stack_cell_track.hpp as they stand.  Every later round r scores the same table on the same Q with the
// masked scores of stack_locate_multi.hpp -- a pair of stack j counts 0 where its lag lies within `guard` of the lag an earlier
// round's track gave that pair in that stack -- and runs the recurrence on those maps:
//     s_j^r(c) = sum over the pairs of M_p^{j,r}[lag_p^j(c)]     T_j^r[c] = s_j^r[c] + max over the neighbours of T_{j+1}^r
// E_p^j(r) is kept as in stack_locate_multi.hpp: LocateCentres[set][pair], word r from round r's track, the set being the
// stack.  Q is never written.
//
// k_track_centres             after round 0's track: word 0 of every (stack, pair) from the track's cell in that stack, the later
//                             rounds' words kLocateNoCentre, and round 0's pairs_in / reserved per stack
// k_cell_track_finish_masked  k_cell_track_finish's pass 0 for a round r >= 1 with the test on every (position, pair): 0.0 for
//                             an excluded pair, the per-position counts, word r of the centres
// The scores of a round are k_locate_scores_masked, the recurrence k_cell_track_step and k_cell_track_best, the runner-up's
// pass k_locate_runner on T_0^r and k_cell_track_finish's pass 1 on the round's records.
#pragma once

#include "stack_cell_track.hpp"
#include "stack_locate_multi.hpp"

namespace tdoa {

// One workgroup per stack (set = track * L + position), after round 0's k_cell_track_finish has left the tracks' cells in
// `cells` [set] and L_0 in best [track] (-1: the zero record):
// centres[set][pair].c[0] = lag_p^j(L_j) where the track was found and the lag lies inside the range; c[1 ..] = none yet;
// pairs[set] = (the pairs inside the range at L_j, 0), (0, 0) for the zero record.
__global__ __launch_bounds__(kLocateThreads) void k_track_centres(LocateGeom g, int L, const int32_t *table, const long long *cdiff,
                                                                  const int32_t *best, const int32_t *cells, LocateCentres *centres,
                                                                  int32_t *pairs)
{
    __shared__ int red_n[kLocateThreads / kWave];
    const int set = blockIdx.x, t = threadIdx.x;
    const int cell = cells[set];
    const bool found = best[set / L] >= 0 && cell >= 0 && cell < g.n_cells;
    int inside = 0;
    for (int p = t; p < g.P; p += kLocateThreads) {
        const int32_t c = found ? locate_centre(g, table, cdiff, set, cell, p) : kLocateNoCentre;
        inside += c != kLocateNoCentre;
        LocateCentres cc;
        cc.c[0] = c;
        for (int r = 1; r < kLocateMaxEmitters; r++) cc.c[r] = kLocateNoCentre;
        centres[(size_t)set * g.P + p] = cc;
    }
    inside = search_wave_sum(inside);
    if ((t & (kWave - 1)) == 0) red_n[t / kWave] = inside;
    __syncthreads();
    if (t != 0) return;
    int n = 0;
    for (int w = 0; w < kLocateThreads / kWave; w++) n += red_n[w];
    pairs[2 * (size_t)set] = n;
    pairs[2 * (size_t)set + 1] = 0;
}

// One workgroup per track: k_cell_track_finish's pass 0 for round mk.round >= 1 (map, D, partial, out, cells, own, lags, corr:
// the round's; arguments as there).  A wave takes whole positions, its lanes the position's pairs, so a position's counts are
// one wave's sum: no atomics, and the same order every time.  A pair inside the range whose lag at L_j lies in
// E_p^j(round) reports its lag and 0.0 and counts in pairs[set][1], not in pairs[set][0].  centres[set][pair].c[round] as
// k_track_centres writes word 0.  The zero record: every per-position output 0, no centre, best = -1.
__global__ __launch_bounds__(kCellTrackThreads) void k_cell_track_finish_masked(const long long *Q, LocateGeom lg, CellTrackGeom g,
                                                                                const int32_t *table, const long long *cdiff,
                                                                                const double *roots, const double *track_roots,
                                                                                const long long *map, const signed char *D,
                                                                                const ClosureCand *partial, LocateMask mk,
                                                                                LocateCentres *centres, int32_t *best, CellTrackOut *out,
                                                                                int32_t *cells, long long *own, int32_t *pairs,
                                                                                int32_t *lags, double *corr)
{
    __shared__ long long red_s[kCellTrackThreads / kWave];
    __shared__ uint32_t red_k[kCellTrackThreads / kWave];
    __shared__ int32_t path[kCellTrackMaxLen];
    const int track = blockIdx.x, t = threadIdx.x;
    long long bs;
    uint32_t bk;
    search_best_candidate(partial + (size_t)track * lg.tiles, lg.tiles, red_s, red_k, bs, bk);
    const int cell = (int)~bk;
    const bool found = bs > 0 && cell >= 0 && cell < g.n_cells;
    const size_t set0 = (size_t)track * g.L;
    const int steps = cell_track_walk(g, map, D, set0, found, cell, path, cells, own);
    const int lane = t & (kWave - 1);
    for (int j = t / kWave; j < g.L; j += kCellTrackThreads / kWave) {
        const size_t set = set0 + j;
        LocateCentres *cen = centres + set * lg.P;
        int counts = 0;                      // pairs inside and not excluded, + 2^16 pairs inside and excluded (P <= 2016)
        for (int p = lane; p < lg.P; p += kWave) {
            int32_t lag = 0, centre = kLocateNoCentre;
            double c = 0.0;
            if (found && locate_pair_value(Q + set * lg.P * lg.n, lg, table, cdiff ? cdiff + set * lg.P : nullptr, path[j], p, roots[set], &lag, &c)) {
                centre = lag;
                if (locate_excluded(lag, cen + p, mk)) {
                    c = 0.0;
                    counts += 1 << 16;
                } else {
                    counts++;
                }
            }
            lags[set * lg.P + p] = lag;
            corr[set * lg.P + p] = c;
            cen[p].c[mk.round] = centre;
        }
        counts = search_wave_sum(counts);
        if (lane == 0) {
            pairs[2 * set] = counts & 0xffff;
            pairs[2 * set + 1] = counts >> 16;
        }
    }
    if (t != 0) return;
    CellTrackOut rec{0, 0, 0, 0, 0, 0, 0.0, 0.0};
    if (found) {
        rec.cell = cell;
        rec.positions = g.L;
        rec.steps = steps;
        rec.score_q = bs;
        rec.score = stack_value(bs, track_roots[track]);
    }
    best[track] = found ? cell : -1;
    out[track] = rec;
}

}  // namespace tdoa
