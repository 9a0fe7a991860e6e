// stack_locate_multi.hpp -- tdoa_process_locate_multi: several emitters per stack, found one after the other on the delay-table
// search's map (include/tdoa_mi355x.h, "several emitters per stack").  Round 0 is the search of stack_locate.hpp as it stands.
// Every later round r scores the same table on the same Q, but a pair counts 0 where its lag lies within `guard` of the lag
// an earlier round's cell gave that pair:
//     score_q^r(c) = sum over the pairs of M_p^r[lag_p(c)]     M_p^r[l] = 0 for l in E_p(r) or outside the range, else |Q_p[l]|
// E_p(r) is kept as its intervals' centres, one int32 per (set, pair, round) -- a pair's kLocateMaxEmitters words lie together,
// 32 bytes, so that the scores fetch them with one scalar load -- kLocateNoCentre where a round added none.  Q is never written.
//
// k_locate_centres         after round 0's finish: the centres the location gives, from best[set]; the later rounds' words
//                          start as kLocateNoCentre
// k_locate_scores_masked   k_locate_scores with the test against the pair's r centres before the gather; the centres are the
//                          same words for the whole workgroup and are read like cdiff, through the scalar cache
// k_locate_finish_masked   k_locate_finish's pass 0 with the test on the best cell's pairs (pairs_in, reserved, 0.0 for an
//                          excluded pair), and the round's centres
// The runner-up's pass of a round is k_locate_runner on the round's map and k_locate_finish's pass 1 on the round's records.
#pragma once

#include "stack_locate.hpp"

namespace tdoa {

constexpr int kLocateMaxEmitters = 8;                           // TDOA_LOCATE_MAX_EMITTERS
constexpr int32_t kLocateNoCentre = INT32_MIN;                  // further than any guard from every lag of the range
// up to here the masked scores keep a cell's delays in registers: at 16 stations the unrolled form with the mask's test needs
// 258 registers, one wave per SIMD, where the re-reading form keeps eight
constexpr int kLocateMaskedRegStations = 15;

struct LocateMask {
    int32_t round;             // the round being scored: rounds 0 .. round - 1 have left centres
    int32_t guard;             // at most the range's length (the host clips it), so lag - kLocateNoCentre is always beyond it
};

// the centres of one (set, pair), word r from round r
struct alignas(32) LocateCentres {
    int32_t c[kLocateMaxEmitters];
};

// l, a lag inside the range, lies in E_p(round).  The range and the guard are far below 2^31, so the distance is taken in 32
// bits: from kLocateNoCentre it is at least 2^31 - max_lag.  The pair's centres come in one load (a scalar one where the pair
// is the same for the whole wave), and only the tests of the rounds gone by are run: mk.round is wave-uniform.
__device__ __forceinline__ bool locate_excluded(int32_t l, const LocateCentres *__restrict__ cen, const LocateMask &mk)
{
    const LocateCentres cc = *cen;
    bool ex = false;
#pragma unroll
    for (int r = 0; r < kLocateMaxEmitters - 1; r++) {
        if (r >= mk.round) break;
        const int32_t d = (int32_t)((uint32_t)l - (uint32_t)cc.c[r]);
        ex |= (d < 0 ? 0u - (uint32_t)d : (uint32_t)d) <= (uint32_t)mk.guard;
    }
    return ex;
}

// M_p^r at a cell's lag
__device__ __forceinline__ long long locate_m_masked(const long long *q, int32_t ti, int32_t tj, const LocateGeom &g, long long cd,
                                                     const LocateCentres *__restrict__ cen, const LocateMask &mk)
{
    const long long l = locate_lag(ti, tj, cd), idx = l - g.lag_lo;
    if (idx < 0 || idx >= g.n || locate_excluded((int32_t)l, cen, mk)) return 0;
    const long long v = q[idx];
    return v < 0 ? -v : v;
}

// lag_p(cell) of pair p of a set where it lies inside the searched range, kLocateNoCentre otherwise: the centre round 0 leaves
__device__ __forceinline__ int32_t locate_centre(const LocateGeom &g, const int32_t *table, const long long *cdiff, int set, int cell, int p)
{
    int i, j;
    locate_pair(p, g.S, &i, &j);
    const long long l = locate_lag(table[(size_t)i * g.n_cells + cell], table[(size_t)j * g.n_cells + cell],
                                   cdiff ? cdiff[(size_t)set * g.P + p] : 0),
                    idx = l - g.lag_lo;
    return idx >= 0 && idx < g.n ? (int32_t)l : kLocateNoCentre;
}

// One workgroup per set, after round 0's finish has left the location's cell in best (-1: none):
// centres[set][pair].c[0] = lag_p(cell*) where the round found a cell and the lag lies inside the range; c[1 ..] = none yet.
__global__ __launch_bounds__(kLocateThreads) void k_locate_centres(LocateGeom g, const int32_t *table, const long long *cdiff,
                                                                   const int32_t *best, LocateCentres *centres)
{
    const int set = blockIdx.x, cell = best[set];
    const bool found = cell >= 0 && cell < g.n_cells;
    for (int p = threadIdx.x; p < g.P; p += kLocateThreads) {
        const int32_t c = found ? locate_centre(g, table, cdiff, set, cell, p) : kLocateNoCentre;
        LocateCentres cc;
        cc.c[0] = c;
        for (int r = 1; r < kLocateMaxEmitters; r++) cc.c[r] = kLocateNoCentre;
        centres[(size_t)set * g.P + p] = cc;
    }
}

// k_locate_scores's grid, arguments and outputs (map and partial: the round's); S_T (at most kLocateMaskedRegStations) and CLK
// as there.  centres [set][pair].
template <int S_T, bool CLK>
__global__ __launch_bounds__(kLocateThreads) void k_locate_scores_masked(const long long *Q, LocateGeom g, const int32_t *table,
                                                                         const long long *__restrict__ cdiff,
                                                                         const LocateCentres *__restrict__ centres, LocateMask mk,
                                                                         long long *map, ClosureCand *partial)
{
    __shared__ long long red_s[kLocateThreads / kWave];
    __shared__ uint32_t red_k[kLocateThreads / kWave];
    const int set = blockIdx.y, t = threadIdx.x;
    const int cell = (int)blockIdx.x * kLocateThreads + t;
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    if (cell < g.n_cells) {
        const long long *q = Q + (size_t)set * g.P * g.n;
        const long long *cd = CLK ? cdiff + (size_t)set * g.P : nullptr;
        const LocateCentres *cen = centres + (size_t)set * g.P;
        const int32_t *tc = table + cell;
        long long s = 0;
        if constexpr (S_T > 0) {
            int32_t d[S_T];
#pragma unroll
            for (int i = 0; i < S_T; i++) d[i] = tc[(size_t)i * g.n_cells];
#pragma unroll
            for (int i = 0; i < S_T; i++)
#pragma unroll
                for (int j = i + 1; j < S_T; j++, q += g.n, cen++) {
                    long long c = 0;
                    if constexpr (CLK) c = *cd++;
                    s += locate_m_masked(q, d[i], d[j], g, c, cen, mk);
                }
        } else {
            for (int i = 0; i < g.S; i++) {
                const int32_t di = tc[(size_t)i * g.n_cells];
                for (int j = i + 1; j < g.S; j++, q += g.n, cen++) {
                    long long c = 0;
                    if constexpr (CLK) c = *cd++;
                    s += locate_m_masked(q, di, tc[(size_t)j * g.n_cells], g, c, cen, mk);
                }
            }
        }
        map[(size_t)set * g.n_cells + cell] = s;
        bs = s;
        bk = ~(uint32_t)cell;
    }
    closure_block_best(bs, bk, red_s, red_k);
    if (t == 0) partial[(size_t)set * g.tiles + blockIdx.x] = ClosureCand{bs, bk, 0};
}

// One workgroup per set: k_locate_finish's pass 0 for round mk.round >= 1 (best, out, lags, corr: the round's).  A pair inside
// the range whose lag at the best cell lies in E_p(round) reports its lag and 0.0 and counts in `reserved`, not in pairs_in.
// centres[set][pair].c[round] as k_locate_centres writes word 0.
__global__ __launch_bounds__(kLocateThreads) void k_locate_finish_masked(const long long *Q, LocateGeom g, const int32_t *table,
                                                                         const long long *cdiff, const double *roots,
                                                                         const ClosureCand *partial, LocateMask mk, LocateCentres *centres,
                                                                         int32_t *best, LocateOut *out, int32_t *lags, double *corr)
{
    __shared__ long long red_s[kLocateThreads / kWave];
    __shared__ uint32_t red_k[kLocateThreads / kWave];
    __shared__ int red_n[kLocateThreads / kWave];
    const int set = blockIdx.x, t = threadIdx.x;
    long long bs;
    uint32_t bk;
    search_best_candidate(partial + (size_t)set * g.tiles, g.tiles, red_s, red_k, bs, bk);
    const double root = roots[set];
    const int cell = (int)~bk;
    const bool found = bs > 0 && cell >= 0 && cell < g.n_cells;
    const long long *q = Q + (size_t)set * g.P * g.n;
    LocateCentres *cen = centres + (size_t)set * g.P;
    int counts = 0;                          // pairs inside and not excluded, + 2^16 pairs inside and excluded (P <= 2016)
    for (int p = t; p < g.P; p += kLocateThreads) {
        int32_t lag = 0, centre = kLocateNoCentre;
        double c = 0.0;
        if (found && locate_pair_value(q, g, table, cdiff ? cdiff + (size_t)set * g.P : nullptr, cell, p, root, &lag, &c)) {
            centre = lag;
            if (locate_excluded(lag, cen + p, mk)) {
                c = 0.0;
                counts += 1 << 16;
            } else {
                counts++;
            }
        }
        lags[(size_t)set * g.P + p] = lag;
        corr[(size_t)set * g.P + p] = c;
        cen[p].c[mk.round] = centre;
    }
    counts = search_wave_sum(counts);
    if ((t & (kWave - 1)) == 0) red_n[t / kWave] = counts;
    __syncthreads();
    if (t != 0) return;
    LocateOut rec{0, 0, 0, 0, 0, 0, 0.0, 0.0};
    if (found) {
        int n = 0;
        for (int w = 0; w < kLocateThreads / kWave; w++) n += red_n[w];
        rec.cell = cell;
        rec.pairs_in = n & 0xffff;
        rec.reserved = n >> 16;
        rec.score_q = bs;
        rec.score = stack_value(bs, root);
    }
    best[set] = found ? cell : -1;
    out[set] = rec;
}

}  // namespace tdoa
