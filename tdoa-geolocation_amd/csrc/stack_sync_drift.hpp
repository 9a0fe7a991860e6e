// stack_sync_drift.hpp -- tdoa_process_sync_drift: the stations' clock offsets and rates from a reference block
// (include/tdoa_mi355x.h, "clock lines").  A line is one block, its positions j = 0 .. L-1 the block's stacks in order.
// Station s has the clock k_s(j) = k_s + shift(h_s, j) at position j, k_s = centre[s] + x_s, |x_s| <= G, |h_s| <= H, station 0
// the gauge, and
//     A_ij = sum over j of Q_{j,ij}[e_ij + k_j(j) - k_i(j)]      F = sum over the pairs of |A_ij|
// is searched station by station: the placing of stations 1 .. S-1 against the stations before them, then R Gauss-Seidel
// sweeps against all the others.  A station's candidates (h, x) compete in the order r = rank(h) (2G+1) + rank(x), the first
// of equal maxima wins.
//
// k_syncline_init    every station on its centre with slope 0: k, h and the clock table cur [line][station][position]
// k_syncline_step    one station's step: grid (tiles of 256 candidates, lines), one candidate per lane.  The partner loop is
//                    outside and the position loop inside, one int64 accumulator per partner whose magnitude is taken
//                    once.  The partners' clocks are the same for the whole workgroup and come from cur through the scalar
//                    cache; the candidate's own shift(h, j) comes from the host-made table tab [rank(h)][position]: no
//                    division in the loops.  The tile's best goes out as a two-word candidate, key = ~r
// k_syncline_commit  one workgroup per line: the tiles' candidates -> the station's (k, h), its row of cur, and `moved`
// k_syncline_finish  F and terms_in; pass 0 keeps F as start_q, pass 1 writes the record, the clocks, the rates, the rows,
//                    the lags and the correlations, all zero where F = 0.  A template over the lag grid: on SyncFineGrid it is
//                    the fine clock lines' finish as well
//
// Everything is integer arithmetic on the Q words of stack_surfaces.hpp; the only floating point is stack_value on the way
// out.  The candidate, its order and the workgroup reductions are the ones all stack searches share (stack_closure.hpp), the
// lag grid the clock search's (SyncGrid, stack_sync.hpp), the pair order the delay-table search's (stack_locate.hpp), shift
// the slope search's (stack_drift.hpp).  syncline_best, the start of a commit kernel, serves the fine clock lines too.
#pragma once

#include "stack_sync.hpp"

namespace tdoa {

constexpr int kSyncLineThreads = kSyncThreads;                  // candidates per tile, threads of the other kernels
constexpr int kSyncLineMaxDrift = 512;

// tdoa_sync_line
struct SyncLineOut {
    int32_t moved, terms_in, positions, reserved;
    long long score_q, start_q;
    double score;
};

struct SyncLineGeom {
    int32_t S, P;              // stations, pairs
    int32_t n, lag_lo;         // lags per row of Q, the first one
    int32_t W, V;              // offsets and slopes of a station: 2 G + 1, 2 H + 1
    int32_t L;                 // positions of a line
    int32_t cands, tiles;      // candidates of a station, W V, and ceil(cands / kSyncLineThreads)
};

// the buffers of a search: the inputs are written by the host, the rest by the kernels
struct SyncLineDev {
    const int32_t *in;         // ref_delay [kSyncMaxStations], then centre [kSyncMaxStations]
    const int32_t *tab;        // shift(h, j) at [rank(h) * L + j]
    long long *cur;            // k_s(j) at [(line * S + s) * L + j]
    long long *k;              // [line][S]
    int32_t *h;                // [line][S]
    ClosureCand *part;         // [line][tile]
    int32_t *moved;            // [line]
    long long *start_q;        // [line]
};

// The start of a commit kernel: the tiles' candidates of a line's step, part[tiles], -> the winner r = rank(slope) W + rank(offset)
// as its two ranks, in every thread.  Every tile holds a candidate, so r < cands.
__device__ __forceinline__ void syncline_best(const ClosureCand *part, int tiles, int cands, int W, long long *red_s, uint32_t *red_k,
                                              uint32_t *rank_h, uint32_t *rank_x)
{
    long long bs;
    uint32_t bk;
    search_best_candidate(part, tiles, red_s, red_k, bs, bk);
    const uint32_t r = min(~bk, (uint32_t)(cands - 1));
    *rank_h = r / (uint32_t)W;
    *rank_x = r - *rank_h * (uint32_t)W;
}

// One workgroup per line.
__global__ __launch_bounds__(kSyncLineThreads) void k_syncline_init(SyncLineGeom g, SyncLineDev d)
{
    const int line = blockIdx.x, t = threadIdx.x;
    const int32_t *centre = d.in + kSyncMaxStations;
    for (int e = t; e < g.S * g.L; e += kSyncLineThreads) d.cur[(size_t)line * g.S * g.L + e] = centre[e / g.L];
    if (t < g.S) {
        d.k[(size_t)line * g.S + t] = centre[t];
        d.h[(size_t)line * g.S + t] = 0;
    }
    if (t == 0) d.moved[line] = 0;
}

// grid (tiles, lines).  Q: [line][position][pair][n].  Station s against the partners i < hi, i != s.
// part[line * tiles + tile] = the tile's best candidate (equal sums: the smaller r).
__global__ __launch_bounds__(kSyncLineThreads) void k_syncline_step(const long long *Q, SyncLineGeom g, const int32_t *__restrict__ in,
                                                                    const int32_t *__restrict__ tab, const long long *__restrict__ cur,
                                                                    int s, int hi, ClosureCand *part)
{
    __shared__ long long red_s[kSyncLineThreads / kWave];
    __shared__ uint32_t red_k[kSyncLineThreads / kWave];
    const int line = blockIdx.y, t = threadIdx.x;
    const int r = (int)blockIdx.x * kSyncLineThreads + t;
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    if (r < g.cands) {
        const int rh = r / g.W;
        const long long ks = (long long)in[kSyncMaxStations + s] + closure_unrank((uint32_t)(r - rh * g.W));
        const int32_t *own = tab + (size_t)rh * g.L;
        const long long *q_line = Q + (size_t)line * g.L * g.P * g.n;
        const long long *cur_line = cur + (size_t)line * g.S * g.L;
        const size_t pos_stride = (size_t)g.P * g.n;
        long long sum = 0;
        for (int i = 0; i < hi; i++) {
            if (i == s) continue;
            // i < s: e_is + k_s(j) - k_i(j); i > s: e_si + k_i(j) - k_s(j)
            const bool below = i < s;
            const long long e = below ? locate_lag(in[i], in[s]) : locate_lag(in[s], in[i]);
            const long long *q = q_line + (size_t)(below ? closure_pair(i, s, g.S) : closure_pair(s, i, g.S)) * g.n;
            const long long *ki = cur_line + (size_t)i * g.L;
            // a term outside the range reads word 0 of its row and adds 0: the loads do not wait for one another
            long long acc = 0;
#pragma unroll 4
            for (int j = 0; j < g.L; j++) {
                const long long dk = ks + own[j] - ki[j];
                const long long idx = (below ? e + dk : e - dk) - g.lag_lo;
                const bool inside = idx >= 0 && idx < g.n;
                const long long v = q[(size_t)j * pos_stride + (inside ? idx : 0)];
                acc += inside ? v : 0;
            }
            sum += acc < 0 ? -acc : acc;
        }
        bs = sum;
        bk = ~(uint32_t)r;
    }
    closure_block_best(bs, bk, red_s, red_k);
    if (t == 0) part[(size_t)line * g.tiles + blockIdx.x] = ClosureCand{bs, bk, 0};
}

// One workgroup per line.  first: the step opens a sweep (the count starts again); count: the step belongs to a sweep.
__global__ __launch_bounds__(kSyncLineThreads) void k_syncline_commit(SyncLineGeom g, SyncLineDev d, int s, int first, int count)
{
    __shared__ long long red_s[kSyncLineThreads / kWave];
    __shared__ uint32_t red_k[kSyncLineThreads / kWave];
    const int line = blockIdx.x, t = threadIdx.x;
    uint32_t rh, rx;
    syncline_best(d.part + (size_t)line * g.tiles, g.tiles, g.cands, g.W, red_s, red_k, &rh, &rx);
    const long long ks = (long long)d.in[kSyncMaxStations + s] + closure_unrank(rx);
    const int32_t hs = closure_unrank(rh);
    for (int j = t; j < g.L; j += kSyncLineThreads) d.cur[((size_t)line * g.S + s) * g.L + j] = ks + d.tab[(size_t)rh * g.L + j];
    if (t == 0) {
        const size_t at = (size_t)line * g.S + s;
        const int changed = d.k[at] != ks || d.h[at] != hs;
        d.k[at] = ks;
        d.h[at] = hs;
        if (count) d.moved[line] = (first ? 0 : d.moved[line]) + changed;
    }
}

// One workgroup per line, for the clock lines (SyncGrid) and the fine clock lines (SyncFineGrid, stack_sync_drift_fine.hpp): g
// and d are the search's own geometry (S, P, L) and buffers (in, cur, moved, start_q); k and h [line][S]: the stations' offsets
// and slopes in the grid's unit; coarse [line]: the records a refinement stands on, nullptr: none.  roots [set]: sqrt(n_w) of a
// position's stack; line_roots [line]: sqrt(N_w).
// pass 0: F into start_q.  pass 1: rec [line]; clock [line][S] in the grid's clock unit and rate [line][S]; rows [set][S]: the
// clock table in 1/16 sample; lags (in the grid's unit) and corr [set][P]: the lag along the line and the signed value of that
// stack's word there, 0 and 0.0 outside the range.  F = 0 or a zero coarse record: all zero.
template <class Grid, class Geom, class Dev, class Rate>
__global__ __launch_bounds__(kSyncLineThreads) void k_syncline_finish(const long long *Q, Grid gr, Geom g, Dev d, const long long *k,
                                                                      const Rate *h, const SyncLineOut *coarse, int pass,
                                                                      const double *roots, const double *line_roots, SyncLineOut *rec,
                                                                      int32_t *clock, int32_t *rate, int32_t *rows, int32_t *lags,
                                                                      double *corr)
{
    __shared__ long long red_s[kSyncLineThreads / kWave];
    __shared__ int red_n[kSyncLineThreads / kWave];
    const int line = blockIdx.x, t = threadIdx.x;
    const long long *q_line = Q + (size_t)line * g.L * g.P * gr.n;
    const long long *cur_line = d.cur + (size_t)line * g.S * g.L;
    const size_t pos_stride = (size_t)g.P * gr.n;
    gr.stage();
    long long f = 0;
    int inside = 0;
    for (int p = t; p < g.P; p += kSyncLineThreads) {
        int i, j;
        locate_pair(p, g.S, &i, &j);
        const long long e = gr.lag(d.in[i], d.in[j]);
        const long long *q = q_line + (size_t)p * gr.n, *ki = cur_line + (size_t)i * g.L, *kj = cur_line + (size_t)j * g.L;
        long long acc = 0;
        for (int x = 0; x < g.L; x++, q += pos_stride) {
            long long v;
            if (!gr.word(q, e + kj[x] - ki[x], &v)) continue;
            acc += v;
            inside++;
        }
        f += acc < 0 ? -acc : acc;
    }
    search_block_sum(f, inside, red_s, red_n);
    if (pass == 0) {
        if (t == 0) d.start_q[line] = f;
        return;
    }
    const bool found = f != 0 && (!coarse || coarse[line].score_q != 0);
    const size_t set0 = (size_t)line * g.L;
    for (int p = t; p < g.P; p += kSyncLineThreads) {
        int i, j;
        locate_pair(p, g.S, &i, &j);
        const long long e = gr.lag(d.in[i], d.in[j]);
        const long long *q = q_line + (size_t)p * gr.n, *ki = cur_line + (size_t)i * g.L, *kj = cur_line + (size_t)j * g.L;
        for (int x = 0; x < g.L; x++, q += pos_stride) {
            const long long l = e + kj[x] - ki[x];
            long long v;
            int32_t lag = 0;
            double c = 0.0;
            if (found && gr.word(q, l, &v)) {
                lag = (int32_t)l;
                c = stack_value(v, roots[set0 + x]);
            }
            lags[(set0 + x) * g.P + p] = lag;
            corr[(set0 + x) * g.P + p] = c;
        }
    }
    for (int e = t; e < g.S * g.L; e += kSyncLineThreads) {
        const int s = e / g.L, x = e - s * g.L;
        rows[(set0 + x) * g.S + s] = found ? (int32_t)(cur_line[e] * gr.unit16()) : 0;
    }
    if (t < g.S) {
        clock[(size_t)line * g.S + t] = found ? (int32_t)(k[(size_t)line * g.S + t] * gr.clock_unit()) : 0;
        rate[(size_t)line * g.S + t] = found ? (int32_t)h[(size_t)line * g.S + t] : 0;
    }
    if (t == 0)
        rec[line] = found ? SyncLineOut{d.moved[line], inside, g.L, 0, f, d.start_q[line], stack_value(f, line_roots[line])}
                          : SyncLineOut{0, 0, 0, 0, 0, 0, 0.0};
}

}  // namespace tdoa
