// stack_locate.hpp -- tdoa_process_locate: a table of candidate positions scored on all pairs' stacked surfaces
// (include/tdoa_mi355x.h, "delay-table search").  Every candidate ("cell") c fixes one delay per station, t[c][s] in units of
// 1/16 sample, hence one lag per pair, and
//     score_q(c) = sum over the pairs (i, j) of M_p[lag_p(c)]        M_p[l] = |Q_p[l]|, a lag outside the range counts 0
// The best cell uses every pair at once and needs no peak to be picked.  The kernels know nothing about the earth: the table
// is data.
//
// k_locate_scores   one cell per lane: its station delays from the station-major table, one lag and one 8-byte gather of Q per
//                   pair; the scores go to the map [set][cell], the tile's best out as a two-word candidate (key = ~cell)
//                   (a second instantiation adds the stack's clock difference of each pair: tdoa_locate_set_clock)
// k_locate_runner   the same grid over the map: the best cell more than min_separation rows or columns from the location
// k_locate_finish   the tiles' candidates -> the record, and the lags and signed correlations of the best cell
//                   (locate_pair_value, shared with the cell tracks of stack_cell_track.hpp); after the runner-up's pass:
//                   runner_q, runner_up, runner_cell
//
// Everything is integer arithmetic on the Q words of stack_surfaces.hpp; the only floating point is stack_value on the way
// out.  The candidate, its order and the workgroup reduction are the closure search's (stack_closure.hpp).
#pragma once

#include "stack_closure.hpp"

namespace tdoa {

constexpr int kLocateThreads = 256;                             // cells per tile
constexpr int kLocateMaxCells = 1 << 22;
constexpr int kLocateMaxStations = 64;
constexpr int kLocateRegStations = 16;                          // up to here a cell's delays stay in registers
constexpr int kLocateMaxSets = 65535;                           // the grid's second dimension
constexpr int kLocateDelayUnit = 16;                            // TDOA_DELAY_UNIT
static_assert(kLocateThreads == kClosureThreads, "closure_block_best reduces kClosureThreads candidates");

// tdoa_location
struct LocateOut {
    int32_t cell, runner_cell, pairs_in, reserved;
    long long score_q, runner_q;
    double score, runner_up;
};

struct LocateGeom {
    int32_t S, P;              // stations, pairs
    int32_t n, lag_lo;         // lags per row of Q, the first one
    int32_t n_cells, n_cols;   // the table's cells; cell c lies at row c div n_cols, column c mod n_cols
    int32_t sep;               // min_separation
    int32_t tiles;             // ceil(n_cells / kLocateThreads)
};

// lag_p(c) = sgn(d) ((2 |d| + 16) div 32), d = t[c][j] - t[c][i] in 64 bits: the nearest integer to d / 16, halves away from
// zero.  With station clocks (tdoa_locate_set_clock) the stack's clock difference of the pair, cd = clock[j] - clock[i], is
// added to d first: it is the same for every cell of a (stack, pair), so the kernels take it as one word per (set, pair).
__device__ __forceinline__ long long locate_lag(int32_t ti, int32_t tj, long long cd = 0)
{
    const long long d = (long long)tj - (long long)ti + cd;
    const long long a = (2 * (d < 0 ? -d : d) + kLocateDelayUnit) / (2 * kLocateDelayUnit);
    return d < 0 ? -a : a;
}

// M_p at a cell's lag, 0 outside the searched range
__device__ __forceinline__ long long locate_m(const long long *q, int32_t ti, int32_t tj, const LocateGeom &g, long long cd = 0)
{
    const long long idx = locate_lag(ti, tj, cd) - g.lag_lo;
    if (idx < 0 || idx >= g.n) return 0;
    const long long v = q[idx];
    return v < 0 ? -v : v;
}

// grid (tiles, n_sets), kLocateThreads threads.  Q: [set][pair][n]; table: [station][n_cells].  S_T: the station count when
// it is at most kLocateRegStations (the delays stay in registers, both loops unrolled), 0: any count, the delays re-read.
// CLK: cdiff [set][pair] holds the pairs' clock differences -- the same word for the whole workgroup, so it is read through
// the scalar cache and costs no vector register; without CLK cdiff is not read and the kernel is the clock-less one.
// map[set][cell] = score_q(cell); partial[set * tiles + tile] = the tile's best candidate (equal scores: the smaller cell).
template <int S_T, bool CLK>
__global__ __launch_bounds__(kLocateThreads) void k_locate_scores(const long long *Q, LocateGeom g, const int32_t *table,
                                                                  const long long *__restrict__ cdiff, long long *map,
                                                                  ClosureCand *partial)
{
    __shared__ long long red_s[kLocateThreads / kWave];
    __shared__ uint32_t red_k[kLocateThreads / kWave];
    const int set = blockIdx.y, t = threadIdx.x;
    const int cell = (int)blockIdx.x * kLocateThreads + t;
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    if (cell < g.n_cells) {
        const long long *q = Q + (size_t)set * g.P * g.n;
        const int32_t *tc = table + cell;
        const long long *cd = CLK ? cdiff + (size_t)set * g.P : nullptr;
        long long s = 0;
        if constexpr (S_T > 0) {
            int32_t d[S_T];
#pragma unroll
            for (int i = 0; i < S_T; i++) d[i] = tc[(size_t)i * g.n_cells];
#pragma unroll
            for (int i = 0; i < S_T; i++)
#pragma unroll
                for (int j = i + 1; j < S_T; j++, q += g.n) {
                    long long c = 0;
                    if constexpr (CLK) c = *cd++;
                    s += locate_m(q, d[i], d[j], g, c);
                }
        } else {
            for (int i = 0; i < g.S; i++) {
                const int32_t di = tc[(size_t)i * g.n_cells];
                for (int j = i + 1; j < g.S; j++, q += g.n) {
                    long long c = 0;
                    if constexpr (CLK) c = *cd++;
                    s += locate_m(q, di, tc[(size_t)j * g.n_cells], g, c);
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

// The same grid.  best[set]: the location's cell, -1 where there is none (no candidate then).  Only the cells with
// max(|row - row*|, |col - col*|) > sep compete; their scores come from the map.
__global__ __launch_bounds__(kLocateThreads) void k_locate_runner(const long long *map, LocateGeom g, const int32_t *best,
                                                                  ClosureCand *partial)
{
    __shared__ long long red_s[kLocateThreads / kWave];
    __shared__ uint32_t red_k[kLocateThreads / kWave];
    const int set = blockIdx.y, t = threadIdx.x;
    const int cell = (int)blockIdx.x * kLocateThreads + t, b = best[set];
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    if (cell < g.n_cells && b >= 0 && b < g.n_cells) {
        const int dr = cell / g.n_cols - b / g.n_cols, dc = cell % g.n_cols - b % g.n_cols;
        if (max(abs(dr), abs(dc)) > g.sep) {
            bs = map[(size_t)set * g.n_cells + cell];
            bk = ~(uint32_t)cell;
        }
    }
    closure_block_best(bs, bk, red_s, red_k);
    if (t == 0) partial[(size_t)set * g.tiles + blockIdx.x] = ClosureCand{bs, bk, 0};
}

// pair number p of S stations -> (i, j), i < j in the library's order
__device__ __forceinline__ void locate_pair(int p, int S, int *i, int *j)
{
    int a = 0;
    for (int c = S - 1; p >= c; c = S - 1 - a) {
        p -= c;
        a++;
    }
    *i = a;
    *j = a + 1 + p;
}

// What the finishing kernels report of one cell for pair p of a set: lag_p(cell) and the signed C of the set's row there;
// false, lag 0 and 0.0 for a pair outside the range.  q: the set's rows [P][n]; cd: the set's clock differences [P], nullptr:
// none.
__device__ __forceinline__ bool locate_pair_value(const long long *q, const LocateGeom &g, const int32_t *table, const long long *cd,
                                                  int cell, int p, double root, int32_t *lag, double *c)
{
    int i, j;
    locate_pair(p, g.S, &i, &j);
    const long long l = locate_lag(table[(size_t)i * g.n_cells + cell], table[(size_t)j * g.n_cells + cell], cd ? cd[p] : 0),
                    idx = l - g.lag_lo;
    *lag = 0;
    *c = 0.0;
    if (idx < 0 || idx >= g.n) return false;
    *lag = (int32_t)l;
    *c = stack_value(q[(size_t)p * g.n + idx], root);
    return true;
}

// One workgroup per set.
// pass 0: the tiles' candidates -> the location into best and the record (cell, pairs_in, score_q, score; the runner-up's
// fields 0), and per pair lag_p(cell*) and the signed C there (0 and 0.0 for a pair outside the range).  A largest score of 0:
// the zero record, zero lags and correlations, best = -1.
// pass 1 (partial now holds the runner-up's pass): runner_q, runner_up and runner_cell of a record that is not the zero
// record, where a cell outside the location's neighbourhood exists.
// roots[set] = sqrt(n_w).
// cdiff: the pairs' clock differences [set][pair], nullptr: none.
__global__ __launch_bounds__(kLocateThreads) void k_locate_finish(const long long *Q, LocateGeom g, const int32_t *table,
                                                                  const long long *cdiff, const double *roots,
                                                                  const ClosureCand *partial, int pass,
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
    if (pass == 1) {
        if (t == 0 && out[set].score_q != 0 && bs >= 0 && cell >= 0 && cell < g.n_cells) {
            out[set].runner_q = bs;
            out[set].runner_up = stack_value(bs, root);
            out[set].runner_cell = cell;
        }
        return;
    }
    const bool found = bs > 0 && cell >= 0 && cell < g.n_cells;
    const long long *q = Q + (size_t)set * g.P * g.n;
    int inside = 0;
    for (int p = t; p < g.P; p += kLocateThreads) {
        int32_t lag = 0;
        double c = 0.0;
        if (found && locate_pair_value(q, g, table, cdiff ? cdiff + (size_t)set * g.P : nullptr, cell, p, root, &lag, &c)) inside++;
        lags[(size_t)set * g.P + p] = lag;
        corr[(size_t)set * g.P + p] = c;
    }
    inside = search_wave_sum(inside);
    if ((t & (kWave - 1)) == 0) red_n[t / kWave] = inside;
    __syncthreads();
    if (t != 0) return;
    LocateOut rec{0, 0, 0, 0, 0, 0, 0.0, 0.0};
    if (found) {
        rec.cell = cell;
        for (int w = 0; w < kLocateThreads / kWave; w++) rec.pairs_in += red_n[w];
        rec.score_q = bs;
        rec.score = stack_value(bs, root);
    }
    best[set] = found ? cell : -1;
    out[set] = rec;
}

}  // namespace tdoa
