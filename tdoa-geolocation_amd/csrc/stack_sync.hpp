// stack_sync.hpp -- tdoa_process_sync: the stations' clock offsets from a block whose emitter is known
// (include/tdoa_mi355x.h, "clock search").  ref_delay fixes the lag e_ij each pair would have from propagation alone; what is
// left of a pair's peak is k_j - k_i, the stations' clocks k_s = centre[s] + x_s, |x_s| <= G, x_0 = 0, and
//     F(k) = sum over the pairs (i, j) of M_ij[e_ij + k_j - k_i]        M_p[l] = |Q_p[l]|, a lag outside the range counts 0
// is searched in three phases: (x_1, x_2) jointly over the whole square, stations 3 .. S-1 placed one after the other against
// the stations before them, then R Gauss-Seidel sweeps over stations 1 .. S-1 against all the others.  Candidates compete in
// the closure search's order, rank(x) = 0, 1, 2, 3, 4 ... for x = 0, +1, -1, +2, -2 ...: the first of equal maxima wins.
//
// k_sync_start   the (2G+1)^2 cells of the joint start, one cell per lane in rank order (cell = rank(x_1) (2G+1) + rank(x_2)),
//                three gathers of Q per cell; the tile's best out as a two-word candidate (key = ~cell).  S >= 3 only
// k_sync_steps   one workgroup per set: the tiles' candidates -> (x_1, x_2) (S = 2: x_1 placed against station 0), the placing
//                and the sweeps one step after the other with k in LDS -- lanes stride over the 2G+1 candidates of the step's
//                station, one gather per partner -- then F, the record, the clocks and the pairs' lags and correlations
//
// Everything is integer arithmetic on the Q words of stack_surfaces.hpp; the only floating point is stack_value on the way
// out.  The candidate, its order and the workgroup reductions (a workgroup's best, the best of the tiles' candidates, the sum
// of F with its count) are the ones all stack searches share (stack_closure.hpp); the rule of e_ij and the pair order are the
// delay-table search's (stack_locate.hpp).  The clock family shares what is stated here: the lag grid (SyncGrid; the 1/U form is
// SyncFineGrid in stack_sync_fine.hpp), the pair objective over it (sync_objective) and the per-set outputs (sync_finish_set).
#pragma once

#include "stack_locate.hpp"

namespace tdoa {

constexpr int kSyncThreads = 256;                               // cells per tile of the start, threads of a step
constexpr int kSyncMaxGate = kClosureMaxGate;
constexpr int kSyncMaxRounds = 16;
constexpr int kSyncMaxStations = kLocateMaxStations;
static_assert(kSyncThreads == kClosureThreads, "closure_block_best reduces kClosureThreads candidates");

// tdoa_sync
struct SyncOut {
    int32_t moved, pairs_in;
    long long score_q, start_q;
    double score;
};

struct SyncGeom {
    int32_t S, P;              // stations, pairs
    int32_t n, lag_lo;         // lags per row of Q, the first one
    int32_t G, R;              // gate, rounds
    int32_t W;                 // candidates of a station: 2 G + 1
    int32_t tiles;             // of the start: ceil(W^2 / kSyncThreads), 0 with two stations
};

// M_p at a lag, 0 outside the searched range
__device__ __forceinline__ long long sync_m(const long long *q, long long lag, const SyncGeom &g)
{
    const long long idx = lag - g.lag_lo;
    if (idx < 0 || idx >= g.n) return 0;
    const long long v = q[idx];
    return v < 0 ? -v : v;
}

// A lag grid is what the clock family's kernels are written over: the lag of a pair from ref_delay, the word of a row at a lag
// (false outside the searched range) and the factors that turn the grid's unit into 1/16 sample (unit16) and into the unit the
// clocks go out in (clock_unit).  This is the whole-lag grid; SyncFineGrid (stack_sync_fine.hpp) is the 1/U one.
struct SyncGrid {
    int32_t n, lag_lo;         // lags per row of Q, the first one
    __device__ __forceinline__ long long lag(int32_t ti, int32_t tj) const { return locate_lag(ti, tj); }
    __device__ __forceinline__ bool word(const long long *row, long long lag, long long *v) const
    {
        const long long idx = lag - lag_lo;
        if (idx < 0 || idx >= n) return false;
        *v = row[idx];
        return true;
    }
    __device__ __forceinline__ int unit16() const { return kLocateDelayUnit; }
    __device__ __forceinline__ int clock_unit() const { return 1; }      // tdoa_sync's clocks are whole lags
    __device__ __forceinline__ void stage() const {}                     // nothing to keep in LDS
};

// F at the clocks k [S] (in LDS, in the grid's unit) and the pairs inside the range, the same in every thread; with `write` the
// pairs' lags and correlations.  q: the set's rows [P][n]; lags and corr: the set's [P].  kSyncThreads threads; ends with a barrier.
template <class Grid>
__device__ __forceinline__ long long sync_objective(const Grid &gr, const long long *q, int S, int P, const int32_t *ref, const long long *k,
                                                    double root, bool write, int32_t *lags, double *corr, long long *red_s, int *red_n,
                                                    int *pairs_in)
{
    long long f = 0;
    int inside = 0;
    for (int p = threadIdx.x; p < P; p += kSyncThreads) {
        int i, j;
        locate_pair(p, S, &i, &j);
        const long long l = gr.lag(ref[i], ref[j]) + k[j] - k[i];
        long long v;
        int32_t lag = 0;
        double c = 0.0;
        if (gr.word(q + (size_t)p * gr.n, l, &v)) {
            f += v < 0 ? -v : v;
            inside++;
            lag = (int32_t)l;
            c = stack_value(v, root);
        }
        if (write) {
            lags[p] = lag;
            corr[p] = c;
        }
    }
    search_block_sum(f, inside, red_s, red_n);
    *pairs_in = inside;
    return f;
}

// The end of a per-set kernel, behind sync_objective with `write`: the set's clocks k [S] in the grid's clock unit and its record.
// rec.score_q == 0 (nothing found): all zero, every thread taking back the pairs it wrote (sync_objective's stride).
template <class Grid>
__device__ __forceinline__ void sync_finish_set(const Grid &gr, int S, int P, const long long *k, const SyncOut &rec, int32_t *lags,
                                                double *corr, int32_t *clock, SyncOut *out)
{
    const int t = threadIdx.x;
    if (rec.score_q == 0) {
        for (int p = t; p < P; p += kSyncThreads) {
            lags[p] = 0;
            corr[p] = 0.0;
        }
        if (t < S) clock[t] = 0;
        if (t == 0) *out = SyncOut{0, 0, 0, 0, 0.0};
        return;
    }
    if (t < S) clock[t] = (int32_t)(k[t] * gr.clock_unit());
    if (t == 0) *out = rec;
}

// grid (tiles, n_sets), kSyncThreads threads; S >= 3.  Q: [set][pair][n]; in: ref_delay [kSyncMaxStations], then centre
// [kSyncMaxStations].  partial[set * tiles + tile] = the tile's best cell (equal scores: the smaller cell, which is the smaller
// rank(x_1), then the smaller rank(x_2)).
__global__ __launch_bounds__(kSyncThreads) void k_sync_start(const long long *Q, SyncGeom g, const int32_t *in, ClosureCand *partial)
{
    __shared__ long long red_s[kSyncThreads / kWave];
    __shared__ uint32_t red_k[kSyncThreads / kWave];
    const int set = blockIdx.y, t = threadIdx.x;
    const long long cell = (long long)blockIdx.x * kSyncThreads + t;
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    if (cell < (long long)g.W * g.W) {
        const int32_t *centre = in + kSyncMaxStations;
        const long long *q01 = Q + (size_t)set * g.P * g.n, *q02 = q01 + g.n, *q12 = q01 + (size_t)(g.S - 1) * g.n;
        const long long k0 = centre[0], k1 = (long long)centre[1] + closure_unrank((uint32_t)(cell / g.W)),
                        k2 = (long long)centre[2] + closure_unrank((uint32_t)(cell % g.W));
        bs = sync_m(q01, locate_lag(in[0], in[1]) + k1 - k0, g) + sync_m(q02, locate_lag(in[0], in[2]) + k2 - k0, g) +
             sync_m(q12, locate_lag(in[1], in[2]) + k2 - k1, g);
        bk = ~(uint32_t)cell;
    }
    closure_block_best(bs, bk, red_s, red_k);
    if (t == 0) partial[(size_t)set * g.tiles + blockIdx.x] = ClosureCand{bs, bk, 0};
}

// One workgroup per set, kSyncThreads threads.  roots[set] = sqrt(n_w).  out [set]; clock [set][S]: k_s; lags and corr
// [set][P]: e_ij + k_j - k_i and the signed C there, 0 and 0.0 for a pair outside the range.  F = 0 at the final k: all zero.
__global__ __launch_bounds__(kSyncThreads) void k_sync_steps(const long long *Q, SyncGeom g, const int32_t *in, const double *roots,
                                                             const ClosureCand *partial, SyncOut *out, int32_t *clock, int32_t *lags,
                                                             double *corr)
{
    __shared__ long long red_s[kSyncThreads / kWave];
    __shared__ uint32_t red_k[kSyncThreads / kWave];
    __shared__ int red_n[kSyncThreads / kWave];
    __shared__ long long k[kSyncMaxStations];
    __shared__ int32_t ref[kSyncMaxStations], centre[kSyncMaxStations];
    const int set = blockIdx.x, t = threadIdx.x;
    const long long *q = Q + (size_t)set * g.P * g.n;
    if (t < g.S) {
        ref[t] = in[t];
        centre[t] = in[kSyncMaxStations + t];
        k[t] = in[kSyncMaxStations + t];                         // x_0 = 0: station 0 is the gauge
    }
    __syncthreads();

    // station s against the partners i < hi, i != s: the new k_s, the same in every thread; k[s] is written and visible on return
    const auto step = [&](int s, int hi) -> long long {
        long long bs = kClosureAbsent;
        uint32_t bk = 0;
        for (int r = t; r < g.W; r += kSyncThreads) {
            const long long ks = (long long)centre[s] + closure_unrank((uint32_t)r);
            long long sum = 0;
            for (int i = 0; i < hi; i++) {
                if (i == s) continue;
                if (i < s)
                    sum += sync_m(q + (size_t)closure_pair(i, s, g.S) * g.n, locate_lag(ref[i], ref[s]) + ks - k[i], g);
                else
                    sum += sync_m(q + (size_t)closure_pair(s, i, g.S) * g.n, locate_lag(ref[s], ref[i]) + k[i] - ks, g);
            }
            const uint32_t key = ~(uint32_t)r;
            if (closure_better(sum, key, bs, bk)) {
                bs = sum;
                bk = key;
            }
        }
        closure_block_best(bs, bk, red_s, red_k);                // (every thread has read k: the reduction's barriers lie between)
        const long long ks = (long long)centre[s] + closure_unrank(~bk);
        if (t == 0) k[s] = ks;
        __syncthreads();
        return ks;
    };

    // F(k) and the pairs inside the range, the same in every thread; with `write` the pairs' lags and correlations
    const double root = roots[set];
    const SyncGrid gr{g.n, g.lag_lo};
    int32_t *set_lags = lags + (size_t)set * g.P;
    double *set_corr = corr + (size_t)set * g.P;
    const auto objective = [&](bool write, int *pairs_in) -> long long {
        return sync_objective(gr, q, g.S, g.P, ref, k, root, write, set_lags, set_corr, red_s, red_n, pairs_in);
    };

    if (g.S == 2) {
        step(1, 1);
    } else {
        long long bs;
        uint32_t bk;
        search_best_candidate(partial + (size_t)set * g.tiles, g.tiles, red_s, red_k, bs, bk);
        const uint32_t cell = ~bk;                               // < W^2: every tile holds a cell
        if (t == 0) {
            k[1] = (long long)centre[1] + closure_unrank(cell / (uint32_t)g.W);
            k[2] = (long long)centre[2] + closure_unrank(cell % (uint32_t)g.W);
        }
        __syncthreads();
        for (int s = 3; s < g.S; s++) step(s, s);
    }
    int inside = 0, moved = 0;
    const long long start_q = objective(false, &inside);
    for (int r = 0; r < g.R; r++) {
        moved = 0;
        for (int s = 1; s < g.S; s++) {
            const long long old = k[s];                          // (read before the step's first barrier; t == 0 writes after it)
            moved += step(s, g.S) != old;
        }
    }
    const long long score_q = objective(true, &inside);
    sync_finish_set(gr, g.S, g.P, k, SyncOut{moved, inside, score_q, start_q, stack_value(score_q, root)}, set_lags, set_corr,
                    clock + (size_t)set * g.S, out + set);
}

}  // namespace tdoa
