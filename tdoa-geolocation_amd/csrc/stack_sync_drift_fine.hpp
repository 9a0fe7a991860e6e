// stack_sync_drift_fine.hpp -- tdoa_process_sync_drift_fine: the clock lines' offsets and rates refined to 1/U sample, U in
// {2, 4, 8, 16} (include/tdoa_mi355x.h, "fine clock lines").  The clock-line search (stack_sync_drift.hpp) runs unchanged and
// leaves k_s and h_s in its buffers; the refinement moves kappa_s = U k_s + y_s and eta_s = U h_s + g_s, |y_s|, |g_s| <= U,
// station 0 the gauge, to raise
//     A^U_ij = sum over x of Q_U,x,ij[e^U_ij + kappa_j(x) - kappa_i(x)]      F_U = sum over the pairs of |A^U_ij|
// with kappa_s(x) = kappa_s + shift(eta_s, x) in 1/U sample, in Rf Gauss-Seidel sweeps over stations 1 .. S-1 against all the
// others.  Q_U is tdoa_locate_set_upsample's and is never materialised: every word is evaluated from the 16 words of Q under
// its taps (sync_fine_word, stack_sync_fine.hpp).  A station's candidates (g, y) compete in the order
// r = rank(g) (2U + 1) + rank(y), the first of equal maxima wins; a term outside the range adds 0.
//
// k_synclinefine_init    kappa = U k, eta = U h and the table cur [line][station][position] = kappa_s(x); `moved` = 0
// k_synclinefine_step    one station's step: grid (tiles of 256 candidates, lines), one candidate per lane, 16 gathers per
//                        term.  The taps go to LDS once (the phase differs per lane).  A tile touches at most 16 fine slopes: their
//                        shift(U h_s + g, x) is computed once per workgroup into LDS while the line is no longer than
//                        kSyncLineFineLdsL positions, and in place above that.  The partner loop is outside and the position
//                        loop inside, one int64 accumulator per partner whose magnitude is taken once; every lane owns its sum,
//                        so the order of work cannot change a byte.  The partners' kappa_i(x) come from cur and are the same for
//                        the whole workgroup.  The tile's best goes out as a two-word candidate, key = ~r
// k_synclinefine_commit  one workgroup per line: the tiles' candidates -> the station's (kappa, eta), its row of cur, `moved`
// k_syncline_finish      (stack_sync_drift.hpp) on SyncFineGrid with kappa, eta and the coarse records: F_U and terms_in; pass 0
//                        keeps F_U as start_q, pass 1 writes the record, clock16, the fine rates, rows, lags and correlations,
//                        all zero where the coarse record is zero or F_U = 0
//
// Integer work only; stack_value on the way out.  The word, its split, e^U and the 1/U grid are stack_sync_fine.hpp's, the
// commit's start (syncline_best) the clock lines', the candidate, its order and the workgroup reductions the ones all stack
// searches share (stack_closure.hpp).
#pragma once

#include "stack_sync_drift.hpp"
#include "stack_sync_fine.hpp"

namespace tdoa {

constexpr int kSyncLineFineThreads = kSyncLineThreads;
constexpr int kSyncLineFineLdsL = 128;                          // positions whose own shifts a step keeps in LDS
// fine slopes a tile of kSyncLineFineThreads candidates can touch: W = 2U + 1 candidates per slope and W slopes in all, a tile
// starts anywhere inside a slope
constexpr int synclinefine_tile_slopes(int U)
{
    return (kSyncLineFineThreads + 2 * U - 1) / (2 * U + 1) + 1 < 2 * U + 1 ? (kSyncLineFineThreads + 2 * U - 1) / (2 * U + 1) + 1 : 2 * U + 1;
}
constexpr int kSyncLineFineSlopes = 17;
static_assert(synclinefine_tile_slopes(2) <= kSyncLineFineSlopes && synclinefine_tile_slopes(4) <= kSyncLineFineSlopes &&
                  synclinefine_tile_slopes(8) <= kSyncLineFineSlopes && synclinefine_tile_slopes(16) <= kSyncLineFineSlopes,
              "the step's LDS table holds every slope of a tile");
static_assert(kSyncLineFineThreads == kUpsamplePhases * kUpsampleTapCount, "one thread stages one tap");

struct SyncLineFineGeom {
    int32_t S, P;              // stations, pairs
    int32_t n;                 // lags per row of Q
    int32_t L;                 // positions of a line
    int32_t U, log_u, W;       // the factor, log2 U, the offsets (and slopes) of a station: 2 U + 1
    int32_t D;                 // drift_den
    int32_t cands, tiles;      // W W, and ceil(cands / kSyncLineFineThreads)
};

// the buffers of a refinement; k, h and coarse are the clock-line search's and only read
struct SyncLineFineDev {
    const int32_t *in;         // ref_delay [kSyncMaxStations] (then centre, not read here)
    const long long *k;        // [line][S]
    const int32_t *h;          // [line][S]
    const SyncLineOut *coarse; // [line]
    long long *cur;            // kappa_s(x) at [(line * S + s) * L + x]
    long long *kappa, *eta;    // [line][S]
    ClosureCand *part;         // [line][tile]
    int32_t *moved;            // [line]
    long long *start_q;        // [line]
};

// the slope search's rule: sgn(h) ((2 |h| x + D) div (2 D))
__device__ __forceinline__ long long synclinefine_shift(long long h, long long x, long long D)
{
    const long long a = (2 * (h < 0 ? -h : h) * x + D) / (2 * D);
    return h < 0 ? -a : a;
}

// One workgroup per line.
__global__ __launch_bounds__(kSyncLineFineThreads) void k_synclinefine_init(SyncLineFineGeom g, SyncLineFineDev d)
{
    const int line = blockIdx.x, t = threadIdx.x;
    for (int e = t; e < g.S * g.L; e += kSyncLineFineThreads) {
        const int s = e / g.L, x = e - s * g.L;
        const size_t at = (size_t)line * g.S + s;
        d.cur[(size_t)line * g.S * g.L + e] = d.k[at] * g.U + synclinefine_shift((long long)d.h[at] * g.U, x, g.D);
    }
    if (t < g.S) {
        const size_t at = (size_t)line * g.S + t;
        d.kappa[at] = d.k[at] * g.U;
        d.eta[at] = (long long)d.h[at] * g.U;
    }
    if (t == 0) d.moved[line] = 0;
}

// grid (tiles, lines).  Q: [line][position][pair][n].  Station s against all the others.
// part[line * tiles + tile] = the tile's best candidate (equal sums: the smaller r).
__global__ __launch_bounds__(kSyncLineFineThreads) void k_synclinefine_step(const long long *Q, SyncLineFineGeom g, SyncLineFineDev d, int s)
{
    __shared__ long long red_s[kSyncLineFineThreads / kWave];
    __shared__ uint32_t red_k[kSyncLineFineThreads / kWave];
    __shared__ int32_t taps_s[kUpsamplePhases * kUpsampleTapCount];
    __shared__ long long own_s[kSyncLineFineSlopes * kSyncLineFineLdsL];
    const int line = blockIdx.y, t = threadIdx.x;
    const int r = (int)blockIdx.x * kSyncLineFineThreads + t;
    const size_t at_s = (size_t)line * g.S + s;
    const long long mid_k = d.k[at_s] * g.U, mid_h = (long long)d.h[at_s] * g.U;      // the window's centre: the coarse line
    const int rg0 = (int)blockIdx.x * kSyncLineFineThreads / g.W;                      // the tile's first slope
    const bool in_lds = g.L <= kSyncLineFineLdsL;
    taps_s[t] = kUpsampleTaps[t / kUpsampleTapCount][t % kUpsampleTapCount];
    if (in_lds)
        for (int e = t; e < min(kSyncLineFineSlopes, g.W - rg0) * g.L; e += kSyncLineFineThreads) {
            const int v = e / g.L, x = e - v * g.L;
            own_s[v * kSyncLineFineLdsL + x] = synclinefine_shift(mid_h + closure_unrank((uint32_t)(rg0 + v)), x, g.D);
        }
    __syncthreads();
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    if (r < g.cands) {
        const int rg = r / g.W;
        const long long kap = mid_k + closure_unrank((uint32_t)(r - rg * g.W)), eta = mid_h + closure_unrank((uint32_t)rg);
        const long long *own = own_s + (rg - rg0) * kSyncLineFineLdsL;
        const long long *q_line = Q + (size_t)line * g.L * g.P * g.n;
        const long long *cur_line = d.cur + (size_t)line * g.S * g.L;
        const size_t pos_stride = (size_t)g.P * g.n;
        const long long half = (long long)(g.n - 1) / 2 * g.U, top = (long long)(g.n - 1) * g.U;      // lam = u - half, 0 <= u <= top
        long long sum = 0;
        for (int i = 0; i < g.S; i++) {
            if (i == s) continue;
            // i < s: e_is + kappa_s(x) - kappa_i(x); i > s: e_si + kappa_i(x) - kappa_s(x)
            const bool below = i < s;
            const long long e = below ? sync_fine_lag(d.in[i], d.in[s], g.U) : sync_fine_lag(d.in[s], d.in[i], g.U);
            const long long *q = q_line + (size_t)(below ? closure_pair(i, s, g.S) : closure_pair(s, i, g.S)) * g.n;
            const long long *ki = cur_line + (size_t)i * g.L;
            long long acc = 0;
            for (int x = 0; x < g.L; x++) {
                const long long dk = kap + (in_lds ? own[x] : synclinefine_shift(eta, x, g.D)) - ki[x];
                const long long u = (below ? e + dk : e - dk) + half;
                if (u >= 0 && u <= top) acc += sync_fine_word(q + (size_t)x * pos_stride, g.n, u, g.log_u, taps_s);
            }
            sum += acc < 0 ? -acc : acc;
        }
        bs = sum;
        bk = ~(uint32_t)r;
    }
    closure_block_best(bs, bk, red_s, red_k);
    if (t == 0) d.part[(size_t)line * g.tiles + blockIdx.x] = ClosureCand{bs, bk, 0};
}

// One workgroup per line.  first: the step opens a sweep (the count starts again).
__global__ __launch_bounds__(kSyncLineFineThreads) void k_synclinefine_commit(SyncLineFineGeom g, SyncLineFineDev d, int s, int first)
{
    __shared__ long long red_s[kSyncLineFineThreads / kWave];
    __shared__ uint32_t red_k[kSyncLineFineThreads / kWave];
    const int line = blockIdx.x, t = threadIdx.x;
    uint32_t rg, ry;
    syncline_best(d.part + (size_t)line * g.tiles, g.tiles, g.cands, g.W, red_s, red_k, &rg, &ry);
    const size_t at = (size_t)line * g.S + s;
    const long long kap = d.k[at] * g.U + closure_unrank(ry);
    const long long eta = (long long)d.h[at] * g.U + closure_unrank(rg);
    for (int x = t; x < g.L; x += kSyncLineFineThreads) d.cur[at * g.L + x] = kap + synclinefine_shift(eta, x, g.D);
    if (t == 0) {
        const int changed = d.kappa[at] != kap || d.eta[at] != eta;
        d.kappa[at] = kap;
        d.eta[at] = eta;
        d.moved[line] = (first ? 0 : d.moved[line]) + changed;
    }
}

}  // namespace tdoa
