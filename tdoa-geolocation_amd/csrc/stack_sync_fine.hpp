// stack_sync_fine.hpp -- tdoa_process_sync_fine: the clock search's clocks refined to 1/U sample, U in {2, 4, 8, 16}
// (include/tdoa_mi355x.h, "fine clock search").  The whole-lag search (stack_sync.hpp) runs unchanged and leaves k_s in its
// clock buffer; the refinement moves kappa_s = U k_s + y_s, |y_s| <= U, y_0 = 0, in units of 1/U sample, to raise
//     F_U(kappa) = sum over the pairs (i, j) of M_ij(e^U_ij + kappa_j - kappa_i)     M_p(lam) = |Q_U,p[lam + (max_lag - 1) U]|
// in Rf Gauss-Seidel sweeps over stations 1 .. S-1 against all the others.  Q_U is tdoa_locate_set_upsample's (stack_upsample.hpp)
// and is never materialised: a sweep's step reads (2U + 1)(S - 1) of its words, the objective P, and each is evaluated from
// the 16 words of Q under its taps.  e^U_ij = sgn(d) ((2 |d| U + 16) div 32) is the upsampled locate's lag rule; candidates
// compete in the order rank(y) (closure_rank, stack_closure.hpp), the first of equal maxima wins; a lag outside the range counts 0.
//
// k_sync_refine  one workgroup per set, behind k_sync_steps on the same stream.  The taps go to LDS once (the phase differs per
//                lane).  A step's 2U + 1 candidates of one partner are consecutive fine lags, inside three input lags: the
//                16 + 2 words under them are loaded once per partner and kept as hi / lo in LDS (9 KB for 64 stations), then
//                every (partner, candidate) gets a lane -- (2U + 1)(S - 1) items, up to 33 x 63, strided over the 256 threads
//                -- which reads its 16-word window and its phase's taps from LDS and adds the word's magnitude to the
//                candidate's word in LDS as an integer, so the order cannot change a byte.  Lanes 0 .. 2U then compete on
//                key = ~rank(y).  The objective and the outputs are the clock search's (sync_objective, sync_finish_set) on the
//                1/U grid SyncFineGrid: the pairs strided, one word formed from Q per pair.
//
// The arithmetic is k_stack_upsample's: Q = hi 2^31 + lo, A = sum h hi and B = sum h lo + 2^14 as 32 x 32 -> 64 multiply-adds,
// the word A 2^16 + (B >> 15); phase 0 is the delta and gives Q back.  It is stated here once more (upsample_word) so that
// k_stack_upsample's code, whose taps are literals, stays what it is.  Integer work only; stack_value on the way out.
#pragma once

#include "stack_sync.hpp"
#include "stack_upsample.hpp"

namespace tdoa {

constexpr int kSyncFineMaxRounds = 16;
constexpr int kSyncFineSpan = kUpsampleTapCount + 2;            // the words under the 2U + 1 candidates of one partner
constexpr int kSyncFineMaxCand = 2 * kUpsampleMax + 1;
constexpr long long kSyncFineMaxCentre = 1ll << 27;             // |centre| + G + 1 below it: 16 kappa / U fits int32

constexpr bool sync_fine_factor_ok(int U) { return U == 2 || U == 4 || U == 8 || U == 16; }

// the word of phase h (16 taps in LDS) over the window w[0 .. 15] given as hi / lo
__device__ __forceinline__ long long upsample_word(const int32_t *h, const int32_t *hi, const int32_t *lo)
{
    long long a = 0, b = 1ll << (kUpsampleShift - 1);
#pragma unroll
    for (int k = 0; k < kUpsampleTapCount; k++) {
        const int32_t hk = h[k];
        a += (long long)hk * hi[k];
        b += (long long)hk * lo[k];
    }
    return a * (1ll << (kUpsampleSplit - kUpsampleShift)) + (b >> kUpsampleShift);
}

__device__ __forceinline__ void upsample_split(long long v, int32_t *hi, int32_t *lo)
{
    *hi = (int32_t)(v >> kUpsampleSplit);
    *lo = (int32_t)(v & ((1ll << kUpsampleSplit) - 1));
}

// Q_U[u] of a row of n lags, any u inside 0 .. (n - 1) U; words outside the row count 0.  log_u = log2 U
__device__ __forceinline__ long long sync_fine_word(const long long *q, int n, long long u, int log_u, const int32_t *taps_s)
{
    const int l = (int)(u >> log_u), r = (int)(u & ((1 << log_u) - 1));
    int32_t hi[kUpsampleTapCount], lo[kUpsampleTapCount];
#pragma unroll
    for (int k = 0; k < kUpsampleTapCount; k++) {
        const int x = l + k - kUpsampleBefore;
        upsample_split(x >= 0 && x < n ? q[x] : 0, &hi[k], &lo[k]);
    }
    return upsample_word(taps_s + (r << (4 - log_u)) * kUpsampleTapCount, hi, lo);
}

// e^U_ij: the nearest 1/U lag to (tj - ti) / 16, halves away from zero
__device__ __forceinline__ long long sync_fine_lag(int32_t ti, int32_t tj, int U)
{
    const long long d = (long long)tj - (long long)ti;
    const long long a = (2 * (d < 0 ? -d : d) * U + kLocateDelayUnit) / (2 * kLocateDelayUnit);
    return d < 0 ? -a : a;
}

// The 1/U lag grid (SyncGrid, stack_sync.hpp, is the whole-lag one): lags in 1/U sample, a row's word formed from the 16 words
// of Q under its taps, clocks out in 1/16 sample (clock16).  taps: the kUpsamplePhases phases' taps in LDS -- a kernel that reads
// them elsewhere too stages them itself and builds the grid on them, any other calls stage().
struct SyncFineGrid {
    int32_t n, U, log_u;       // lags per row of Q, the factor, log2 U
    const int32_t *taps;
    __device__ __forceinline__ long long lag(int32_t ti, int32_t tj) const { return sync_fine_lag(ti, tj, U); }
    __device__ __forceinline__ bool word(const long long *row, long long lam, long long *v) const
    {
        const long long u = lam + (long long)(n - 1) / 2 * U;        // lam = u - half, 0 <= u <= top
        if (u < 0 || u > (long long)(n - 1) * U) return false;
        *v = sync_fine_word(row, n, u, log_u, taps);
        return true;
    }
    __device__ __forceinline__ int unit16() const { return kLocateDelayUnit / U; }
    __device__ __forceinline__ int clock_unit() const { return kLocateDelayUnit / U; }
    // kSyncThreads threads, one tap each; ends with the barrier that makes them readable
    __device__ __forceinline__ void stage()
    {
        __shared__ int32_t taps_s[kUpsamplePhases * kUpsampleTapCount];
        taps_s[threadIdx.x] = kUpsampleTaps[threadIdx.x / kUpsampleTapCount][threadIdx.x % kUpsampleTapCount];
        __syncthreads();
        taps = taps_s;
    }
};
static_assert(kSyncThreads == kUpsamplePhases * kUpsampleTapCount, "one thread stages one tap");

// One workgroup per set, kSyncThreads threads, after k_sync_steps.  coarse [set] and k [set][S]: that kernel's records and
// clocks.  out [set]; clock16 [set][S]: kappa_s 16 / U; lags [set][P] in 1/U sample and corr [set][P]: e^U_ij + kappa_j - kappa_i
// and the signed value of the word there, 0 and 0.0 for a pair outside.  A zero coarse record or F_U = 0 at the end: all zero.
__global__ __launch_bounds__(kSyncThreads) void k_sync_refine(const long long *Q, SyncGeom g, int U, int rounds, const int32_t *in,
                                                              const double *roots, const SyncOut *coarse, const int32_t *k,
                                                              SyncOut *out, int32_t *clock16, int32_t *lags, double *corr)
{
    __shared__ long long red_s[kSyncThreads / kWave];
    __shared__ uint32_t red_k[kSyncThreads / kWave];
    __shared__ int red_n[kSyncThreads / kWave];
    __shared__ int32_t taps_s[kUpsamplePhases * kUpsampleTapCount];
    __shared__ unsigned long long sum_s[kSyncFineMaxCand];      // by y + U
    __shared__ long long kap[kSyncMaxStations], mid[kSyncMaxStations];
    __shared__ int32_t ref[kSyncMaxStations];
    __shared__ long long u0_s[kSyncMaxStations];                // a step's first candidate per partner, as an index of Q_U
    __shared__ int32_t win_hi[kSyncMaxStations * kSyncFineSpan], win_lo[kSyncMaxStations * kSyncFineSpan];
    const int set = blockIdx.x, t = threadIdx.x;
    const int log_u = 31 - __clz(U);
    const long long *q = Q + (size_t)set * g.P * g.n;
    const long long half = (long long)(g.n - 1) / 2 * U, top = (long long)(g.n - 1) * U;      // lam = u - half, 0 <= u <= top
    const bool found = coarse[set].score_q != 0;                 // (the same in every thread)
    taps_s[t] = kUpsampleTaps[t / kUpsampleTapCount][t % kUpsampleTapCount];
    if (t < g.S) {
        ref[t] = in[t];
        mid[t] = (long long)k[(size_t)set * g.S + t] * U;
        kap[t] = mid[t];
    }
    __syncthreads();

    // station s against all its partners: the new kappa_s, the same in every thread; kap[s] is written and visible on return
    const auto step = [&](int s) -> long long {
        if (t < kSyncFineMaxCand) sum_s[t] = 0;
        // lam(y) = base + y for a partner before s, base - y for one after: u = u0 .. u0 + 2U either way
        if (t < g.S && t != s) {
            const long long base = t < s ? sync_fine_lag(ref[t], ref[s], U) + mid[s] - kap[t] : sync_fine_lag(ref[s], ref[t], U) + kap[t] - mid[s];
            u0_s[t] = base - U + half;
        }
        __syncthreads();
        // the 16 + 2 words under a partner's candidates, once, as hi / lo
        for (int w = t; w < g.S * kSyncFineSpan; w += kSyncThreads) {
            const int i = w / kSyncFineSpan, x = w % kSyncFineSpan;
            if (i == s) continue;
            const long long *row = q + (size_t)(i < s ? closure_pair(i, s, g.S) : closure_pair(s, i, g.S)) * g.n;
            const long long l = (u0_s[i] >> log_u) + x - kUpsampleBefore;
            upsample_split(l >= 0 && l < g.n ? row[l] : 0, &win_hi[w], &win_lo[w]);
        }
        __syncthreads();
        // one (partner, candidate) per lane: its window and its phase's taps from LDS
        for (int it = t; it < g.S * (2 * U + 1); it += kSyncThreads) {
            const int i = it / (2 * U + 1), c = it % (2 * U + 1);
            if (i == s) continue;
            const long long u0 = u0_s[i], u = u0 + c;
            if (u < 0 || u > top) continue;
            const int at = i * kSyncFineSpan + (int)((u >> log_u) - (u0 >> log_u)), r = (int)(u & (U - 1));
            const long long v = upsample_word(taps_s + (r << (4 - log_u)) * kUpsampleTapCount, win_hi + at, win_lo + at);
            atomicAdd(&sum_s[i < s ? c : 2 * U - c], (unsigned long long)(v < 0 ? -v : v));
        }
        __syncthreads();
        long long bs = kClosureAbsent;
        uint32_t bk = 0;
        if (t <= 2 * U) {
            bs = (long long)sum_s[closure_unrank((uint32_t)t) + U];
            bk = ~(uint32_t)t;
        }
        closure_block_best(bs, bk, red_s, red_k);                // (its barriers lie between these reads and the next step's writes)
        const long long ks = mid[s] + closure_unrank(~bk);
        if (t == 0) kap[s] = ks;
        __syncthreads();
        return ks;
    };

    // F_U(kappa) and the pairs inside the range, the same in every thread; with `write` the pairs' lags and correlations
    const double root = roots[set];
    const SyncFineGrid gr{g.n, U, log_u, taps_s};
    int32_t *set_lags = lags + (size_t)set * g.P;
    double *set_corr = corr + (size_t)set * g.P;
    const auto objective = [&](bool write, int *pairs_in) -> long long {
        return sync_objective(gr, q, g.S, g.P, ref, kap, root, write, set_lags, set_corr, red_s, red_n, pairs_in);
    };

    int inside = 0, moved = 0;
    long long start_q = 0, score_q = 0;
    if (found) {
        start_q = objective(false, &inside);
        for (int r = 0; r < rounds; r++) {
            moved = 0;
            for (int s = 1; s < g.S; s++) {
                const long long old = kap[s];                    // (read before the step's first barrier; t == 0 writes after it)
                moved += step(s) != old;
            }
        }
        score_q = objective(true, &inside);
    }
    sync_finish_set(gr, g.S, g.P, kap, SyncOut{moved, inside, score_q, start_q, stack_value(score_q, root)}, set_lags, set_corr,
                    clock16 + (size_t)set * g.S, out + set);
}

}  // namespace tdoa
