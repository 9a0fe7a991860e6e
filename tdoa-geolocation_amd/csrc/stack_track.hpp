// stack_track.hpp -- tdoa_process_track: one lag per window of a stack, consecutive lags at most J apart, chosen so that the
// sum of the windows' fixed-point values along the track is largest (include/tdoa_mi355x.h, "delay tracks").  Dynamic
// programming over the surfaces the step already has, from the stack's last window back to its first, both polarities
// side by side:
//     T_j[l] = s q_j[l] + max over |d| <= J, l + d inside the range, of T_{j+1}[l + d]        D_j[l] = that d
//
// k_track_step    one launch per window position j (the stacks' last positions start the recurrence): T_{j+1} -> T_j, D_j
// k_track_finish  T_0 -> the polarity, L_0, the walk along D (lags, values), the score, total and the float surface
//
// Everything is integer arithmetic on the q words of stack_surfaces.hpp; the only floating point is stack_term on the way
// in and stack_value on the way out.
#pragma once

#include "stack_surfaces.hpp"

namespace tdoa {

constexpr int kTrackThreads = 256;
constexpr int kTrackLags = 4;                                   // lags per thread
constexpr int kTrackTile = kTrackLags * kTrackThreads;          // lags per workgroup
constexpr int kTrackMaxStep = 64;                               // the largest J: the halo on each side of a tile
constexpr long long kTrackAbsent = (long long)0x8000000000000000ull;   // a lag outside the range: never the strict maximum

// T of one lag: the best sum over the tracks that start there, for the polarity +1 and for -1
struct alignas(16) TrackPair {
    long long plus, minus;
};

// where the stack-pairs' windows are: pos[stack-pair * mm + j] = the pair-window (row of surf) at position j, -1 past the
// end of a shorter stack; n_w[stack-pair] = its windows
struct TrackTable {
    const int32_t *pos;
    const int32_t *n_w;
    int32_t mm;
};

// grid (n_stacks * P, ceil(n / kTrackTile)), kTrackThreads threads, one launch per position j = mm - 1 .. 0.
// The workgroup owns the lags l0 .. l0 + kTrackTile - 1 of one stack-pair at position j.  It stages T_{j+1} of those lags and
// of J more on each side in LDS, the two polarities in two arrays (consecutive lanes read consecutive 8-byte words), a lag
// outside 0 .. n - 1 as kTrackAbsent; reads its window's row once; scans d = 0, +1, -1, +2, -2, ... with a strict >, which
// is the tie rule (the smaller |d|, then the positive d; d = 0 is always inside the range, so an absent lag never wins);
// writes T_j to t_out and D_j[l] as two bytes (polarity +1, -1).  A stack's last position (j = n_w - 1) starts the
// recurrence: T_j = s q_j, nothing staged, no D.  A position beyond a shorter stack returns at once and touches nothing.
// t_in / t_out: [stack-pair][n] TrackPair, the two halves of a ping-pong; D: [stack-pair][mm][n][2] int8.
__global__ __launch_bounds__(kTrackThreads) void k_track_step(const float *surf, size_t stride, int n, const PWDesc *pw,
                                                              const double *scales, const double *slot_gain, TrackTable tab,
                                                              int j, int J, const TrackPair *t_in, TrackPair *t_out,
                                                              signed char *D)
{
    __shared__ long long st_p[kTrackTile + 2 * kTrackMaxStep], st_m[kTrackTile + 2 * kTrackMaxStep];
    const int sp = blockIdx.x;
    const int i = tab.pos[(size_t)sp * tab.mm + j];
    if (i < 0) return;                       // (the same for every thread of the workgroup)
    const bool last = j == tab.n_w[sp] - 1;
    const int t = threadIdx.x, l0 = (int)blockIdx.y * kTrackTile;
    if (!last) {
        const TrackPair *src = t_in + (size_t)sp * n;
        for (int e = t; e < kTrackTile + 2 * J; e += kTrackThreads) {
            const int x = l0 - J + e;
            TrackPair v{kTrackAbsent, kTrackAbsent};
            if (x >= 0 && x < n) v = src[x];
            st_p[e] = v.plus;
            st_m[e] = v.minus;
        }
        __syncthreads();
    }
    const int slot = pw[i].out_index;
    const double s = scales[slot], g = slot_gain ? slot_gain[slot] : 1.0;
    const float *row = surf + (size_t)i * stride;
    TrackPair *dst = t_out + (size_t)sp * n;
    signed char *d_out = D + ((size_t)sp * tab.mm + j) * (size_t)n * 2;
#pragma unroll
    for (int u = 0; u < kTrackLags; u++) {
        const int e0 = u * kTrackThreads + t, l = l0 + e0;
        if (l >= n) continue;
        const long long q = stack_term(row[l], s, g, slot_gain != nullptr);
        long long bp = 0, bm = 0;
        int dp = 0, dm = 0;
        if (!last) {
            const long long *wp = st_p + e0 + J, *wm = st_m + e0 + J;
            bp = wp[0];
            bm = wm[0];
            for (int k = 1; k <= J; k++) {
                long long c = wp[k];
                if (c > bp) { bp = c; dp = k; }
                c = wp[-k];
                if (c > bp) { bp = c; dp = -k; }
                c = wm[k];
                if (c > bm) { bm = c; dm = k; }
                c = wm[-k];
                if (c > bm) { bm = c; dm = -k; }
            }
            *reinterpret_cast<char2 *>(d_out + (size_t)l * 2) = make_char2((signed char)dp, (signed char)dm);
        }
        dst[l] = TrackPair{q + bp, bm - q};
    }
}

// the workgroup's maximum of v in every thread; red: WAVES words of LDS, free again on return
template <int WAVES>
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long *red)
{
    v = wave_max_u64(v);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    unsigned long long r = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; w++) r = red[w] > r ? red[w] : r;
    __syncthreads();
    return r;
}

// int64 <-> a word whose unsigned order is the signed order
__device__ __forceinline__ unsigned long long track_biased(long long v) { return (unsigned long long)v ^ 0x8000000000000000ull; }

// One workgroup per stack-pair.  t0: T_0 [stack-pair][n].  max T_0 of both polarities, as integers; the polarity with the
// larger one (a tie: +1); L_0 = the lag of that maximum, equal maxima by the order of a peak_key's lag field (the smaller
// |l|, then the positive l).  Thread 0 walks L_{j+1} = L_j + D_j[L_j] and writes lags[j] and values[j] = q_j[L_j] 2^-32, q
// from the window's raw surface row; positions past the stack's end, and every position when max T_0 = 0, hold 0.
// score: lag L_0, corr = stack_value(s max T_0), abs_corr its float magnitude (max T_0 = 0: the zero record).
// total[l] = s T_0[l], out[l] = (float)stack_value(total[l]).
__global__ __launch_bounds__(kTrackThreads) void k_track_finish(const TrackPair *t0, const signed char *D, const float *surf,
                                                                size_t stride, int n, int lag_lo, int n_pairs, const PWDesc *pw,
                                                                const double *scales, const double *slot_gain,
                                                                const double *roots, TrackTable tab, PeakOut *score,
                                                                int32_t *lags, double *values, long long *total, float *out)
{
    __shared__ unsigned long long red[kTrackThreads / kWave];
    const int sp = blockIdx.x, t = threadIdx.x;
    const TrackPair *T = t0 + (size_t)sp * n;
    unsigned long long bp = 0, bm = 0;       // (biased: 0 is below every value)
    for (int l = t; l < n; l += kTrackThreads) {
        const TrackPair v = T[l];
        const unsigned long long p = track_biased(v.plus), m = track_biased(v.minus);
        bp = p > bp ? p : bp;
        bm = m > bm ? m : bm;
    }
    bp = block_max_u64<kTrackThreads / kWave>(bp, red);
    bm = block_max_u64<kTrackThreads / kWave>(bm, red);
    const bool neg = bm > bp;
    const long long top = (long long)track_biased(neg ? bm : bp);
    const double root = roots[sp / n_pairs];
    long long *tot = total + (size_t)sp * n;
    float *o = out + (size_t)sp * n;
    unsigned long long key = 0;
    for (int l = t; l < n; l += kTrackThreads) {
        const TrackPair v = T[l];
        const long long mine = neg ? v.minus : v.plus, signed_sum = neg ? -mine : mine;
        tot[l] = signed_sum;
        o[l] = (float)stack_value(signed_sum, root);
        if (mine == top) {
            const unsigned long long k = peak_key(1.0f, l + lag_lo);
            key = k > key ? k : key;
        }
    }
    key = block_max_u64<kTrackThreads / kWave>(key, red);
    const int n_w = tab.n_w[sp];
    int32_t *lg = lags + (size_t)sp * tab.mm;
    double *vl = values + (size_t)sp * tab.mm;
    const bool none = top == 0;
    for (int j = t; j < tab.mm; j += kTrackThreads)
        if (none || j >= n_w) {
            lg[j] = 0;
            vl[j] = 0.0;
        }
    if (t != 0) return;
    PeakOut rec{0, 0.0f, 0.0};
    if (!none) {
        rec.lag = key_lag(key);
        rec.corr = stack_value(neg ? -top : top, root);
        rec.abs_corr = (float)fabs(rec.corr);
        int l = rec.lag - lag_lo;
        for (int j = 0; j < n_w; j++) {
            const int i = tab.pos[(size_t)sp * tab.mm + j];
            const int slot = pw[i].out_index;
            const double s = scales[slot], g = slot_gain ? slot_gain[slot] : 1.0;
            lg[j] = l + lag_lo;
            vl[j] = (double)stack_term(surf[(size_t)i * stride + l], s, g, slot_gain != nullptr) * (1.0 / 4294967296.0);
            if (j + 1 < n_w) l += D[(((size_t)sp * tab.mm + j) * (size_t)n + l) * 2 + (neg ? 1 : 0)];
        }
    }
    score[sp] = rec;
}

}  // namespace tdoa
