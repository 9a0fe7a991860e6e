// stack_drift.hpp -- tdoa_process_stacked_drift: the stack taken along a lag slope, searched over 2H+1 slopes per
// (stack, pair) (include/tdoa_mi355x.h, "drift-compensated stacking").  Shift-and-add, the structure of incoherent
// dedispersion: hypothesis h reads window j of a stack at the lag offset shift(h, j), the nearest integer to h j / D.
//
// k_stack_shear_search        surf rows -> the K5 key of the maximum of (float)C_h per (stack-pair, hypothesis)
// k_stack_pick_drift          those keys -> h* per stack-pair and the decoded profile
// k_stack_accumulate_sheared  k_stack_accumulate with every window read at the shift of its stack-pair's h* -> Q_{h*}
// then launch_stack_finish (stacked_api.inc) as it is.
//
// The shifts come from one table the host computes, tab[(h + H) * mm + j] (mm: the stack length): integers only, one place.
#pragma once

#include "stack_surfaces.hpp"

namespace tdoa {

constexpr int kShearLags = 4;                                   // lags per thread
constexpr int kShearTile = kShearLags * kStackThreads;          // lags per workgroup (= kStackTile)
constexpr int kShearHyp = 8;                                    // most hypotheses per workgroup
// LDS budget of the staged span, in q words: 32 KB, so that five workgroups share a CU's 160 KB and the loads of one hide
// behind the adds of another (one window is staged at a time, two barriers per window)
constexpr int kShearSpan = 4096;
constexpr int kShearSpread = kShearSpan - kShearTile;           // the widest spread of a block's shifts that still fits

// what the three kernels share of the search's geometry
struct ShearGeom {
    int32_t H, mm, wpb, P;                   // hypotheses -H .. H, stack length, windows per block, pairs
};

// position of the pair-window with this out_index in its stack
__device__ __forceinline__ int stack_position(int out_index, const ShearGeom &g) { return ((out_index / g.P) % g.wpb) % g.mm; }

// grid (n_stacks * P, ceil(n / kShearTile), ceil((2H+1) / HB)), kStackThreads threads.  The workgroup owns the lags
// l0 = y * kShearTile .. + kShearTile - 1 of one stack-pair and the hypotheses h_lo = -H + z * HB .. h_hi.  Per window j it
// stages q of the lags l0 + shift(h_lo, j) .. l0 + kShearTile - 1 + shift(h_hi, j) in LDS (shift grows with h; a lag
// outside the searched range is staged as 0), each value converted once; thread t then adds, for every hypothesis, the
// words at t + 256 u + shift(h, j) - shift(h_lo, j): consecutive lanes read consecutive 8-byte words.  The host picks HB so
// that the spread shift(h_hi, j) - shift(h_lo, j) stays within kShearSpread for every j (HB = 1: no spread at all).
// keys[stack-pair][2H+1] (zeroed before) takes the largest peak_key of (float)C_h, one atomicMax per hypothesis.
template <int HB>
__global__ __launch_bounds__(kStackThreads) void k_stack_shear_search(const float *surf, size_t stride, int n, int lag_lo,
                                                                     const PWDesc *pw, const StackDesc *desc, const int32_t *list,
                                                                     const double *scales, const double *slot_gain,
                                                                     const double *roots, const int32_t *tab, ShearGeom g,
                                                                     unsigned long long *keys)
{
    __shared__ long long stage[kShearSpan];
    __shared__ unsigned long long red[HB][kStackThreads / kWave];
    const StackDesc d = desc[blockIdx.x];
    const int t = threadIdx.x, l0 = (int)blockIdx.y * kShearTile;
    const int n_hyp = 2 * g.H + 1, z0 = (int)blockIdx.z * HB;              // hypothesis index h + H of the block's first
    const int n_here = min(HB, n_hyp - z0);
    long long acc[HB][kShearLags];
#pragma unroll
    for (int b = 0; b < HB; b++)
#pragma unroll
        for (int u = 0; u < kShearLags; u++) acc[b][u] = 0;
    for (int r = 0; r < d.count; r++) {
        const int i = list[d.first + r];
        const int slot = pw[i].out_index;
        const int j = stack_position(slot, g);
        const double s = scales[slot], gn = slot_gain ? slot_gain[slot] : 1.0;
        int sh[HB];                          // (a hypothesis past the block's last repeats it: read, never committed)
#pragma unroll
        for (int b = 0; b < HB; b++) sh[b] = tab[(size_t)(z0 + min(b, n_here - 1)) * g.mm + j];
        const int span = kShearTile + sh[HB - 1] - sh[0];
        const float *row = surf + (size_t)i * stride;
        __syncthreads();                     // the previous window's words have been read
        for (int e = t; e < span; e += kStackThreads) {
            const int x = l0 + sh[0] + e;
            stage[e] = x >= 0 && x < n ? stack_term(row[x], s, gn, slot_gain != nullptr) : 0;
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < HB; b++) {
            const long long *w = stage + (sh[b] - sh[0]) + t;
#pragma unroll
            for (int u = 0; u < kShearLags; u++) acc[b][u] += w[u * kStackThreads];
        }
    }
    const double root = roots[blockIdx.x / g.P];
#pragma unroll
    for (int b = 0; b < HB; b++) {
        if (b >= n_here) break;              // (the same for every thread of the workgroup)
        unsigned long long best = 0;
#pragma unroll
        for (int u = 0; u < kShearLags; u++) {
            const int l = l0 + u * kStackThreads + t;
            if (l < n) k5_max(best, (float)stack_value(acc[b][u], root), l + lag_lo);
        }
        const int32_t slot = (int32_t)blockIdx.x * n_hyp + z0 + b;
        k5_commit<kStackThreads / kWave>(best, red[b], &slot, keys);
    }
}

// One wave per stack-pair: h* = the hypothesis with the largest abs_corr, ties to the smaller |h|, then the positive h (the
// order of a peak_key with h in the place of the lag; the peaks' lags take no part); no live key: 0.
// profile[stack-pair][h + H] = the key decoded at unit scale.
__global__ __launch_bounds__(kWave) void k_stack_pick_drift(const unsigned long long *keys, int H, int32_t *drift, PeakOut *profile)
{
    const int n_hyp = 2 * H + 1;
    const unsigned long long *k = keys + (size_t)blockIdx.x * n_hyp;
    PeakOut *prof = profile + (size_t)blockIdx.x * n_hyp;
    unsigned long long best = 0;
    for (int idx = threadIdx.x; idx < n_hyp; idx += kWave) {
        const unsigned long long key = k[idx];
        prof[idx] = decode_peak(key, 1.0, nullptr);
        if (key_live(key)) {
            const unsigned long long c = peak_key(__uint_as_float((unsigned int)(key >> 32)), idx - H);
            best = c > best ? c : best;
        }
    }
    best = wave_max_u64(best);
    if (threadIdx.x == 0) drift[blockIdx.x] = best ? key_lag(best) : 0;
}

// the shift of a row of stack-pair's chosen hypothesis: shifts = the table's row of h*
struct ShearOf {
    static constexpr bool shear = true;
    const int32_t *shifts;
    ShearGeom g;
    __device__ __forceinline__ int operator()(int slot) const { return shifts[stack_position(slot, g)]; }
};

// grid and layout of k_stack_accumulate; drift[stack-pair] = h*.  Q[stack-pair][l] = Q_{h*}[l].
__global__ __launch_bounds__(kStackThreads) void k_stack_accumulate_sheared(const float *surf, size_t stride, int n, const PWDesc *pw,
                                                                           const StackDesc *desc, const int32_t *list,
                                                                           const double *scales, const double *slot_gain,
                                                                           const int32_t *tab, const int32_t *drift, ShearGeom g,
                                                                           long long *Q)
{
    const int l0 = 4 * ((int)blockIdx.y * kStackThreads + (int)threadIdx.x);
    if (l0 >= n) return;
    long long acc[4] = {0, 0, 0, 0};
    stack_accumulate_rows(surf, stride, n, pw, desc[blockIdx.x], list, scales, slot_gain, l0,
                          ShearOf{tab + (size_t)(drift[blockIdx.x] + g.H) * g.mm, g}, acc);
    long long *q = Q + (size_t)blockIdx.x * n + l0;
#pragma unroll
    for (int u = 0; u < 4; u++)
        if (l0 + u < n) q[u] = acc[u];
}

}  // namespace tdoa
