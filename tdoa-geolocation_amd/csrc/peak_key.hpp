// peak_key.hpp -- the 64-bit peak key and K5, the "pick the peak" tail of every inverse, in one place.
//
// key -> : peak_key builds it, key_live / key_lag / key_value / decode_peak take it apart; nothing else knows the layout.
// K5     : a kernel offers each of its values with k5_offer (lag filter, NaN left out, key maximum, surface dump) and ends
//          with k5_commit (wave maximum, LDS, one atomicMax per workgroup).  The dumped surface is therefore bit for bit
//          the floats the keys were built from, in every kernel (peak_select.hpp relies on it).
#pragma once

#include "device_common.hpp"

namespace tdoa {

struct PeakOut {      // mirrors tdoa_peak
    int32_t lag;
    float abs_corr;
    double corr;
};

// 64-bit peak key: [ |v| bits : 32 ][ (0x7fffffff - rank) : 31 ][ sign : 1 ]
// rank orders lags 0, +1, -1, +2, -2, ... so the larger key is the larger |v|,
// then the smaller |lag|, then the positive lag (processor.go:596-611 order).  rank <= 2 |lag| has 31 bits:
// |lag| <= 2^30 - 1 (every search range is far inside; tdoa_debug_select_peaks refuses a surface that is not).
__device__ __forceinline__ unsigned long long peak_key(float v, int lag)
{
    unsigned int mag = __float_as_uint(fabsf(v));
    unsigned int a = lag < 0 ? (unsigned int)(-lag) : (unsigned int)lag;
    unsigned int rank = 2u * a - (lag > 0 ? 1u : 0u);
    unsigned int low = ((0x7fffffffu - rank) << 1) | (v < 0.0f ? 1u : 0u);
    return ((unsigned long long)mag << 32) | low;
}

// a key that holds a peak: some candidate entered it, and not with |v| = 0
__device__ __forceinline__ bool key_live(unsigned long long k) { return k != 0 && (unsigned int)(k >> 32) != 0; }

// the lag of a peak_key
__device__ __forceinline__ int key_lag(unsigned long long k)
{
    const unsigned int rank = 0x7fffffffu - ((unsigned int)k >> 1);
    return rank == 0 ? 0 : ((rank & 1u) ? (int)((rank + 1u) >> 1) : -(int)(rank >> 1));
}

// the sign of the value behind a peak_key
__device__ __forceinline__ bool key_negative(unsigned long long k) { return ((unsigned int)k & 1u) != 0; }

// the value of a peak_key on the caller's scale: |v| x scale (x *gain, the single-look path's slot gain; nullptr: none),
// then the sign
__device__ __forceinline__ double key_value(unsigned long long k, double scale, const double *gain = nullptr)
{
    double v = (double)__uint_as_float((unsigned int)(k >> 32)) * scale;
    if (gain) v *= *gain;
    return key_negative(k) ? -v : v;
}

// key -> record; a key that is not live gives the zero record
__device__ __forceinline__ PeakOut decode_peak(unsigned long long k, double scale, const double *gain)
{
    PeakOut p{0, 0.0f, 0.0};
    if (key_live(k)) {
        p.lag = key_lag(k);
        p.corr = key_value(k, scale, gain);
        p.abs_corr = (float)fabs(p.corr);
    }
    return p;
}

// ---------------------------------------------------------------------------
// K5
// ---------------------------------------------------------------------------
// v at `lag` against the thread's best key; NaN never enters
__device__ __forceinline__ void k5_max(unsigned long long &best, float v, int lag)
{
    if (v == v) {
        const unsigned long long k = peak_key(v, lag);
        best = k > best ? k : best;
    }
}

// one value of an inverse: inside [lag_lo, lag_hi] it is a candidate and goes to the lag surface (lag_dump: the
// pair-window's row, lag lag_lo first; nullptr: no surface wanted)
template <typename L>
__device__ __forceinline__ void k5_offer(unsigned long long &best, float v, L lag, int lag_lo, int lag_hi, float *lag_dump,
                                         float dump_scale)
{
    if (lag >= lag_lo && lag <= lag_hi) {
        k5_max(best, v, (int)lag);
        if (lag_dump) lag_dump[lag - lag_lo] = v * dump_scale;
    }
}

// the workgroup's (WAVES waves) maximum into keys[*slot] (zeroed before the step); red: WAVES words of LDS.  Only thread 0
// reads *slot.  Every thread of the workgroup must call it.
template <int WAVES>
__device__ __forceinline__ void k5_commit(unsigned long long best, unsigned long long *red, const int32_t *slot,
                                          unsigned long long *keys)
{
    best = wave_max_u64(best);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long bb = red[0];
#pragma unroll
        for (int w = 1; w < WAVES; w++) bb = red[w] > bb ? red[w] : bb;
        if (bb) atomicMax(&keys[*slot], bb);
    }
}

// refinement neighbours c[lag-1], c[lag], c[lag+1] of a slot's peak from the lag array a K5 kernel left behind:
// lags[li] = c[li - zero_index], li < n_lags, unscaled like the keys; a neighbour outside the array is reported as 0
__device__ __forceinline__ void refine_from_lag_array(const float *lags, int n_lags, int zero_index, unsigned long long k,
                                                      float *raw3)
{
    float r[3] = {0.0f, 0.0f, 0.0f};
    if (key_live(k)) {
        const int lag = key_lag(k);
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int li = lag - 1 + q + zero_index;
            r[q] = li >= 0 && li < n_lags ? lags[li] : 0.0f;
        }
    }
#pragma unroll
    for (int q = 0; q < 3; q++) raw3[q] = r[q];
}

}  // namespace tdoa
