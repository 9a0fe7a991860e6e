// peak_select.hpp -- what a pair-window's correlation surface holds beyond its argmax (tdoa_process_peaks,
// tdoa_process_lags): the K strongest separate peaks, and the surfaces themselves in the caller's layout.
//
// The surfaces are the lag arrays the K5 kernels dump while they search (lag d of the batch's pair-window i at
// dump[i * stride + d - lag_lo]): raw, unscaled values, bit for bit the floats the peak keys were built from (one step
// offers a value to the key and writes it to the surface: k5_offer, peak_key.hpp).
//
// Selection rule (include/tdoa_mi355x.h, tdoa_process_peaks):
//   peak 1 is tdoa_process's peak, decoded from the same key;
//   each next peak is the largest |c[l]| over the lags l that are a local maximum of |c| (|c[l]| >= |c[l-1]| and
//   |c[l]| >= |c[l+1]|, a neighbour outside the range counting as smaller), lie more than min_sep lags from every peak
//   already chosen, and hold neither NaN nor 0; ties go to the smaller |lag|, then to the positive lag -- the order of
//   peak_key, so one 64-bit maximum decides a round.
//
// One workgroup per pair-window.  Thread t owns the lags t, t + T, t + 2T, ... and keeps the best key among its own
// candidates that no chosen peak suppresses.  A round takes the workgroup's maximum; only the threads whose best lies
// within min_sep of the new peak scan their lags again (removing other elements from a set does not change its
// maximum), so a step reads each surface once plus a few strided rescans per round.
#pragma once

#include "device_common.hpp"
#include "fft_stockham.hpp"
#include "peak_key.hpp"

namespace tdoa {

constexpr int kSelThreads = 512;
constexpr int kSelMaxK = 16;             // tdoa_process_peaks: k in 1 .. kSelMaxK

// key of index l of an n-lag surface when l is a candidate, else 0 (NaN and 0 never are; a NaN neighbour fails the
// comparison, so its neighbours are not local maxima either)
__device__ __forceinline__ unsigned long long sel_candidate(const float *c, int l, int n, int lag_lo)
{
    const float v = c[l], a = fabsf(v);
    if (!(a > 0.0f)) return 0ull;
    if (l > 0 && !(a >= fabsf(c[l - 1]))) return 0ull;
    if (l + 1 < n && !(a >= fabsf(c[l + 1]))) return 0ull;
    return peak_key(v, l + lag_lo);
}

// grid (n_pw), kSelThreads threads.  surf + i * stride: pair-window i's n raw values, lag lag_lo + l at l.
// pw: the pair-windows' slots (nullptr: slot i).  keys (nullptr: peak 1 from the surface like the others): the K5 keys
// of the slots.  Record r of slot s at out[s * k + r], scaled like k_decode_peaks: raw x scales[s] (x slot_gain[s] on
// the single-look path), sign kept.  Unused records are zero; count[s] = records written.
__global__ __launch_bounds__(kSelThreads) void k_select_peaks(const float *surf, size_t stride, int n, int lag_lo,
                                                              const PWDesc *pw, const unsigned long long *keys,
                                                              const double *scales, const double *slot_gain, int k,
                                                              int min_sep, PeakOut *out, int32_t *count)
{
    __shared__ unsigned long long red[kSelThreads / kWave];
    __shared__ int chosen[kSelMaxK];
    const int t = threadIdx.x;
    const int slot = pw ? pw[blockIdx.x].out_index : (int)blockIdx.x;
    const float *c = surf + (size_t)blockIdx.x * stride;
    unsigned long long best = 0;
    for (int l = t; l < n; l += kSelThreads) {
        const unsigned long long q = sel_candidate(c, l, n, lag_lo);
        best = q > best ? q : best;
    }
    int got = 0;
    for (int r = 0; r < k; r++) {
        unsigned long long b;
        if (r == 0 && keys) {
            b = keys[slot];
        } else {
            const unsigned long long w = wave_max_u64(best);
            if ((t & (kWave - 1)) == 0) red[t / kWave] = w;
            __syncthreads();
            b = red[0];
            for (int j = 1; j < kSelThreads / kWave; j++) b = red[j] > b ? red[j] : b;
            __syncthreads();                 // red is written again next round
        }
        if (!key_live(b)) break;                             // no key, or |c| = 0 everywhere: nothing qualifies
        const int lag = key_lag(b);
        if (t == 0) {
            out[(size_t)slot * k + r] = decode_peak(b, scales[slot], slot_gain ? slot_gain + slot : nullptr);
            chosen[r] = lag;
        }
        got = r + 1;
        if (got == k) break;
        __syncthreads();                     // chosen[r]
        if (best && abs(key_lag(best) - lag) <= min_sep) {
            best = 0;
            for (int l = t; l < n; l += kSelThreads) {
                const int d = l + lag_lo;
                bool near = false;
                for (int j = 0; j <= r; j++) near |= abs(d - chosen[j]) <= min_sep;
                if (near) continue;
                const unsigned long long q = sel_candidate(c, l, n, lag_lo);
                best = q > best ? q : best;
            }
        }
    }
    if (t == 0) {
        for (int r = got; r < k; r++) out[(size_t)slot * k + r] = PeakOut{0, 0.0f, 0.0};
        count[slot] = got;
    }
}

// the surfaces of a step in the caller's layout out[slot][n]: raw x scales[slot] (x slot_gain[slot] on the single-look
// path), the reference's scale, rounded once to float.  grid (n_pw, ceil(n / 1024)), 256 threads.
__global__ __launch_bounds__(256) void k_surface_out(const float *surf, size_t stride, int n, const PWDesc *pw,
                                                     const double *scales, const double *slot_gain, float *out)
{
    const int slot = pw[blockIdx.x].out_index;
    const float *c = surf + (size_t)blockIdx.x * stride;
    float *o = out + (size_t)slot * n;
    const double s = scales[slot], g = slot_gain ? slot_gain[slot] : 1.0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int l = blockIdx.y * 1024 + u * 256 + threadIdx.x;
        if (l < n) o[l] = slot_gain ? (float)((double)c[l] * s * g) : (float)((double)c[l] * s);
    }
}

}  // namespace tdoa
