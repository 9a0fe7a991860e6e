// stack_surfaces.hpp -- tdoa_process_stacked: the correlation surfaces of a run of windows of one block added lag by lag,
// one peak set per (stack, pair) instead of one per pair-window (include/tdoa_mi355x.h, "stacked correlation").
//
// The sum is carried in fixed point: every surface value on the reference's scale, (double)raw * scale (* slot_gain) -- the
// expression of k_surface_out before its rounding to float --, becomes q = llrint(c * 2^32), and the stack is the int64 sum
// Q of its windows' q.  Integer addition is associative, so Q does not depend on the launch grouping, on which rank owned
// which window, or on the order a host adds the ranks' partial sums in; C = (double)Q * 2^-32 / sqrt(n_w) is derived from
// Q in one place (stack_value).  |c| <= sqrt(window_len) <= 2^13 and a few thousand windows stay far inside int64.
//
// k_stack_accumulate  surf rows of the owned pair-windows -> Q        (streaming: each surface value read once)
// k_stack_finish      Q -> (float)C in the caller's layout + the K5 key of the maximum per stack-pair
// k_select_peaks      (peak_select.hpp) on the float stack surfaces, unit scales, peak 1 from that key
// k_stack_fine        the records' corr as the double C[lag], and the parabola of peak 1 from C[d-1], C[d], C[d+1]
#pragma once

#include "device_common.hpp"
#include "fft_stockham.hpp"
#include "peak_key.hpp"
#include "peak_select.hpp"

namespace tdoa {

constexpr int kStackThreads = 256;
constexpr int kStackTile = 4 * kStackThreads;        // lags per workgroup: four consecutive lags per thread

struct StackDesc {         // one (stack, pair): its owned pair-windows are list[first .. first + count)
    int32_t first;
    int32_t count;
};

// 2^32 x the reference-scale value, rounded to nearest even: one term of Q
__device__ __forceinline__ long long stack_term(float raw, double s, double g, bool gain)
{
    const double c = gain ? (double)raw * s * g : (double)raw * s;
    return llrint(c * 4294967296.0);
}

// C[l] of a stack of n_w windows; root = sqrt(n_w), rounded on the host
__device__ __forceinline__ double stack_value(long long q, double root) { return (double)q * (1.0 / 4294967296.0) / root; }

// every row of a stack read at its own lags: the plain stack
struct NoShear {
    static constexpr bool shear = false;
    __device__ __forceinline__ int operator()(int) const { return 0; }
};

// The body of k_stack_accumulate and of k_stack_accumulate_sheared (stack_drift.hpp): the rows of stack-pair d added into
// the four lags l0 .. l0 + 3 of a thread, acc[u] += q of row r at lag l0 + u + shift(slot of r).  Without a shear (NoShear)
// a row whose four lags start on a 16-byte boundary is read as float4, the others and the last lags of a row as single
// floats of the same 16 bytes; with one (Shift::shear) every lag is read alone and a lag outside the row adds 0.
template <class Shift>
__device__ __forceinline__ void stack_accumulate_rows(const float *surf, size_t stride, int n, const PWDesc *pw, const StackDesc d,
                                                      const int32_t *list, const double *scales, const double *slot_gain,
                                                      int l0, const Shift shift, long long acc[4])
{
    const bool whole = l0 + 3 < n;
#pragma unroll 2
    for (int r = 0; r < d.count; r++) {
        const int i = list[d.first + r];
        const int slot = pw[i].out_index;
        const double s = scales[slot], g = slot_gain ? slot_gain[slot] : 1.0;
        const size_t off = (size_t)i * stride + (size_t)l0;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (Shift::shear) {
            const int sh = shift(slot);
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (l0 + u < n && l0 + u + sh >= 0 && l0 + u + sh < n) v[u] = surf[(size_t)i * stride + (size_t)(l0 + u + sh)];
        } else if (whole && (off & 3) == 0) {
            const float4 x = *reinterpret_cast<const float4 *>(surf + off);
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (l0 + u < n) v[u] = surf[off + u];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) acc[u] += stack_term(v[u], s, g, slot_gain != nullptr);
    }
}

// grid (n_stacks * P, ceil(n / kStackTile)), kStackThreads threads.  surf + i * stride: the n raw values of the rank's
// pair-window i (the K5 kernels' dump); list: pair-window numbers grouped by stack-pair, desc[stack-pair] its run.
// Thread t of tile y owns the lags 4 (y * 256 + t) .. + 3 in registers for every row.  n is odd, so only every fourth row
// starts on a 16-byte boundary (surf itself does).  Q[stack-pair][l] is written for every l, zero where the rank owns no
// window.
__global__ __launch_bounds__(kStackThreads) void k_stack_accumulate(const float *surf, size_t stride, int n, const PWDesc *pw,
                                                                   const StackDesc *desc, const int32_t *list,
                                                                   const double *scales, const double *slot_gain,
                                                                   long long *Q)
{
    const int l0 = 4 * ((int)blockIdx.y * kStackThreads + (int)threadIdx.x);
    if (l0 >= n) return;
    long long acc[4] = {0, 0, 0, 0};
    stack_accumulate_rows(surf, stride, n, pw, desc[blockIdx.x], list, scales, slot_gain, l0, NoShear{}, acc);
    long long *q = Q + (size_t)blockIdx.x * n + l0;
#pragma unroll
    for (int u = 0; u < 4; u++)
        if (l0 + u < n) q[u] = acc[u];
}

// grid (n_stacks * P, ceil(n / kStackTile)), kStackThreads threads.  out[stack-pair][l] = (float)C[l]; keys[stack-pair]
// (zeroed before) = the largest peak_key of those floats, NaN left out: the key k_decode_peaks and k_select_peaks decode.
// roots[stack] = sqrt(n_w).
__global__ __launch_bounds__(kStackThreads) void k_stack_finish(const long long *Q, int n, int lag_lo, int n_pairs,
                                                               const double *roots, float *out, unsigned long long *keys)
{
    __shared__ unsigned long long red[kStackThreads / kWave];
    const double root = roots[blockIdx.x / n_pairs];
    const long long *q = Q + (size_t)blockIdx.x * n;
    float *o = out + (size_t)blockIdx.x * n;
    unsigned long long best = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int l = (int)blockIdx.y * kStackTile + u * kStackThreads + (int)threadIdx.x;
        if (l < n) {
            const float v = (float)stack_value(q[l], root);
            o[l] = v;
            k5_max(best, v, l + lag_lo);
        }
    }
    const int32_t slot = blockIdx.x;
    k5_commit<kStackThreads / kWave>(best, red, &slot, keys);
}

// One thread per stack-pair.  The records k_select_peaks wrote carry (float)C as corr: corr becomes the double C[lag]
// (abs_corr, its float magnitude, is the same number either way).  fine (may be nullptr): the parabola and gate of
// k_decode_fine on y_q = s C[d - 1 + q], s = sign(C[d]), d the lag of peak 1; a neighbour outside the searched range is
// reported as 0 and leaves frac at 0.
__global__ void k_stack_fine(const long long *Q, int n, int lag_lo, int n_pairs, int n_sp, const double *roots,
                             const unsigned long long *keys, int k, PeakOut *peaks, const int32_t *count, FineOut *fine,
                             double gate)
{
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_sp) return;
    const double root = roots[id / n_pairs];
    const long long *q = Q + (size_t)id * n;
    if (peaks) {
        const int got = count[id];
        for (int r = 0; r < got; r++) {
            PeakOut p = peaks[(size_t)id * k + r];
            p.corr = stack_value(q[p.lag - lag_lo], root);
            p.abs_corr = (float)fabs(p.corr);
            peaks[(size_t)id * k + r] = p;
        }
    }
    if (!fine) return;
    FineOut f;
    f.delay = 0.0;
    f.frac = 0.0f;
    f.y[0] = f.y[1] = f.y[2] = 0.0f;
    f.reserved = 0;
    const unsigned long long key = keys[id];
    if (key_live(key)) {
        const int lag = key_lag(key), l = lag - lag_lo;
        const double y0r = stack_value(q[l], root);
        const double sg = y0r < 0.0 ? -1.0 : 1.0;
        const bool inside = l > 0 && l + 1 < n;
        const double ym = l > 0 ? sg * stack_value(q[l - 1], root) : 0.0, y0 = sg * y0r,
                     yp = l + 1 < n ? sg * stack_value(q[l + 1], root) : 0.0;
        const double den = ym - 2.0 * y0 + yp;
        double fr = 0.0;
        if (inside && den < 0.0) {
            fr = 0.5 * (ym - yp) / den;
            fr = fr > 0.5 ? 0.5 : (fr < -0.5 ? -0.5 : fr);
        }
        f.frac = (float)fr;
        f.delay = (double)lag + fr;
        f.y[0] = (float)ym; f.y[1] = (float)y0; f.y[2] = (float)yp;
    }
    f.plausible = fabs(f.delay) <= gate ? 1 : 0;
    fine[id] = f;
}

}  // namespace tdoa
