// stack_upsample.hpp -- tdoa_locate_set_upsample: the stacked surfaces Q on a lag grid of 1/U sample, U in {2, 4, 8, 16}, for
// the delay-table family (include/tdoa_mi355x.h, "sub-sample locate").  A row Q[l], 0 <= l < n, becomes n_U = (n - 1) U + 1
// words
//     Q_U[U l + r] = floor((sum over k = 0 .. 15 of h_r[k] Q[l + k - 7]  +  2^14) / 2^15)      r = 0 .. U - 1, Q outside the row = 0
// with h_r = kUpsampleTaps[r 16 / U]: 16 phases of a 16-tap Kaiser-windowed sinc (beta = 6) at scale 2^15, committed as
// literals -- nobody computes a tap at run time.  Phase 0 is the delta: Q_U[U l] = Q[l].
//
// The sum is exact.  |Q| reaches 2^60, so h Q does not fit 64 bits: Q = hi 2^31 + lo with lo the low 31 bits (>= 0) and hi the
// arithmetic shift (32 bits while |Q| < 2^62), A = sum h hi and B = sum h lo as 32 x 32 -> 64 multiply-adds, and the word is
// A 2^16 + ((B + 2^14) >> 15): 2^31 A + B is the sum, 2^15 divides 2^31 A, and |B| < 2.04 2^15 2^31 (kUpsampleTapsAbsMax).
//
// k_stack_upsample    one workgroup per (row, tile of 256 input lags): the tile's 256 + 15 words once into LDS, one input lag
//                     per thread with its 16-word window as hi / lo in registers, its U words phase-major into LDS, then the
//                     tile's 256 U words out with consecutive lanes on consecutive words.  (A row of n_U words starts 8 bytes
//                     off a 16-byte line in every other row -- n_U is odd -- so a lane's own run of U words could not go out as
//                     16-byte stores; through LDS every wave-instruction writes 512 contiguous bytes.)  The taps are
//                     compile-time literals of the unrolled loops: no vector register holds one.
// k_locate_scale_i32  out[i] = U in[i]: the delay table in units of 1/(16 U) sample, so that the family's lag rule
// k_locate_scale_i64  sgn(d) ((2 |d| + 16) div 32) on U d is the nearest 1/U lag; the same for the clock differences
#pragma once

#include "stack_locate.hpp"

namespace tdoa {

constexpr int kUpsampleThreads = 256;                           // input lags per tile
constexpr int kUpsampleTapCount = 16;
constexpr int kUpsamplePhases = 16;
constexpr int kUpsampleBefore = 7;                              // tap k of a window is the word at lag l + k - 7
constexpr int kUpsampleShift = 15;                              // the taps' scale
constexpr int kUpsampleSplit = 31;                              // Q = hi 2^31 + lo
constexpr int kUpsampleMax = 16;

// h16[rho][k] = rint(2^15 sinc(x) kaiser_6(x / 8)), x = k - 7 - rho / 16.  Normative: tdoa_amd/upsample.py holds the same 256
// literals.  The largest sum of magnitudes of a phase is 66828 = 2.039 2^15 (phases 7 and 9).
constexpr int32_t kUpsampleTaps[kUpsamplePhases][kUpsampleTapCount] = {
    {     0,      0,      0,      0,      0,      0,      0,  32768,      0,      0,      0,      0,      0,      0,      0,      0},
    {   -18,     52,   -119,    236,   -439,    820,  -1825,  32552,   2090,   -893,    473,   -256,    130,    -59,     21,     -4},
    {   -33,     97,   -223,    445,   -828,   1544,  -3360,  31911,   4414,  -1828,    964,   -522,    267,   -122,     45,    -10},
    {   -44,    133,   -308,    620,  -1158,   2151,  -4593,  30859,   6933,  -2773,   1454,   -788,    406,   -186,     70,    -16},
    {   -51,    159,   -374,    757,  -1419,   2629,  -5517,  29423,   9600,  -3692,   1923,  -1043,    540,   -250,     95,    -23},
    {   -55,    176,   -419,    855,  -1606,   2970,  -6136,  27636,  12362,  -4544,   2350,  -1275,    663,   -310,    120,    -30},
    {   -56,    184,   -444,    911,  -1717,   3172,  -6460,  25543,  15162,  -5291,   2714,  -1473,    769,   -363,    142,    -38},
    {   -54,    184,   -448,    928,  -1755,   3237,  -6510,  23192,  17942,  -5893,   2994,  -1625,    852,   -406,    162,    -45},
    {   -50,    176,   -435,    907,  -1722,   3174,  -6311,  20639,  20639,  -6311,   3174,  -1722,    907,   -435,    176,    -50},
    {   -45,    162,   -406,    852,  -1625,   2994,  -5893,  17942,  23192,  -6510,   3237,  -1755,    928,   -448,    184,    -54},
    {   -38,    142,   -363,    769,  -1473,   2714,  -5291,  15162,  25543,  -6460,   3172,  -1717,    911,   -444,    184,    -56},
    {   -30,    120,   -310,    663,  -1275,   2350,  -4544,  12362,  27636,  -6136,   2970,  -1606,    855,   -419,    176,    -55},
    {   -23,     95,   -250,    540,  -1043,   1923,  -3692,   9600,  29423,  -5517,   2629,  -1419,    757,   -374,    159,    -51},
    {   -16,     70,   -186,    406,   -788,   1454,  -2773,   6933,  30859,  -4593,   2151,  -1158,    620,   -308,    133,    -44},
    {   -10,     45,   -122,    267,   -522,    964,  -1828,   4414,  31911,  -3360,   1544,   -828,    445,   -223,     97,    -33},
    {    -4,     21,    -59,    130,   -256,    473,   -893,   2090,  32552,  -1825,    820,   -439,    236,   -119,     52,    -18},
};

constexpr long long upsample_taps_abs_max()
{
    long long worst = 0;
    for (int p = 0; p < kUpsamplePhases; p++) {
        long long s = 0;
        for (int k = 0; k < kUpsampleTapCount; k++) s += kUpsampleTaps[p][k] < 0 ? -(long long)kUpsampleTaps[p][k] : kUpsampleTaps[p][k];
        worst = s > worst ? s : worst;
    }
    return worst;
}
constexpr long long kUpsampleTapsAbsMax = upsample_taps_abs_max();
static_assert(kUpsampleTapsAbsMax <= (4ll << kUpsampleShift), "B = sum h lo stays below 2^48 and |Q_U| <= 4 |Q| + 1");
static_assert(kUpsampleTaps[0][kUpsampleBefore] == (1 << kUpsampleShift), "phase 0 is the delta");

constexpr bool upsample_factor_ok(int U) { return U == 1 || U == 2 || U == 4 || U == 8 || U == 16; }

// the words of an upsampled row of n lags
constexpr long long upsample_len(long long n, int U) { return (n - 1) * U + 1; }

// The phase-major staging rows are kUpsampleThreads + pad words long.  The tile's words go out in the row's order: lane i of a
// wave reads phase i mod U of input lag i div U, at 8-byte word (i mod U) (256 + pad) + i div U.  A half wave (ds_read_b64's
// lane group) covers U phases of 32 / U lags and the 64 banks once when pad (i mod U) + i div U takes 32 different values mod
// 32: pad = 32 / U.
constexpr int upsample_pad(int U) { return 32 / U; }

// grid (rows * tiles), kUpsampleThreads threads; block b works on row b div tiles, tile b mod tiles.  Q: [rows][n];
// out: [rows][n_U], every word written.
template <int U>
__global__ __launch_bounds__(kUpsampleThreads) void k_stack_upsample(const long long *__restrict__ Q, int n, int tiles,
                                                                     long long *__restrict__ out)
{
    constexpr int kSpan = kUpsampleThreads + kUpsampleTapCount - 1, kRow = kUpsampleThreads + upsample_pad(U);
    __shared__ long long in_s[kSpan];
    __shared__ long long out_s[U * kRow];
    const int t = threadIdx.x;
    const size_t row = blockIdx.x / (unsigned)tiles;
    const int l0 = (int)(blockIdx.x % (unsigned)tiles) * kUpsampleThreads;
    const long long *q = Q + row * (size_t)n;
    for (int i = t; i < kSpan; i += kUpsampleThreads) {
        const int l = l0 + i - kUpsampleBefore;
        in_s[i] = l >= 0 && l < n ? q[l] : 0;
    }
    __syncthreads();
    int32_t hi[kUpsampleTapCount], lo[kUpsampleTapCount];
#pragma unroll
    for (int k = 0; k < kUpsampleTapCount; k++) {
        const long long v = in_s[t + k];
        hi[k] = (int32_t)(v >> kUpsampleSplit);
        lo[k] = (int32_t)(v & ((1ll << kUpsampleSplit) - 1));
    }
    out_s[t] = in_s[t + kUpsampleBefore];                        // phase 0
#pragma unroll
    for (int r = 1; r < U; r++) {
        long long a = 0, b = 1ll << (kUpsampleShift - 1);
#pragma unroll
        for (int k = 0; k < kUpsampleTapCount; k++) {
            constexpr int kStep = kUpsamplePhases / U;
            const int32_t h = kUpsampleTaps[r * kStep][k];         // (a literal once both loops are unrolled)
            a += (long long)h * hi[k];
            b += (long long)h * lo[k];
        }
        out_s[r * kRow + t] = a * (1ll << (kUpsampleSplit - kUpsampleShift)) + (b >> kUpsampleShift);
    }
    __syncthreads();
    const long long n_u = upsample_len(n, U), w0 = (long long)l0 * U;
    long long *o = out + row * (size_t)n_u + w0;
#pragma unroll
    for (int i = 0; i < U; i++) {
        const int w = i * kUpsampleThreads + t;
        if (w0 + w < n_u) o[w] = out_s[(w % U) * kRow + w / U];
    }
}

// out[i] = U in[i], i < count
__global__ __launch_bounds__(256) void k_locate_scale_i32(const int32_t *__restrict__ in, int U, size_t count, int32_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = in[i] * U;
}
__global__ __launch_bounds__(256) void k_locate_scale_i64(const long long *__restrict__ in, int U, size_t count, long long *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = in[i] * U;
}

}  // namespace tdoa
