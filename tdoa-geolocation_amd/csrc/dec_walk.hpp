// dec_walk.hpp -- the COLUMN WALK of the decimated pair step, once: K3 + the 16:1 decimating FIR of fft_radix8.hpp
// (k_pair_decimate16's filter, same taps, same outputs) with one thread per spectrum column.  k_pair_decimate_cols
// (dec_stream.hpp: a row's operands from memory, taps from LDS) and k_pair_decimate_staged (dec_staged.hpp: operands from
// an LDS ring, taps through the scalar cache) both walk with what is here.
//
// Consecutive bins k = k2 + N2 k1 run down the columns of the [k2][k1] spectrum, so G[j] = sum_t h[t] Q[16 j + t] is a
// stencil DOWN the columns.  k_pair_decimate16 gathers 4096 consecutive bins (16 or 8 columns) into an LDS image and
// runs the FIR there with per-lane taps; on the 4096 x 4096 plan (ten-second windows, BASELINE config 3) such a tile is
// one column -- 8-byte pieces of 4096 rows -- and the plan had no decimated inverse at all.  Here a thread owns a column
// and walks its rows; what a wave reads is contiguous along k1 like every other row pass, and there is no LDS image, no
// quad sums:
//   * The forward row pass leaves the UNPACKED spectra U (the station's half of K3, k_fwd_row4096_unpack<true>) in place,
//     row-major.  K3's other half needs U[k] and U[Nc - k] of both stations, (k2, k1) and (N2 - k2, 4095 - k1): one pair of
//     loads per station yields Q[k] AND Q[Nc - k] (pair_u_pk).  Thread k1 < 2048 therefore walks column k1 downwards
//     (rows 0 .. N2 - 1) and, with the same values, column km = 4095 - k1 upwards (rows N2 - 1 .. 1); the two rows 0 pair
//     inside row 0 and are evaluated on their own, before and after the loop.  Every bin is evaluated exactly once.
//   * A row r = 16 g + p feeds the kDecSteps outputs i = g + C - s with the tap of (phase p, step s): the same twelve numbers
//     for every lane (the tile kernel's lanes differ in the phase).  Twelve accumulators per walk in registers, shifted by
//     one every 16 rows.  By the filter's symmetry the upward walk uses the same twelve taps as the downward one:
//       downward walk: row (g, p) -> output g + C - s in at[s], tap (p, s).
//       upward walk: row N2 - 16 g - p of column km.  p > 0: phase 16 - p of its group gb = NG - 1 - g; slot u holds output
//       gb - (C - 1) + u, step S - 1 - u, and tap(16 - p, S - 1 - u) = h[-(16 (u - C) + p)] = tap(p, u): the SAME twelve.
//       p = 0: phase 0 of group NG - g, the last row of that group: tap(0, S - 1 - u) -- the REVERSED row of phase 0 -- then
//       the group's finished output NG - g + C leaves and the slots move up.
//   * Output i (0 .. N2/16 - 1) of column c is G[(N2/16) c + i], stored as the small plan's row i: coalesced.  The six
//     outputs next to either end of a column also need bins of the neighbouring column; a walk leaves what ITS bins add to
//     them in X[pw][12][4096] (slot 6 + i': output i' = 0..5 of the NEXT column; slot i' + 6, i' = -6..-1: output N2/16 + i'
//     of the PREVIOUS one) and k_inv_rows_plain_r8 adds slot rows of the neighbouring columns when it loads G -- coalesced
//     like G itself.  No thread ever waits for another.
//   * The phase of a row is a RUN-TIME value: a kernel's loop is not unrolled over a group's 16 phases -- unrolled, every
//     form of the tap fetch (scalar loads, LDS reads) was hoisted to the top of the group by the compiler and the 192
//     values spilled, SGPRs into vector lanes (880 v_readlane / v_writelane per group), VGPRs into scratch.
#pragma once

#include <utility>

#include "fft_radix8.hpp"

namespace tdoa {

constexpr int kDecShareRows = 2 * kDecEdge;            // X: rows per pair-window (each 4096 columns)

// The walk's register stencil is written for 8 or 12 steps per phase (whole float4 of taps): a measurement build
// with another filter length (TDOA_DEC_STEPS=14: the 140 dB filter of rounds 2-3) has the tile form only -- the library
// then runs without the column walk (ctx->dec_cols off: no decimated inverse on the two-sweep plans).
#if TDOA_DEC_STEPS == 8 || TDOA_DEC_STEPS == 12
#define TDOA_HAVE_DEC_COLS 1

// The taps of a phase (the same for every lane), S floats at a wave-uniform address.  A complex value times a real tap is
// ONE v_pk_fma_f32 whose tap operand is a register PAIR read through op_sel -- the low half for both lanes (tap 2 j) or the
// high half (tap 2 j + 1) -- so the twelve taps stay the six pairs they were loaded as (written in C the compiler copied
// every tap into both halves of a pair of its own first: 24 v_mov and 24 registers per row).
typedef float walk_v2f __attribute__((ext_vector_type(2)));
template <int S>
struct TapRow { walk_v2f h2[S / 2]; };

template <int S>
__device__ __forceinline__ TapRow<S> walk_tap_row(const float *taps_of_phase)
{
    static_assert(S == 8 || S == 12, "steps per phase: whole float4 of taps");
    const float4 *tp = reinterpret_cast<const float4 *>(taps_of_phase);
    TapRow<S> r;
#pragma unroll
    for (int s = 0; s < S / 4; s++) {
        const float4 v = tp[s];
        r.h2[2 * s] = walk_v2f{v.x, v.y};
        r.h2[2 * s + 1] = walk_v2f{v.z, v.w};
    }
    return r;
}

// acc += tap[s] q.  SCALAR_TAPS: the pair sits in SGPRs (the staged walk's, read through the scalar cache), else in VGPRs
template <bool SCALAR_TAPS, int s, int S>
__device__ __forceinline__ void walk_mac(float2 &acc, const TapRow<S> &tr, float2 q_)
{
#define TDOA_WALK_FMA(c_) \
    if (s & 1) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(a) : "v"(q), c_(tr.h2[s / 2])); \
    else asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "+v"(a) : "v"(q), c_(tr.h2[s / 2]))
    walk_v2f a = {acc.x, acc.y};
    const walk_v2f q = {q_.x, q_.y};
    if constexpr (SCALAR_TAPS) { TDOA_WALK_FMA("s"); }
    else { TDOA_WALK_FMA("v"); }
    acc = make_float2(a.x, a.y);
#undef TDOA_WALK_FMA
}
template <bool SCALAR_TAPS, int S, int... s>
__device__ __forceinline__ void walk_mac_all(float2 (&acc)[S], const TapRow<S> &tr, float2 q, std::integer_sequence<int, s...>)
{
    (walk_mac<SCALAR_TAPS, s>(acc[s], tr, q), ...);
}

// W_N^num, N = 2 Nc, num = k2 + N2 k1 < Nc <= 2^24 (exact as a float).  N2 is the kernels' template argument itself (round 5:
// 2560 = 5 x 512 next to the powers of two); where it is not a power of two the roots (N = 5 x 2^k) come from unit_root_any.
template <int N2>
__device__ __forceinline__ float2 walk_root(const FftPlan &pl, float invNc, float num)      // invNc = 1 / Nc, worked out once per walk
{
    if constexpr ((N2 & (N2 - 1)) == 0) return unit_root(num, invNc, false);
    else return unit_root_any(num, 0.5f * (float)pl.Nc, 2.0f * invNc, false);
}

// The two stencils of one thread's walk and where their values leave to.  A kernel brings a row's four operands, its
// rotation and its taps, and keeps its own loop.
template <int N2, bool SCALAR_TAPS>
struct WalkStencil {
    static constexpr int N1 = 4096, C = kDecCentre, S = kDecSteps, NG = N2 / 16;   // NG: groups of 16 rows = outputs per column
    static_assert(NG >= 2 * C + 2, "a column's own outputs and its neighbours' shares do not overlap");
    float2 at[S], ab[S];        // at[s]: output g + C - s of column k1;  ab[u]: output gb - (C - 1) + u of column km
    float2 *g_top, *g_bot, *x_top, *x_bot;

    // pair-window pwu, columns k1 (downwards) and km = 4095 - k1 (upwards); both stencils empty
    __device__ __forceinline__ void start(float2 *G, float2 *X, const FftPlan &pl, unsigned int pwu, int k1)
    {
        const int km = N1 - 1 - k1;
        const size_t rc = (size_t)(pl.Nc / kDecD);
        g_top = G + (size_t)pwu * rc + k1, g_bot = G + (size_t)pwu * rc + km;
        x_top = X + (size_t)pwu * kDecShareRows * N1 + k1, x_bot = X + (size_t)pwu * kDecShareRows * N1 + km;
#pragma unroll
        for (int s = 0; s < S; s++) at[s] = ab[s] = make_float2(0.0f, 0.0f);
    }
    __device__ __forceinline__ void mac_top(const TapRow<S> &tr, float2 q) { walk_mac_all<SCALAR_TAPS>(at, tr, q, std::make_integer_sequence<int, S>{}); }
    __device__ __forceinline__ void mac_bottom(const TapRow<S> &tr, float2 q) { walk_mac_all<SCALAR_TAPS>(ab, tr, q, std::make_integer_sequence<int, S>{}); }
    __device__ __forceinline__ void shift_t()
    {
#pragma unroll
        for (int s = S - 1; s > 0; s--) at[s] = at[s - 1];
        at[0] = make_float2(0.0f, 0.0f);
    }
    __device__ __forceinline__ void shift_b()
    {
#pragma unroll
        for (int u = S - 1; u > 0; u--) ab[u] = ab[u - 1];
        ab[0] = make_float2(0.0f, 0.0f);
    }
    // at[S - 1] / ab[S - 1] is output i of its column, complete as far as that column's bins go: to G, or as a share to X
    __device__ __forceinline__ void top_leaves(int i)
    {
        if (i < 0) x_top[(size_t)(kDecEdge + i) * N1] = at[S - 1];
        else if (i < NG) g_top[(size_t)i * N1] = at[S - 1];
        else x_top[(size_t)(kDecEdge + i - NG) * N1] = at[S - 1];
        shift_t();
    }
    __device__ __forceinline__ void bottom_leaves(int i)
    {
        if (i >= NG) x_bot[(size_t)(kDecEdge + i - NG) * N1] = ab[S - 1];
        else if (i >= 0) g_bot[(size_t)i * N1] = ab[S - 1];
        else x_bot[(size_t)(kDecEdge + i) * N1] = ab[S - 1];
        shift_b();
    }
    // the output 6 places before a column gets nothing from it (|t| >= 96)
    __device__ __forceinline__ void slot0_is_zero()
    {
        x_top[0] = make_float2(0.0f, 0.0f);
        x_bot[0] = make_float2(0.0f, 0.0f);
    }

    // One row k2 > 0 (row 0 comes as zeros: row0_top / row0_bottom): K3 (pair_u_pk) on the four values, then the twelve
    // multiply-adds of either walk.  rot = W_N^(k2 + N2 k1).  tr: the taps of the row's phase; tb (FIRST, the only row of an
    // iteration whose phase can be 0): the upward walk's -- tr, or in phase 0 the reversed row; after that row (k2 > 0) the
    // caller lets the finished output NG - k2 / 16 + C leave the upward stencil.  Once the loop is through, at[s] holds output
    // NG + C - 1 - s (NG - 5 .. NG - 1 column k1's own, NG .. NG + 5 the next column's first six) and, after row0_bottom, ab[u]
    // output u - (C - 1) (C .. 0 column km's own, -1 .. -5 the previous column's last five): the kernels drain them in that order.
    template <bool FIRST>
    __device__ __forceinline__ void row(float2 ua, float2 uam, float2 ub, float2 ubm, int k2, float2 rot, const TapRow<S> &tr, const TapRow<S> &tb)
    {
        float2 q, qm;
        pair_u_pk(ua, uam, ub, ubm, rot, false, q, qm);
        if (FIRST && k2 == 0) q = qm = make_float2(0.0f, 0.0f);
        mac_top(tr, q);
        mac_bottom(FIRST ? tb : tr, qm);
    }
    // row 0 of a column pairs inside row 0: (0, c) with (0, 4096 - c); bin 0 carries (A+[0], A-[0]).  For column k1 it is
    // the first row of the downward walk (phase 0 of group 0: output C - s in at[s]; tr = phase 0): u, up = row 0 at k1 and
    // at (4096 - k1) mod 4096, root = W_N^(N2 k1).  For column km it pairs with (0, k1 + 1) and is the upward walk's LAST
    // row (tr = phase 0 reversed), root = W_N^(N2 km).
    __device__ __forceinline__ void row0_top(float2 ua, float2 uap, float2 ub, float2 ubp, float2 root, bool bin0, const TapRow<S> &tr)
    {
        float2 q, qm;
        pair_u_pk(ua, uap, ub, ubp, root, bin0, q, qm);
        mac_top(tr, q);
    }
    __device__ __forceinline__ void row0_bottom(float2 ua, float2 uap, float2 ub, float2 ubp, float2 root, const TapRow<S> &tr)
    {
        float2 q, qm;
        pair_u_pk(ua, uap, ub, ubp, root, false, q, qm);
        mac_bottom(tr, q);
    }
};
#else
#define TDOA_HAVE_DEC_COLS 0
#endif

}  // namespace tdoa
