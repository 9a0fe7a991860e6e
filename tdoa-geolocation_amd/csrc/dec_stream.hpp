// dec_stream.hpp -- the pair step of the decimated inverse as a COLUMN WALK (round 4), one pair-window per wave with the rows
// straight from memory.  The walk itself -- what a thread computes, where its outputs and neighbour shares go -- is
// dec_walk.hpp; this kernel brings it the rows through four moving per-lane pointers, double-buffered, and the taps from LDS
// (three ds_read_b128 at a wave-uniform address per row).  No LDS image, no barrier after the taps are in.
// grid (32 column blocks of 64, ceil(n_pw / kDecWavesPerWg)), 64 kDecWavesPerWg threads, 1 KB of LDS (the taps).
#pragma once

#include "dec_walk.hpp"

namespace tdoa {

#ifndef TDOA_DEC_STREAM_BATCH
#define TDOA_DEC_STREAM_BATCH 2
#endif
#ifndef TDOA_DEC_STREAM_WAVES
#define TDOA_DEC_STREAM_WAVES 3
#endif
constexpr int kDecStreamBatch = TDOA_DEC_STREAM_BATCH; // rows fetched ahead, per buffer (two buffers)
#ifndef TDOA_DEC_WAVES_PER_WG
#define TDOA_DEC_WAVES_PER_WG 4
#endif
constexpr int kDecWavesPerWg = TDOA_DEC_WAVES_PER_WG;  // pair-windows per workgroup (one wave each, the same 64 columns)

#if TDOA_HAVE_DEC_COLS
// taps: the tile kernel's table [16 phases][16 steps] (256 floats), then rot[16] = W_N^p as float2 (N = 2 Nc)
// (N2 is the template argument itself: dec_walk.hpp, walk_root)
template <int N2_>
__global__ __launch_bounds__(64 * kDecWavesPerWg) __attribute__((amdgpu_waves_per_eu(TDOA_DEC_STREAM_WAVES, TDOA_DEC_STREAM_WAVES))) void k_pair_decimate_cols(const PWDesc *pw, const float2 *U, float2 *G, float2 *X, FftPlan pl,
                                                              const float *__restrict__ taps, int n_pw)
{
    constexpr int N2 = N2_, N1 = 4096, S = kDecSteps, B = kDecStreamBatch;
    // A workgroup = kDecWavesPerWg waves, every one of them the SAME 64 columns (and their 64 partners) of a DIFFERENT
    // pair-window: wave w of workgroup (cb, q) walks pair-window kDecWavesPerWg q + w.  Consecutive pair-windows are a
    // window's pairs in the order (0,1), (0,2), ... -- they mostly share the template station, so the waves of a workgroup ask
    // for the same template rows within a few hundred cycles of each other: one of them brings a row in, the others find it
    // in the CU's L1 / the XCD's L2.  (One 256-column block of ONE pair-window per workgroup pulled 24 GB per cfg4 step through
    // the fabric for 5.6 GB of spectra: walks that share a station started whenever a slot came free, tens of microseconds
    // apart against an L2 turnover of ~6.)
    constexpr int W = kDecWavesPerWg;                               // (grid.x: the 32 column blocks of 64 of the left half)
    static_assert(N2 % (2 * B) == 0 && 16 % (2 * B) == 0, "loop geometry");
    // LDS: the taps [phase][step]; phase 16 = phase 0 with its steps reversed (the upward walk's row of phase 0); then the 16
    // row rotations
    __shared__ __attribute__((aligned(16))) float ltaps[17 * S];
    __shared__ __attribute__((aligned(16))) float2 lrot[16];
    const int t = threadIdx.x;
    for (int e = t; e < 17 * S; e += 64 * W) {
        const int p = e / S, s = e % S;
        ltaps[e] = p < 16 ? taps[16 * p + s] : taps[S - 1 - s];
    }
    if (t < 16) lrot[t] = reinterpret_cast<const float2 *>(taps + 256)[t];
    __syncthreads();
    const unsigned int cbu = blockIdx.x, pwu = (unsigned int)blockIdx.y * W + (unsigned int)__builtin_amdgcn_readfirstlane(t >> 6);
    if (pwu >= (unsigned int)n_pw) return;
    const int k1 = (int)cbu * 64 + (t & 63), km = N1 - 1 - k1;
    const PWDesc d = pw[pwu];
    const float2 *Ua = U + (size_t)d.sw_a * pl.Zs, *Ub = U + (size_t)d.sw_b * pl.Zs;
    const int zpad = pl.zpad;
    auto row_at = [&](const float2 *base, int k2) { return base + (size_t)k2 * N1 + (size_t)(k2 >> 8) * zpad; };
    const float invNc = 1.0f / (float)pl.Nc;
    typedef WalkStencil<N2, false> Walk;
    Walk st;
    st.start(G, X, pl, pwu, k1);
    auto tap_row = [&](int p) { return walk_tap_row<S>(ltaps + S * p); };
    {                                                               // row 0 of column k1 (dec_walk.hpp, row0_top)
        const float2 *ra = row_at(Ua, 0), *rb = row_at(Ub, 0);
        const int kp = (N1 - k1) & (N1 - 1);
        st.row0_top(ra[k1], ra[kp], rb[k1], rb[kp], walk_root<N2>(pl, invNc, (float)k1 * (float)N2), k1 == 0, tap_row(0));
    }
    st.slot0_is_zero();

    // rows (k2, k1) of both stations and their partners (N2 - k2, 4095 - k1), through four per-lane pointers that move one
    // row per fetch (+ the plan's padding after every 256 rows).  The partner of row 0 is not a row of the walk: its slot
    // reads row 0 again (the value is dropped) and the pointers then jump to row N2 - 1.
    // (wave-uniform row pointers + a 32-bit lane offset: global_load with an SGPR base, no vector instruction per address)
    const float2 *rta = row_at(Ua, 0), *rtb = row_at(Ub, 0), *rma = rta, *rmb = rtb;
    const unsigned int off_t = 8u * (unsigned int)k1, off_m = 8u * (unsigned int)km;
    auto at_off = [](const float2 *base, unsigned int byte_off) {
        return *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(base) + byte_off);
    };
    auto fetch_row = [&](float2 (&dst)[4], int k2) {                // row k2, then on to row k2 + 1
        // (the two lane offsets pass through an empty asm per fetch: hoisted out of the loop as 64-bit values they cost a
        // v_lshl_add_u64 per load; seen as 32-bit values next to the load they become its offset operand -- global_load v, v_off, s[base])
        unsigned int ot = off_t, om = off_m;
        asm volatile("" : "+v"(ot), "+v"(om));
        dst[0] = at_off(rta, ot);
        dst[1] = at_off(rma, om);
        dst[2] = at_off(rtb, ot);
        dst[3] = at_off(rmb, om);
        long long dt = N1 + ((k2 & 255) == 255 ? zpad : 0);         // row k2 + 1 starts a block of 256 rows
        long long dm = -(long long)N1 - ((k2 & 255) == 0 ? zpad : 0);   // row N2 - k2 ends one (going down)
        if (k2 == 0) dm = (long long)(N2 - 1) * N1 + (long long)((N2 - 1) >> 8) * zpad;
        if (k2 >= N2 - 1) dt = dm = 0;                              // (the prefetch past the last row re-reads it)
        rta += dt;
        rtb += dt;
        rma += dm;
        rmb += dm;
    };
    // (the leaves go through lambdas of this kernel: called on the stencil directly from the loop they cost 2 VGPRs and 3 v_mov_b64 per four rows)
    auto bottom_leaves = [&](int i) { st.bottom_leaves(i); };
    auto top_leaves = [&](int i) { st.top_leaves(i); };
    float2 wg = make_float2(1.0f, 0.0f);
    auto row = [&](const float2 (&v)[4], int k2, auto first_c) {
        constexpr bool FIRST = decltype(first_c)::value;            // the only row of an iteration whose phase can be 0
        const int p = k2 & 15, g = k2 >> 4;
        const TapRow<S> tr = tap_row(p);
        float2 q, qm;
        pair_u_pk(v[0], v[1], v[2], v[3], cmul(wg, lrot[p]), false, q, qm);
        if (FIRST && k2 == 0) q = qm = make_float2(0.0f, 0.0f);     // row 0: done above
        st.mac_top(tr, q);
        if (!FIRST) {
            st.mac_bottom(tr, qm);
        } else {
            const TapRow<S> tb = tap_row(p ? p : 16);               // (phase 0: the reversed row)
            st.mac_bottom(tb, qm);
            if (p == 0 && g > 0) bottom_leaves(Walk::NG - g + Walk::C);
        }
    };
    float2 bufa[B][4], bufb[B][4];
#pragma unroll
    for (int r = 0; r < B; r++) fetch_row(bufa[r], r);
#pragma unroll 1
    for (int k2 = 0; k2 < N2; k2 += 2 * B) {
        if ((k2 & 15) == 0) wg = walk_root<N2>(pl, invNc, (float)k2 + (float)k1 * (float)N2);     // W_N^(16 g + N2 k1): < 2^24, exact
#pragma unroll
        for (int r = 0; r < B; r++) fetch_row(bufb[r], k2 + B + r);
        row(bufa[0], k2, std::true_type{});
#pragma unroll
        for (int r = 1; r < B; r++) row(bufa[r], k2 + r, std::false_type{});
#pragma unroll
        for (int r = 0; r < B; r++) fetch_row(bufa[r], k2 + 2 * B + r);
#pragma unroll
        for (int r = 0; r < B; r++) row(bufb[r], k2 + B + r, std::false_type{});
        if ((k2 & 15) == 16 - 2 * B) top_leaves((k2 >> 4) - (S - 1 - Walk::C));       // group g of the downward walk is complete: output g - 5
    }
#pragma unroll
    for (int n = 0; n < S - 1; n++) top_leaves(Walk::NG - (S - 1 - Walk::C) + n);
    {                                                               // row 0 of column km, the upward walk's last row (row0_bottom)
        const float2 *ra = row_at(Ua, 0), *rb = row_at(Ub, 0);
        st.row0_bottom(ra[km], ra[k1 + 1], rb[km], rb[k1 + 1], walk_root<N2>(pl, invNc, (float)km * (float)N2), tap_row(16));
    }
#pragma unroll
    for (int n = 0; n < S; n++) bottom_leaves(Walk::C - n);
}
#endif

}  // namespace tdoa
