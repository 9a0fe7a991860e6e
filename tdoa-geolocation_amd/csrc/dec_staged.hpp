// dec_staged.hpp -- the column walk of the decimated pair step with the stations' rows STAGED IN LDS (round 5).
//
// The walk itself is dec_walk.hpp.  k_pair_decimate_cols (dec_stream.hpp) gives every pair-window its own: each loads the rows
// of its two stations itself, so a window of S stations and P pairs asks for 2 P / S = S - 1 times its spectra and leaves it to the caches to
// serve the repeats.  They do so poorly: the walks that share a station drift apart by more than the L2 holds, and the
// memory-side counters showed 2.1 x (8 stations, BASELINE config 4) and 3.2 x (16 stations, config 5) the compulsory bytes
// coming through the fabric.  Here one workgroup owns 64 columns (and their 64 partner columns) of ONE window
// for a GROUP of its pairs:
//   * a LOADER wave brings the rows (k2, N2 - k2) of every station the group's pairs touch into LDS by LDS-DMA
//     (global_load_lds_dwordx4: one wave-instruction = the 512 bytes of a station's row piece + the 512 bytes of its partner
//     row piece -- one KB line of the paired layout below --, no VGPR in between), R rows per phase into a ring of two (or
//     more) phases -- a phase's bytes are asked for while the phase before it is read;
//   * every COMPUTE wave walks one pair: the register stencil of dec_walk.hpp (twelve accumulators per walk, K3 on
//     packed pairs), its four operands per row four ds_read_b64, the row's taps through the scalar cache into SGPR pairs;
//   * one raw s_barrier per phase; the loader waits with a counted vmcnt (later phases stay in flight across the barrier).
// (Or no loader wave at all -- the FOLDED form below: sixteen walks, the last waves each bring one station -- where that makes
// fewer workgroups: 13 - 16 stations.)
// Which pairs a workgroup takes comes from a table the host builds once (StgGroup, build_stg_groups in tdoa_mi355x.hip): up to
// eight stations consecutive runs of the window's pair list, more than eight a greedy share-out that keeps every group within
// eight stations -- a station sits in the ring at its RANK among the group's stations, so eight rows per phase fit for any S.
// A station's row piece comes from memory once per GROUP; the groups of one (window, column block) take consecutive slots
// of one XCD and start together, so later groups find rows in that XCD's L2.
// Where the plan leaves room (N2 = 256, 512) the row pass writes the spectra in BLOCKS of 64 columns, as PAIRED LINES (round 9,
// stg_paired_at below): U[cb (32)][k2][128], line [cb][k2] = the 64 columns of block cb of row k2, then the 64 columns of block
// 63 - cb of the partner row N2 - k2 -- exactly the KB the ring holds for a station and row.  One LDS-DMA instruction then
// reads one contiguous KB (lane l its bytes 16 l ..), a station's rows follow each other in memory through the whole walk
// (one ascending stream per station: R KB per phase), row 0's partner lies in its own line and phase 0 goes out like every
// other phase.  Where a window's pairs are ONE group every staged byte has one reader in the launch, and the loader wave asks
// for it non-temporally (kStgLayoutNt; several groups keep the default policy: the later ones find the rows in their XCD's L2).
// Before round 9 the blocks were [column / 64][k2][column % 64] -- the forward piece and the partner piece of a ring line in
// different blocks, lanes 0..31 ascending through one and lanes 32..63 descending through the other: two 512-byte pieces per
// instruction, two 4 KB runs per station and phase, phase 0 (row 0 pairs with row 0) row by row through the hand-laid block.
// That form stays behind TDOA_NO_STG_PAIRED=1, non-temporal loads behind TDOA_NO_STG_NT=1; measured: DESIGN.md section 9.
// Outputs: exactly k_pair_decimate_cols's -- G[pw][N2/16][4096] and the neighbour shares X[pw][12][4096] -- or, with MERGE_, G
// with the shares of a block's inner columns already added (the same bits the row pass would produce) and X at the block-edge
// columns only.
//
// What bounds it (round 5, measurement build -DTDOA_STG_TIMING + scripts/microbench/lds_dma_probe.hip, profiles/r05_staged_walk_*):
// the walks' vector issue.  The counters first read otherwise -- the walks 28 - 37 % of their cycles at the barrier, the loader
// 73 - 82 % of its cycles inside its issue loop -- but (a) with the loader's priority raised (s_setprio 3) its issue share falls
// to 35 - 38 %, it waits 38 - 46 % at the barrier, and the kernel takes the same time: the loader was only being served last, in
// slots the walks left; (b) with the walks idle the loaders alone need half the kernel's time (cfg4 1.55 of 3.0 ms, cfg5 32 of
// 72); (c) a walk's time "at the barrier" is mostly spent while the other walks of its SIMD issue -- the oldest wave runs
// ahead and waits for its neighbours.  What is left: 42 vector instructions per row and pair (24 of them the filter), issue
// share 0.70, fourteen or fifteen walks on four SIMDs.  Nothing on the loader's side changes the time: a second loader wave,
// a branch-free block, the cache-policy bits, the layout of the spectra.
//
// grid: 8 x ceil(windows 32 / 8) x groups workgroups (1-D), 64 (compute waves + 1) threads; dynamic LDS nb x R x slots KB.
#pragma once

#include "dec_walk.hpp"

namespace tdoa {

constexpr int kStgMaxStations = 16;          // station slots in LDS (1 KB per row and station)
constexpr int kStgMaxWaves = 16;
constexpr int kStgLdsBytes = 128 * 1024;     // the ring: phases x rows per phase x stations x 1 KB
constexpr int kStgMaxInFlight = 60;          // LDS-DMA instructions a loader wave leaves outstanding (the counter holds 63)
// merged shares: a walk holds 4 C - 2 more values (44 VGPRs) for its whole run and the kernel grows from 99 / 101 / 113 VGPRs
// at four waves per SIMD (R = 2 / 4 / 8) to 177 / 179 / 191 at two, no scratch -- the waves of a CU that may run it.  (At
// three waves per SIMD, 168 registers, the compiler spills nine of them: -DTDOA_STG_MERGE_WAVES=12.)
#ifndef TDOA_STG_MERGE_WAVES
#define TDOA_STG_MERGE_WAVES 8
#endif
constexpr int kStgMergeWaves = TDOA_STG_MERGE_WAVES;
constexpr int kStgBlockCols = 64;            // columns per block of the unpacked spectra (paired lines, or [column / 64][row k2][column % 64])
// one workgroup's share of a window's pairs: `n` of them, by their index in the window's pair list, and the stations they touch
// (bit s = the window's station s); a station's place in the LDS ring is its rank among the set bits
struct StgGroup {
    uint32_t mask;
    int32_t n;
    uint8_t pair[16];
};

// what the launch tells the kernel about the unpacked spectra and the loader's loads (k_pair_decimate_staged's `layout`)
enum : int {
    kStgLayoutBlocked = 1,      // blocks of 64 columns (either form below); 0: row-major rows, in place
    kStgLayoutPaired = 2,       // ... the PAIRED blocks of stg_paired_at
    kStgLayoutNt = 4            // the loader wave's LDS-DMA non-temporal: every staged byte has one reader in this launch
};

// The PAIRED block layout of a station-window's unpacked spectrum (4096 columns x N2 rows, N2 = 256 / 512 a power of two):
// U[cb (32)][k2 (N2)][128].  Line [cb][k2] is the 1 KB the LDS ring holds for that station and row -- columns 64 cb .. 64 cb + 63
// of row k2, then columns 4032 - 64 cb .. 4095 - 64 cb of the partner row (N2 - k2) mod N2 (rows 0 and N2 / 2 pair with
// themselves), both ascending -- so one LDS-DMA instruction reads ONE contiguous KB, a station's rows follow each other in memory
// through the whole walk (8 KB per phase of eight rows, one ascending stream), and phase 0 is a phase like any other.
// The element index of (row, column); used by the row pass that writes the layout (k_fwd_row4096_unpack), by both loaders and
// by the walk's row-0 reads below, and exported to the tests (tdoa_debug_stg_paired_index).
__host__ __device__ inline size_t stg_paired_at(int n2, int row, int col)
{
    const int b = col >> 6;
    return b < 32 ? ((size_t)b * (size_t)n2 + (size_t)row) * 128 + (size_t)(col & 63)
                  : ((size_t)(63 - b) * (size_t)n2 + (size_t)((n2 - row) & (n2 - 1))) * 128 + 64 + (size_t)(col & 63);
}

#if TDOA_HAVE_DEC_COLS

// One station's R_ rows of a phase by LDS-DMA, as ONE asm statement: M0 (the LDS destination) is written and read inside the
// same statement, the compiler can put nothing between its parts, and the wait state an M0 write needs before the next LDS-DMA
// is in the text: the s_nop after the first write, the v_add between every later write and the next load.  M0 is the
// compiler's own register: the statement leaves it as it found it.  (Naming it as clobbered instead is refused -- "clobber list
// contains reserved registers: m0 ... may lead to undefined behaviour", once per instantiation.)
// A row is 1 KB further on in LDS; in memory `step` further per lane.
// (hipcc counts none of these loads: the caller waits with stg_wait_vm.)
#define TDOA_STG_ROW(mod_, step_) "global_load_lds_dwordx4 %[v], %[b]" mod_ "\n\ts_add_u32 m0, m0, 0x400\n\tv_add_u32 %[v], " step_ ", %[v]\n\t"
#define TDOA_STG_ROWS2(mod_, step_) TDOA_STG_ROW(mod_, step_) TDOA_STG_ROW(mod_, step_)
#define TDOA_STG_ROWS4(mod_, step_) TDOA_STG_ROWS2(mod_, step_) TDOA_STG_ROWS2(mod_, step_)
#define TDOA_STG_ROWS8(mod_, step_) TDOA_STG_ROWS4(mod_, step_) TDOA_STG_ROWS4(mod_, step_)
#define TDOA_STG_STATION(rows_, ...)                                                                                           \
    asm volatile("s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[dst]\n\ts_nop 0\n\t" rows_ "s_mov_b32 m0, %[keep]"                    \
                 : [keep] "=&s"(keep), [v] "+v"(v) : [b] "s"(base), [dst] "s"(dst), ##__VA_ARGS__ : "memory", "scc")
// paired layout: lane l reads bytes 16 l .. 16 l + 15 of a line, the next row's line is the next KB.  NT_: non-temporal.
template <int R_, bool NT_>
__device__ __forceinline__ void stg_dma_lines(unsigned int v, unsigned long long base, unsigned int dst)
{
    static_assert(R_ == 2 || R_ == 4 || R_ == 8, "rows per phase");
    unsigned int keep;
    if constexpr (NT_) {
        if constexpr (R_ == 8) TDOA_STG_STATION(TDOA_STG_ROWS8(" nt", "0x400"));
        else if constexpr (R_ == 4) TDOA_STG_STATION(TDOA_STG_ROWS4(" nt", "0x400"));
        else TDOA_STG_STATION(TDOA_STG_ROWS2(" nt", "0x400"));
    } else {
        if constexpr (R_ == 8) TDOA_STG_STATION(TDOA_STG_ROWS8("", "0x400"));
        else if constexpr (R_ == 4) TDOA_STG_STATION(TDOA_STG_ROWS4("", "0x400"));
        else TDOA_STG_STATION(TDOA_STG_ROWS2("", "0x400"));
    }
}
// [column / 64][k2][column % 64] blocks: lanes 0..31 the forward piece (the next row 512 bytes up), lanes 32..63 the partner
// piece of block 63 - cb (512 bytes down): dv = +-512 per lane
template <int R_>
__device__ __forceinline__ void stg_dma_halves(unsigned int v, int dv, unsigned long long base, unsigned int dst)
{
    static_assert(R_ == 2 || R_ == 4 || R_ == 8, "rows per phase");
    unsigned int keep;
    if constexpr (R_ == 8) TDOA_STG_STATION(TDOA_STG_ROWS8("", "%[dv]"), [dv] "v"(dv));
    else if constexpr (R_ == 4) TDOA_STG_STATION(TDOA_STG_ROWS4("", "%[dv]"), [dv] "v"(dv));
    else TDOA_STG_STATION(TDOA_STG_ROWS2("", "%[dv]"), [dv] "v"(dv));
}
#undef TDOA_STG_STATION
#undef TDOA_STG_ROWS8
#undef TDOA_STG_ROWS4
#undef TDOA_STG_ROWS2
#undef TDOA_STG_ROW

#ifdef TDOA_STG_TIMING
// measurement build: wave-cycles [0] walks in total, [1] walks at the barrier, [2] loaders in total, [3] loaders waiting for
// their LDS-DMA to land, [4] loaders at the barrier, [5] walks counted, [6] loaders counted, [7] loaders inside issue() (read and
// cleared through tdoa_debug_stg_prof; bench.py prints them with TDOA_STG_PROF=1)
__device__ unsigned long long g_stg_prof[8];
#define TDOA_STG_T(...) __VA_ARGS__
#else
#define TDOA_STG_T(...)
#endif

// one s_waitcnt vmcnt(n) for a run-time n (the field is an immediate): n = the LDS-DMA instructions of the later phases that
// may stay in flight, a multiple of 2 (rows per phase) up to kStgMaxInFlight
__device__ __forceinline__ void stg_wait_vm(int n)
{
    switch (n) {
#define TDOA_VM(n_) case n_: asm volatile("s_waitcnt vmcnt(" #n_ ")" ::: "memory"); break;
        TDOA_VM(0) TDOA_VM(2) TDOA_VM(4) TDOA_VM(6) TDOA_VM(8) TDOA_VM(10) TDOA_VM(12) TDOA_VM(14) TDOA_VM(16) TDOA_VM(18)
        TDOA_VM(20) TDOA_VM(22) TDOA_VM(24) TDOA_VM(26) TDOA_VM(28) TDOA_VM(30) TDOA_VM(32) TDOA_VM(34) TDOA_VM(36) TDOA_VM(38)
        TDOA_VM(40) TDOA_VM(42) TDOA_VM(44) TDOA_VM(46) TDOA_VM(48) TDOA_VM(50) TDOA_VM(52) TDOA_VM(54) TDOA_VM(56) TDOA_VM(58)
        TDOA_VM(60)
#undef TDOA_VM
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// (Round 5 also built the ring WITHOUT barriers -- two LDS counters per slot, `ready` set by the loader and `done` by the walks,
// bounded spins, the walks free to drift nb - 2 phases apart: bit-identical and slower on every geometry, cfg4 3.98-5.78 ms
// against 3.45-3.61, cfg5 124-159 against 89.6 (profiles/r05_staged_walk_flag_ring_sweep.txt): an LDS atomic round trip per
// phase and wave costs more than the barrier it replaces.  Commit 73f2769 holds it.)
// R_: rows (and partner rows) per phase = per barrier; nb: phases in the ring (nb - 1 of them are in flight or being read:
// what hides the memory latency is (nb - 2) R S KB per workgroup)
// MERGE_ (blocked plans, workgroups of at most kStgMergeWaves waves): the neighbour shares of the 126 inner columns never
// reach memory -- see "merged shares" below; X then holds the block-edge columns' shares only.
template <int N2_, int R_, bool MERGE_ = false>
// (plain ds_read_b64 with immediate row offsets: left to itself the backend pairs the reads of two rows into ds_read2st64_b64,
//  which the LDS serves at half the rate of two plain reads -- MI355X_MICROARCH.md, LDS table; -DTDOA_STG_PAIRED_READS for the A/B)
#ifdef TDOA_STG_PAIRED_READS
#define TDOA_STG_DS_OPS
#else
#define TDOA_STG_DS_OPS TDOA_PLAIN_DS_OPS
#endif
__global__ __launch_bounds__(64 * (MERGE_ ? kStgMergeWaves : kStgMaxWaves))
__attribute__((amdgpu_waves_per_eu(MERGE_ ? kStgMergeWaves / 4 : 4, MERGE_ ? kStgMergeWaves / 4 : 4) TDOA_STG_DS_OPS)) void k_pair_decimate_staged(const PWDesc *pw, const float2 *U, float2 *G, float2 *X, FftPlan pl,
                                                                             const float *__restrict__ taps, const StgGroup *__restrict__ groups,
                                                                             int n_items, int P, int S, int n_cw, int n_groups, int nb,
                                                                             long long u_stride, int layout)
{
    constexpr int N2 = N2_, N1 = 4096, SS = kDecSteps, R = R_;
    static_assert(16 % R == 0 && N2 % R == 0 && R % 2 == 0, "ring and loop geometry");
    // the ring: [phase slot][station][row of the phase][fwd | partner][64] float2 -- the row index innermost, so that a walk's
    // four operand addresses change once per PHASE (one v_add each) and the row inside the phase is an immediate offset
    extern __shared__ __attribute__((aligned(16))) unsigned char stage_raw[];
    const int t = threadIdx.x;
    const bool blocked = (layout & kStgLayoutBlocked) != 0, paired = (layout & kStgLayoutPaired) != 0, nt = (layout & kStgLayoutNt) != 0;
    // workgroup -> (window, column block, group of pairs): the groups of an item are consecutive slots of one XCD
    const unsigned int b = blockIdx.x, xcd = b & 7u, slot = b >> 3;
    const int item = (int)(xcd + 8u * (slot / (unsigned int)n_groups)), grp = (int)(slot % (unsigned int)n_groups);
    if (item >= n_items) return;                                   // (the whole workgroup: no barrier is left waiting)
    const int w = item >> 5, cb = item & 31;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const PWDesc *wpw = pw + (size_t)w * P;
    const int sw_base = wpw[0].sw_a;                               // the window's stations are sw_base .. (pair 0 = stations 0, 1)
    const StgGroup *gd = groups + grp;
    const int p_cnt = gd->n;
    const unsigned int mask = gd->mask;                            // stations this group's pairs touch: S or fewer
    const int zpad = pl.zpad;
    // where element (row 0, column c) of a station's spectrum lives: row-major rows (in place, the 4096 x 2048 and larger plans)
    // or blocks of 64 columns: paired (stg_paired_at) or [c / 64][k2][c % 64] (kStgBlockCols; see the loader)
    auto row0_at = [&](const float2 *base, int c) {
        return paired ? base + stg_paired_at(N2, 0, c) : blocked ? base + (size_t)(c >> 6) * ((size_t)N2 * 64) + (c & 63) : base + c;
    };
    constexpr int NP = N2 / R;                                     // phases

    // FOLDED form (no loader wave: blockDim = 64 n_cw; blocked layout, two phases in the ring): the LAST popcount(mask) waves of the
    // workgroup -- idle ones first -- each bring ONE station's rows, at the top of a phase for the next one: 3 instructions per
    // LDS-DMA next to the 336 of a walk's phase.  All sixteen waves can then walk: 28 pairs are 16 + 12 walks (four and three per
    // SIMD) instead of 14 + 14 (two SIMDs a wave short in both).
    const int n_waves = (int)(blockDim.x >> 6);
    const bool folded = n_waves == n_cw;
    const int duty = folded ? n_waves - 1 - wave : -1;                 // this wave's station: the duty-th of the group's (by rank)
    const bool has_duty = folded && duty < __builtin_popcount(mask);
    unsigned long long duty_base = 0;
    if (has_duty) {
        unsigned int m = mask;
        for (int i = 0; i < duty; i++) m &= m - 1;
        duty_base = (unsigned long long)(uintptr_t)(U + (size_t)(sw_base + __builtin_ctz(m)) * (size_t)u_stride);
    }
    typedef __attribute__((address_space(3))) unsigned char *lds_ptr_f;
    const unsigned int lds0_f = (unsigned int)(uintptr_t)((lds_ptr_f)stage_raw);
    auto issue_one = [&](int ph, int buf_) {                           // rows ph R .. ph R + R - 1 of the duty station -> ring slot buf_
        const unsigned int dst = lds0_f + (unsigned int)(buf_ * S * R + duty * R) * 1024u;
        if (paired) {                                                  // lines [cb][ph R ..]: R KB in a row, every phase alike
            stg_dma_lines<R, false>(16u * (unsigned int)lane + 1024u * (unsigned int)(cb * N2 + ph * R), duty_base, dst);
        } else if (ph > 0) {                                           // a station's pieces of consecutive rows: 512 bytes apart
            const int k2 = ph * R, km2 = N2 - k2;
            const unsigned int of = 8u * ((unsigned int)cb * (N2 * 64u) + (unsigned int)k2 * 64u);
            const unsigned int om = 8u * ((unsigned int)(63 - cb) * (N2 * 64u) + (unsigned int)km2 * 64u);
            stg_dma_halves<R>(16u * (unsigned int)(lane & 31) + (lane < 32 ? of : om), lane < 32 ? 512 : -512, duty_base, dst);
        } else {                                                       // (row 0 pairs with row 0, not with row N2)
            unsigned int keep;
            asm volatile("s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[dst]" : [keep] "=&s"(keep) : [dst] "s"(dst) : "memory");
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int k2 = r, km2 = k2 ? N2 - k2 : 0;
                const unsigned int of = 8u * ((unsigned int)cb * (N2 * 64u) + (unsigned int)k2 * 64u);
                const unsigned int om = 8u * ((unsigned int)(63 - cb) * (N2 * 64u) + (unsigned int)km2 * 64u);
                const unsigned int v = 16u * (unsigned int)(lane & 31) + (lane < 32 ? of : om);
                asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %[v], %[b]\n\ts_add_u32 m0, m0, 0x400" : : [v] "v"(v), [b] "s"(duty_base) : "memory", "scc");
            }
            asm volatile("s_mov_b32 m0, %[keep]" : : [keep] "s"(keep) : "memory");
        }
    };
    if (has_duty) issue_one(0, 0);                                     // phase 0; phase ph + 1 goes out at the top of phase ph

    if (wave >= n_cw) {
        // ---- loader: rows (k2, N2 - k2) of the stations in `mask`, phase by phase, nb - 1 phases ahead of the readers -----------
        // lanes 0..31: 16 bytes each of row k2, columns [64 cb, 64 cb + 64); lanes 32..63: of the partner row, columns
        // [4032 - 64 cb, 4096 - 64 cb) -- 1 KB per instruction, contiguous in LDS: [row of the phase][station][fwd | partner].
        // The instruction is spelled out (global_load_lds_dwordx4 v_off, s[base]: the station's base in a scalar pair, ONE lane
        // offset per row for all stations): built from per-lane 64-bit pointers through the compiler's builtin a loader wave
        // spent ~20 instructions per LDS-DMA and two of them were slower than the fourteen walks they feed (cfg4 pair step
        // 4.6-5.1 ms against 4.08 for the per-pair walk).
        // loader lw of n_lw takes every n_lw-th of the group's stations (by rank = LDS slot), from the lw-th
        const int lw = wave - n_cw, n_lw = (int)(blockDim.x >> 6) - n_cw;
        unsigned int mine = 0;
        {
            unsigned int m = mask;
            for (int i = 0; m; i++, m &= m - 1)
                if (i % n_lw == lw) mine |= m & (0u - m);
        }
        const int per_phase = R * __builtin_popcount(mine);         // (the counted wait is this wave's own counter)
        const unsigned int lane_off = 8u * (unsigned int)(lane < 32 ? 64 * cb + 2 * lane : (4032 - 64 * cb) + 2 * (lane - 32));
        unsigned long long sbase[kStgMaxStations];
#pragma unroll
        for (int s_ = 0; s_ < kStgMaxStations; s_++) sbase[s_] = (unsigned long long)(uintptr_t)(U + (size_t)(sw_base + s_) * (size_t)u_stride);
        typedef __attribute__((address_space(3))) unsigned char *lds_ptr;
        const unsigned int lds0 = (unsigned int)(uintptr_t)((lds_ptr)stage_raw);      // the ring's LDS byte address
        auto issue = [&](int ph, int buf) {
            // blocked layouts: station by station, a station's R rows back to back (row by row across the stations the same loads
            // took 6 % longer on sixteen stations: cfg5 78.8 -> 73.8 ms, 8 stations: equal).
            // PAIRED: the lines [cb][ph R .. ph R + R - 1] of every station -- R KB in a row, one lane offset for all stations and
            // phases, phase 0 included; non-temporal where the launch says that nobody reads a line twice.
            if (paired) {
                const unsigned int voff0 = 16u * (unsigned int)lane + 1024u * (unsigned int)(cb * N2 + ph * R);
                unsigned int dst = lds0 + (unsigned int)(buf * S * R + lw * R) * 1024u;
#pragma unroll
                for (int s_ = 0; s_ < kStgMaxStations; s_++) {
                    if ((mine >> s_) & 1u) {
                        if (nt) stg_dma_lines<R, true>(voff0, sbase[s_], dst);
                        else stg_dma_lines<R, false>(voff0, sbase[s_], dst);
                        dst += (unsigned int)(n_lw * R) * 1024u;
                    }
                }
                return;
            }
            // [column / 64][k2][column % 64] blocks, every phase but the first (whose row 0 pairs with row 0, not with row N2): a
            // station's 512-byte pieces are consecutive in memory (forward: ascending, partner: descending), 4 KB runs
            if (blocked && ph > 0) {
                const int k2 = ph * R, km2 = N2 - k2;
                const unsigned int of = 8u * ((unsigned int)cb * (N2 * 64u) + (unsigned int)k2 * 64u);
                const unsigned int om = 8u * ((unsigned int)(63 - cb) * (N2 * 64u) + (unsigned int)km2 * 64u);
                const unsigned int voff0 = 16u * (unsigned int)(lane & 31) + (lane < 32 ? of : om);
                const int dv = lane < 32 ? 512 : -512;
                unsigned int dst = lds0 + (unsigned int)(buf * S * R + lw * R) * 1024u;
#pragma unroll
                for (int s_ = 0; s_ < kStgMaxStations; s_++) {
                    if ((mine >> s_) & 1u) {
                        stg_dma_halves<R>(voff0, dv, sbase[s_], dst);
                        dst += (unsigned int)(n_lw * R) * 1024u;
                    }
                }
                return;
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int k2 = ph * R + r, km2 = k2 ? N2 - k2 : 0;
                unsigned int voff;
                if (blocked) {      // block cb, row k2 | block 63 - cb, row km2: 512 contiguous bytes each, the next row right behind
                    const unsigned int of = 8u * ((unsigned int)cb * (N2 * 64u) + (unsigned int)k2 * 64u);
                    const unsigned int om = 8u * ((unsigned int)(63 - cb) * (N2 * 64u) + (unsigned int)km2 * 64u);
                    voff = 16u * (unsigned int)(lane & 31) + (lane < 32 ? of : om);
                } else {
                    const unsigned int of = 8u * ((unsigned int)k2 * N1 + (unsigned int)(k2 >> 8) * (unsigned int)zpad);
                    const unsigned int om = 8u * ((unsigned int)km2 * N1 + (unsigned int)(km2 >> 8) * (unsigned int)zpad);
                    voff = lane_off + (lane < 32 ? of : om);
                }
                const unsigned int dst_row = lds0 + (unsigned int)(buf * S * R + lw * R + r) * 1024u;      // + n_lw R KB per station of this loader
                // One block for the row's stations, laid out by hand: a station that is present FALLS THROUGH to its LDS-DMA
                // (bit test, untaken branch, the load, M0 += the station stride: four issue slots).  Written as sixteen `if`s the
                // compiler moved every present station out of line -- two taken branches, three scalar operations for the LDS
                // address and an M0 save / restore around each load, ~90 cycles per LDS-DMA on a wave that can issue one
                // instruction every four: the loader needed 5.8 k cycles per phase of cfg4 (64 loads) against the 5.4 k its
                // fourteen walks compute in, and twice the walks' time on cfg5 (measurement build -DTDOA_STG_TIMING: the walks
                // spent 32 - 45 % of their cycles at the barrier).  The instructions between an M0 write and the next LDS-DMA
                // (bit test + branch) are the wait state that pair needs.
                unsigned int keep, tmp;
#ifndef TDOA_STG_DMA_MOD
#define TDOA_STG_DMA_MOD ""                  // cache-policy bits of the LDS-DMA (measurement builds: " nt", " sc1", ...)
#endif
#define TDOA_STG_DMA(k_)                                                                                                       \
    "s_bitcmp1_b32 %[mm], " #k_ "\n\ts_cbranch_scc0 .Lstg%=_" #k_ "\n\tglobal_load_lds_dwordx4 %[voff], %[b" #k_ "]" TDOA_STG_DMA_MOD "\n\t" \
    "s_add_u32 m0, m0, %[stride]\n.Lstg%=_" #k_ ":\n\t"
#define TDOA_STG_MORE(k_) "s_lshr_b32 %[tmp], %[mm], " #k_ "\n\ts_cbranch_scc0 .Lstg%=_end\n\t"
                asm volatile("s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[dst]\n\t"
                             TDOA_STG_DMA(0) TDOA_STG_DMA(1) TDOA_STG_DMA(2) TDOA_STG_DMA(3) TDOA_STG_MORE(4)
                             TDOA_STG_DMA(4) TDOA_STG_DMA(5) TDOA_STG_DMA(6) TDOA_STG_DMA(7) TDOA_STG_MORE(8)
                             TDOA_STG_DMA(8) TDOA_STG_DMA(9) TDOA_STG_DMA(10) TDOA_STG_DMA(11) TDOA_STG_MORE(12)
                             TDOA_STG_DMA(12) TDOA_STG_DMA(13) TDOA_STG_DMA(14) TDOA_STG_DMA(15)
                             ".Lstg%=_end:\n\ts_mov_b32 m0, %[keep]"
                             : [keep] "=&s"(keep), [tmp] "=&s"(tmp)
                             : [voff] "v"(voff), [mm] "s"(mine), [dst] "s"(dst_row), [stride] "s"((unsigned int)(n_lw * R) * 1024u),
                               [b0] "s"(sbase[0]), [b1] "s"(sbase[1]), [b2] "s"(sbase[2]), [b3] "s"(sbase[3]), [b4] "s"(sbase[4]),
                               [b5] "s"(sbase[5]), [b6] "s"(sbase[6]), [b7] "s"(sbase[7]), [b8] "s"(sbase[8]), [b9] "s"(sbase[9]),
                               [b10] "s"(sbase[10]), [b11] "s"(sbase[11]), [b12] "s"(sbase[12]), [b13] "s"(sbase[13]),
                               [b14] "s"(sbase[14]), [b15] "s"(sbase[15])
                             : "memory", "scc");
#undef TDOA_STG_DMA
#undef TDOA_STG_MORE
            }
        };
        // phases 0 .. nb - 2 go out at once; at barrier ph the readers are through with phase ph - 1, whose buffer then takes
        // phase ph + nb - 1
        TDOA_STG_T(const unsigned long long t_in = __builtin_readcyclecounter(); unsigned long long t_vm = 0, t_bar = 0, t_iss = 0;)
        for (int ph = 0; ph < nb - 1 && ph < NP; ph++) issue(ph, ph);
        int buf_next = (nb - 1) % nb;
        for (int ph = 0; ph < NP; ph++) {
            const int later = NP - 1 - ph < nb - 2 ? NP - 1 - ph : nb - 2;      // phases issued after ph that may stay in flight
            TDOA_STG_T(const unsigned long long t0 = __builtin_readcyclecounter();)
            stg_wait_vm(later * per_phase);                        // phase ph has landed
            TDOA_STG_T(const unsigned long long t1 = __builtin_readcyclecounter();)
            __builtin_amdgcn_s_barrier();
            TDOA_STG_T(const unsigned long long t2 = __builtin_readcyclecounter(); t_vm += t1 - t0; t_bar += t2 - t1;)
            TDOA_STG_T(const unsigned long long t3 = __builtin_readcyclecounter();)
            if (ph + nb - 1 < NP) issue(ph + nb - 1, buf_next);
            TDOA_STG_T(t_iss += __builtin_readcyclecounter() - t3;)
            buf_next = buf_next + 1 == nb ? 0 : buf_next + 1;
        }
        TDOA_STG_T(if (lane == 0) { atomicAdd(&g_stg_prof[2], __builtin_readcyclecounter() - t_in); atomicAdd(&g_stg_prof[3], t_vm);
                                    atomicAdd(&g_stg_prof[4], t_bar); atomicAdd(&g_stg_prof[6], 1ull); atomicAdd(&g_stg_prof[7], t_iss); })
        return;
    }
    if (wave >= p_cnt) {                                           // a compute wave without a pair (last group): barriers only
        for (int ph = 0; ph < NP; ph++) {
            if (has_duty) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (has_duty && ph + 1 < NP) issue_one(ph + 1, (ph + 1) & 1);
        }
        return;
    }

    // ---- compute: the walk of dec_walk.hpp for pair-window pwu, operands from LDS ----------------------------------------------
    const int pidx = gd->pair[wave];
    const unsigned int pwu = (unsigned int)(w * P + pidx);
    const PWDesc d = wpw[pidx];
    const int sa = __builtin_popcount(mask & ((1u << (d.sw_a - sw_base)) - 1u)), sb = __builtin_popcount(mask & ((1u << (d.sw_b - sw_base)) - 1u));
    const int k1 = cb * 64 + lane, km = N1 - 1 - k1;
    const float2 *Ua = U + (size_t)d.sw_a * (size_t)u_stride, *Ub = U + (size_t)d.sw_b * (size_t)u_stride;
    const float invNc = 1.0f / (float)pl.Nc;
    typedef WalkStencil<N2, true> Walk;
    constexpr int C = Walk::C, NG = Walk::NG;
    Walk st;
    st.start(G, X, pl, pwu, k1);
    // The taps of a row's phase are the same twelve numbers for every lane AND every wave: they are read through the scalar
    // cache into SGPR pairs (s_load_dwordx8 + x4 at a wave-uniform address, issued next to the rows' LDS reads) and enter the
    // multiply-adds as the scalar operand (v_pk_fma_f32 v, v, s[lo:hi] with op_sel picking the half).  From LDS they were three
    // ds_read_b128 per row and wave -- 3 KB of LDS traffic beside the 2 KB of operands, the LDS pipe at ~95 % of the walks'
    // issue time (cfg4 pair step 3.45 -> 3.08 ms, cfg5 83.7 -> 79.2).  Table: [16 phases][16 steps] floats, rot16 at 256, phase 0
    // with its steps reversed at 288 (ensure_decimation).
    const float2 *rot16 = reinterpret_cast<const float2 *>(taps + 256);
    auto tap_row = [&](int p) { return walk_tap_row<SS>(taps + (p < 16 ? 16 * p : 288)); };
    // row 0 of column k1 (dec_walk.hpp, row0_top): straight from memory, once per walk
    {
        const int kp = (N1 - k1) & (N1 - 1);
        st.row0_top(*row0_at(Ua, k1), *row0_at(Ua, kp), *row0_at(Ub, k1), *row0_at(Ub, kp), walk_root<N2>(pl, invNc, (float)k1 * (float)N2), k1 == 0, tap_row(0));
    }
    // ---- merged shares (MERGE_) ----------------------------------------------------------------------------------------------
    // A share and the output it belongs to leave their walks a whole column apart in time: the downward walk of column k1 is through
    // with its first C - 1 shares (slots 1 .. C - 1, for the LAST outputs of column k1 - 1) and with its own outputs 0 .. C - 1 after
    // 2 C - 1 groups of rows, while the shares those outputs wait for (slots C .. 2 C - 1 of column k1 - 1) are that walk's last
    // values; the upward walk mirrors it.  So a walk HOLDS the first 2 C - 1 values that leave each of its two stencils (held_t,
    // held_b: 4 C - 2 float2, pushed in front so that every index is a constant) and settles everything after its last row:
    //   * lane l takes from lane l + 1 the shares that lane held (ds_bpermute) and adds each to its own late output;
    //   * lane l takes from lane l - 1 that lane's late shares and adds each to the output it held.
    // An output receives exactly ONE share (k_inv_rows_plain_r8's merge adds one slot row of one neighbouring column to a row
    // of G: rows 0 .. C - 1 slot C + row of the column to the left, rows N2' - C + 1 .. N2' - 1 slot row - (N2' - C) of the
    // column to the right; slot 0 is never read), and the sum here is that kernel's: the f32 addition G + share of the same two
    // values, so the bits are the same.  Lanes 0 and 63 have one neighbour in another workgroup: columns = 0 (mod 64) still
    // write slots 1 .. C - 1 to X and columns = 63 (mod 64) slots C .. 2 C - 1, and the row pass adds those alone.
    constexpr int H = MERGE_ ? 2 * C - 1 : 1;
    [[maybe_unused]] float2 held_t[H], held_b[H];
    [[maybe_unused]] auto hold = [&](float2 (&h)[H], float2 v) {
#pragma unroll
        for (int u = H - 1; u > 0; u--) h[u] = h[u - 1];
        h[0] = v;
    };
    [[maybe_unused]] auto lane_from = [&](float2 v, int src) {
        return make_float2(__int_as_float(__builtin_amdgcn_ds_bpermute(4 * src, __float_as_int(v.x))),
                           __int_as_float(__builtin_amdgcn_ds_bpermute(4 * src, __float_as_int(v.y))));
    };
    [[maybe_unused]] const int lane_up = (lane + 1) & 63, lane_dn = (lane + 63) & 63;
    if constexpr (!MERGE_) st.slot0_is_zero();
    auto bottom_leaves = [&](int i) {
        if constexpr (MERGE_) {                                    // (inside the loop: i = NG + C - 1 down to C + 1)
            if (i > NG - C) hold(held_b, st.ab[SS - 1]);           // held_b[j]: the value of i = NG - (C - 1) + j
            else st.g_bot[(size_t)i * N1] = st.ab[SS - 1];
            st.shift_b();
        } else {
            st.bottom_leaves(i);
        }
    };
    auto top_leaves = [&](int i) {
        if constexpr (MERGE_) {                                    // (inside the loop: i = -(C - 1) .. NG - C)
            if (i < C) hold(held_t, st.at[SS - 1]);                // held_t[j]: the value of i = C - 1 - j
            else st.g_top[(size_t)i * N1] = st.at[SS - 1];
            st.shift_t();
        } else {
            st.top_leaves(i);
        }
    };
    // LDS byte offsets of this lane's four operands inside a (phase, row) block of S KB: column k1 of the forward piece,
    // column km = 4095 - k1 of the partner piece (its block is stored ascending: lane 63 - l)
    const unsigned int o_af = (unsigned int)(sa * R) * 1024u + 8u * (unsigned int)lane, o_am = (unsigned int)(sa * R) * 1024u + 512u + 8u * (unsigned int)(63 - lane);
    const unsigned int o_bf = (unsigned int)(sb * R) * 1024u + 8u * (unsigned int)lane, o_bm = (unsigned int)(sb * R) * 1024u + 512u + 8u * (unsigned int)(63 - lane);
    auto lds_at = [&](unsigned int off) { return *reinterpret_cast<const float2 *>(stage_raw + off); };
    float2 wg = make_float2(1.0f, 0.0f);
    auto row = [&](const float2 (&v)[4], int k2, auto first_c, const TapRow<SS> &tr, const TapRow<SS> &tb) {
        constexpr bool FIRST = decltype(first_c)::value;            // the only row of a phase whose FIR phase can be 0
        const int p = k2 & 15, g = k2 >> 4;
        st.template row<FIRST>(v[0], v[1], v[2], v[3], k2, cmul(wg, rot16[p]), tr, tb);
        if (FIRST && p == 0 && g > 0) bottom_leaves(NG - g + C);
    };
    int buf = 0;
    TDOA_STG_T(const unsigned long long t_in = __builtin_readcyclecounter(); unsigned long long t_bar = 0;)
#pragma unroll 1
    for (int ph = 0; ph < NP; ph++) {
        TDOA_STG_T(const unsigned long long t0 = __builtin_readcyclecounter();)
        if (has_duty) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's share of phase ph has landed
        __builtin_amdgcn_s_barrier();                              // phase ph is in LDS
        asm volatile("" ::: "memory");                             // ... and no read of the ring is moved above the barrier
        TDOA_STG_T(t_bar += __builtin_readcyclecounter() - t0;)
        if (has_duty && ph + 1 < NP) issue_one(ph + 1, (ph + 1) & 1);      // (folded form: nb = 2)
        const unsigned int base = (unsigned int)(buf * R) * (unsigned int)S * 1024u;
        const unsigned int a_af = base + o_af, a_am = base + o_am, a_bf = base + o_bf, a_bm = base + o_bm;      // this phase's operands
        if (++buf == nb) buf = 0;
        const int k2 = ph * R;
        if ((k2 & 15) == 0) wg = walk_root<N2>(pl, invNc, (float)k2 + (float)k1 * (float)N2);
        // two rows at a time (their eight reads in flight together; four rows' worth of operands did not fit 128 registers)
#pragma unroll
        for (int r0 = 0; r0 < R; r0 += 2) {
            float2 v[2][4];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                v[r][0] = lds_at(a_af + 1024u * (unsigned int)(r0 + r));
                v[r][1] = lds_at(a_am + 1024u * (unsigned int)(r0 + r));
                v[r][2] = lds_at(a_bf + 1024u * (unsigned int)(r0 + r));
                v[r][3] = lds_at(a_bm + 1024u * (unsigned int)(r0 + r));
            }
            const int p0 = (k2 + r0) & 15;
            const TapRow<SS> t0 = tap_row(p0), t1 = tap_row(p0 + 1);
            // t0, t1: the taps of the two rows' phases; tb (the phase's first row only): the upward walk's -- phase 0: the reversed row
            if (r0 == 0) row(v[0], k2, std::true_type{}, t0, tap_row(p0 ? p0 : 16));
            else row(v[0], k2 + r0, std::false_type{}, t0, t0);
            row(v[1], k2 + r0 + 1, std::false_type{}, t1, t1);
        }
        if (((k2 + R - 1) & 15) == 15) top_leaves((k2 >> 4) - (SS - 1 - C));
    }
    if constexpr (MERGE_) {
        static_assert(!MERGE_ || SS == 2 * C, "the held values: C - 1 shares and C outputs per stencil");
#pragma unroll
        for (int n = 0; n < SS - 1; n++) {                         // the values of i = NG - (C - 1) + n
            const float2 v = st.at[SS - 1];
            if (n < C - 1) {                                       // output i: + slot n + 1 of column k1 + 1 (that walk's i = n + 1 - C)
                const float2 s = lane_from(held_t[2 * C - 2 - n], lane_up);
                st.g_top[(size_t)(NG - (C - 1) + n) * N1] = lane < 63 ? make_float2(v.x + s.x, v.y + s.y) : v;
            } else {                                               // slot C + r: the share of output r of column k1 + 1
                const int r = n - (C - 1);
                const float2 s = lane_from(v, lane_dn), g = held_t[C - 1 - r];
                st.g_top[(size_t)r * N1] = lane > 0 ? make_float2(g.x + s.x, g.y + s.y) : g;
                if (lane == 63) st.x_top[(size_t)(C + r) * N1] = v;
            }
            st.shift_t();
        }
        if (lane == 0) {
#pragma unroll
            for (int s = 1; s < C; s++) st.x_top[(size_t)s * N1] = held_t[2 * C - 1 - s];
        }
    } else {
#pragma unroll
        for (int n = 0; n < SS - 1; n++) top_leaves(NG - (SS - 1 - C) + n);
    }
    st.row0_bottom(*row0_at(Ua, km), *row0_at(Ua, k1 + 1), *row0_at(Ub, km), *row0_at(Ub, k1 + 1), walk_root<N2>(pl, invNc, (float)km * (float)N2), tap_row(16));
    if constexpr (MERGE_) {
#pragma unroll
        for (int n = 0; n < SS; n++) {                             // the values of i = C - n
            const float2 v = st.ab[SS - 1];
            if (n == 0) {
                st.g_bot[(size_t)C * N1] = v;
            } else if (n <= C) {                                   // output r: + slot C + r of column km - 1 (lane + 1; that walk's i = NG + r)
                const int r = C - n;
                const float2 s = lane_from(held_b[C - 1 + r], lane_up);
                st.g_bot[(size_t)r * N1] = lane < 63 ? make_float2(v.x + s.x, v.y + s.y) : v;
            } else {                                               // slot s: the share of output NG - C + s of column km - 1 (lane + 1)
                const int sl = 2 * C - n;
                const float2 s = lane_from(v, lane_dn), g = held_b[sl - 1];
                st.g_bot[(size_t)(NG - C + sl) * N1] = lane > 0 ? make_float2(g.x + s.x, g.y + s.y) : g;
                if (lane == 63) st.x_bot[(size_t)sl * N1] = v;
            }
            st.shift_b();
        }
        if (lane == 0) {
#pragma unroll
            for (int s = C; s < 2 * C; s++) st.x_bot[(size_t)s * N1] = held_b[s - 1];
        }
    } else {
#pragma unroll
        for (int n = 0; n < SS; n++) bottom_leaves(C - n);
    }
    TDOA_STG_T(if (lane == 0) { atomicAdd(&g_stg_prof[0], __builtin_readcyclecounter() - t_in); atomicAdd(&g_stg_prof[1], t_bar);
                                atomicAdd(&g_stg_prof[5], 1ull); })
}

#endif  // TDOA_HAVE_DEC_COLS

}  // namespace tdoa
