// stack_map_stats.hpp -- tdoa_locate_set_stats: exact order statistics and the peak's footprint of every judged plane of the
// delay-table family (include/tdoa_mi355x.h, "map statistics").  A plane is n_cells int64 words v[c] >= 0 whose largest word
// the record reports as score_q: a map of the searches, T_0 of the cell tracks.  A cell is live when v[c] > 0.
//
// The selection is a radix selection over 11-bit digits, from the top digit down: kMapPasses passes of
//   k_map_hist   every workgroup histograms the digits of its chunk's live words into LDS -- one histogram per rank whose
//                prefix (the digits fixed so far) differs from every earlier rank's, counting the words under that prefix --
//                and adds the non-empty bins to hist[plane][rank][2048] (integer adds: no arrival order in the result)
//   k_map_pick   one workgroup per plane scans the bins, fixes each rank's digit and remaining index, and clears the bins
// with k_map_begin in front (zero records, zero bins, the planes' state) and k_map_foot behind (the footprint's counts and box
// against level_q).  A pass whose digit window lies wholly above the highest set bit of the plane's own score_q returns at
// once, plane by plane; the first pass that does run counts all live words under the empty prefix, so it is shared by all
// ranks and its total is n_live.
//
// Everything is integer arithmetic; the only floating point is stack_value on the way out.  All the state is written by
// vector stores of single lanes and vector atomics.
#pragma once

#include "stack_locate.hpp"

namespace tdoa {

constexpr int kMapStatsMaxRanks = 8;                            // TDOA_MAP_STATS_MAX_RANKS
constexpr int kMapDigitBits = 11;
constexpr int kMapBins = 1 << kMapDigitBits;
constexpr int kMapPasses = 6;                                   // 66 bits: every positive int64
constexpr int kMapThreads = 256;
constexpr int kMapChunk = 16384;                                // cells of a plane per workgroup of k_map_hist and k_map_foot
static_assert(kMapChunk % 2 == 0, "a chunk starts at an even cell: only the plane's own start decides the alignment");
static_assert(kMapBins % kMapThreads == 0, "k_map_pick gives every thread the same number of consecutive bins");

// tdoa_map_stats
struct MapStatsOut {
    long long quantile_q[kMapStatsMaxRanks];
    double quantile[kMapStatsMaxRanks];
    long long level_q;
    int32_t n_live, foot_cells, foot_near, row_lo, row_hi, col_lo, col_hi, reserved;
};

// a plane's selection between the passes
struct MapStatsState {
    unsigned long long prefix[kMapStatsMaxRanks];               // the digits fixed so far, the first one on top
    unsigned long long remain[kMapStatsMaxRanks];               // the rank's index among the live words under its prefix
    int32_t own[kMapStatsMaxRanks];                             // the first rank with the same prefix: whose histogram counts for this one
    int32_t started, pad;                                       // a pass has run: remain holds indices
};

// what the four kernels share
struct MapStatsGeom {
    int32_t n_cells, n_cols, sep;                               // the plane; min_separation
    int32_t n_ranks, foot;                                      // the setting
    int32_t n_roots;                                            // plane p is judged with roots[(plane0 + p) mod n_roots]
    int32_t plane0;                                             // the launch's first plane in the call's order
    int32_t chunks;                                             // ceil(n_cells / kMapChunk)
    size_t stride;                                              // words from a plane to the next
};

__device__ __forceinline__ int map_pass_shift(int pass) { return kMapDigitBits * (kMapPasses - 1 - pass); }

// the pass has nothing to tell of a plane whose largest word is `best`: a zero record, or every word's digits from this
// window up are 0
__device__ __forceinline__ bool map_pass_dead(long long best, int pass) { return best <= 0 || (best >> map_pass_shift(pass)) == 0; }

typedef long long map_ll2 __attribute__((ext_vector_type(2)));

// The words of cells [c0, c0 + n) of a plane, two per lane and step: f(v0, v1, i0) with i0 the first word's index from c0 (the
// second is i0 + 1); a word outside the range comes as 0, which is no live cell.  16-byte loads where both words exist --
// pair k holds the words 2k - head and 2k - head + 1, head = 1 when the plane starts 8 bytes off a 16-byte line -- and 8-byte
// loads at the two edges.  Every lane of the workgroup makes every step (f may vote across the wave).
template <typename F>
__device__ __forceinline__ void map_for_each_pair(const long long *pp, int n, int t, F f)
{
    const int head = (int)((reinterpret_cast<uintptr_t>(pp) >> 3) & 1);
    const int n_pairs = (n + head + 1) / 2;
    for (int k0 = 0; k0 < n_pairs; k0 += kMapThreads) {
        const int k = k0 + t, i0 = 2 * k - head;
        long long v0 = 0, v1 = 0;
        if (k < n_pairs) {
            if (i0 >= 0 && i0 + 1 < n) {
                const map_ll2 v = *reinterpret_cast<const map_ll2 *>(pp + i0);
                v0 = v.x;
                v1 = v.y;
            } else {
                if (i0 >= 0 && i0 < n) v0 = pp[i0];
                if (i0 + 1 >= 0 && i0 + 1 < n) v1 = pp[i0 + 1];
            }
        }
        f(v0, v1, i0);
    }
}

// one count into an LDS histogram for every lane with `hit`; a wave whose hitting lanes all name one bin adds their number
// once (the top digits of a noise map are nearly constant: 64 adds to one address would serialise)
__device__ __forceinline__ void map_hist_add(uint32_t *h, bool hit, uint32_t bin)
{
    const unsigned long long m = __ballot(hit);
    if (m == 0) return;
    const int first = __ffsll((long long)m) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)bin, first, kWave);
    if (__ballot(hit && bin == b0) == m) {
        if ((int)(threadIdx.x & (kWave - 1)) == first) atomicAdd(&h[b0], (uint32_t)__popcll(m));
    } else if (hit) {
        atomicAdd(&h[bin], 1u);
    }
}

// grid (planes), kMapThreads threads: the zero record, zero bins and the empty prefixes of every plane of the launch
__global__ __launch_bounds__(kMapThreads) void k_map_begin(MapStatsGeom g, uint32_t *hist, MapStatsState *state, MapStatsOut *out)
{
    const int pl = blockIdx.x, t = threadIdx.x;
    uint32_t *h = hist + (size_t)pl * g.n_ranks * kMapBins;
    for (int i = t; i < g.n_ranks * kMapBins; i += kMapThreads) h[i] = 0;
    auto *o = reinterpret_cast<unsigned long long *>(out + g.plane0 + pl);
    for (int i = t; i < (int)(sizeof(MapStatsOut) / 8); i += kMapThreads) o[i] = 0;
    auto *s = reinterpret_cast<unsigned long long *>(state + pl);
    for (int i = t; i < (int)(sizeof(MapStatsState) / 8); i += kMapThreads) s[i] = 0;
}

// grid (chunks, planes), kMapThreads threads, n_ranks * kMapBins words of dynamic LDS.  planes: the launch's first plane;
// rec: its record (the search's and the tracks' records share cell and score_q).  hist[plane][rank][bin] += the chunk's live
// words under the rank's prefix whose digit of this pass is bin, for every rank that owns its histogram.
__global__ __launch_bounds__(kMapThreads) void k_map_hist(const long long *planes, MapStatsGeom g, const LocateOut *rec, int pass,
                                                          const MapStatsState *state, uint32_t *hist)
{
    extern __shared__ uint32_t map_lds[];
    const int pl = blockIdx.y, t = threadIdx.x;
    const long long best = rec[pl].score_q;                     // (one word for the whole workgroup)
    if (map_pass_dead(best, pass)) return;
    const MapStatsState &st = state[pl];
    const int shift = map_pass_shift(pass);
    unsigned long long prefix[kMapStatsMaxRanks];
    bool mine[kMapStatsMaxRanks];
#pragma unroll
    for (int r = 0; r < kMapStatsMaxRanks; r++) {
        mine[r] = r < g.n_ranks && st.own[r] == r;
        prefix[r] = r < g.n_ranks ? st.prefix[r] : 0;
    }
#pragma unroll
    for (int r = 0; r < kMapStatsMaxRanks; r++)
        if (mine[r])
            for (int i = t; i < kMapBins; i += kMapThreads) map_lds[r * kMapBins + i] = 0;
    __syncthreads();
    const int c0 = (int)blockIdx.x * kMapChunk, n = min(kMapChunk, g.n_cells - c0);
    const auto count = [&](long long v) {
        const bool live = v > 0;
        const unsigned long long u = (unsigned long long)v;
        const unsigned long long above = pass == 0 ? 0 : u >> (shift + kMapDigitBits);
        const uint32_t bin = (uint32_t)(u >> shift) & (kMapBins - 1);
#pragma unroll
        for (int r = 0; r < kMapStatsMaxRanks; r++)
            if (mine[r]) map_hist_add(map_lds + r * kMapBins, live && above == prefix[r], bin);
    };
    map_for_each_pair(planes + (size_t)pl * g.stride + c0, n, t, [&](long long v0, long long v1, int) {
        count(v0);
        count(v1);
    });
    __syncthreads();
    uint32_t *gh = hist + (size_t)pl * g.n_ranks * kMapBins;
#pragma unroll
    for (int r = 0; r < kMapStatsMaxRanks; r++)
        if (mine[r])
            for (int i = t; i < kMapBins; i += kMapThreads) {
                const uint32_t c = map_lds[r * kMapBins + i];
                if (c) atomicAdd(&gh[r * kMapBins + i], c);
            }
}

// grid (planes), kMapThreads threads.  Per rank: the bin that holds the rank's index among the words under its prefix becomes
// the next digit, the words below it leave the index.  The first pass that runs takes n_live from its total and the indices
// from ranks [n_ranks] (values 0 .. 65535): (rank (n_live - 1)) div 65535.  The last pass writes the words, level_q and, with
// a footprint asked for, the box's starting corners.  The bins are cleared for the next pass.
__global__ __launch_bounds__(kMapThreads) void k_map_pick(MapStatsGeom g, const LocateOut *rec, const double *roots, const int32_t *ranks,
                                                          int pass, MapStatsState *state, uint32_t *hist, MapStatsOut *out)
{
    constexpr int kPer = kMapBins / kMapThreads;
    __shared__ unsigned long long scan[2][kMapThreads];
    __shared__ unsigned long long pick_digit[kMapStatsMaxRanks], pick_below[kMapStatsMaxRanks];
    const int pl = blockIdx.x, t = threadIdx.x;
    const long long best = rec[pl].score_q;
    if (map_pass_dead(best, pass)) return;
    MapStatsState &st = state[pl];
    MapStatsOut &o = out[g.plane0 + pl];
    uint32_t *gh = hist + (size_t)pl * g.n_ranks * kMapBins;
    const bool first = st.started == 0;
    for (int r = 0; r < g.n_ranks; r++) {
        const uint32_t *h = gh + (size_t)(st.own[r] & (kMapStatsMaxRanks - 1)) * kMapBins;
        uint32_t c[kPer];
        unsigned long long sum = 0;
#pragma unroll
        for (int i = 0; i < kPer; i++) sum += c[i] = h[t * kPer + i];
        // inclusive scan of the threads' sums
        int cur = 0;
        scan[0][t] = sum;
        __syncthreads();
        for (int off = 1; off < kMapThreads; off <<= 1) {
            scan[cur ^ 1][t] = scan[cur][t] + (t >= off ? scan[cur][t - off] : 0);
            cur ^= 1;
            __syncthreads();
        }
        const unsigned long long total = scan[cur][kMapThreads - 1];
        unsigned long long below = scan[cur][t] - sum;          // the words in the bins before this thread's
        unsigned long long want = st.remain[r];
        if (first) want = total ? ((unsigned long long)(uint32_t)(ranks[r] & 0xffff) * (total - 1)) / 65535ull : 0;
        if (t == 0) {                                            // (a total of 0 cannot be: score_q > 0 is a live word)
            pick_digit[r] = 0;
            pick_below[r] = want;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kPer; i++) {
            if (want >= below && want < below + c[i]) {          // exactly one bin of one thread
                pick_digit[r] = (unsigned long long)(t * kPer + i);
                pick_below[r] = want - below;
            }
            below += c[i];
        }
        if (first && r == 0 && t == 0) o.n_live = (int32_t)total;
        __syncthreads();
    }
    // every rank has read its bins: clear them, and fix the state with one lane's stores
    for (int i = t; i < g.n_ranks * kMapBins; i += kMapThreads) gh[i] = 0;
    if (t != 0) return;
    unsigned long long px[kMapStatsMaxRanks];
    for (int r = 0; r < g.n_ranks; r++) {
        px[r] = (st.prefix[r] << kMapDigitBits) | pick_digit[r];
        st.prefix[r] = px[r];
        st.remain[r] = pick_below[r];
        int own = r;
        for (int e = r - 1; e >= 0; e--)
            if (px[e] == px[r]) own = e;
        st.own[r] = own;
    }
    st.started = 1;
    if (pass != kMapPasses - 1) return;
    const double root = roots[(g.plane0 + pl) % g.n_roots];
    for (int r = 0; r < g.n_ranks; r++) {
        o.quantile_q[r] = (long long)px[r];
        o.quantile[r] = stack_value((long long)px[r], root);
    }
    if (g.foot > 0) {
        const long long q0 = (long long)px[0];
        const unsigned long long d = (unsigned long long)(best > q0 ? best - q0 : 0), f = (unsigned long long)g.foot;
        o.level_q = q0 + (long long)((d >> 16) * f + (((d & 0xffff) * f) >> 16));
        o.row_lo = INT_MAX;                                      // (the best cell is in the footprint: k_map_foot lowers both)
        o.col_lo = INT_MAX;
    }
}

// grid (chunks, planes), kMapThreads threads; launched with foot > 0 only.  The chunk's live words >= level_q: their number,
// how many lie within sep rows and columns of the record's cell, and their rows' and columns' extremes, reduced over the
// workgroup and then one atomic each.
__global__ __launch_bounds__(kMapThreads) void k_map_foot(const long long *planes, MapStatsGeom g, const LocateOut *rec, MapStatsOut *out)
{
    __shared__ int32_t red[kMapThreads / kWave][6];
    const int pl = blockIdx.y, t = threadIdx.x;
    const long long best = rec[pl].score_q;
    if (best <= 0) return;
    MapStatsOut &o = out[g.plane0 + pl];
    const long long level = o.level_q;
    const int b = rec[pl].cell;
    const bool has_b = b >= 0 && b < g.n_cells;
    const int rb = has_b ? b / g.n_cols : 0, cb = has_b ? b % g.n_cols : 0;
    const int c0 = (int)blockIdx.x * kMapChunk, n = min(kMapChunk, g.n_cells - c0);
    int32_t cnt = 0, near = 0, rlo = INT_MAX, rhi = -1, clo = INT_MAX, chi = -1;
    const auto take = [&](long long v, int cell) {
        if (v <= 0 || v < level) return;
        const int row = cell / g.n_cols, col = cell % g.n_cols;
        cnt++;
        if (has_b && abs(row - rb) <= g.sep && abs(col - cb) <= g.sep) near++;
        rlo = min(rlo, row);
        rhi = max(rhi, row);
        clo = min(clo, col);
        chi = max(chi, col);
    };
    map_for_each_pair(planes + (size_t)pl * g.stride + c0, n, t, [&](long long v0, long long v1, int i0) {
        take(v0, c0 + i0);                                       // (a word outside the range is 0 and leaves before its index is used)
        take(v1, c0 + i0 + 1);
    });
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off, kWave);
        near += __shfl_xor(near, off, kWave);
        rlo = min(rlo, __shfl_xor(rlo, off, kWave));
        rhi = max(rhi, __shfl_xor(rhi, off, kWave));
        clo = min(clo, __shfl_xor(clo, off, kWave));
        chi = max(chi, __shfl_xor(chi, off, kWave));
    }
    if ((t & (kWave - 1)) == 0) {
        int32_t *w = red[t / kWave];
        w[0] = cnt, w[1] = near, w[2] = rlo, w[3] = rhi, w[4] = clo, w[5] = chi;
    }
    __syncthreads();
    if (t != 0) return;
    for (int w = 1; w < kMapThreads / kWave; w++) {
        cnt += red[w][0];
        near += red[w][1];
        rlo = min(rlo, red[w][2]);
        rhi = max(rhi, red[w][3]);
        clo = min(clo, red[w][4]);
        chi = max(chi, red[w][5]);
    }
    if (cnt == 0) return;
    atomicAdd(&o.foot_cells, cnt);
    if (near) atomicAdd(&o.foot_near, near);
    atomicMin(&o.row_lo, rlo);
    atomicMax(&o.row_hi, rhi);
    atomicMin(&o.col_lo, clo);
    atomicMax(&o.col_hi, chi);
}

}  // namespace tdoa
