// stack_closure.hpp -- tdoa_process_closure: one consistent lag set per station triple of a stack (include/tdoa_mi355x.h,
// "closure search").  The delays of three stations i < j < k close, lag(i,j) + lag(j,k) = lag(i,k), so the three pairs'
// stacked surfaces are searched together: over the cells (u, v) around the pairs' centres,
//     score_q(u,v) = M_ij[c_ij + u] + M_ik[c_ik + v] + M_jk[c_jk + v - u]        M_p[l] = |Q_p[l]|
// and the largest one gives the three lags at once.
//
// k_closure_search   one (stack, triple) and one tile of u per workgroup: the best cell of the tile, as a two-word candidate;
//                    run twice -- the joint cell, then the runner-up, the cells more than min_separation from (u*, v*)
// k_closure_finish   the tiles' candidates -> (u*, v*) and the record, with the three pairs' own maxima (own_q, residual);
//                    after the second search: runner_q and runner_up
//
// Everything is integer arithmetic on the Q words of stack_surfaces.hpp; the only floating point is stack_value on the way
// out.  The candidate (ClosureCand), its order and the workgroup reductions (closure_block_best, search_best_candidate,
// search_block_sum, search_wave_sum / _min / _max) serve the delay-table and the clock searches too: every search header
// includes this one.
#pragma once

#include "stack_surfaces.hpp"

namespace tdoa {

constexpr int kClosureThreads = 256;
constexpr int kClosureTileU = 32;                               // values of u per workgroup
constexpr int kClosureMaxGate = 1023;                           // the largest G: two staged rows of 2 G + 1 words are 32 KB of LDS
constexpr int kClosureMaxStations = 64;
constexpr long long kClosureAbsent = -1;                        // a lag outside the searched range: no magnitude is negative

// tdoa_closure
struct ClosureOut {
    int32_t lag_ij, lag_ik, lag_jk, residual;
    long long score_q, own_q, runner_q;
    double corr_ij, corr_ik, corr_jk;
    double score, runner_up;
};

// A cell's score and where it is.  key: the larger one wins among equal scores -- kClosureKeyTop - (rank(u) << 12 | rank(v))
// with rank(x) = 0, 1, 2, 3, 4 ... for x = 0, +1, -1, +2, -2 ...: the smaller |u|, then the positive u, then the smaller |v|,
// then the positive v.  No cell: score kClosureAbsent.  (A score has up to 59 bits: it does not fit into one word with the
// coordinates, so this is not a peak_key.)
struct alignas(16) ClosureCand {
    long long score;
    uint32_t key, pad;
};
constexpr uint32_t kClosureKeyTop = 0xFFFFFFu;

struct ClosureBest {       // (u*, v*) of a (stack, triple), 0, 0 where there is no joint cell
    int32_t u, v;
};

struct ClosureGeom {
    int32_t S, P, T;       // stations, pairs, triples
    int32_t n, lag_lo;     // lags per row of Q, the first one
    int32_t G, sep;        // gate, min_separation
    int32_t tiles;         // tiles of u: ceil((2 G + 1) / kClosureTileU)
};

__device__ __forceinline__ uint32_t closure_rank(int x) { return (uint32_t)(2 * (x < 0 ? -x : x) - (x > 0 ? 1 : 0)); }
__device__ __forceinline__ int closure_unrank(uint32_t r) { return (r & 1u) ? (int)((r + 1) >> 1) : -(int)(r >> 1); }
__device__ __forceinline__ bool closure_better(long long s, uint32_t k, long long bs, uint32_t bk)
{
    return s > bs || (s == bs && k > bk);
}

// triple number t of S stations, i < j < k in lexicographic order, and the library's pair numbers
__device__ __forceinline__ void closure_triple(int t, int S, int *i, int *j, int *k)
{
    int a = 0;
    for (int c = (S - 1) * (S - 2) / 2; t >= c; c = (S - 1 - a) * (S - 2 - a) / 2) {
        t -= c;
        a++;
    }
    int b = a + 1;
    for (int c = S - 1 - b; t >= c; c = S - 1 - b) {
        t -= c;
        b++;
    }
    *i = a;
    *j = b;
    *k = b + 1 + t;
}
__device__ __forceinline__ int closure_pair(int i, int j, int S) { return i * S - i * (i + 1) / 2 + (j - i - 1); }

// M_p at the lag c + x: |Q_p|, or kClosureAbsent outside the range (c is a difference of two int32: 64 bits)
__device__ __forceinline__ long long closure_m(const long long *q, long long c, int x, const ClosureGeom &g)
{
    const long long idx = c + x - g.lag_lo;
    if (idx < 0 || idx >= g.n) return kClosureAbsent;
    const long long v = q[idx];
    return v < 0 ? -v : v;
}

// the workgroup's best candidate in every thread; red_s / red_k: one word per wave of LDS, free again on return
__device__ __forceinline__ void closure_block_best(long long &s, uint32_t &k, long long *red_s, uint32_t *red_k)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long os = __shfl_xor(s, off, kWave);
        const uint32_t ok = __shfl_xor(k, off, kWave);
        if (closure_better(os, ok, s, k)) {
            s = os;
            k = ok;
        }
    }
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red_s[w] = s;
        red_k[w] = k;
    }
    __syncthreads();
    s = red_s[0];
    k = red_k[0];
#pragma unroll
    for (int x = 1; x < kClosureThreads / kWave; x++)
        if (closure_better(red_s[x], red_k[x], s, k)) {
            s = red_s[x];
            k = red_k[x];
        }
    __syncthreads();
}

// The workgroup reductions of every stack search (closure, delay table, clocks), stated here once.  Each is for the
// kClosureThreads threads the searches' kernels all have; a header whose kernels use another constant asserts that it is equal.

// The start of a finishing kernel: the tiles' candidates of the workgroup's set, line or track, cand[tiles], -> the best of them
// in every thread (equal scores: the larger key).  Ends with closure_block_best's barrier.
__device__ __forceinline__ void search_best_candidate(const ClosureCand *cand, int tiles, long long *red_s, uint32_t *red_k, long long &bs,
                                                      uint32_t &bk)
{
    bs = kClosureAbsent;
    bk = 0;
    for (int y = threadIdx.x; y < tiles; y += kClosureThreads) {
        const ClosureCand c = cand[y];
        if (closure_better(c.score, c.key, bs, bk)) {
            bs = c.score;
            bk = c.key;
        }
    }
    closure_block_best(bs, bk, red_s, red_k);
}

// a wave's sum, smallest and largest word, in every lane
__device__ __forceinline__ int search_wave_sum(int v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
__device__ __forceinline__ int search_wave_min(int v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ __forceinline__ int search_wave_max(int v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
    return v;
}

// the workgroup's sums of f and n in every thread; red_s / red_n: one word per wave of LDS, free again on return
__device__ __forceinline__ void search_block_sum(long long &f, int &n, long long *red_s, int *red_n)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        f += __shfl_xor(f, off, kWave);
        n += __shfl_xor(n, off, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red_s[threadIdx.x / kWave] = f;
        red_n[threadIdx.x / kWave] = n;
    }
    __syncthreads();
    f = 0;
    n = 0;
#pragma unroll
    for (int w = 0; w < kClosureThreads / kWave; w++) {
        f += red_s[w];
        n += red_n[w];
    }
    __syncthreads();
}

// LDS words of k_closure_search: the rows M_ik and M_jk over the whole gate, M_ij over the tile, the reduction's words
__host__ __device__ constexpr size_t closure_lds_bytes(int G)
{
    return sizeof(long long) * (size_t)(2 * (2 * G + 1) + kClosureTileU + 2 * (kClosureThreads / kWave));
}

// grid (n_sets * T, tiles), kClosureThreads threads, closure_lds_bytes(G) of dynamic LDS.  Q: [set][pair][n]; centre:
// [S].  The workgroup owns the cells u0 <= u < u0 + kClosureTileU of one (set, triple).  It stages M_ik[c_ik + v] and
// M_jk[c_jk + d] for every |v|, |d| <= G and M_ij[c_ij + u] for its own u, a lag outside the range as kClosureAbsent; then
// lanes run along v and the loop over u, so both varying reads are consecutive words.  A cell exists when none of its three
// words is absent.  best == nullptr: every cell competes.  Otherwise only the cells with max(|u - u*|, |v - v*|) > sep
// (the runner-up's pass).  partial[(set, triple) * tiles + tile] = the tile's best candidate.
__global__ __launch_bounds__(kClosureThreads) void k_closure_search(const long long *Q, ClosureGeom g, const int32_t *centre,
                                                                    const ClosureBest *best, ClosureCand *partial)
{
    extern __shared__ long long closure_lds[];
    const int W = 2 * g.G + 1;
    long long *m_ik = closure_lds, *m_jk = m_ik + W, *m_ij = m_jk + W, *red_s = m_ij + kClosureTileU;
    uint32_t *red_k = reinterpret_cast<uint32_t *>(red_s + kClosureThreads / kWave);
    const int st = blockIdx.x, set = st / g.T, t = threadIdx.x;
    int i, j, k;
    closure_triple(st % g.T, g.S, &i, &j, &k);
    const long long ci = centre[i], cj = centre[j], ck = centre[k];
    const long long *q_set = Q + (size_t)set * g.P * g.n;
    const long long *q_ij = q_set + (size_t)closure_pair(i, j, g.S) * g.n, *q_ik = q_set + (size_t)closure_pair(i, k, g.S) * g.n,
                    *q_jk = q_set + (size_t)closure_pair(j, k, g.S) * g.n;
    const int u0 = -g.G + (int)blockIdx.y * kClosureTileU, u1 = min(u0 + kClosureTileU - 1, g.G);
    for (int e = t; e < W; e += kClosureThreads) {
        m_ik[e] = closure_m(q_ik, ck - ci, e - g.G, g);
        m_jk[e] = closure_m(q_jk, ck - cj, e - g.G, g);
    }
    if (t <= u1 - u0) m_ij[t] = closure_m(q_ij, cj - ci, u0 + t, g);
    __syncthreads();
    int us = 0, vs = 0;
    if (best) {
        us = best[st].u;
        vs = best[st].v;
    }
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    for (int u = u0; u <= u1; u++) {
        const long long mu = m_ij[u - u0];
        if (mu < 0) continue;                // (the same for every thread)
        const uint32_t ru = closure_rank(u) << 12;
        const bool u_near = best && abs(u - us) <= g.sep;
        const int v_hi = min(g.G, u + g.G);
        for (int v = max(-g.G, u - g.G) + t; v <= v_hi; v += kClosureThreads) {
            const long long a = m_ik[v + g.G], e = m_jk[v - u + g.G];
            if ((a | e) < 0) continue;
            if (u_near && abs(v - vs) <= g.sep) continue;
            const long long s = mu + a + e;
            const uint32_t key = kClosureKeyTop - (ru | closure_rank(v));
            if (closure_better(s, key, bs, bk)) {
                bs = s;
                bk = key;
            }
        }
    }
    closure_block_best(bs, bk, red_s, red_k);
    if (t == 0) partial[(size_t)st * g.tiles + blockIdx.y] = ClosureCand{bs, bk, 0};
}

// One workgroup per (set, triple).
// pass 0: the tiles' candidates -> the joint cell (u*, v*) into best, and the record: the three lags, score_q, the signed C
// at the three lags, score; the three pairs' own maxima over their gated windows (equal maxima: the smaller |x|, then the
// positive x) give own_q and residual = x*_ij + x*_jk - x*_ik (the centres close, so they drop out); runner_q and runner_up
// 0.  No cell, or a largest score of 0: the zero record and (0, 0).
// pass 1 (partial now holds the runner-up's pass): runner_q and runner_up of a record that is not the zero record.
// roots[set] = sqrt(n_w).
__global__ __launch_bounds__(kClosureThreads) void k_closure_finish(const long long *Q, ClosureGeom g, const int32_t *centre,
                                                                    const double *roots, const ClosureCand *partial, int pass,
                                                                    ClosureBest *best, ClosureOut *out)
{
    __shared__ long long red_s[kClosureThreads / kWave];
    __shared__ uint32_t red_k[kClosureThreads / kWave];
    const int st = blockIdx.x, set = st / g.T, t = threadIdx.x;
    long long bs;
    uint32_t bk;
    search_best_candidate(partial + (size_t)st * g.tiles, g.tiles, red_s, red_k, bs, bk);
    const double root = roots[set];
    if (pass == 1) {
        if (t == 0 && out[st].score_q != 0) {
            const long long r = bs > 0 ? bs : 0;
            out[st].runner_q = r;
            out[st].runner_up = stack_value(r, root);
        }
        return;
    }
    int i, j, k;
    closure_triple(st % g.T, g.S, &i, &j, &k);
    const long long ci = centre[i], cj = centre[j], ck = centre[k];
    const long long *q_set = Q + (size_t)set * g.P * g.n;
    const long long *q_p[3] = {q_set + (size_t)closure_pair(i, j, g.S) * g.n, q_set + (size_t)closure_pair(i, k, g.S) * g.n,
                               q_set + (size_t)closure_pair(j, k, g.S) * g.n};
    const long long c_p[3] = {cj - ci, ck - ci, ck - cj};
    long long own = 0;
    int x_own[3];
#pragma unroll
    for (int p = 0; p < 3; p++) {
        long long ms = kClosureAbsent;
        uint32_t mk = 0;
        for (int x = -g.G + t; x <= g.G; x += kClosureThreads) {
            const long long m = closure_m(q_p[p], c_p[p], x, g);
            const uint32_t key = kClosureKeyTop - closure_rank(x);
            if (m >= 0 && closure_better(m, key, ms, mk)) {
                ms = m;
                mk = key;
            }
        }
        closure_block_best(ms, mk, red_s, red_k);
        own += ms > 0 ? ms : 0;
        x_own[p] = ms >= 0 ? closure_unrank(kClosureKeyTop - mk) : 0;
    }
    if (t != 0) return;
    ClosureOut rec{0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0};
    ClosureBest b{0, 0};
    if (bs > 0) {
        const uint32_t cell = kClosureKeyTop - bk;
        b.u = closure_unrank(cell >> 12);
        b.v = closure_unrank(cell & 0xFFFu);
        rec.lag_ij = (int32_t)(c_p[0] + b.u);
        rec.lag_ik = (int32_t)(c_p[1] + b.v);
        rec.lag_jk = rec.lag_ik - rec.lag_ij;
        rec.residual = x_own[0] + x_own[2] - x_own[1];
        rec.score_q = bs;
        rec.own_q = own;
        rec.corr_ij = stack_value(q_p[0][rec.lag_ij - g.lag_lo], root);
        rec.corr_ik = stack_value(q_p[1][rec.lag_ik - g.lag_lo], root);
        rec.corr_jk = stack_value(q_p[2][rec.lag_jk - g.lag_lo], root);
        rec.score = stack_value(bs, root);
    }
    best[st] = b;
    out[st] = rec;
}

}  // namespace tdoa
