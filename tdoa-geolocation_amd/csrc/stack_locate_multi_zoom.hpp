// stack_locate_multi_zoom.hpp -- tdoa_process_locate_multi_zoom: behind the rounds of stack_locate_multi.hpp, every round's
// best cell is searched again on the fine table (include/tdoa_mi355x.h, "zoomed rounds").  Round r of stack s scores the zoom's
// window (stack_locate_zoom.hpp) around Z x that round's coarse cell under the mask that round's coarse scores ran under, M_p^r:
// a pair whose lag lies within `guard` of a centre left by rounds 0 .. r - 1 counts 0.  The stage runs after the last round:
// round r's coarse cell lies in its record coarse[r][set] (a centre where score_q > 0) and all rounds' centres' words lie in
// the pairs' LocateCentres, of which round r tests words 0 .. r - 1 only.  So the round is a grid dimension, and the stage is
// two launches for any K.
//
// k_locate_zoom_scores_masked   k_locate_zoom_scores with locate_m_masked in place of locate_m and the mask's round from
//                               blockIdx.z; round 0 runs none of the tests (locate_excluded stops at the mask's round), so its
//                               plane is k_locate_zoom_scores's
// k_locate_zoom_finish_masked   k_locate_zoom_finish with locate_excluded on the cell's pairs (pairs_in, reserved, 0.0 for an
//                               excluded pair) and the counts [round][set][2]; one workgroup per (round, set)
//
// Two kernels of their own, not a MASKED parameter on the zoom's two: those read their centre from best[set] and are
// instantiated by three searches whose code objects and graph keys keep their bytes this way.
#pragma once

#include "stack_locate_multi.hpp"
#include "stack_locate_zoom.hpp"

namespace tdoa {

// up to here the masked window scores keep a cell's delays in registers (k_locate_scores_masked's limit: the same loop)
constexpr int kLocateZoomMaskedRegStations = kLocateMaskedRegStations;

// round r's coarse cell of a set as the window's centre: the record's cell where the round found one, -1 otherwise
__device__ __forceinline__ int locate_round_centre(const LocateZoomGeom &z, const LocateOut *coarse, size_t at)
{
    return coarse[at].score_q > 0 ? locate_zoom_centre(z, coarse[at].cell) : -1;
}

// grid (z.tiles, n_sets, K), kLocateThreads threads; plane = blockIdx.z * n_sets + set indexes coarse, zmap and partial.
// Q, gf, z, table, cdiff as k_locate_zoom_scores takes them (Q, cdiff and the centres are the set's, whatever the round);
// S_T (at most kLocateZoomMaskedRegStations) and CLK as there.  coarse [round][set]: the rounds' records; centres [set][pair]
// (allocated for K = 1 too: its words are loaded, never tested); guard: the mask's (locate_mask).
// zmap[plane][pos] = the masked score_q of pos's fine cell, -1 where pos does not compete; partial[plane * z.tiles + tile] =
// the tile's best candidate, key = ~fine cell.
template <int S_T, bool CLK>
__global__ __launch_bounds__(kLocateThreads) void k_locate_zoom_scores_masked(const long long *Q, LocateGeom gf, LocateZoomGeom z,
                                                                              const int32_t *table, const long long *__restrict__ cdiff,
                                                                              const LocateCentres *__restrict__ centres, int guard,
                                                                              const LocateOut *coarse, long long *zmap, ClosureCand *partial)
{
    __shared__ long long red_s[kLocateThreads / kWave];
    __shared__ uint32_t red_k[kLocateThreads / kWave];
    const int set = blockIdx.y, t = threadIdx.x;
    const size_t plane = (size_t)blockIdx.z * gridDim.y + set;
    const LocateMask mk{(int32_t)blockIdx.z, guard};
    const int pos = (int)blockIdx.x * kLocateThreads + t, b = locate_round_centre(z, coarse, plane);
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    if (pos < z.n_pos) {
        int row, col;
        const int cell = b >= 0 ? locate_zoom_cell(z, gf, b, pos, &row, &col) : -1;
        long long s = -1;
        if (cell >= 0) {
            const long long *q = Q + (size_t)set * gf.P * gf.n;
            const int32_t *tc = table + cell;
            const long long *cd = CLK ? cdiff + (size_t)set * gf.P : nullptr;
            const LocateCentres *cen = centres + (size_t)set * gf.P;
            s = 0;
            if constexpr (S_T > 0) {
                int32_t d[S_T];
#pragma unroll
                for (int i = 0; i < S_T; i++) d[i] = tc[(size_t)i * gf.n_cells];
#pragma unroll
                for (int i = 0; i < S_T; i++)
#pragma unroll
                    for (int j = i + 1; j < S_T; j++, q += gf.n, cen++) {
                        long long c = 0;
                        if constexpr (CLK) c = *cd++;
                        s += locate_m_masked(q, d[i], d[j], gf, c, cen, mk);
                    }
            } else {
                for (int i = 0; i < gf.S; i++) {
                    const int32_t di = tc[(size_t)i * gf.n_cells];
                    for (int j = i + 1; j < gf.S; j++, q += gf.n, cen++) {
                        long long c = 0;
                        if constexpr (CLK) c = *cd++;
                        s += locate_m_masked(q, di, tc[(size_t)j * gf.n_cells], gf, c, cen, mk);
                    }
                }
            }
            bs = s;
            bk = ~(uint32_t)cell;
        }
        zmap[plane * z.n_pos + pos] = s;
    }
    closure_block_best(bs, bk, red_s, red_k);
    if (t == 0) partial[plane * z.tiles + blockIdx.x] = ClosureCand{bs, bk, 0};
}

// grid (n_sets, K), kLocateThreads threads: one workgroup per (round, set), plane = blockIdx.y * n_sets + set.
// k_locate_zoom_finish on the round's masked window: the tiles' candidates -> the round's fine cell; n_best, the box and the
// runner-up on zmap[plane]; per pair lag_p(cell) and the signed C there -- 0 and 0.0 for a pair outside the range, the lag and
// 0.0 for a pair whose lag lies in E_p(round), which counts in pairs[plane][1] (reserved) and not in pairs_in.  A largest
// masked score of 0, no competing position or no coarse cell: the zero record, zero counts, lags and correlations.
// out, pairs, lags, corr: [round][set][...].
__global__ __launch_bounds__(kLocateThreads) void k_locate_zoom_finish_masked(const long long *Q, LocateGeom gf, LocateZoomGeom z,
                                                                              const int32_t *table, const long long *cdiff,
                                                                              const double *roots, const LocateCentres *centres, int guard,
                                                                              const LocateOut *coarse, const long long *zmap,
                                                                              const ClosureCand *partial, LocateZoomOut *out, int32_t *pairs,
                                                                              int32_t *lags, double *corr)
{
    constexpr int kWaves = kLocateThreads / kWave;
    __shared__ long long red_s[kWaves];
    __shared__ uint32_t red_k[kWaves];
    __shared__ int red_n[kWaves], red_in[kWaves], red_box[4][kWaves];
    const int set = blockIdx.x, t = threadIdx.x;
    const size_t plane = (size_t)blockIdx.y * gridDim.x + set;
    const LocateMask mk{(int32_t)blockIdx.y, guard};
    const int b = locate_round_centre(z, coarse, plane);
    long long bs;
    uint32_t bk;
    search_best_candidate(partial + plane * z.tiles, z.tiles, red_s, red_k, bs, bk);
    const double root = roots[set];
    const int cell = (int)~bk;
    const bool found = b >= 0 && bs > 0 && cell >= 0 && cell < gf.n_cells;      // (uniform over the workgroup)
    // the window: the count and box of the best score, the runner-up
    long long rs = kClosureAbsent;
    uint32_t rk = 0;
    int n_best = 0, row_lo = INT_MAX, row_hi = INT_MIN, col_lo = INT_MAX, col_hi = INT_MIN;
    if (found) {
        const int row_z = cell / gf.n_cols, col_z = cell % gf.n_cols;
        const long long *zm = zmap + plane * z.n_pos;
        for (int pos = t; pos < z.n_pos; pos += kLocateThreads) {
            int row, col;
            const int c = locate_zoom_cell(z, gf, b, pos, &row, &col);
            if (c < 0) continue;
            const long long s = zm[pos];
            if (s == bs) {
                n_best++;
                row_lo = min(row_lo, row);
                row_hi = max(row_hi, row);
                col_lo = min(col_lo, col);
                col_hi = max(col_hi, col);
            }
            if (max(abs(row - row_z), abs(col - col_z)) > gf.sep && closure_better(s, ~(uint32_t)c, rs, rk)) {
                rs = s;
                rk = ~(uint32_t)c;
            }
        }
    }
    closure_block_best(rs, rk, red_s, red_k);
    // the cell's pairs
    const long long *q = Q + (size_t)set * gf.P * gf.n;
    const LocateCentres *cen = centres + (size_t)set * gf.P;
    int counts = 0;                          // pairs inside and not excluded, + 2^16 pairs inside and excluded (P <= 2016)
    for (int p = t; p < gf.P; p += kLocateThreads) {
        int32_t lag = 0;
        double c = 0.0;
        if (found && locate_pair_value(q, gf, table, cdiff ? cdiff + (size_t)set * gf.P : nullptr, cell, p, root, &lag, &c)) {
            if (locate_excluded(lag, cen + p, mk)) {
                c = 0.0;
                counts += 1 << 16;
            } else {
                counts++;
            }
        }
        lags[plane * gf.P + p] = lag;
        corr[plane * gf.P + p] = c;
    }
    n_best = search_wave_sum(n_best);
    counts = search_wave_sum(counts);
    row_lo = search_wave_min(row_lo);
    row_hi = search_wave_max(row_hi);
    col_lo = search_wave_min(col_lo);
    col_hi = search_wave_max(col_hi);
    if ((t & (kWave - 1)) == 0) {
        const int w = t / kWave;
        red_n[w] = n_best;
        red_in[w] = counts;
        red_box[0][w] = row_lo;
        red_box[1][w] = row_hi;
        red_box[2][w] = col_lo;
        red_box[3][w] = col_hi;
    }
    __syncthreads();
    if (t != 0) return;
    LocateZoomOut rec{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0};
    int reserved = 0;
    if (found) {
        int n = 0;
        rec.cell = cell;
        rec.row_lo = red_box[0][0];
        rec.row_hi = red_box[1][0];
        rec.col_lo = red_box[2][0];
        rec.col_hi = red_box[3][0];
        for (int w = 0; w < kWaves; w++) {
            rec.n_best += red_n[w];
            n += red_in[w];
            rec.row_lo = min(rec.row_lo, red_box[0][w]);
            rec.row_hi = max(rec.row_hi, red_box[1][w]);
            rec.col_lo = min(rec.col_lo, red_box[2][w]);
            rec.col_hi = max(rec.col_hi, red_box[3][w]);
        }
        rec.pairs_in = n & 0xffff;
        reserved = n >> 16;
        rec.score_q = bs;
        rec.score = stack_value(bs, root);
        const int runner = (int)~rk;
        if (rs >= 0 && runner >= 0 && runner < gf.n_cells) {
            rec.runner_cell = runner;
            rec.runner_q = rs;
            rec.runner_up = stack_value(rs, root);
        }
    }
    out[plane] = rec;
    pairs[2 * plane] = rec.pairs_in;
    pairs[2 * plane + 1] = reserved;
}

}  // namespace tdoa
