// stack_locate_zoom.hpp -- tdoa_process_locate_zoom: behind the delay-table search (stack_locate.hpp), every stack's best cell
// is searched again on a second, finer table (include/tdoa_mi355x.h, "zoom locate").  The fine table covers the whole area at
// Z cells per coarse cell; stack s with the location (r*, c*) scores only the window of (2 H + 1)^2 fine cells around
// (Z r*, Z c*).  The window's centre is the word best[set] the coarse finish left in device memory: it is data, not a launch
// argument, so one captured graph serves every block.
//
// k_locate_zoom_scores   one window position per lane: the lanes of a window row read consecutive words of the station-major
//                        fine table; the position's score_q exactly as k_locate_scores forms it (locate_m); the scores go to
//                        zmap [set][position] (-1: the position does not compete), the tile's best out as a candidate with
//                        key = ~fine cell
// k_locate_zoom_finish   the tiles' candidates -> the zoom's cell; one pass over the set's window for n_best, the box and the
//                        runner-up; pairs_in, the lags and signed correlations of the cell (locate_pair_value); the record
//
// Everything is integer arithmetic on the Q words the coarse stage ran on (with the setting U > 1 the upsampled ones, the fine
// table and the clock differences times U); the only floating point is stack_value on the way out.
#pragma once

#include "stack_locate.hpp"

namespace tdoa {

constexpr int kLocateZoomMaxZ = 64;
constexpr int kLocateZoomMaxH = 64;

// tdoa_zoom
struct LocateZoomOut {
    int32_t cell, runner_cell, pairs_in, n_best;
    int32_t row_lo, row_hi, col_lo, col_hi;
    long long score_q, runner_q;
    double score, runner_up;
};

struct LocateZoomGeom {
    int32_t Z, H;              // fine cells per coarse cell, the window's half side
    int32_t side, n_pos;       // 2 H + 1, side^2
    int32_t coarse_cells, coarse_cols;       // the coarse table's shape: best[set] -> (r*, c*)
    int32_t tiles;             // ceil(n_pos / kLocateThreads)
};

// best[set] as the kernels take it: the location's coarse cell, -1 where there is none (a word that is no cell of the coarse
// table counts as none)
__device__ __forceinline__ int locate_zoom_centre(const LocateZoomGeom &z, int b) { return b >= 0 && b < z.coarse_cells ? b : -1; }

// window position pos of a set whose location is the coarse cell b -> its fine row and column, and its fine cell: -1 where the
// position does not compete (a row or column outside the fine table, a cell past its short last row).  gf: the fine table's shape.
__device__ __forceinline__ int locate_zoom_cell(const LocateZoomGeom &z, const LocateGeom &gf, int b, int pos, int *row, int *col)
{
    *row = z.Z * (b / z.coarse_cols) - z.H + pos / z.side;       // (Z r* <= 64 * 2^22: 32 bits hold it)
    *col = z.Z * (b % z.coarse_cols) - z.H + pos % z.side;
    if (*row < 0 || *col < 0 || *col >= gf.n_cols) return -1;
    const long long cell = (long long)*row * gf.n_cols + *col;
    return cell < gf.n_cells ? (int)cell : -1;
}

// grid (z.tiles, n_sets), kLocateThreads threads.  Q: [set][pair][n]; table: the fine table [station][gf.n_cells]; gf: the
// coarse run's geometry with the fine table's n_cells and n_cols.  S_T and CLK are k_locate_scores' (the family's one
// station-count table instantiates both kernels).  best[set]: the location's coarse cell, -1 where there is none: then every
// position's word is -1 and the tiles have no candidate.
// zmap[set][pos] = score_q(fine cell of pos), -1 where pos does not compete; partial[set * z.tiles + tile] = the tile's best
// candidate (equal scores: the smaller fine cell).
template <int S_T, bool CLK>
__global__ __launch_bounds__(kLocateThreads) void k_locate_zoom_scores(const long long *Q, LocateGeom gf, LocateZoomGeom z,
                                                                       const int32_t *table, const long long *__restrict__ cdiff,
                                                                       const int32_t *best, long long *zmap, ClosureCand *partial)
{
    __shared__ long long red_s[kLocateThreads / kWave];
    __shared__ uint32_t red_k[kLocateThreads / kWave];
    const int set = blockIdx.y, t = threadIdx.x;
    const int pos = (int)blockIdx.x * kLocateThreads + t, b = locate_zoom_centre(z, best[set]);
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
            s = 0;
            if constexpr (S_T > 0) {
                int32_t d[S_T];
#pragma unroll
                for (int i = 0; i < S_T; i++) d[i] = tc[(size_t)i * gf.n_cells];
#pragma unroll
                for (int i = 0; i < S_T; i++)
#pragma unroll
                    for (int j = i + 1; j < S_T; j++, q += gf.n) {
                        long long c = 0;
                        if constexpr (CLK) c = *cd++;
                        s += locate_m(q, d[i], d[j], gf, c);
                    }
            } else {
                for (int i = 0; i < gf.S; i++) {
                    const int32_t di = tc[(size_t)i * gf.n_cells];
                    for (int j = i + 1; j < gf.S; j++, q += gf.n) {
                        long long c = 0;
                        if constexpr (CLK) c = *cd++;
                        s += locate_m(q, di, tc[(size_t)j * gf.n_cells], gf, c);
                    }
                }
            }
            bs = s;
            bk = ~(uint32_t)cell;
        }
        zmap[(size_t)set * z.n_pos + pos] = s;
    }
    closure_block_best(bs, bk, red_s, red_k);
    if (t == 0) partial[(size_t)set * z.tiles + blockIdx.x] = ClosureCand{bs, bk, 0};
}

// One workgroup per set, kLocateThreads threads.  The tiles' candidates -> the zoom's cell (the largest score, equal scores: the
// smaller fine cell).  A largest score of 0, no competing position or no location: the zero record, zero lags and correlations.
// Otherwise one pass over the set's window on zmap: n_best and the box of the positions with exactly score_q, and the runner-up,
// the best position with max(|row - row_z|, |col - col_z|) > gf.sep (fine_separation), by the same order; then per pair
// lag_p(cell) and the signed C there (0 and 0.0 for a pair outside the range) and pairs_in.  roots[set] = sqrt(n_w); cdiff: the
// pairs' clock differences [set][pair], nullptr: none.
__global__ __launch_bounds__(kLocateThreads) void k_locate_zoom_finish(const long long *Q, LocateGeom gf, LocateZoomGeom z,
                                                                       const int32_t *table, const long long *cdiff,
                                                                       const double *roots, const int32_t *best, const long long *zmap,
                                                                       const ClosureCand *partial, LocateZoomOut *out, int32_t *lags,
                                                                       double *corr)
{
    constexpr int kWaves = kLocateThreads / kWave;
    __shared__ long long red_s[kWaves];
    __shared__ uint32_t red_k[kWaves];
    __shared__ int red_n[kWaves], red_in[kWaves], red_box[4][kWaves];
    const int set = blockIdx.x, t = threadIdx.x, b = locate_zoom_centre(z, best[set]);
    long long bs;
    uint32_t bk;
    search_best_candidate(partial + (size_t)set * z.tiles, z.tiles, red_s, red_k, bs, bk);
    const double root = roots[set];
    const int cell = (int)~bk;
    const bool found = b >= 0 && bs > 0 && cell >= 0 && cell < gf.n_cells;      // (uniform over the workgroup)
    // the window: the count and box of the best score, the runner-up
    long long rs = kClosureAbsent;
    uint32_t rk = 0;
    int n_best = 0, row_lo = INT_MAX, row_hi = INT_MIN, col_lo = INT_MAX, col_hi = INT_MIN;
    if (found) {
        const int row_z = cell / gf.n_cols, col_z = cell % gf.n_cols;
        const long long *zm = zmap + (size_t)set * z.n_pos;
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
    int inside = 0;
    for (int p = t; p < gf.P; p += kLocateThreads) {
        int32_t lag = 0;
        double c = 0.0;
        if (found && locate_pair_value(q, gf, table, cdiff ? cdiff + (size_t)set * gf.P : nullptr, cell, p, root, &lag, &c)) inside++;
        lags[(size_t)set * gf.P + p] = lag;
        corr[(size_t)set * gf.P + p] = c;
    }
    n_best = search_wave_sum(n_best);
    inside = search_wave_sum(inside);
    row_lo = search_wave_min(row_lo);
    row_hi = search_wave_max(row_hi);
    col_lo = search_wave_min(col_lo);
    col_hi = search_wave_max(col_hi);
    if ((t & (kWave - 1)) == 0) {
        const int w = t / kWave;
        red_n[w] = n_best;
        red_in[w] = inside;
        red_box[0][w] = row_lo;
        red_box[1][w] = row_hi;
        red_box[2][w] = col_lo;
        red_box[3][w] = col_hi;
    }
    __syncthreads();
    if (t != 0) return;
    LocateZoomOut rec{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0};
    if (found) {
        rec.cell = cell;
        rec.row_lo = red_box[0][0];
        rec.row_hi = red_box[1][0];
        rec.col_lo = red_box[2][0];
        rec.col_hi = red_box[3][0];
        for (int w = 0; w < kWaves; w++) {
            rec.n_best += red_n[w];
            rec.pairs_in += red_in[w];
            rec.row_lo = min(rec.row_lo, red_box[0][w]);
            rec.row_hi = max(rec.row_hi, red_box[1][w]);
            rec.col_lo = min(rec.col_lo, red_box[2][w]);
            rec.col_hi = max(rec.col_hi, red_box[3][w]);
        }
        rec.score_q = bs;
        rec.score = stack_value(bs, root);
        const int runner = (int)~rk;
        if (rs >= 0 && runner >= 0 && runner < gf.n_cells) {
            rec.runner_cell = runner;
            rec.runner_q = rs;
            rec.runner_up = stack_value(rs, root);
        }
    }
    out[set] = rec;
}

}  // namespace tdoa
