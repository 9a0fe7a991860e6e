// stack_cell_track.hpp -- tdoa_process_locate_track: one cell per stack of a block, consecutive cells at most J rows and
// columns apart, chosen so that the sum of the stacks' delay-table scores along the track is largest
// (include/tdoa_mi355x.h, "cell tracks").  Dynamic programming over the maps the delay-table search leaves on the device
// (stack_locate.hpp, map[stack][cell] = s_j[cell], clocks applied), from the block's last stack back to its first:
//     T_j[c] = s_j[c] + max over |dr| <= J, |dc| <= J, (row + dr, col + dc) a cell, of T_{j+1}[that cell]     D_j[c] = that (dr, dc)
//
// k_cell_track_step    one launch per position j = L - 2 .. 0 (T_{L-1} is the last stack's map itself): T_{j+1} -> T_j, D_j
// k_cell_track_best    T_0 -> the tiles' best candidates (key = ~cell)
// k_cell_track_finish  the candidates -> L_0, the walk along D (cells, own scores, steps), the positions' lags and signed
//                      correlations, the record; after k_locate_runner's pass over T_0: runner_q, runner_up, runner_cell
//
// Everything is integer arithmetic on the map's words; the only floating point is stack_value on the way out.  The candidate,
// its order and the workgroup reduction are the closure search's (stack_closure.hpp), the absent word is the delay track's.
#pragma once

#include "stack_locate.hpp"
#include "stack_track.hpp"

namespace tdoa {

constexpr int kCellTrackThreads = 256;
constexpr int kCellTrackW = 64;                                 // a tile's columns: one wave's lanes lie along a row
constexpr int kCellTrackH = 16;                                 // a tile's rows
constexpr int kCellTrackMaxStep = 16;                           // the largest J: the halo on every side of a tile
constexpr int kCellTrackMaxLen = 4096;                          // the largest L: the finish keeps a track's cells in LDS
static_assert(kCellTrackW == kWave, "a lane per column of the tile");
static_assert(kCellTrackThreads == kLocateThreads, "closure_block_best reduces kClosureThreads candidates");

// tdoa_cell_track
struct CellTrackOut {
    int32_t cell, runner_cell, positions, steps;
    long long score_q, runner_q;
    double score, runner_up;
};

struct CellTrackGeom {
    int32_t n_cells, n_cols;   // the table's cells; cell c lies at row c div n_cols, column c mod n_cols
    int32_t tiles_x;           // ceil(n_cols / kCellTrackW); the grid's x is tiles_x * ceil(rows / kCellTrackH)
    int32_t L, J;              // positions of a track, the largest step
};

// LDS of k_cell_track_step: T_{j+1} of the tile and its halo (the rows' maxima take their place), and the maxima's dc
__host__ __device__ constexpr size_t cell_track_lds_bytes(int J)
{
    return (size_t)(kCellTrackH + 2 * J) * ((size_t)(kCellTrackW + 2 * J) * 8 + (size_t)kCellTrackW);
}
static_assert(cell_track_lds_bytes(kCellTrackMaxStep) <= 65536, "the largest halo fits the 64 KB a launch may ask for");

// grid (tiles, n_tracks), kCellTrackThreads threads, cell_track_lds_bytes(J) of LDS; one launch per position j = L - 2 .. 0.
// The workgroup owns kCellTrackH x kCellTrackW cells of one track at position j.
//   stage   T_{j+1} of those cells and of J more rows and columns on every side, as int64, a neighbour that does not exist
//           (row < 0, column outside 0 .. n_cols - 1, index >= n_cells) as kTrackAbsent.  A wave stages whole rows, its
//           lanes consecutive columns.
//   rows    for every staged row and every column of the tile, the maximum over dc = 0, +1, -1, +2 ... with a strict >, and
//           that dc: the smaller rank(dc) of equal maxima.  A row belongs to one wave, which has read all of it before it
//           writes, so the maxima go back into the row, at the tile's columns.
//   columns for every cell the maximum of those over dr = 0, +1, -1 ... with a strict >: the smaller rank(dr), and within
//           that row the smaller rank(dc) -- the order of the direct scan over (dr, dc).  (0, 0) exists for every cell, so an
//           absent word never wins.
// Every LDS read and write of a half-wave covers 32 consecutive 8-byte words of one row: all 64 banks once, whatever the
// rows' pitch, so the staged rows need no padding.
// t_in: T_{j+1}, track t at t * in_stride (the first launch reads the maps of the blocks' last stacks, in_stride = L n_cells;
// the others the ping-pong's other half, in_stride = n_cells); map: [track * L + position][n_cells]; t_out: [track][n_cells];
// D: [track * L + position][n_cells][2] int8 (dr, dc).
__global__ __launch_bounds__(kCellTrackThreads) void k_cell_track_step(const long long *t_in, size_t in_stride, const long long *map,
                                                                       CellTrackGeom g, int j, long long *t_out, signed char *D)
{
    extern __shared__ long long ct_lds[];
    const int J = g.J, pitch = kCellTrackW + 2 * J, rows = kCellTrackH + 2 * J;
    long long *st = ct_lds;                                      // [rows][pitch]: T_{j+1}, then the rows' maxima at columns J .. J + 63
    signed char *hd = reinterpret_cast<signed char *>(st + (size_t)rows * pitch);      // [rows][kCellTrackW]
    const int track = blockIdx.y, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int row0 = ((int)blockIdx.x / g.tiles_x) * kCellTrackH, col0 = ((int)blockIdx.x % g.tiles_x) * kCellTrackW;
    const long long *src = t_in + (size_t)track * in_stride;
    for (int r = wave; r < rows; r += kCellTrackThreads / kWave) {
        const long long row = (long long)row0 - J + r;
        for (int c = lane; c < pitch; c += kWave) {
            const int col = col0 - J + c;
            const long long cell = row * g.n_cols + col;
            long long v = kTrackAbsent;
            if (row >= 0 && col >= 0 && col < g.n_cols && cell < g.n_cells) v = src[cell];
            st[r * pitch + c] = v;
        }
    }
    __syncthreads();
    for (int r = wave; r < rows; r += kCellTrackThreads / kWave) {
        long long *w = st + r * pitch + J + lane;
        long long b = w[0];
        int d = 0;
#pragma unroll 4
        for (int k = 1; k <= J; k++) {
            long long c = w[k];
            if (c > b) { b = c; d = k; }
            c = w[-k];
            if (c > b) { b = c; d = -k; }
        }
        w[0] = b;                                                // (every lane of the row's wave has read by now)
        hd[r * kCellTrackW + lane] = (signed char)d;
    }
    __syncthreads();
    const int col = col0 + lane;
    const size_t set = (size_t)track * g.L + j;
    for (int r = wave; r < kCellTrackH; r += kCellTrackThreads / kWave) {
        const long long cell = (long long)(row0 + r) * g.n_cols + col;
        if (col >= g.n_cols || cell >= g.n_cells) continue;
        const long long *w = st + (r + J) * pitch + J + lane;
        long long b = w[0];
        int dr = 0;
#pragma unroll 4
        for (int k = 1; k <= J; k++) {
            long long c = w[k * pitch];
            if (c > b) { b = c; dr = k; }
            c = w[-k * pitch];
            if (c > b) { b = c; dr = -k; }
        }
        t_out[(size_t)track * g.n_cells + cell] = map[set * g.n_cells + cell] + b;
        *reinterpret_cast<char2 *>(D + (set * g.n_cells + cell) * 2) = make_char2((signed char)dr, hd[(r + J + dr) * kCellTrackW + lane]);
    }
}

// grid (ceil(n_cells / kCellTrackThreads), n_tracks): every cell of T_0 competes; partial[track * tiles + tile] = the tile's
// best candidate (equal sums: the smaller cell), as k_locate_scores leaves them for k_locate_finish.
__global__ __launch_bounds__(kCellTrackThreads) void k_cell_track_best(const long long *t0, int n_cells, ClosureCand *partial)
{
    __shared__ long long red_s[kCellTrackThreads / kWave];
    __shared__ uint32_t red_k[kCellTrackThreads / kWave];
    const int cell = (int)blockIdx.x * kCellTrackThreads + (int)threadIdx.x;
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    if (cell < n_cells) {
        bs = t0[(size_t)blockIdx.y * n_cells + cell];
        bk = ~(uint32_t)cell;
    }
    closure_block_best(bs, bk, red_s, red_k);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ClosureCand{bs, bk, 0};
}

// The walk of both finishes' pass 0, for the track whose stacks are set0 .. set0 + L - 1.  Found, with L_0 = cell: thread 0
// walks L_{j+1} = L_j + D_j[L_j] and writes path[j] (LDS, for the per-position outputs), cells[j] and own[j] = s_j[L_j]; not
// found: cells and own 0.  Ends with a barrier; returns the number of steps in thread 0.
__device__ __forceinline__ int cell_track_walk(const CellTrackGeom &g, const long long *map, const signed char *D, size_t set0, bool found,
                                               int cell, int32_t *path, int32_t *cells, long long *own)
{
    const int t = threadIdx.x;
    int steps = 0;
    if (!found) {
        for (int j = t; j < g.L; j += kCellTrackThreads) {
            cells[set0 + j] = 0;
            own[set0 + j] = 0;
        }
    } else if (t == 0) {
        int c = cell;
        for (int j = 0; j < g.L; j++) {
            path[j] = c;
            cells[set0 + j] = c;
            own[set0 + j] = map[(set0 + j) * g.n_cells + c];
            if (j + 1 == g.L) break;
            const signed char *d = D + ((set0 + j) * g.n_cells + c) * 2;
            const long long next = (long long)c + (long long)d[0] * g.n_cols + d[1];
            if (next != c && next >= 0 && next < g.n_cells) {        // (D_j of a cell that exists names a cell that exists)
                c = (int)next;
                steps++;
            }
        }
    }
    __syncthreads();
    return steps;
}

// One workgroup per track.  lg: the search's geometry (its sets are the stacks, its tiles the candidates' per track); map
// and D as above; roots[stack] = sqrt(n_w), track_roots[track] = sqrt(N_w); cdiff: the pairs' clock differences
// [stack][pair], nullptr: none.
// pass 0 (partial holds k_cell_track_best's candidates): max T_0 and L_0 (equal maxima: the smaller cell); thread 0 walks
// L_{j+1} = L_j + D_j[L_j] and writes cells[j], own[j] = s_j[L_j] and the number of steps; then, per position and pair,
// lag_p(L_j) and the signed C there on the stack's own scale, as k_locate_finish writes them for its best cell; the record
// (the runner-up's fields 0) and best[track] = L_0.
// max T_0 = 0: the zero record, every per-position output 0, best = -1.
// pass 1 (partial holds k_locate_runner's pass over T_0): runner_q, runner_up and runner_cell of a record that is not the
// zero record, where a cell outside L_0's neighbourhood exists.
__global__ __launch_bounds__(kCellTrackThreads) void k_cell_track_finish(const long long *Q, LocateGeom lg, CellTrackGeom g,
                                                                         const int32_t *table, const long long *cdiff,
                                                                         const double *roots, const double *track_roots,
                                                                         const long long *map, const signed char *D,
                                                                         const ClosureCand *partial, int pass,
                                                                         int32_t *best, CellTrackOut *out, int32_t *cells,
                                                                         long long *own, int32_t *lags, double *corr)
{
    __shared__ long long red_s[kCellTrackThreads / kWave];
    __shared__ uint32_t red_k[kCellTrackThreads / kWave];
    __shared__ int32_t path[kCellTrackMaxLen];
    const int track = blockIdx.x, t = threadIdx.x;
    long long bs;
    uint32_t bk;
    search_best_candidate(partial + (size_t)track * lg.tiles, lg.tiles, red_s, red_k, bs, bk);
    const double root = track_roots[track];
    const int cell = (int)~bk;
    if (pass == 1) {
        if (t == 0 && out[track].score_q != 0 && bs >= 0 && cell >= 0 && cell < g.n_cells) {
            out[track].runner_q = bs;
            out[track].runner_up = stack_value(bs, root);
            out[track].runner_cell = cell;
        }
        return;
    }
    const bool found = bs > 0 && cell >= 0 && cell < g.n_cells;
    const size_t set0 = (size_t)track * g.L;
    const int steps = cell_track_walk(g, map, D, set0, found, cell, path, cells, own);
    for (int e = t; e < g.L * lg.P; e += kCellTrackThreads) {
        const int j = e / lg.P, p = e % lg.P;
        const size_t set = set0 + j;
        int32_t lag = 0;
        double c = 0.0;
        if (found) locate_pair_value(Q + set * lg.P * lg.n, lg, table, cdiff ? cdiff + set * lg.P : nullptr, path[j], p, roots[set], &lag, &c);
        lags[set * lg.P + p] = lag;
        corr[set * lg.P + p] = c;
    }
    if (t != 0) return;
    CellTrackOut rec{0, 0, 0, 0, 0, 0, 0.0, 0.0};
    if (found) {
        rec.cell = cell;
        rec.positions = g.L;
        rec.steps = steps;
        rec.score_q = bs;
        rec.score = stack_value(bs, root);
    }
    best[track] = found ? cell : -1;
    out[track] = rec;
}

}  // namespace tdoa
