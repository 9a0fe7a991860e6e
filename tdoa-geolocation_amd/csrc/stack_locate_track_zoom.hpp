// stack_locate_track_zoom.hpp -- tdoa_process_locate_track_zoom: behind the cell tracks (stack_cell_track.hpp), every track is
// followed again on the fine table (include/tdoa_mi355x.h, "zoomed cell tracks").  Position j of a track has the zoom's window
// (stack_locate_zoom.hpp) around the track's coarse cell C_j; the windows' origins differ from stack to stack by
// Z (C_{j+1} - C_j), which the recurrence reads from device memory: the centres are data, so one captured graph serves every
// block, every table and every clock table of the same shape.
//
// k_track_zoom_centres   ctrack_cells and the tracks' records -> centre[set], -1 for the sets of a track with the zero record
// (k_locate_zoom_scores  as it stands, with centre for best: w_j into the window maps)
// k_track_zoom_steps     one workgroup per track, one launch: F_{j+1} stays in LDS as int64 over j = L - 2 .. 0, a row maximum
//                        followed by a column maximum, E_j out to memory, F_0 out as ztotal
// k_track_zoom_finish    one workgroup per track: the best F_0, the walk through E, the runner-up, the positions' lags and
//                        correlations (locate_pair_value), the record
//
// Everything is integer arithmetic on the window maps' words; the only floating point is stack_value on the way out.
#pragma once

#include "stack_cell_track.hpp"
#include "stack_locate_zoom.hpp"

namespace tdoa {

constexpr int kTrackZoomMaxStep = 16;                           // the largest fine_step
constexpr int kTrackZoomThreads = 1024;                         // k_track_zoom_steps: 16 waves, a wave per row of the plane
constexpr int kTrackZoomWaves = kTrackZoomThreads / kWave;
constexpr int kTrackZoomMaxSide = 2 * kLocateZoomMaxH + 1;

// k_track_zoom_steps' instantiations: a wave owns the rows wave, wave + 16 ... (ROWS of them: side <= ROWS x 16) and a lane the
// columns lane, lane + 64 ... of each (COLS: side <= COLS x 64).  `launch` is called with std::integral_constant<int, ROWS> and
// <int, COLS> for the smallest that holds the window: a small one pays for no more registers or guards than it needs.
template <class Launch> void track_zoom_steps_dispatch(int side, Launch &&launch)
{
    using std::integral_constant;
    if (side <= 2 * kTrackZoomWaves)
        launch(integral_constant<int, 2>{}, integral_constant<int, 1>{});                    // H <= 15
    else if (side <= 4 * kTrackZoomWaves)
        launch(integral_constant<int, 4>{}, integral_constant<int, 1>{});                    // H <= 31
    else if (side <= 6 * kTrackZoomWaves)
        launch(integral_constant<int, 6>{}, integral_constant<int, 2>{});                    // H <= 47
    else
        launch(integral_constant<int, 9>{}, integral_constant<int, 3>{});                    // H <= 64
}
static_assert(9 * kTrackZoomWaves >= kTrackZoomMaxSide && 3 * kWave >= kTrackZoomMaxSide, "the largest window");
static_assert(4 * kTrackZoomWaves <= kWave && 6 * kTrackZoomWaves <= 2 * kWave, "a case's rows fit its columns");

struct TrackZoomGeom {
    int32_t L, Jf;             // positions of a track, fine_step
    int32_t n_sets;
};

// LDS of k_track_zoom_steps: the plane F [n_pos] int64 and the row maxima's dc [n_pos] int8
__host__ __device__ constexpr size_t track_zoom_lds_bytes(int n_pos) { return (size_t)n_pos * 8 + (((size_t)n_pos + 7) & ~(size_t)7); }
static_assert(track_zoom_lds_bytes(kTrackZoomMaxSide * kTrackZoomMaxSide) <= 160 * 1024, "the largest window's plane fits a CU's 160 KB");

// grid ceil(n_sets / kLocateThreads).  cells: the coarse tracks' cells [set]; out: their records [track].
__global__ __launch_bounds__(kLocateThreads) void k_track_zoom_centres(TrackZoomGeom g, const int32_t *cells, const CellTrackOut *out, int32_t *centre)
{
    const int set = (int)blockIdx.x * kLocateThreads + (int)threadIdx.x;
    if (set >= g.n_sets) return;
    centre[set] = out[set / g.L].score_q > 0 ? cells[set] : -1;
}

// window j + 1's origin minus window j's, in fine rows and columns (centres that are cells of the coarse table)
__device__ __forceinline__ void track_zoom_offset(const LocateZoomGeom &z, int c0, int c1, int *orow, int *ocol)
{
    *orow = z.Z * (c1 / z.coarse_cols - c0 / z.coarse_cols);
    *ocol = z.Z * (c1 % z.coarse_cols - c0 % z.coarse_cols);
}

// word i of n words `pitch` apart, -1 for an i outside 0 .. n - 1: the load is from a clamped index and the test a select, so the
// scans below have no branch in them and their loads go out back to back
__device__ __forceinline__ long long track_zoom_word(const long long *p, int i, int n, int pitch)
{
    const long long v = p[min(max(i, 0), n - 1) * pitch];
    return i >= 0 && i < n ? v : -1;
}

// grid n_tracks, kTrackZoomThreads threads, track_zoom_lds_bytes(z.n_pos) of LDS.  zmap: the window maps [set][n_pos] (w_j);
// centre: [set].  The plane in LDS holds F_{j+1} in window j + 1's coordinates.  Per position j = L - 2 .. 0:
//   rows     a wave owns whole rows of the plane.  For row a' of window j + 1 and every column wb of window j, the maximum over
//            dc = 0, +1, -1 ... of F_{j+1}[a'][wb + dc - ocol] with a strict >, a column outside the window as -1, and that
//            dc; a lane holds its words of the row in registers until the whole wave has read, then the maxima replace the row.
//   columns  for every position (wa, wb) of window j the maximum of those over dr = 0, +1, -1 ... (row wa + dr - orow, outside
//            the window: -1) with a strict >: the order (rank(dr), rank(dc)) of the direct scan.  A -1 never replaces
//            anything, so it does not count; a maximum of -1 is no continuation: F_j = -1, E_j = (0, 0).  A thread holds the
//            F_j of its positions in registers until the workgroup has read the plane, then they replace it.
// Lanes lie along a row in both passes: an LDS access of a half-wave covers 32 consecutive words.
// E: [set][n_pos][2] int8 (dr, dc), written for j < L - 1; total[track][n_pos] = F_0.  A track whose centres are -1: total -1
// throughout (its window maps are), E is not written and not read.
template <int ROWS, int COLS>
__global__ __launch_bounds__(kTrackZoomThreads) void k_track_zoom_steps(LocateZoomGeom z, TrackZoomGeom g, const int32_t *centre,
                                                                        const long long *zmap, signed char *E, long long *total)
{
    extern __shared__ long long tz_lds[];
    long long *F = tz_lds;
    signed char *hd = reinterpret_cast<signed char *>(F + z.n_pos);
    const int track = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const size_t set0 = (size_t)track * g.L;
    const int side = z.side, n_pos = z.n_pos, Jf = g.Jf;
    long long *tot = total + (size_t)track * n_pos;
    if (locate_zoom_centre(z, centre[set0]) < 0) {
        for (int pos = t; pos < n_pos; pos += kTrackZoomThreads) tot[pos] = -1;
        return;
    }
    {
        const long long *w = zmap + (set0 + g.L - 1) * n_pos;
        for (int pos = t; pos < n_pos; pos += kTrackZoomThreads) F[pos] = w[pos];
    }
    for (int j = g.L - 2; j >= 0; j--) {
        int orow, ocol;
        track_zoom_offset(z, centre[set0 + j], centre[set0 + j + 1], &orow, &ocol);      // (uniform: the scalar cache)
        __syncthreads();
        for (int r = wave; r < side; r += kTrackZoomWaves) {
            long long *row = F + r * side;
            long long b[COLS];
            int d[COLS];
#pragma unroll
            for (int k = 0; k < COLS; k++) {
                const int wb = lane + k * kWave, c0 = wb - ocol;
                b[k] = -1;
                d[k] = 0;
                if (wb >= side) continue;
                b[k] = track_zoom_word(row, c0, side, 1);
#pragma unroll 4
                for (int s = 1; s <= Jf; s++) {
                    long long c = track_zoom_word(row, c0 + s, side, 1);
                    if (c > b[k]) { b[k] = c; d[k] = s; }
                    c = track_zoom_word(row, c0 - s, side, 1);
                    if (c > b[k]) { b[k] = c; d[k] = -s; }
                }
            }
#pragma unroll
            for (int k = 0; k < COLS; k++) {               // (every lane of the row's wave has read by now)
                const int wb = lane + k * kWave;
                if (wb >= side) continue;
                row[wb] = b[k];
                hd[r * side + wb] = (signed char)d[k];
            }
        }
        __syncthreads();
        const long long *w = zmap + (set0 + j) * n_pos;
        signed char *e = E + (set0 + j) * n_pos * 2;
        long long f[ROWS][COLS];
        int wave_j = wave, lane_j = lane;
        asm volatile("" : "+v"(wave_j), "+v"(lane_j));                  // (a position's offsets are made where they are used, in every
                                                                         // j: held over the loop they cost more registers than the F_j)
#pragma unroll
        for (int m = 0; m < ROWS; m++) {
            const int wa = wave_j + m * kTrackZoomWaves, a0 = wa - orow;
#pragma unroll
            for (int k = 0; k < COLS; k++) {
                const int wb = lane_j + k * kWave;
                f[m][k] = -1;
                if (wa >= side || wb >= side) continue;
                int dr = 0;
                long long b = track_zoom_word(F + wb, a0, side, side);
#pragma unroll 4
                for (int s = 1; s <= Jf; s++) {
                    long long c = track_zoom_word(F + wb, a0 + s, side, side);
                    if (c > b) { b = c; dr = s; }
                    c = track_zoom_word(F + wb, a0 - s, side, side);
                    if (c > b) { b = c; dr = -s; }
                }
                const int pos = wa * side + wb;
                const long long own = w[pos];
                signed char dc = 0;
                if (b >= 0) dc = hd[(a0 + dr) * side + wb];              // (b >= 0: row a0 + dr is inside the window)
                else dr = 0;
                *reinterpret_cast<char2 *>(e + (size_t)pos * 2) = make_char2((signed char)dr, dc);
                if (own >= 0 && b >= 0) f[m][k] = own + b;
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < ROWS; m++)
#pragma unroll
            for (int k = 0; k < COLS; k++) {
                const int wa = wave + m * kTrackZoomWaves, wb = lane + k * kWave;
                if (wa < side && wb < side) F[wa * side + wb] = f[m][k];
            }
    }
    __syncthreads();
    for (int pos = t; pos < n_pos; pos += kTrackZoomThreads) tot[pos] = F[pos];
}

// One workgroup per track, kLocateThreads threads.  gf: the coarse run's geometry with the fine table's shape and
// fine_separation; table: the fine table; Q, cdiff, roots as the zoom's finish takes them; track_roots[track] = sqrt(N_w).
// The best F_0 (equal maxima: the smaller fine cell) is f_0; thread 0 walks f_{j+1} = f_j + E_j[f_j] and writes cells[j], own[j]
// = w_j[f_j] and the steps; the runner-up is the best F_0 >= 0 with max(|row - row_0|, |col - col_0|) > gf.sep, by the same
// order; then per position and pair lag_p(f_j) and the signed C there on the stack's own scale.  A track without centres or
// with a largest F_0 <= 0: the zero record, every per-position output 0.
__global__ __launch_bounds__(kLocateThreads) void k_track_zoom_finish(const long long *Q, LocateGeom gf, LocateZoomGeom z, TrackZoomGeom g,
                                                                      const int32_t *table, const long long *cdiff, const double *roots,
                                                                      const double *track_roots, const int32_t *centre,
                                                                      const long long *zmap, const signed char *E, const long long *total,
                                                                      CellTrackOut *out, int32_t *cells, long long *own, int32_t *lags,
                                                                      double *corr)
{
    __shared__ long long red_s[kLocateThreads / kWave];
    __shared__ uint32_t red_k[kLocateThreads / kWave];
    __shared__ int32_t path[kCellTrackMaxLen];
    __shared__ int steps_s;
    const int track = blockIdx.x, t = threadIdx.x;
    const size_t set0 = (size_t)track * g.L;
    const int b0 = locate_zoom_centre(z, centre[set0]);
    const long long *tot = total + (size_t)track * z.n_pos;
    long long bs = kClosureAbsent;
    uint32_t bk = 0;
    if (b0 >= 0)
        for (int pos = t; pos < z.n_pos; pos += kLocateThreads) {
            int row, col;
            const int c = locate_zoom_cell(z, gf, b0, pos, &row, &col);
            const long long s = tot[pos];
            if (c >= 0 && s >= 0 && closure_better(s, ~(uint32_t)c, bs, bk)) {
                bs = s;
                bk = ~(uint32_t)c;
            }
        }
    closure_block_best(bs, bk, red_s, red_k);
    const int cell = (int)~bk;
    const bool found = b0 >= 0 && bs > 0 && cell >= 0 && cell < gf.n_cells;       // (uniform over the workgroup)
    const int row_0 = found ? cell / gf.n_cols : 0, col_0 = found ? cell % gf.n_cols : 0;
    // the runner-up
    long long rs = kClosureAbsent;
    uint32_t rk = 0;
    if (found)
        for (int pos = t; pos < z.n_pos; pos += kLocateThreads) {
            int row, col;
            const int c = locate_zoom_cell(z, gf, b0, pos, &row, &col);
            const long long s = tot[pos];
            if (c >= 0 && s >= 0 && max(abs(row - row_0), abs(col - col_0)) > gf.sep && closure_better(s, ~(uint32_t)c, rs, rk)) {
                rs = s;
                rk = ~(uint32_t)c;
            }
        }
    closure_block_best(rs, rk, red_s, red_k);
    // the walk
    if (!found) {
        for (int j = t; j < g.L; j += kLocateThreads) {
            cells[set0 + j] = 0;
            own[set0 + j] = 0;
        }
    } else if (t == 0) {
        int wa = row_0 - (z.Z * (b0 / z.coarse_cols) - z.H), wb = col_0 - (z.Z * (b0 % z.coarse_cols) - z.H), c = cell, steps = 0;
        for (int j = 0; j < g.L; j++) {
            const size_t at = (set0 + j) * z.n_pos + (size_t)(wa * z.side + wb);
            path[j] = c;
            cells[set0 + j] = c;
            own[set0 + j] = zmap[at];
            if (j + 1 == g.L) break;
            const int b1 = locate_zoom_centre(z, centre[set0 + j + 1]);
            if (b1 < 0) continue;                                    // (a track with centres has all of them)
            int orow, ocol, row, col;
            track_zoom_offset(z, centre[set0 + j], b1, &orow, &ocol);
            const int na = wa + E[at * 2] - orow, nb = wb + E[at * 2 + 1] - ocol;
            if (na < 0 || na >= z.side || nb < 0 || nb >= z.side) continue;      // (E_j of a position with F_j >= 0 names one inside window j + 1)
            const int next = locate_zoom_cell(z, gf, b1, na * z.side + nb, &row, &col);
            if (next < 0) continue;
            wa = na;
            wb = nb;
            if (next != c) steps++;
            c = next;
        }
        steps_s = steps;
    }
    __syncthreads();
    for (int e = t; e < g.L * gf.P; e += kLocateThreads) {
        const int j = e / gf.P, p = e % gf.P;
        const size_t set = set0 + j;
        int32_t lag = 0;
        double c = 0.0;
        if (found) locate_pair_value(Q + set * gf.P * gf.n, gf, table, cdiff ? cdiff + set * gf.P : nullptr, path[j], p, roots[set], &lag, &c);
        lags[set * gf.P + p] = lag;
        corr[set * gf.P + p] = c;
    }
    if (t != 0) return;
    CellTrackOut rec{0, 0, 0, 0, 0, 0, 0.0, 0.0};
    if (found) {
        const double root = track_roots[track];
        rec.cell = cell;
        rec.positions = g.L;
        rec.steps = steps_s;
        rec.score_q = bs;
        rec.score = stack_value(bs, root);
        const int runner = (int)~rk;
        if (rs >= 0 && runner >= 0 && runner < gf.n_cells) {
            rec.runner_cell = runner;
            rec.runner_q = rs;
            rec.runner_up = stack_value(rs, root);
        }
    }
    out[track] = rec;
}

}  // namespace tdoa
