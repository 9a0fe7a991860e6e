// locate_track_multi_api.inc -- several emitters per block, host side: the rounds' buffers, the kernels' launches (shared by a
// context's own step, step_products.inc, the group's merged sum and tdoa_debug_locate_track_multi_from_q) and the checks the
// entries share.  Round 0 is launch_locate and launch_locate_track (locate_api.inc, locate_track_api.inc) as they stand; the
// rounds' records, cells, own scores, counts, lags and correlations are [round] planes of the cell tracks' and the search's
// own buffers, round 0 on plane 0.
// What a round keeps and what it shares (L = the stacks of a track):
//   maps  L > 1: one plane [stack][cell], every round's scores overwrite it (a round's finish has read it by then);
//         L = 1: K planes, because a track of one stack never leaves its map and T_0 of every round goes to the caller
//   D     one plane, L > 1 only: a round's finish walks it before the next round's steps write it
//   T     L > 1 only: ctx->ctrack_t = [T_0 of round 0][the ping-pong's other half][T_0 of round 1] ... [T_0 of round K - 1]:
//         the first two are launch_locate_track's halves, and every later round steps between its own T_0 and the shared other
//         half, so that every round's T_0 is there for the download
// Included by tdoa_mi355x.hip after locate_track_api.inc and locate_multi_api.inc and before step_products.inc.

extern "C" {

// the arguments the three entries share; they need no device
static const char *check_locate_track_multi_args(int max_step, int n_emitters, int guard, int min_separation, const void *track)
{
    if (n_emitters < 1 || n_emitters > kLocateMaxEmitters) return "n_emitters outside 1 .. 8";
    if (guard < 0) return "guard < 0";
    return check_locate_track_args(max_step, min_separation, track);
}

// the buffers of K rounds for n_sets stacks in tracks of L (above); the larger ones first, so that the search's and the
// tracks' own ensure calls find them large enough
static int ensure_locate_track_multi(tdoa_ctx *ctx, size_t n_sets, int L, int K, const LocateGeom &g)
{
    int rc;
    const size_t n_tracks = n_sets / L, map_planes = L > 1 ? 1 : (size_t)K;
    if (ensure(ctx, ctx->locate_map, sizeof(long long) * map_planes * n_sets * g.n_cells) ||
        (L > 1 && ensure(ctx, ctx->ctrack_t, sizeof(long long) * (size_t)(K + 1) * n_tracks * g.n_cells))) {
        char buf[320];
        snprintf(buf, sizeof(buf),
                 "the rounds' maps [%zu][%zu stacks][%d cells] (%.1f MB) and the tracks' sums [%d rounds + 1][%zu tracks][%d cells] (%.1f MB) "
                 "do not fit in device memory: %s",
                 map_planes, n_sets, (int)g.n_cells, 8.0 * (double)map_planes * (double)n_sets * g.n_cells / 1e6, K, n_tracks,
                 (int)g.n_cells, L > 1 ? 8.0 * (double)(K + 1) * (double)n_tracks * g.n_cells / 1e6 : 0.0, ctx->last_error.c_str());
        return fail(ctx, TDOA_ERR_NOMEM, buf);
    }
    if ((rc = ensure(ctx, ctx->locate_lags, sizeof(int32_t) * K * n_sets * g.P))) return rc;
    if ((rc = ensure(ctx, ctx->locate_corr, sizeof(double) * K * n_sets * g.P))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_out, sizeof(CellTrackOut) * K * n_tracks))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_cells, sizeof(int32_t) * K * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_own, sizeof(long long) * K * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_pairs, 2 * sizeof(int32_t) * K * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->locate_centres, sizeof(LocateCentres) * n_sets * g.P))) return rc;
    if ((rc = ensure_locate(ctx, n_sets, g))) return rc;
    if ((rc = ensure_locate_track(ctx, n_sets, L, g))) return rc;
    return ensure_map_stats(ctx, K * n_tracks);
}

// T_0 of round r's tracks (above)
static const long long *locate_track_multi_total(const tdoa_ctx *ctx, size_t n_sets, int L, int r, const LocateGeom &g)
{
    if (L == 1) return ctx->locate_map.as<const long long>() + (size_t)r * n_sets * g.n_cells;
    return ctx->ctrack_t.as<const long long>() + (size_t)(r == 0 ? 0 : r + 1) * (n_sets / L) * g.n_cells;
}

// Q [n_sets][P][n] -> K planes of the tracks' records, cells, own scores, counts, lags and correlations, and every round's
// T_0: the one place the rounds are launched.  Round 0 is the search and the track as they stand, then the centres its track
// gives; every later round is the masked scores, the recurrence, the masked finish and the runner-up's pass on the round's
// planes.  The tracks' roots are in ctx->ctrack_roots (upload_locate_track_roots).  Kernel launches only (the step graph
// captures them).
static void launch_locate_track_multi(tdoa_ctx *ctx, const long long *Q, const double *roots, int n_sets, int L, int J, int K, int guard,
                                      const LocateGeom &lg)
{
    launch_locate(ctx, Q, roots, n_sets, lg, false);
    launch_locate_track(ctx, Q, roots, n_sets, L, J, lg, false);
    hipStream_t st = ctx->stream;
    const CellTrackGeom g = cell_track_geom(lg, L, J);
    const unsigned n_tracks = (unsigned)(n_sets / L);
    const size_t half = (size_t)n_tracks * g.n_cells;
    auto *table = ctx->locate_table.as<const int32_t>();
    const long long *cdiff = ctx->clock_stacks ? ctx->locate_clock.as<const long long>() : nullptr;
    auto *D = ctx->ctrack_d.as<signed char>();
    auto *part = ctx->locate_part.as<ClosureCand>();
    auto *best = ctx->locate_best.as<int32_t>();
    auto *centres = ctx->locate_centres.as<LocateCentres>();
    const double *track_roots = ctx->ctrack_roots.as<const double>();
    const dim3 sgrid((unsigned)lg.tiles, (unsigned)n_sets), sets((unsigned)n_sets), tgrid((unsigned)lg.tiles, n_tracks), one(n_tracks);
    hipLaunchKernelGGL(k_track_centres, sets, dim3(kLocateThreads), 0, st, lg, L, table, cdiff, static_cast<const int32_t *>(best),
                       ctx->ctrack_cells.as<const int32_t>(), centres, ctx->ctrack_pairs.as<int32_t>());
    const int rows = (int)(((long long)g.n_cells + g.n_cols - 1) / g.n_cols);
    const dim3 tiles((unsigned)g.tiles_x * (unsigned)((rows + kCellTrackH - 1) / kCellTrackH), n_tracks);
    for (int r = 1; r < K; r++) {
        const LocateMask mk = locate_mask(r, guard, lg);
        auto *map = ctx->locate_map.as<long long>() + (L > 1 ? 0 : (size_t)r * n_sets * g.n_cells);
        auto *t0 = const_cast<long long *>(locate_track_multi_total(ctx, n_sets, L, r, lg));
        auto *other = ctx->ctrack_t.as<long long>() + half;
        auto *out = ctx->ctrack_out.as<CellTrackOut>() + (size_t)r * n_tracks;
        auto *cells = ctx->ctrack_cells.as<int32_t>() + (size_t)r * n_sets;
        auto *own = ctx->ctrack_own.as<long long>() + (size_t)r * n_sets;
        auto *pairs = ctx->ctrack_pairs.as<int32_t>() + 2 * (size_t)r * n_sets;
        auto *lags = ctx->locate_lags.as<int32_t>() + (size_t)r * n_sets * lg.P;
        auto *corr = ctx->locate_corr.as<double>() + (size_t)r * n_sets * lg.P;
        switch (lg.S <= kLocateMaskedRegStations ? lg.S : 0) {
#define TDOA_LOCATE_CASE(s)                                                                                                      \
    case s:                                                                                                                      \
        if (cdiff)                                                                                                               \
            hipLaunchKernelGGL((k_locate_scores_masked<s, true>), sgrid, dim3(kLocateThreads), 0, st, Q, lg, table, cdiff,       \
                               static_cast<const LocateCentres *>(centres), mk, map, part);                                      \
        else                                                                                                                     \
            hipLaunchKernelGGL((k_locate_scores_masked<s, false>), sgrid, dim3(kLocateThreads), 0, st, Q, lg, table, cdiff,      \
                               static_cast<const LocateCentres *>(centres), mk, map, part);                                      \
        break;
        TDOA_LOCATE_CASE(2) TDOA_LOCATE_CASE(3) TDOA_LOCATE_CASE(4) TDOA_LOCATE_CASE(5) TDOA_LOCATE_CASE(6) TDOA_LOCATE_CASE(7)
        TDOA_LOCATE_CASE(8) TDOA_LOCATE_CASE(9) TDOA_LOCATE_CASE(10) TDOA_LOCATE_CASE(11) TDOA_LOCATE_CASE(12) TDOA_LOCATE_CASE(13)
        TDOA_LOCATE_CASE(14) TDOA_LOCATE_CASE(15)
        default:
            TDOA_LOCATE_CASE(0)
        }
#undef TDOA_LOCATE_CASE
        for (int j = L - 2; j >= 0; j--) {
            // position L - 1 is the last stack's map as it stands; an even position writes the round's T_0, an odd one the other half
            const long long *t_in = j == L - 2 ? map + (size_t)(L - 1) * g.n_cells : ((j + 1) & 1) ? other : t0;
            const size_t in_stride = j == L - 2 ? (size_t)L * g.n_cells : (size_t)g.n_cells;
            hipLaunchKernelGGL(k_cell_track_step, tiles, dim3(kCellTrackThreads), cell_track_lds_bytes(J), st, t_in, in_stride,
                               static_cast<const long long *>(map), g, j, (j & 1) ? other : t0, D);
        }
        hipLaunchKernelGGL(k_cell_track_best, tgrid, dim3(kCellTrackThreads), 0, st, static_cast<const long long *>(t0), g.n_cells, part);
        hipLaunchKernelGGL(k_cell_track_finish_masked, one, dim3(kCellTrackThreads), 0, st, Q, lg, g, table, cdiff, roots, track_roots,
                           static_cast<const long long *>(map), static_cast<const signed char *>(D), static_cast<const ClosureCand *>(part),
                           mk, centres, best, out, cells, own, pairs, lags, corr);
        hipLaunchKernelGGL(k_locate_runner, tgrid, dim3(kLocateThreads), 0, st, static_cast<const long long *>(t0), lg,
                           static_cast<const int32_t *>(best), part);
        hipLaunchKernelGGL(k_cell_track_finish, one, dim3(kCellTrackThreads), 0, st, Q, lg, g, table, cdiff, roots, track_roots,
                           static_cast<const long long *>(map), static_cast<const signed char *>(D), static_cast<const ClosureCand *>(part), 1,
                           best, out, cells, own, lags, corr);
    }
    // the statistics of every round's T_0, in the records' order: K planes one behind the other for L = 1; otherwise round 0's
    // and then the K - 1 others' (none with K = 1), which lie behind the ping-pong's other half
    const size_t plane = (size_t)g.n_cells;
    if (L == 1) {
        launch_map_stats(ctx, locate_track_multi_total(ctx, n_sets, L, 0, lg), plane, K * (int)n_tracks, lg, ctx->ctrack_out.p, track_roots, (int)n_tracks);
    } else {
        launch_map_stats(ctx, locate_track_multi_total(ctx, n_sets, L, 0, lg), plane, (int)n_tracks, lg, ctx->ctrack_out.p, track_roots, (int)n_tracks);
        launch_map_stats(ctx, locate_track_multi_total(ctx, n_sets, L, 1, lg), plane, (K - 1) * (int)n_tracks, lg,
                         ctx->ctrack_out.as<CellTrackOut>() + n_tracks, track_roots, (int)n_tracks, (int)n_tracks);
    }
}

// the outputs to the host (all but track may be NULL): the K planes lie one behind the other, but for T_0 of L > 1, which
// comes round by round; asynchronous on ctx->stream
static int download_locate_track_multi(tdoa_ctx *ctx, size_t n_sets, int L, int K, const LocateGeom &g, tdoa_cell_track *track,
                                       int32_t *cells, int64_t *own, int32_t *pairs, int32_t *lags, double *corr, int64_t *total)
{
    hipStream_t st = ctx->stream;
    const size_t n_tracks = n_sets / L, plane = n_tracks * g.n_cells;
    HIPCHK(ctx, hipMemcpyAsync(track, ctx->ctrack_out.p, sizeof(CellTrackOut) * K * n_tracks, hipMemcpyDeviceToHost, st));
    if (cells) HIPCHK(ctx, hipMemcpyAsync(cells, ctx->ctrack_cells.p, sizeof(int32_t) * K * n_sets, hipMemcpyDeviceToHost, st));
    if (own) HIPCHK(ctx, hipMemcpyAsync(own, ctx->ctrack_own.p, sizeof(int64_t) * K * n_sets, hipMemcpyDeviceToHost, st));
    if (pairs) HIPCHK(ctx, hipMemcpyAsync(pairs, ctx->ctrack_pairs.p, 2 * sizeof(int32_t) * K * n_sets, hipMemcpyDeviceToHost, st));
    if (lags) HIPCHK(ctx, hipMemcpyAsync(lags, ctx->locate_lags.p, sizeof(int32_t) * K * n_sets * g.P, hipMemcpyDeviceToHost, st));
    if (corr) HIPCHK(ctx, hipMemcpyAsync(corr, ctx->locate_corr.p, sizeof(double) * K * n_sets * g.P, hipMemcpyDeviceToHost, st));
    if (total)
        for (int r = 0; r < K; r++)
            HIPCHK(ctx, hipMemcpyAsync(total + (size_t)r * plane, locate_track_multi_total(ctx, n_sets, L, r, g), sizeof(int64_t) * plane,
                                       hipMemcpyDeviceToHost, st));
    return download_map_stats(ctx, K * n_tracks);
}

// the rounds on a group's merged sum (finish_from_host, stacked_api.inc)
static int locate_track_multi_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack, int max_step, int K, int guard,
                                        int min_separation, tdoa_cell_track *track, int32_t *cells, int64_t *own, int32_t *pairs,
                                        int32_t *lags, double *corr, int64_t *total)
{
    const LocateGeom g = locate_geom(ctx, min_separation);
    int wpb = 0;
    if (int rc = tdoa_num_windows(ctx, &wpb, nullptr)) return fail(ctx, rc, "captures missing or too small");
    const int L = stack_geom(wpb, windows_per_stack).spb;
    const std::vector<double> track_roots = block_track_roots(wpb);          // (lives until finish_from_host has synchronised)
    return finish_from_host(
        ctx, q_sum, windows_per_stack,
        [&](int n_stacks, const double *roots) -> int {
            int rc;
            if ((rc = ensure_locate_track_multi(ctx, n_stacks, L, K, g))) return rc;
            if ((rc = upload_locate_track_roots(ctx, track_roots))) return rc;
            launch_locate_track_multi(ctx, ctx->stack_q.as<const long long>(), roots, n_stacks, L, max_step, K, guard, g);
            return TDOA_OK;
        },
        [&](int n_stacks) { return download_locate_track_multi(ctx, n_stacks, L, K, g, track, cells, own, pairs, lags, corr, total); });
}

}  // extern "C"
