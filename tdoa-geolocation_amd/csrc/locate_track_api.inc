// locate_track_api.inc -- cell tracks, host side: the recurrence's buffers, the kernels' launches (shared by a context's own
// step, step_products.inc, the group's merged sum and tdoa_debug_locate_track_from_q) and the checks the entries share.
// Everything runs behind launch_locate (locate_api.inc): the maps it leaves in ctx->locate_map are the recurrence's input.
// Included by tdoa_mi355x.hip after locate_api.inc and before step_products.inc.

extern "C" {

static CellTrackGeom cell_track_geom(const LocateGeom &lg, int L, int J)
{
    CellTrackGeom g;
    g.n_cells = lg.n_cells;
    g.n_cols = lg.n_cols;
    g.tiles_x = (std::min(lg.n_cols, lg.n_cells) + kCellTrackW - 1) / kCellTrackW;     // (a row holds at most n_cells cells)
    g.L = L;
    g.J = J;
    return g;
}

// the arguments the three entries share; they need no device
static const char *check_locate_track_args(int max_step, int min_separation, const void *track)
{
    if (max_step < 0 || max_step > kCellTrackMaxStep) return "max_step outside 0 .. 16";
    if (min_separation < 1) return "min_separation < 1";
    if (!track) return "track_host is NULL";
    return nullptr;
}

// what tdoa_process_locate_track and the group's call refuse beyond check_locate_state: a track's sum could overflow, too
// many positions.  *what receives the message.
static int check_locate_track_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what)
{
    if (const int rc = check_locate_state(ctx, windows_per_stack, what)) return rc;
    int wpb = 0;
    (void)tdoa_num_windows(ctx, &wpb, nullptr);              // (check_locate_state has seen it succeed)
    const int S = (int)ctx->caps.size();
    if (locate_overflows(S * (S - 1) / 2, wpb)) {
        *what = "pairs x windows per block > 2^17: a track's sum could overflow";
        return TDOA_ERR_UNSUPPORTED;
    }
    if (stack_geom(wpb, windows_per_stack).spb > kCellTrackMaxLen) {
        *what = "a track of more than 4096 stacks";
        return TDOA_ERR_UNSUPPORTED;
    }
    return TDOA_OK;
}

// the buffers of the recurrence for n_sets stacks in tracks of L, beside the search's own (ensure_locate): D, the two halves
// of T (a track of one stack has neither: T_0 is its map), the tracks' roots, records, cells and own scores
static int ensure_locate_track(tdoa_ctx *ctx, size_t n_sets, int L, const LocateGeom &g)
{
    int rc;
    const size_t n_tracks = n_sets / L;
    if (L > 1 && (ensure(ctx, ctx->ctrack_d, 2 * n_sets * g.n_cells) || ensure(ctx, ctx->ctrack_t, 2 * sizeof(long long) * n_tracks * g.n_cells))) {
        char buf[256];
        snprintf(buf, sizeof(buf),
                 "the cell tracks' steps [%zu stacks][%d cells] (%.1f MB) and sums [2][%zu tracks][%d cells] (%.1f MB) do not fit in device memory: %s",
                 n_sets, (int)g.n_cells, 2.0 * (double)n_sets * g.n_cells / 1e6, n_tracks, (int)g.n_cells,
                 16.0 * (double)n_tracks * g.n_cells / 1e6, ctx->last_error.c_str());
        return fail(ctx, TDOA_ERR_NOMEM, buf);
    }
    if ((rc = ensure(ctx, ctx->ctrack_roots, sizeof(double) * n_tracks))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_out, sizeof(CellTrackOut) * n_tracks))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_cells, sizeof(int32_t) * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_own, sizeof(long long) * n_sets))) return rc;
    return ensure_map_stats(ctx, n_tracks);
}

// sqrt(N_w) of every track to ctx->ctrack_roots; the caller synchronises before `roots` goes
static int upload_locate_track_roots(tdoa_ctx *ctx, const std::vector<double> &roots)
{
    HIPCHK(ctx, hipMemcpyAsync(ctx->ctrack_roots.p, roots.data(), sizeof(double) * roots.size(), hipMemcpyHostToDevice, ctx->stream));
    return TDOA_OK;
}

// T_0 of every track: a track of one stack never leaves its map; otherwise position 0 writes the ping-pong's first half
static const long long *locate_track_total(const tdoa_ctx *ctx, int L)
{
    return L > 1 ? ctx->ctrack_t.as<const long long>() : ctx->locate_map.as<const long long>();
}

// The maps launch_locate left for n_sets stacks -> the tracks' records in ctx->ctrack_out, cells, own scores, T_0, and the
// positions' lags and correlations where the search keeps its best cells' (ctx->locate_lags, ctx->locate_corr): the one
// place the recurrence is launched.  The search's candidates and best cells (ctx->locate_part, ctx->locate_best) are free by
// now and serve the tracks, which are never more than the stacks.  judged: T_0 is what the call judges (the rounds go on from
// here), so its statistics follow when the setting is on, on the tracks' own scale.  Kernel launches only (the step graph
// captures them).
static void launch_locate_track(tdoa_ctx *ctx, const long long *Q, const double *roots, int n_sets, int L, int J, const LocateGeom &lg,
                                bool judged = true)
{
    hipStream_t st = ctx->stream;
    const CellTrackGeom g = cell_track_geom(lg, L, J);
    const unsigned n_tracks = (unsigned)(n_sets / L);
    const size_t half = (size_t)n_tracks * g.n_cells;
    auto *map = ctx->locate_map.as<const long long>();
    auto *table = ctx->locate_table.as<const int32_t>();
    const long long *cdiff = ctx->clock_stacks ? ctx->locate_clock.as<const long long>() : nullptr;
    auto *D = ctx->ctrack_d.as<signed char>();
    auto *part = ctx->locate_part.as<ClosureCand>();
    auto *best = ctx->locate_best.as<int32_t>();
    const int rows = (int)(((long long)g.n_cells + g.n_cols - 1) / g.n_cols);
    const dim3 tiles((unsigned)g.tiles_x * (unsigned)((rows + kCellTrackH - 1) / kCellTrackH), n_tracks);
    for (int j = L - 2; j >= 0; j--) {
        // position L - 1 is the last stack's map as it stands; position j writes half j & 1 and reads the other
        const long long *t_in = j == L - 2 ? map + (size_t)(L - 1) * g.n_cells : ctx->ctrack_t.as<const long long>() + (size_t)((j + 1) & 1) * half;
        const size_t in_stride = j == L - 2 ? (size_t)L * g.n_cells : (size_t)g.n_cells;
        hipLaunchKernelGGL(k_cell_track_step, tiles, dim3(kCellTrackThreads), cell_track_lds_bytes(J), st, t_in, in_stride, map, g, j,
                           ctx->ctrack_t.as<long long>() + (size_t)(j & 1) * half, D);
    }
    const long long *t0 = locate_track_total(ctx, L);
    const dim3 grid((unsigned)lg.tiles, n_tracks), one(n_tracks);
    hipLaunchKernelGGL(k_cell_track_best, grid, dim3(kCellTrackThreads), 0, st, t0, g.n_cells, part);
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1) hipLaunchKernelGGL(k_locate_runner, grid, dim3(kLocateThreads), 0, st, t0, lg, static_cast<const int32_t *>(best), part);
        hipLaunchKernelGGL(k_cell_track_finish, one, dim3(kCellTrackThreads), 0, st, Q, lg, g, table, cdiff, roots,
                           ctx->ctrack_roots.as<const double>(), map, static_cast<const signed char *>(D),
                           static_cast<const ClosureCand *>(part), pass, best, ctx->ctrack_out.as<CellTrackOut>(),
                           ctx->ctrack_cells.as<int32_t>(), ctx->ctrack_own.as<long long>(), ctx->locate_lags.as<int32_t>(),
                           ctx->locate_corr.as<double>());
    }
    if (judged) launch_map_stats(ctx, t0, (size_t)g.n_cells, (int)n_tracks, lg, ctx->ctrack_out.p, ctx->ctrack_roots.as<const double>(), (int)n_tracks);
}

// the outputs to the host (all but track may be NULL); asynchronous on ctx->stream
static int download_locate_track(tdoa_ctx *ctx, size_t n_sets, int L, const LocateGeom &g, tdoa_cell_track *track, int32_t *cells,
                                 int64_t *own, int32_t *lags, double *corr, int64_t *total)
{
    hipStream_t st = ctx->stream;
    const size_t n_tracks = n_sets / L;
    HIPCHK(ctx, hipMemcpyAsync(track, ctx->ctrack_out.p, sizeof(CellTrackOut) * n_tracks, hipMemcpyDeviceToHost, st));
    if (cells) HIPCHK(ctx, hipMemcpyAsync(cells, ctx->ctrack_cells.p, sizeof(int32_t) * n_sets, hipMemcpyDeviceToHost, st));
    if (own) HIPCHK(ctx, hipMemcpyAsync(own, ctx->ctrack_own.p, sizeof(int64_t) * n_sets, hipMemcpyDeviceToHost, st));
    if (lags) HIPCHK(ctx, hipMemcpyAsync(lags, ctx->locate_lags.p, sizeof(int32_t) * n_sets * g.P, hipMemcpyDeviceToHost, st));
    if (corr) HIPCHK(ctx, hipMemcpyAsync(corr, ctx->locate_corr.p, sizeof(double) * n_sets * g.P, hipMemcpyDeviceToHost, st));
    if (total)
        HIPCHK(ctx, hipMemcpyAsync(total, locate_track_total(ctx, L), sizeof(int64_t) * n_tracks * g.n_cells, hipMemcpyDeviceToHost, st));
    return download_map_stats(ctx, n_tracks);
}

// sqrt(N_w) of the three blocks' tracks: a track holds all the windows of its block
static std::vector<double> block_track_roots(int wpb) { return std::vector<double>(3, std::sqrt((double)wpb)); }

// the cell tracks on a group's merged sum (finish_from_host, stacked_api.inc)
static int locate_track_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack, int max_step, int min_separation,
                                  tdoa_cell_track *track, int32_t *cells, int64_t *own, int32_t *lags, double *corr, int64_t *total)
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
            if ((rc = ensure_locate(ctx, n_stacks, g))) return rc;
            if ((rc = ensure_locate_track(ctx, n_stacks, L, g))) return rc;
            if ((rc = upload_locate_track_roots(ctx, track_roots))) return rc;
            launch_locate(ctx, ctx->stack_q.as<const long long>(), roots, n_stacks, g, false);
            launch_locate_track(ctx, ctx->stack_q.as<const long long>(), roots, n_stacks, L, max_step, g);
            return TDOA_OK;
        },
        [&](int n_stacks) { return download_locate_track(ctx, n_stacks, L, g, track, cells, own, lags, corr, total); });
}

}  // extern "C"
