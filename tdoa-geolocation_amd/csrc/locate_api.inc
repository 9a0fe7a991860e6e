// locate_api.inc -- the delay-table search, host side: the table and the station clocks a context keeps, the search's buffers, the kernels' launches
// (shared by a context's own step, step_products.inc, the group's merged sum and tdoa_debug_locate_from_q), the host-only
// grid table.  Included by tdoa_mi355x.hip after closure_api.inc and before step_products.inc.

extern "C" {

static LocateGeom locate_geom(const tdoa_ctx *ctx, int min_separation)
{
    LocateGeom g;
    g.S = ctx->locate_stations;
    g.P = g.S * (g.S - 1) / 2;
    g.n = 2 * ctx->prm.max_lag - 1;
    g.lag_lo = -(ctx->prm.max_lag - 1);
    g.n_cells = ctx->locate_cells;
    g.n_cols = ctx->locate_cols;
    g.sep = min_separation;
    g.tiles = (g.n_cells + kLocateThreads - 1) / kLocateThreads;
    return g;
}

// the arguments the three locate entries share; they need no device
static const char *check_locate_args(int min_separation, const void *loc)
{
    if (min_separation < 1) return "min_separation < 1";
    if (!loc) return "loc_host is NULL";
    return nullptr;
}

// what a search on S stations needs of the context's table; nullptr when it is there
static const char *check_locate_table(const tdoa_ctx *ctx, int S)
{
    if (ctx->locate_cells == 0) return "no delay table (tdoa_locate_set_table)";
    if (ctx->locate_stations != S) return "the delay table's n_stations differs from the stations searched";
    return nullptr;
}

// what a search on n_sets stacks of S stations needs of the context's clock table, when there is one
static const char *check_locate_clock(const tdoa_ctx *ctx, int n_sets, int S)
{
    if (ctx->clock_stacks == 0) return nullptr;
    if (ctx->clock_stacks != n_sets) return "the clock table's n_stacks differs from the stacks searched";
    if (ctx->clock_stations != S) return "the clock table's n_stations differs from the stations searched";
    return nullptr;
}

// every sum of P magnitudes of at most n_w 2^45 stays below 2^62
static bool locate_overflows(int P, long long n_w) { return (long long)P * n_w > (1ll << 17); }

int tdoa_locate_set_table(tdoa_ctx *ctx, const int32_t *delay, int n_cells, int n_cols, int n_stations)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (!delay || n_cells == 0) {            // forget the table (the buffer stays: a cached step graph may still name it)
        ctx->locate_cells = ctx->locate_cols = ctx->locate_stations = 0;
        return TDOA_OK;
    }
    if (n_cells < 1 || n_cells > kLocateMaxCells || n_cols < 1 || n_stations < 2 || n_stations > kLocateMaxStations)
        return fail(ctx, TDOA_ERR_INVALID, "n_cells outside 1 .. 2^22, n_cols < 1 or n_stations outside 2 .. 64");
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    std::vector<int32_t> t((size_t)n_cells * n_stations);      // station-major: a wave's cells read consecutive words
    for (int c = 0; c < n_cells; c++)
        for (int s = 0; s < n_stations; s++) t[(size_t)s * n_cells + c] = delay[(size_t)c * n_stations + s];
    if ((rc = ensure(ctx, ctx->locate_table, sizeof(int32_t) * t.size()))) {
        ctx->locate_cells = ctx->locate_cols = ctx->locate_stations = 0;
        return rc;
    }
    ctx->locate_cells = n_cells;
    ctx->locate_cols = n_cols;
    ctx->locate_stations = n_stations;
    HIPCHK(ctx, hipMemcpyAsync(ctx->locate_table.p, t.data(), sizeof(int32_t) * t.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // t goes out of scope
    return TDOA_OK;
}

int tdoa_locate_set_clock(tdoa_ctx *ctx, const int32_t *clock, int n_stacks, int n_stations)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (!clock || n_stacks == 0) {           // forget the clocks (the buffer stays: a cached step graph may still name it)
        ctx->clock_stacks = ctx->clock_stations = 0;
        return TDOA_OK;
    }
    if (n_stacks < 1 || n_stacks > kLocateMaxSets || n_stations < 2 || n_stations > kLocateMaxStations)
        return fail(ctx, TDOA_ERR_INVALID, "n_stacks outside 1 .. 65535 or n_stations outside 2 .. 64");
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    const int S = n_stations, P = S * (S - 1) / 2;
    std::vector<long long> cd((size_t)n_stacks * P);           // per (stack, pair) clock[j] - clock[i]: what the kernels add to d
    for (int sid = 0; sid < n_stacks; sid++) {
        const int32_t *k = clock + (size_t)sid * S;
        long long *row = cd.data() + (size_t)sid * P;
        for (int i = 0; i < S; i++)
            for (int j = i + 1; j < S; j++) *row++ = (long long)k[j] - (long long)k[i];
    }
    if ((rc = ensure(ctx, ctx->locate_clock, sizeof(long long) * cd.size()))) {
        ctx->clock_stacks = ctx->clock_stations = 0;
        return rc;
    }
    ctx->clock_stacks = n_stacks;
    ctx->clock_stations = n_stations;
    HIPCHK(ctx, hipMemcpyAsync(ctx->locate_clock.p, cd.data(), sizeof(long long) * cd.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // cd goes out of scope
    return TDOA_OK;
}

// the buffers of the search for n_sets stacks: the map, the tiles' candidates, the locations' cells, the records and the
// best cells' lags and correlations
static int ensure_locate(tdoa_ctx *ctx, size_t n_sets, const LocateGeom &g)
{
    int rc;
    if ((rc = ensure(ctx, ctx->locate_map, sizeof(long long) * n_sets * g.n_cells))) {
        char buf[256];
        snprintf(buf, sizeof(buf), "the delay-table search's map [%zu stacks][%d cells] (%.1f MB) does not fit in device memory: %s",
                 n_sets, (int)g.n_cells, 8.0 * (double)n_sets * g.n_cells / 1e6, ctx->last_error.c_str());
        return fail(ctx, TDOA_ERR_NOMEM, buf);
    }
    if ((rc = ensure(ctx, ctx->locate_part, sizeof(ClosureCand) * n_sets * g.tiles))) return rc;
    if ((rc = ensure(ctx, ctx->locate_best, sizeof(int32_t) * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->locate_out, sizeof(LocateOut) * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->locate_lags, sizeof(int32_t) * n_sets * g.P))) return rc;
    if ((rc = ensure(ctx, ctx->locate_corr, sizeof(double) * n_sets * g.P))) return rc;
    return ensure_map_stats(ctx, n_sets);
}

// Q [n_sets][P][n] -> the records in ctx->locate_out, the map, lags and correlations: the one place the search is launched.
// With a clock table (its shape checked by the caller: n_sets stacks of g.S stations) the scores' clock instantiation runs
// and the finish adds the same differences.  judged: the maps are what the call judges (the rounds and the cell tracks go on
// from here and judge their own planes), so their statistics follow when the setting is on.  Kernel launches only (the step
// graph captures them).
static void launch_locate(tdoa_ctx *ctx, const long long *Q, const double *roots, int n_sets, const LocateGeom &g, bool judged = true)
{
    hipStream_t st = ctx->stream;
    const dim3 grid((unsigned)g.tiles, (unsigned)n_sets), one((unsigned)n_sets);
    auto *table = ctx->locate_table.as<const int32_t>();
    const long long *cdiff = ctx->clock_stacks ? ctx->locate_clock.as<const long long>() : nullptr;
    auto *map = ctx->locate_map.as<long long>();
    auto *part = ctx->locate_part.as<ClosureCand>();
    auto *best = ctx->locate_best.as<int32_t>();
    auto *out = ctx->locate_out.as<LocateOut>();
    auto *lags = ctx->locate_lags.as<int32_t>();
    auto *corr = ctx->locate_corr.as<double>();
    switch (g.S <= kLocateRegStations ? g.S : 0) {
#define TDOA_LOCATE_CASE(s)                                                                                                      \
    case s:                                                                                                                      \
        if (cdiff)                                                                                                               \
            hipLaunchKernelGGL((k_locate_scores<s, true>), grid, dim3(kLocateThreads), 0, st, Q, g, table, cdiff, map, part);    \
        else                                                                                                                     \
            hipLaunchKernelGGL((k_locate_scores<s, false>), grid, dim3(kLocateThreads), 0, st, Q, g, table, cdiff, map, part);   \
        break;
    TDOA_LOCATE_CASE(2) TDOA_LOCATE_CASE(3) TDOA_LOCATE_CASE(4) TDOA_LOCATE_CASE(5) TDOA_LOCATE_CASE(6) TDOA_LOCATE_CASE(7)
    TDOA_LOCATE_CASE(8) TDOA_LOCATE_CASE(9) TDOA_LOCATE_CASE(10) TDOA_LOCATE_CASE(11) TDOA_LOCATE_CASE(12) TDOA_LOCATE_CASE(13)
    TDOA_LOCATE_CASE(14) TDOA_LOCATE_CASE(15) TDOA_LOCATE_CASE(16)
    default:
        TDOA_LOCATE_CASE(0)
    }
#undef TDOA_LOCATE_CASE
    hipLaunchKernelGGL(k_locate_finish, one, dim3(kLocateThreads), 0, st, Q, g, table, cdiff, roots, static_cast<const ClosureCand *>(part), 0,
                       best, out, lags, corr);
    hipLaunchKernelGGL(k_locate_runner, grid, dim3(kLocateThreads), 0, st, static_cast<const long long *>(map), g,
                       static_cast<const int32_t *>(best), part);
    hipLaunchKernelGGL(k_locate_finish, one, dim3(kLocateThreads), 0, st, Q, g, table, cdiff, roots, static_cast<const ClosureCand *>(part), 1,
                       best, out, lags, corr);
    if (judged) launch_map_stats(ctx, map, (size_t)g.n_cells, n_sets, g, out, roots, n_sets);
}

// the outputs to the host (all but loc may be NULL); asynchronous on ctx->stream
static int download_locate(tdoa_ctx *ctx, size_t n_sets, const LocateGeom &g, tdoa_location *loc, int32_t *lags, double *corr,
                           int64_t *map)
{
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(loc, ctx->locate_out.p, sizeof(LocateOut) * n_sets, hipMemcpyDeviceToHost, st));
    if (lags) HIPCHK(ctx, hipMemcpyAsync(lags, ctx->locate_lags.p, sizeof(int32_t) * n_sets * g.P, hipMemcpyDeviceToHost, st));
    if (corr) HIPCHK(ctx, hipMemcpyAsync(corr, ctx->locate_corr.p, sizeof(double) * n_sets * g.P, hipMemcpyDeviceToHost, st));
    if (map) HIPCHK(ctx, hipMemcpyAsync(map, ctx->locate_map.p, sizeof(int64_t) * n_sets * g.n_cells, hipMemcpyDeviceToHost, st));
    return download_map_stats(ctx, n_sets);
}

// the delay-table search on a group's merged sum (finish_from_host, stacked_api.inc)
static int locate_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack, int min_separation, tdoa_location *loc,
                            int32_t *lags, double *corr, int64_t *map)
{
    const LocateGeom g = locate_geom(ctx, min_separation);
    return finish_from_host(
        ctx, q_sum, windows_per_stack,
        [&](int n_stacks, const double *roots) -> int {
            if (int rc = ensure_locate(ctx, n_stacks, g)) return rc;
            launch_locate(ctx, ctx->stack_q.as<const long long>(), roots, n_stacks, g);
            return TDOA_OK;
        },
        [&](int n_stacks) { return download_locate(ctx, n_stacks, g, loc, lags, corr, map); });
}

// what tdoa_process_locate and the group's call refuse once the arguments are in range: the lag mode, the captures, the
// station count, the table, the overflow bound, the clock table's shape.  *what receives the message.
static int check_locate_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what)
{
    const auto refuse = [&](int status, const char *why) {
        *what = why;
        return status;
    };
    if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse(TDOA_ERR_UNSUPPORTED, "the delay-table search with TDOA_LAGS_GO");
    if (ctx->caps.empty()) return refuse(TDOA_ERR_STATE, "captures missing");
    const int S = (int)ctx->caps.size();
    if (S < 2 || S > kLocateMaxStations) return refuse(TDOA_ERR_UNSUPPORTED, "the delay-table search needs 2 .. 64 stations");
    if (const char *bad = check_locate_table(ctx, S)) return refuse(TDOA_ERR_STATE, bad);
    int wpb = 0;
    if (tdoa_num_windows(ctx, &wpb, nullptr)) return refuse(TDOA_ERR_STATE, "captures missing or too small");
    if (locate_overflows(S * (S - 1) / 2, stack_geom(wpb, windows_per_stack).mm))
        return refuse(TDOA_ERR_UNSUPPORTED, "pairs x stack length > 2^17: a cell's score could overflow");
    if (3ll * wpb > kLocateMaxSets) return refuse(TDOA_ERR_UNSUPPORTED, "more than 65535 stacks");
    if (const char *bad = check_locate_clock(ctx, stack_geom(wpb, windows_per_stack).n_stacks, S)) return refuse(TDOA_ERR_STATE, bad);
    return TDOA_OK;
}

// Host only: the delays of a latitude / longitude grid at one height, cell r * cols + c at (lat0 + r dlat, lon0 + c dlon)
int tdoa_locate_grid_table(const double *stations_lle, int n_stations, double lat0, double lon0, double dlat, double dlon, int rows,
                           int cols, double height_m, double sample_rate, int32_t *delay)
{
    if (!stations_lle || !delay || n_stations < 1 || rows < 1 || cols < 1 || (long long)rows * cols > kLocateMaxCells) return TDOA_ERR_INVALID;
    for (const double x : {lat0, lon0, dlat, dlon, height_m, sample_rate})
        if (!std::isfinite(x)) return TDOA_ERR_INVALID;
    if (!(sample_rate > 0.0)) return TDOA_ERR_INVALID;
    std::vector<double> st((size_t)n_stations * 3);
    for (int s = 0; s < n_stations; s++) {
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(stations_lle[3 * s + k])) return TDOA_ERR_INVALID;
        tdoa_latlon_to_ecef(stations_lle[3 * s], stations_lle[3 * s + 1], stations_lle[3 * s + 2], &st[3 * (size_t)s]);
    }
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) {
            double x[3];
            tdoa_latlon_to_ecef(lat0 + r * dlat, lon0 + c * dlon, height_m, x);
            for (int s = 0; s < n_stations; s++) {
                const double d = kLocateDelayUnit * sample_rate * geo::range(x, &st[3 * (size_t)s]) / geo::kC;
                if (!(d < 2147483647.0)) return TDOA_ERR_INVALID;      // (a range is never negative)
                delay[((size_t)r * cols + c) * n_stations + s] = (int32_t)std::llrint(d);
            }
        }
    return TDOA_OK;
}

}  // extern "C"
