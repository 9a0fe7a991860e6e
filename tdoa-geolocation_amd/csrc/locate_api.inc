// locate_api.inc -- the delay-table family, host side: the table and the station clocks a context keeps and the host-only grid
// table.  The family's runs on them are in locate_run.inc.  Included by tdoa_mi355x.hip after map_stats_api.inc and before
// locate_run.inc, sync_api.inc and sync_drift_api.inc (locate_overflows).

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

// every sum of P magnitudes of at most n_w 2^45 stays below 2^62; on upsampled surfaces (U > 1) a magnitude is at most
// 2.04 n_w 2^45 + 1, and the bound is tightened by the factor 4
static bool locate_overflows(int P, long long n_w, int U = 1) { return (U > 1 ? 4ll : 1ll) * P * n_w > (1ll << 17); }

// U x the table, U x the zoom's fine table and U x the clock differences beside the originals, for the searches on upsampled
// surfaces (stack_upsample.hpp): remade whenever one of them or U changes, so that they are data of a replayed graph like the
// originals.  Nothing to do with U = 1.  (An entry with |t| U >= 2^31 wraps here; the calls refuse such a table:
// check_locate_upsample, LocateZoomSearch::check_fine.)
static int remake_locate_scaled(tdoa_ctx *ctx)
{
    const int U = ctx->locate_up;
    if (U == 1 || (ctx->locate_cells == 0 && ctx->clock_stacks == 0 && ctx->fine_cells == 0)) return TDOA_OK;
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (ctx->fine_cells) {
        const size_t n = (size_t)ctx->fine_stations * ctx->fine_cells;
        if ((rc = ensure(ctx, ctx->locate_fine_up, sizeof(int32_t) * n))) return rc;
        hipLaunchKernelGGL(k_locate_scale_i32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->locate_fine.as<const int32_t>(), U, n,
                           ctx->locate_fine_up.as<int32_t>());
    }
    if (ctx->locate_cells) {
        const size_t n = (size_t)ctx->locate_stations * ctx->locate_cells;
        if ((rc = ensure(ctx, ctx->locate_table_up, sizeof(int32_t) * n))) return rc;
        hipLaunchKernelGGL(k_locate_scale_i32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->locate_table.as<const int32_t>(), U, n,
                           ctx->locate_table_up.as<int32_t>());
    }
    if (ctx->clock_stacks) {
        const size_t n = (size_t)ctx->clock_stacks * (ctx->clock_stations * (ctx->clock_stations - 1) / 2);
        if ((rc = ensure(ctx, ctx->locate_clock_up, sizeof(long long) * n))) return rc;
        hipLaunchKernelGGL(k_locate_scale_i64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->locate_clock.as<const long long>(), U, n,
                           ctx->locate_clock_up.as<long long>());
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TDOA_OK;
}

// a delay table of the context, the table or the fine table: the caller's [cell][station] words station-major into buf, the
// shape and the largest magnitude into the context's words, then the scaled copies
static int set_delay_table(tdoa_ctx *ctx, const int32_t *delay, int n_cells, int n_cols, int n_stations, DevBuf &buf, int *cells, int *cols,
                           int *stations, long long *largest)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (!delay || n_cells == 0) {            // forget the table (the buffer stays: a cached step graph may still name it)
        *cells = *cols = *stations = 0;
        return TDOA_OK;
    }
    if (n_cells < 1 || n_cells > kLocateMaxCells || n_cols < 1 || n_stations < 2 || n_stations > kLocateMaxStations)
        return fail(ctx, TDOA_ERR_INVALID, "n_cells outside 1 .. 2^22, n_cols < 1 or n_stations outside 2 .. 64");
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    std::vector<int32_t> t((size_t)n_cells * n_stations);      // station-major: a wave's cells read consecutive words
    long long t_max = 0;
    for (int c = 0; c < n_cells; c++)
        for (int s = 0; s < n_stations; s++) {
            const int32_t d = delay[(size_t)c * n_stations + s];
            t[(size_t)s * n_cells + c] = d;
            t_max = std::max(t_max, std::llabs((long long)d));
        }
    if ((rc = ensure(ctx, buf, sizeof(int32_t) * t.size()))) {
        *cells = *cols = *stations = 0;
        return rc;
    }
    *cells = n_cells;
    *cols = n_cols;
    *stations = n_stations;
    *largest = t_max;
    HIPCHK(ctx, hipMemcpyAsync(buf.p, t.data(), sizeof(int32_t) * t.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // t goes out of scope
    return remake_locate_scaled(ctx);
}

int tdoa_locate_set_table(tdoa_ctx *ctx, const int32_t *delay, int n_cells, int n_cols, int n_stations)
{
    if (!ctx) return TDOA_ERR_INVALID;
    return set_delay_table(ctx, delay, n_cells, n_cols, n_stations, ctx->locate_table, &ctx->locate_cells, &ctx->locate_cols, &ctx->locate_stations,
                           &ctx->locate_table_max);
}

// the zoom locate's second table (locate_zoom_api.inc): the same upload, beside the table
int tdoa_locate_set_fine_table(tdoa_ctx *ctx, const int32_t *delay, int n_cells, int n_cols, int n_stations)
{
    if (!ctx) return TDOA_ERR_INVALID;
    return set_delay_table(ctx, delay, n_cells, n_cols, n_stations, ctx->locate_fine, &ctx->fine_cells, &ctx->fine_cols, &ctx->fine_stations,
                           &ctx->locate_fine_max);
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
    long long k_max = 0;
    for (size_t i = 0; i < (size_t)n_stacks * S; i++) k_max = std::max(k_max, std::llabs((long long)clock[i]));
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
    ctx->locate_clock_max = k_max;
    HIPCHK(ctx, hipMemcpyAsync(ctx->locate_clock.p, cd.data(), sizeof(long long) * cd.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));            // cd goes out of scope
    return remake_locate_scaled(ctx);
}

// the lag grid of the family's surfaces: 1 / U sample (stack_upsample.hpp); a setting: with U > 1 and a table or clocks set,
// their scaled copies are made here
int tdoa_locate_set_upsample(tdoa_ctx *ctx, int U)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (!upsample_factor_ok(U)) return fail(ctx, TDOA_ERR_INVALID, "U is not one of 1, 2, 4, 8, 16");
    if (U == ctx->locate_up) return TDOA_OK;
    const int before = ctx->locate_up;
    ctx->locate_up = U;
    if (const int rc = remake_locate_scaled(ctx)) {
        ctx->locate_up = before;
        return rc;
    }
    return TDOA_OK;
}

// Host only: the U phases' taps, taps[r][k] = h16[r 16 / U][k]
int tdoa_locate_upsample_taps(int U, int32_t *taps)
{
    if (!taps || !upsample_factor_ok(U)) return TDOA_ERR_INVALID;
    for (int r = 0; r < U; r++) std::memcpy(taps + (size_t)r * kUpsampleTapCount, kUpsampleTaps[r * (kUpsamplePhases / U)], sizeof(kUpsampleTaps[0]));
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
