// sync_locate_api.inc -- clocks to fix in one call (include/tdoa_mi355x.h), host side: the search as a StackSearch
// (stack_search.inc) that holds the fine clock search (SyncFineSearch, sync_fine_api.inc) and the zoom locate (LocateZoomSearch,
// locate_zoom_api.inc) and puts k_clock_mix (stack_clock_mix.hpp) between their launches, so that the stacks' clocks go from the
// one to the other on the device, inside one step graph behind one accumulation of the stacks.  The zoom locate runs under the
// call's own clock differences (LocateClocks, locate_run.inc): the context's clock table is neither read nor changed.  Also the
// host-only statement of the mix and the kernel alone on the caller's clocks.
// Included by tdoa_mi355x.hip after locate_zoom_api.inc and sync_fine_api.inc.

namespace {

static_assert(sizeof(ClockMix) == sizeof(tdoa_clock_mix) && sizeof(tdoa_clock_mix) == 16, "tdoa_clock_mix layout");

// what every entry refuses of m mix entries over n stacks' clocks; nullptr when they are in range
const char *check_clock_mix(const tdoa_clock_mix *mix, int m, int n)
{
    for (int t = 0; mix && t < m; t++) {
        const tdoa_clock_mix &x = mix[t];
        if (x.a < 0 || x.a >= n || x.b < 0 || x.b >= n) return "a mix entry names a stack outside 0 .. n_stacks - 1";
        if (x.wa < 0 || x.wb < 0) return "a mix entry has a negative weight";
        if ((long long)x.wa + x.wb < 1 || (long long)x.wa + x.wb > kClockMixMaxDen) return "a mix entry's wa + wb outside 1 .. 65536";
    }
    return nullptr;
}

void launch_clock_mix(tdoa_ctx *ctx, const int32_t *c16, int n_sets, int S, int U)
{
    hipLaunchKernelGGL(k_clock_mix, dim3((unsigned)n_sets), dim3(kClockMixThreads), 0, ctx->stream, c16, ctx->mix_in.as<const ClockMix>(), S,
                       S * (S - 1) / 2, U, ctx->mix_rows.as<int32_t>(), ctx->mix_cdiff.as<long long>(), ctx->mix_cdiff_up.as<long long>());
}

// the mix, the rows, the differences and U x them for n_sets stacks of S stations
int ensure_clock_mix(tdoa_ctx *ctx, size_t n_sets, int S)
{
    int rc;
    const size_t sp = n_sets * (size_t)(S * (S - 1) / 2);
    if ((rc = ensure(ctx, ctx->mix_in, sizeof(ClockMix) * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->mix_rows, sizeof(int32_t) * n_sets * S))) return rc;
    if ((rc = ensure(ctx, ctx->mix_cdiff, sizeof(long long) * sp))) return rc;
    return ensure(ctx, ctx->mix_cdiff_up, sizeof(long long) * sp);
}

struct SyncLocateSearch : StackSearch {
    SyncFineSearch fine;
    LocateZoomSearch zoom;
    const tdoa_clock_mix *mix;               // [set], NULL: every stack its own clock
    int32_t *rows;                           // [set][station], may be NULL
    std::vector<ClockMix> mix_in;            // bind: the mix as it is uploaded

    SyncLocateSearch(const SyncFineSearch &f, const tdoa_clock_mix *mix, int32_t *rows_host, const LocateZoomSearch &z)
        : StackSearch("clocks to fix in one call with TDOA_LAGS_GO", nullptr), fine(f), zoom(z), mix(mix), rows(rows_host)
    {
        zoom.coarse.own_clocks = true;       // before the checks: they ask nothing of the context's clock table
    }
    const char *check_args() const override
    {
        if (const char *bad = fine.check_args()) return bad;
        return zoom.check_args();
    }
    // U_loc x a row must fit 32 bits like U_loc x a clock table's entry: |row| <= 16 (|centre| + gate + 1), a convex combination
    int check_scaled(const tdoa_ctx *ctx, int S, const char **what) const
    {
        const long long U = ctx->locate_up;
        for (int s = 0; U > 1 && s < S; s++) {
            const long long c = fine.coarse.centre ? std::llabs((long long)fine.coarse.centre[s]) : 0;
            if (16 * (c + fine.coarse.G + 1) * U >= (1ll << 31))
                return refuse_with(what, TDOA_ERR_UNSUPPORTED, "a clock table entry times the upsampling factor does not fit 32 bits");
        }
        return TDOA_OK;
    }
    int check_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what) const override
    {
        if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse_with(what, TDOA_ERR_UNSUPPORTED, go_what);
        if (const int rc = fine.check_state(ctx, windows_per_stack, what)) return rc;
        int wpb = 0;
        (void)tdoa_num_windows(ctx, &wpb, nullptr);
        const int n_stacks = stack_geom(wpb, windows_per_stack).n_stacks;
        if (const char *bad = check_clock_mix(mix, n_stacks, n_stacks)) return refuse_with(what, TDOA_ERR_INVALID, bad);
        if (const int rc = zoom.check_state(ctx, windows_per_stack, what)) return rc;
        return check_scaled(ctx, (int)ctx->caps.size(), what);
    }
    int check_sets(const tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what) const override
    {
        if (const int rc = fine.check_sets(ctx, q, n_sets, track_len, n_stations, n_w, what)) return rc;
        if (const char *bad = check_clock_mix(mix, n_sets, n_sets)) return refuse_with(what, TDOA_ERR_INVALID, bad);
        if (const int rc = zoom.check_sets(ctx, q, n_sets, track_len, n_stations, n_w, what)) return rc;
        return check_scaled(ctx, n_stations, what);
    }
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override
    {
        fine.bind(ctx, sh);
        zoom.coarse.clocks = LocateClocks{&ctx->mix_cdiff, &ctx->mix_cdiff_up};
        zoom.bind(ctx, sh);
        mix_in.resize((size_t)sh.n_sets);
        for (int t = 0; t < sh.n_sets; t++) mix_in[t] = mix ? ClockMix{mix[t].a, mix[t].b, mix[t].wa, mix[t].wb} : ClockMix{t, t, 1, 0};
    }
    // both held searches' words; the locate's clock flag is on (the mix is data)
    void key(std::vector<uint64_t> *key, int m) const override
    {
        key->push_back(StepProduct::SyncLocate);
        fine.key(key, m);
        zoom.key(key, m);
    }
    int reserve(tdoa_ctx *ctx) const override
    {
        if (int rc = fine.reserve(ctx)) return rc;
        if (int rc = ensure_clock_mix(ctx, mix_in.size(), fine.coarse.g.S)) return rc;
        return zoom.reserve(ctx);
    }
    // the delays and centres, the mix: a call that changes only them replays the same graph
    int refresh(tdoa_ctx *ctx) const override
    {
        if (int rc = fine.refresh(ctx)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->mix_in.p, mix_in.data(), sizeof(ClockMix) * mix_in.size(), hipMemcpyHostToDevice, ctx->stream));
        return zoom.refresh(ctx);
    }
    // the fine clock search, the rows and differences from the clocks it left in ctx->sfine_clock, the zoom locate under them
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
    {
        fine.launch(ctx, Q, roots);
        launch_clock_mix(ctx, ctx->sfine_clock.as<const int32_t>(), (int)mix_in.size(), fine.coarse.g.S, zoom.coarse.run.U);
        zoom.launch(ctx, Q, roots);
    }
    int download(tdoa_ctx *ctx) const override
    {
        if (int rc = fine.download(ctx)) return rc;
        if (rows)
            HIPCHK(ctx, hipMemcpyAsync(rows, ctx->mix_rows.p, sizeof(int32_t) * mix_in.size() * fine.coarse.g.S, hipMemcpyDeviceToHost, ctx->stream));
        return zoom.download(ctx);
    }
};

}  // namespace

extern "C" {

#define TDOA_SYNC_LOCATE_SEARCH(s)                                                                                               \
    SyncLocateSearch s(SyncFineSearch(gate, rounds, U, fine_rounds, ref_delay, centre, SyncHost{sync_host, clock_host, lags_host, corr_host}, \
                                      SyncFineHost{fine_host, clock16_host, fine_lags_host, fine_corr_host}),                   \
                       mix, rows_host,                                                                                           \
                       LocateZoomSearch(min_separation, Z, H, fine_separation, loc_host, loc_lags_host, loc_corr_host, map_host,  \
                                        LocateZoomHost{zoom_host, zlags_host, zcorr_host, zmap_host}))

int tdoa_process_sync_locate(tdoa_ctx *ctx, int windows_per_stack, int gate, int rounds, int U, int fine_rounds, const int32_t *ref_delay,
                             const int32_t *centre, const tdoa_clock_mix *mix, int min_separation, int Z, int H, int fine_separation,
                             tdoa_sync *sync_host, int32_t *clock_host, int32_t *lags_host, double *corr_host, tdoa_sync *fine_host,
                             int32_t *clock16_host, int32_t *fine_lags_host, double *fine_corr_host, int32_t *rows_host,
                             tdoa_location *loc_host, int32_t *loc_lags_host, double *loc_corr_host, int64_t *map_host, tdoa_zoom *zoom_host,
                             int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host)
{
    TDOA_SYNC_LOCATE_SEARCH(s);
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_sync_locate(tdoa_group *g, int windows_per_stack, int gate, int rounds, int U, int fine_rounds,
                                   const int32_t *ref_delay, const int32_t *centre, const tdoa_clock_mix *mix, int min_separation, int Z, int H,
                                   int fine_separation, tdoa_sync *sync_host, int32_t *clock_host, int32_t *lags_host, double *corr_host,
                                   tdoa_sync *fine_host, int32_t *clock16_host, int32_t *fine_lags_host, double *fine_corr_host,
                                   int32_t *rows_host, tdoa_location *loc_host, int32_t *loc_lags_host, double *loc_corr_host,
                                   int64_t *map_host, tdoa_zoom *zoom_host, int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host)
{
    TDOA_SYNC_LOCATE_SEARCH(s);
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_debug_sync_locate_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int gate, int rounds, int U,
                                  int fine_rounds, const int32_t *ref_delay, const int32_t *centre, const tdoa_clock_mix *mix,
                                  int min_separation, int Z, int H, int fine_separation, tdoa_sync *sync_host, int32_t *clock_host,
                                  int32_t *lags_host, double *corr_host, tdoa_sync *fine_host, int32_t *clock16_host, int32_t *fine_lags_host,
                                  double *fine_corr_host, int32_t *rows_host, tdoa_location *loc_host, int32_t *loc_lags_host,
                                  double *loc_corr_host, int64_t *map_host, tdoa_zoom *zoom_host, int32_t *zlags_host, double *zcorr_host,
                                  int64_t *zmap_host)
{
    TDOA_SYNC_LOCATE_SEARCH(s);
    return debug_search_from_q(ctx, q, n_sets, 0, n_stations, n_w, s);
}
#undef TDOA_SYNC_LOCATE_SEARCH

// Host only: the plain-C statement of the mix, to the mix what tdoa_sync_line_clock is to the lines
int tdoa_clock_mix_rows(const int32_t *clock16, int n_stacks, int n_stations, const tdoa_clock_mix *mix, int n_rows, int32_t *rows)
{
    if (!clock16 || !mix || !rows || n_stacks < 1 || n_stations < 1 || n_rows < 1) return TDOA_ERR_INVALID;
    if (check_clock_mix(mix, n_rows, n_stacks)) return TDOA_ERR_INVALID;
    for (int t = 0; t < n_rows; t++)
        for (int s = 0; s < n_stations; s++)
            rows[(size_t)t * n_stations + s] = clock_mix_row(clock16[(size_t)mix[t].a * n_stations + s], clock16[(size_t)mix[t].b * n_stations + s],
                                                             mix[t].wa, mix[t].wb);
    return TDOA_OK;
}

// k_clock_mix alone on the caller's clocks, with U_loc an argument (the context's setting is not read): the rows, the pairs'
// differences and U_loc x them
int tdoa_debug_clock_mix(tdoa_ctx *ctx, const int32_t *clock16, int n_stacks, int n_stations, const tdoa_clock_mix *mix, int n_rows, int U_loc,
                         int32_t *rows, int64_t *cdiff, int64_t *cdiff_up)
{
    int rc;
    if (!ctx) return TDOA_ERR_INVALID;
    if (!clock16 || !mix || !rows || !cdiff || !cdiff_up || n_stacks < 1 || n_stacks > kLocateMaxSets || n_rows < 1 || n_rows > kLocateMaxSets ||
        n_stations < 2 || n_stations > kLocateMaxStations || !upsample_factor_ok(U_loc))
        return fail(ctx, TDOA_ERR_INVALID, "a pointer is NULL, n_stacks or n_rows outside 1 .. 65535, n_stations outside 2 .. 64 or U_loc is not one of 1, 2, 4, 8, 16");
    if (const char *bad = check_clock_mix(mix, n_rows, n_stacks)) return fail(ctx, TDOA_ERR_INVALID, bad);
    const size_t S = (size_t)n_stations, sp = (size_t)n_rows * (S * (S - 1) / 2);
    if ((rc = check_ctx(ctx))) return rc;
    if ((rc = ensure(ctx, ctx->mix_debug, sizeof(int32_t) * (size_t)n_stacks * S))) return rc;
    if ((rc = ensure_clock_mix(ctx, (size_t)n_rows, n_stations))) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->mix_debug.p, clock16, sizeof(int32_t) * (size_t)n_stacks * S, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->mix_in.p, mix, sizeof(ClockMix) * (size_t)n_rows, hipMemcpyHostToDevice, st));
    launch_clock_mix(ctx, ctx->mix_debug.as<const int32_t>(), n_rows, n_stations, U_loc);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(rows, ctx->mix_rows.p, sizeof(int32_t) * (size_t)n_rows * S, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(cdiff, ctx->mix_cdiff.p, sizeof(long long) * sp, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(cdiff_up, ctx->mix_cdiff_up.p, sizeof(long long) * sp, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return TDOA_OK;
}

}  // extern "C"
