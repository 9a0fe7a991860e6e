// locate_zoom_api.inc -- the zoom locate (stack_locate_zoom.hpp), host side: the search as a StackSearch (stack_search.inc)
// that holds the delay-table search (LocateSearch, locate_run.inc) for its coarse stage and adds the window's two kernels behind
// that search's launches, and the search's three entries.  The fine table is context state beside the table (locate_api.inc).
// Included by tdoa_mi355x.hip after locate_run.inc.

namespace {

// the outputs the zoom adds to the locate's (all but zoom may be NULL)
struct LocateZoomHost {
    tdoa_zoom *zoom = nullptr;               // [set]
    int32_t *lags = nullptr;                 // [set][pair], 1/U sample
    double *corr = nullptr;                  // [set][pair]
    int64_t *map = nullptr;                  // [set][(2H+1)^2]
};

// what a search on the context's fine table on S stations needs of it, after the locate's own checks (the zoom locate and the
// zoomed cell tracks, locate_track_zoom_api.inc)
int check_locate_fine(const tdoa_ctx *ctx, int S, const char **what)
{
    if (ctx->fine_cells == 0) return refuse_with(what, TDOA_ERR_STATE, "no fine delay table (tdoa_locate_set_fine_table)");
    if (ctx->fine_stations != S) return refuse_with(what, TDOA_ERR_STATE, "the fine delay table's n_stations differs from the stations searched");
    if (ctx->locate_up > 1 && ctx->locate_fine_max * ctx->locate_up >= (1ll << 31))
        return refuse_with(what, TDOA_ERR_UNSUPPORTED, "a fine delay table entry times the upsampling factor does not fit 32 bits");
    return TDOA_OK;
}

// The window on the context's fine table that such a search scores behind its coarse run: what the zoom locate and the zoomed
// cell tracks share of their arguments, geometry, key words and launches
struct LocateFineWindow {
    int Z, H, sep;                           // fine cells per cell, the window's half side, fine_separation
    LocateGeom gf{};                         // bind: the coarse run's geometry with the fine table's shape, fine_separation and the window's tiles
    LocateZoomGeom z{};

    // between: what the holder refuses of an argument of its own that the entries name between H and fine_separation
    const char *check_args(const char *between = nullptr) const
    {
        if (Z < 1 || Z > kLocateZoomMaxZ) return "Z outside 1 .. 64";
        if (H < 0 || H > kLocateZoomMaxH) return "H outside 0 .. 64";
        if (between) return between;
        return sep < 1 ? "fine_separation < 1" : nullptr;
    }
    void bind(const tdoa_ctx *ctx, const LocateGeom &g)
    {
        z.Z = Z;
        z.H = H;
        z.side = 2 * H + 1;
        z.n_pos = z.side * z.side;
        z.coarse_cells = g.n_cells;
        z.coarse_cols = g.n_cols;
        z.tiles = (z.n_pos + kLocateThreads - 1) / kLocateThreads;
        gf = g;                              // S, P and the lags (with U > 1 the fine ones) are the coarse run's
        gf.n_cells = ctx->fine_cells;
        gf.n_cols = ctx->fine_cols;
        gf.sep = sep;
        gf.tiles = z.tiles;
    }
    // the holder's kind, the window, the holder's word, the fine table's shape (its contents are data)
    void key(std::vector<uint64_t> *key, uint64_t kind, uint64_t word) const
    {
        key->insert(key->end(), {kind, (uint64_t)Z | ((uint64_t)H << 32), word, (uint64_t)gf.n_cells | ((uint64_t)gf.n_cols << 32)});
    }
    // the (fine) table scale, clock differences and words the coarse run ran on
    void select(const tdoa_ctx *ctx, const LocateSearch &coarse, const int32_t **table, const long long **cdiff, const long long **Q) const
    {
        const bool up = coarse.run.U > 1;
        *table = (up ? ctx->locate_fine_up : ctx->locate_fine).as<const int32_t>();
        *cdiff = coarse.clocks.get(up);
        if (up) *Q = ctx->locate_qu.as<const long long>();
    }
};

struct LocateZoomSearch : StackSearch {
    LocateSearch coarse;
    LocateFineWindow w;
    LocateZoomHost o;

    LocateZoomSearch(int min_separation, int zoom, int half, int fine_separation, tdoa_location *loc, int32_t *lags, double *corr, int64_t *map,
                     const LocateZoomHost &host)
        : StackSearch("the zoom locate with TDOA_LAGS_GO", nullptr), coarse(locate_search_call(false, 1, 0, min_separation, loc, lags, corr, map)),
          w{zoom, half, fine_separation}, o(host)
    {
    }
    const char *check_args() const override
    {
        if (const char *bad = coarse.check_args()) return bad;
        if (const char *bad = w.check_args()) return bad;
        return o.zoom ? nullptr : "zoom_host is NULL";
    }
    int check_fine(const tdoa_ctx *ctx, int S, const char **what) const { return check_locate_fine(ctx, S, what); }
    int check_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what) const override
    {
        if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse_with(what, TDOA_ERR_UNSUPPORTED, go_what);
        if (const int rc = coarse.check_state(ctx, windows_per_stack, what)) return rc;
        return check_fine(ctx, (int)ctx->caps.size(), what);
    }
    int check_sets(const tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what) const override
    {
        if (const int rc = coarse.check_sets(ctx, q, n_sets, track_len, n_stations, n_w, what)) return rc;
        return check_fine(ctx, n_stations, what);
    }
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override
    {
        coarse.bind(ctx, sh);
        w.bind(ctx, coarse.run.g);
    }
    // the window and the fine table's shape (its contents are data), then the locate's words
    void key(std::vector<uint64_t> *key, int m) const override
    {
        w.key(key, StepProduct::LocateZoom, (uint64_t)w.sep);
        coarse.key(key, m);
    }
    // the locate's buffers, then the window maps, the tiles' candidates, the records, lags and correlations
    int reserve(tdoa_ctx *ctx) const override
    {
        int rc;
        const size_t n_sets = coarse.run.n_sets, sp = n_sets * w.gf.P;
        if ((rc = coarse.reserve(ctx))) return rc;
        if (ensure(ctx, ctx->zoom_map, sizeof(long long) * n_sets * w.z.n_pos)) {
            char buf[320];
            snprintf(buf, sizeof(buf), "the zoom locate's window maps [%zu stacks][%d x %d positions] (%.1f MB) do not fit in device memory: %s", n_sets,
                     (int)w.z.side, (int)w.z.side, 8.0 * (double)n_sets * (double)w.z.n_pos / 1e6, ctx->last_error.c_str());
            return fail(ctx, TDOA_ERR_NOMEM, buf);
        }
        if ((rc = ensure(ctx, ctx->zoom_part, sizeof(ClosureCand) * n_sets * w.z.tiles))) return rc;
        if ((rc = ensure(ctx, ctx->zoom_out, sizeof(LocateZoomOut) * n_sets))) return rc;
        if ((rc = ensure(ctx, ctx->zoom_lags, sizeof(int32_t) * sp))) return rc;
        return ensure(ctx, ctx->zoom_corr, sizeof(double) * sp);
    }
    int refresh(tdoa_ctx *ctx) const override { return coarse.refresh(ctx); }
    // the locate's launches, then the window's scores around the best cells its finish left in ctx->locate_best and the zoom's
    // finish, on the words, clock differences and (fine) table scale the locate ran on
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
    {
        coarse.launch(ctx, Q, roots);
        const int32_t *table;
        const long long *cdiff;
        w.select(ctx, coarse, &table, &cdiff, &Q);
        const int32_t *best = ctx->locate_best.as<const int32_t>();
        long long *zmap = ctx->zoom_map.as<long long>();
        ClosureCand *part = ctx->zoom_part.as<ClosureCand>();
        const dim3 grid((unsigned)w.z.tiles, (unsigned)coarse.run.n_sets), one((unsigned)coarse.run.n_sets), block(kLocateThreads);
        hipStream_t st = ctx->stream;
        const LocateGeom g = w.gf;
        const LocateZoomGeom zg = w.z;
        locate_scores_dispatch(g.S, kLocateRegStations, cdiff != nullptr, [&](auto s, auto clk) {
            hipLaunchKernelGGL((k_locate_zoom_scores<decltype(s)::value, decltype(clk)::value>), grid, block, 0, st, Q, g, zg, table, cdiff, best, zmap, part);
        });
        hipLaunchKernelGGL(k_locate_zoom_finish, one, block, 0, st, Q, g, zg, table, cdiff, roots, best, static_cast<const long long *>(zmap),
                           static_cast<const ClosureCand *>(part), ctx->zoom_out.as<LocateZoomOut>(), ctx->zoom_lags.as<int32_t>(),
                           ctx->zoom_corr.as<double>());
    }
    int download(tdoa_ctx *ctx) const override
    {
        hipStream_t st = ctx->stream;
        const size_t n_sets = coarse.run.n_sets, sp = n_sets * w.gf.P;
        if (int rc = coarse.download(ctx)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(o.zoom, ctx->zoom_out.p, sizeof(LocateZoomOut) * n_sets, hipMemcpyDeviceToHost, st));
        if (o.lags) HIPCHK(ctx, hipMemcpyAsync(o.lags, ctx->zoom_lags.p, sizeof(int32_t) * sp, hipMemcpyDeviceToHost, st));
        if (o.corr) HIPCHK(ctx, hipMemcpyAsync(o.corr, ctx->zoom_corr.p, sizeof(double) * sp, hipMemcpyDeviceToHost, st));
        if (o.map) HIPCHK(ctx, hipMemcpyAsync(o.map, ctx->zoom_map.p, sizeof(int64_t) * n_sets * w.z.n_pos, hipMemcpyDeviceToHost, st));
        return TDOA_OK;
    }
};

}  // namespace

extern "C" {

int tdoa_process_locate_zoom(tdoa_ctx *ctx, int windows_per_stack, int min_separation, int Z, int H, int fine_separation,
                             tdoa_location *loc_host, int32_t *lags_host, double *corr_host, int64_t *map_host, tdoa_zoom *zoom_host,
                             int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host)
{
    LocateZoomSearch s(min_separation, Z, H, fine_separation, loc_host, lags_host, corr_host, map_host,
                       LocateZoomHost{zoom_host, zlags_host, zcorr_host, zmap_host});
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_locate_zoom(tdoa_group *g, int windows_per_stack, int min_separation, int Z, int H, int fine_separation,
                                   tdoa_location *loc_host, int32_t *lags_host, double *corr_host, int64_t *map_host, tdoa_zoom *zoom_host,
                                   int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host)
{
    LocateZoomSearch s(min_separation, Z, H, fine_separation, loc_host, lags_host, corr_host, map_host,
                       LocateZoomHost{zoom_host, zlags_host, zcorr_host, zmap_host});
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_debug_locate_zoom_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int min_separation, int Z, int H,
                                  int fine_separation, tdoa_location *loc, int32_t *lags, double *corr, int64_t *map, tdoa_zoom *zoom,
                                  int32_t *zlags, double *zcorr, int64_t *zmap)
{
    LocateZoomSearch s(min_separation, Z, H, fine_separation, loc, lags, corr, map, LocateZoomHost{zoom, zlags, zcorr, zmap});
    return debug_search_from_q(ctx, q, n_sets, 0, n_stations, n_w, s);
}

}  // extern "C"
