// locate_multi_zoom_api.inc -- the zoomed rounds (stack_locate_multi_zoom.hpp), host side: the search as a StackSearch
// (stack_search.inc) that holds the rounds (LocateSearch with rounds, locate_run.inc) for its coarse stage and the zoom's window
// (LocateFineWindow, locate_zoom_api.inc), and adds the masked window's two kernels behind the rounds' launches -- two launches
// for any K, the round a grid dimension -- and the search's three entries.  The K planes of the window maps, candidates, records,
// lags and correlations lie in the zoom locate's buffers; the counts have one of their own.
// Included by tdoa_mi355x.hip after locate_zoom_api.inc.

namespace {

// the outputs the zoomed rounds add to the rounds' (all but zoom may be NULL), all [round][set][...]
struct LocateMultiZoomHost {
    tdoa_zoom *zoom = nullptr;               // [round][set]
    int32_t *pairs = nullptr;                // [round][set][2]: pairs_in, reserved
    int32_t *lags = nullptr;                 // [round][set][pair], 1/U sample
    double *corr = nullptr;                  // [round][set][pair]
    int64_t *map = nullptr;                  // [round][set][(2H+1)^2]
};

struct LocateMultiZoomSearch : StackSearch {
    LocateSearch coarse;
    LocateFineWindow w;
    LocateMultiZoomHost o;

    LocateMultiZoomSearch(int n_emitters, int guard, int min_separation, int zoom, int half, int fine_separation, tdoa_location *loc,
                          int32_t *lags, double *corr, int64_t *map, const LocateMultiZoomHost &host)
        : StackSearch("the zoomed rounds with TDOA_LAGS_GO", nullptr),
          coarse(locate_search_call(true, n_emitters, guard, min_separation, loc, lags, corr, map)), w{zoom, half, fine_separation}, o(host)
    {
    }
    const char *check_args() const override
    {
        if (const char *bad = coarse.check_args()) return bad;
        if (const char *bad = w.check_args()) return bad;
        return o.zoom ? nullptr : "zoom_host is NULL";
    }
    int check_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what) const override
    {
        if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse_with(what, TDOA_ERR_UNSUPPORTED, go_what);
        if (const int rc = coarse.check_state(ctx, windows_per_stack, what)) return rc;
        return check_locate_fine(ctx, (int)ctx->caps.size(), what);
    }
    int check_sets(const tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what) const override
    {
        if (const int rc = coarse.check_sets(ctx, q, n_sets, track_len, n_stations, n_w, what)) return rc;
        return check_locate_fine(ctx, n_stations, what);
    }
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override
    {
        coarse.bind(ctx, sh);
        w.bind(ctx, coarse.run.g);
    }
    // the window and the fine table's shape (its contents are data), then the rounds' words (K and the guard among them)
    void key(std::vector<uint64_t> *key, int m) const override
    {
        w.key(key, StepProduct::LocateMultiZoom, (uint64_t)w.sep);
        coarse.key(key, m);
    }
    size_t planes() const { return (size_t)coarse.run.K * coarse.run.n_sets; }
    // the rounds' buffers and the centres (with K = 1 the rounds need none, the window's scores load their words), then K planes
    // of the window maps, the tiles' candidates, the records, the counts, lags and correlations
    int reserve(tdoa_ctx *ctx) const override
    {
        int rc;
        const size_t n = planes(), sp = (size_t)coarse.run.n_sets * w.gf.P;
        if ((rc = coarse.reserve(ctx))) return rc;
        if ((rc = ensure(ctx, ctx->locate_centres, sizeof(LocateCentres) * sp))) return rc;
        if (ensure(ctx, ctx->zoom_map, sizeof(long long) * n * w.z.n_pos)) {
            char buf[320];
            snprintf(buf, sizeof(buf), "the zoomed rounds' window maps [%d rounds][%d stacks][%d x %d positions] (%.1f MB) do not fit in device memory: %s",
                     coarse.run.K, coarse.run.n_sets, (int)w.z.side, (int)w.z.side, 8.0 * (double)n * (double)w.z.n_pos / 1e6, ctx->last_error.c_str());
            return fail(ctx, TDOA_ERR_NOMEM, buf);
        }
        if ((rc = ensure(ctx, ctx->zoom_part, sizeof(ClosureCand) * n * w.z.tiles))) return rc;
        if ((rc = ensure(ctx, ctx->zoom_out, sizeof(LocateZoomOut) * n))) return rc;
        if ((rc = ensure(ctx, ctx->mzoom_pairs, 2 * sizeof(int32_t) * n))) return rc;
        if ((rc = ensure(ctx, ctx->zoom_lags, sizeof(int32_t) * n * w.gf.P))) return rc;
        return ensure(ctx, ctx->zoom_corr, sizeof(double) * n * w.gf.P);
    }
    int refresh(tdoa_ctx *ctx) const override { return coarse.refresh(ctx); }
    // the rounds' launches, then every round's window at once: the scores around the cells the rounds' records keep in
    // ctx->locate_out under the centres in ctx->locate_centres, and the finish, on the words, clock differences and (fine) table
    // scale the rounds ran on.  The one place the two kernels are launched
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
    {
        coarse.launch(ctx, Q, roots);
        const int32_t *table;
        const long long *cdiff;
        w.select(ctx, coarse, &table, &cdiff, &Q);
        const LocateOut *rec = ctx->locate_out.as<const LocateOut>();
        const LocateCentres *centres = ctx->locate_centres.as<const LocateCentres>();
        long long *zmap = ctx->zoom_map.as<long long>();
        ClosureCand *part = ctx->zoom_part.as<ClosureCand>();
        const unsigned n_sets = (unsigned)coarse.run.n_sets, K = (unsigned)coarse.run.K;
        const dim3 grid((unsigned)w.z.tiles, n_sets, K), one(n_sets, K), block(kLocateThreads);
        hipStream_t st = ctx->stream;
        const LocateGeom g = w.gf;
        const LocateZoomGeom zg = w.z;
        const int guard = locate_mask(0, coarse.run.guard, g).guard;
        locate_scores_dispatch(g.S, kLocateZoomMaskedRegStations, cdiff != nullptr, [&](auto s, auto clk) {
            if constexpr (decltype(s)::value <= kLocateZoomMaskedRegStations)      // (the table's last case is the unmasked kernels' alone)
                hipLaunchKernelGGL((k_locate_zoom_scores_masked<decltype(s)::value, decltype(clk)::value>), grid, block, 0, st, Q, g, zg, table, cdiff,
                                   centres, guard, rec, zmap, part);
        });
        hipLaunchKernelGGL(k_locate_zoom_finish_masked, one, block, 0, st, Q, g, zg, table, cdiff, roots, centres, guard, rec,
                           static_cast<const long long *>(zmap), static_cast<const ClosureCand *>(part), ctx->zoom_out.as<LocateZoomOut>(),
                           ctx->mzoom_pairs.as<int32_t>(), ctx->zoom_lags.as<int32_t>(), ctx->zoom_corr.as<double>());
    }
    int download(tdoa_ctx *ctx) const override
    {
        hipStream_t st = ctx->stream;
        const size_t n = planes(), sp = n * w.gf.P;
        if (int rc = coarse.download(ctx)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(o.zoom, ctx->zoom_out.p, sizeof(LocateZoomOut) * n, hipMemcpyDeviceToHost, st));
        if (o.pairs) HIPCHK(ctx, hipMemcpyAsync(o.pairs, ctx->mzoom_pairs.p, 2 * sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        if (o.lags) HIPCHK(ctx, hipMemcpyAsync(o.lags, ctx->zoom_lags.p, sizeof(int32_t) * sp, hipMemcpyDeviceToHost, st));
        if (o.corr) HIPCHK(ctx, hipMemcpyAsync(o.corr, ctx->zoom_corr.p, sizeof(double) * sp, hipMemcpyDeviceToHost, st));
        if (o.map) HIPCHK(ctx, hipMemcpyAsync(o.map, ctx->zoom_map.p, sizeof(int64_t) * n * w.z.n_pos, hipMemcpyDeviceToHost, st));
        return TDOA_OK;
    }
};

}  // namespace

extern "C" {

int tdoa_process_locate_multi_zoom(tdoa_ctx *ctx, int windows_per_stack, int n_emitters, int guard, int min_separation, int Z, int H,
                                   int fine_separation, tdoa_location *loc_host, int32_t *lags_host, double *corr_host, int64_t *map_host,
                                   tdoa_zoom *zoom_host, int32_t *zpairs_host, int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host)
{
    LocateMultiZoomSearch s(n_emitters, guard, min_separation, Z, H, fine_separation, loc_host, lags_host, corr_host, map_host,
                            LocateMultiZoomHost{zoom_host, zpairs_host, zlags_host, zcorr_host, zmap_host});
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_locate_multi_zoom(tdoa_group *g, int windows_per_stack, int n_emitters, int guard, int min_separation, int Z, int H,
                                         int fine_separation, tdoa_location *loc_host, int32_t *lags_host, double *corr_host,
                                         int64_t *map_host, tdoa_zoom *zoom_host, int32_t *zpairs_host, int32_t *zlags_host,
                                         double *zcorr_host, int64_t *zmap_host)
{
    LocateMultiZoomSearch s(n_emitters, guard, min_separation, Z, H, fine_separation, loc_host, lags_host, corr_host, map_host,
                            LocateMultiZoomHost{zoom_host, zpairs_host, zlags_host, zcorr_host, zmap_host});
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_debug_locate_multi_zoom_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int n_emitters, int guard,
                                        int min_separation, int Z, int H, int fine_separation, tdoa_location *loc, int32_t *lags,
                                        double *corr, int64_t *map, tdoa_zoom *zoom, int32_t *zpairs, int32_t *zlags, double *zcorr,
                                        int64_t *zmap)
{
    LocateMultiZoomSearch s(n_emitters, guard, min_separation, Z, H, fine_separation, loc, lags, corr, map,
                            LocateMultiZoomHost{zoom, zpairs, zlags, zcorr, zmap});
    return debug_search_from_q(ctx, q, n_sets, 0, n_stations, n_w, s);
}

}  // extern "C"
