// locate_track_zoom_api.inc -- the zoomed cell tracks (stack_locate_track_zoom.hpp), host side: the search as a StackSearch
// (stack_search.inc) that holds the cell tracks (LocateSearch, locate_run.inc) for its coarse stage and adds the windows' scores,
// the recurrence and its finish behind that search's launches, and the search's three entries.  What it needs of the fine table
// is the zoom locate's check (check_locate_fine); the window maps, their tiles' candidates and the fine lags and
// correlations lie in the zoom locate's buffers, which have their shapes.
// Included by tdoa_mi355x.hip after locate_zoom_api.inc.

namespace {

// the outputs the zoomed tracks add to the tracks' (all but track may be NULL)
struct LocateTrackZoomHost {
    tdoa_cell_track *track = nullptr;        // [track]
    int32_t *cells = nullptr;                // [track][L], fine cells
    int64_t *own = nullptr;                  // [track][L]
    int32_t *lags = nullptr;                 // [set][pair], 1/U sample
    double *corr = nullptr;                  // [set][pair]
    int64_t *map = nullptr;                  // [set][(2H+1)^2]
    int64_t *total = nullptr;                // [track][(2H+1)^2]
};

struct LocateTrackZoomSearch : StackSearch {
    LocateSearch coarse;
    LocateFineWindow w;                      // (locate_zoom_api.inc)
    int Jf;                                  // fine_step
    LocateTrackZoomHost o;
    TrackZoomGeom tz{};

    LocateTrackZoomSearch(int max_step, int min_separation, int zoom, int half, int fine_step, int fine_separation, tdoa_cell_track *track,
                          int32_t *cells, int64_t *own, int32_t *lags, double *corr, int64_t *total, const LocateTrackZoomHost &host)
        : StackSearch("the zoomed cell tracks with TDOA_LAGS_GO", nullptr),
          coarse(locate_track_call(false, max_step, 1, 0, min_separation, track, cells, own, nullptr, lags, corr, total)),
          w{zoom, half, fine_separation}, Jf(fine_step), o(host)
    {
    }
    const char *check_args() const override
    {
        if (const char *bad = coarse.check_args()) return bad;
        if (const char *bad = w.check_args(Jf < 0 || Jf > kTrackZoomMaxStep ? "fine_step outside 0 .. 16" : nullptr)) return bad;
        return o.track ? nullptr : "ztrack_host is NULL";
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
        tz.L = coarse.run.L;
        tz.Jf = Jf;
        tz.n_sets = coarse.run.n_sets;
    }
    // the window, the fine step and the fine table's shape (its contents are data), then the tracks' words
    void key(std::vector<uint64_t> *key, int m) const override
    {
        w.key(key, StepProduct::LocateTrackZoom, (uint64_t)Jf | ((uint64_t)w.sep << 32));
        coarse.key(key, m);
    }
    // the tracks' buffers, then the window maps, the steps E and the sums F_0 (the three that can be large), the tiles'
    // candidates, the centres, the records, cells, own scores, lags and correlations
    int reserve(tdoa_ctx *ctx) const override
    {
        int rc;
        const size_t n_sets = coarse.run.n_sets, n_tracks = coarse.run.n_tracks(), sp = n_sets * w.gf.P;
        if ((rc = coarse.reserve(ctx))) return rc;
        if (ensure(ctx, ctx->zoom_map, sizeof(long long) * n_sets * w.z.n_pos) || ensure(ctx, ctx->tzoom_e, 2 * n_sets * w.z.n_pos) ||
            ensure(ctx, ctx->tzoom_total, sizeof(long long) * n_tracks * w.z.n_pos)) {
            char buf[400];
            snprintf(buf, sizeof(buf),
                     "the zoomed cell tracks' window maps [%zu stacks][%d x %d positions] (%.1f MB), steps (%.1f MB) and sums [%zu tracks] (%.1f MB) "
                     "do not fit in device memory: %s",
                     n_sets, (int)w.z.side, (int)w.z.side, 8.0 * (double)n_sets * (double)w.z.n_pos / 1e6, 2.0 * (double)n_sets * (double)w.z.n_pos / 1e6,
                     n_tracks, 8.0 * (double)n_tracks * (double)w.z.n_pos / 1e6, ctx->last_error.c_str());
            return fail(ctx, TDOA_ERR_NOMEM, buf);
        }
        if ((rc = ensure(ctx, ctx->zoom_part, sizeof(ClosureCand) * n_sets * w.z.tiles))) return rc;
        if ((rc = ensure(ctx, ctx->tzoom_centre, sizeof(int32_t) * n_sets))) return rc;
        if ((rc = ensure(ctx, ctx->tzoom_out, sizeof(CellTrackOut) * n_tracks))) return rc;
        if ((rc = ensure(ctx, ctx->tzoom_cells, sizeof(int32_t) * n_sets))) return rc;
        if ((rc = ensure(ctx, ctx->tzoom_own, sizeof(long long) * n_sets))) return rc;
        if ((rc = ensure(ctx, ctx->zoom_lags, sizeof(int32_t) * sp))) return rc;
        if ((rc = ensure(ctx, ctx->zoom_corr, sizeof(double) * sp))) return rc;
        rc = TDOA_OK;
        track_zoom_steps_dispatch(w.z.side, [&](auto rows, auto cols) {
            rc = set_lds(ctx, k_track_zoom_steps<decltype(rows)::value, decltype(cols)::value>, track_zoom_lds_bytes(w.z.n_pos));
        });
        return rc;
    }
    int refresh(tdoa_ctx *ctx) const override { return coarse.refresh(ctx); }
    // the tracks' launches, then the centres from the cells and records their finish left on the device, the windows' scores
    // around them, the recurrence and the finish, on the words, clock differences and (fine) table scale the tracks ran on
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
    {
        coarse.launch(ctx, Q, roots);
        const int32_t *table;
        const long long *cdiff;
        w.select(ctx, coarse, &table, &cdiff, &Q);
        const unsigned n_sets = (unsigned)coarse.run.n_sets, n_tracks = (unsigned)coarse.run.n_tracks();
        const LocateRound p = locate_run_round(ctx, coarse.run, 0);
        int32_t *centre = ctx->tzoom_centre.as<int32_t>();
        long long *zmap = ctx->zoom_map.as<long long>(), *total = ctx->tzoom_total.as<long long>();
        signed char *E = ctx->tzoom_e.as<signed char>();
        const dim3 grid((unsigned)w.z.tiles, n_sets), block(kLocateThreads);
        hipStream_t st = ctx->stream;
        const LocateGeom g = w.gf;
        const LocateZoomGeom zg = w.z;
        const TrackZoomGeom tg = tz;
        hipLaunchKernelGGL(k_track_zoom_centres, dim3((n_sets + kLocateThreads - 1) / kLocateThreads), block, 0, st, tg,
                           static_cast<const int32_t *>(p.cells), static_cast<const CellTrackOut *>(p.track), centre);
        locate_scores_dispatch(g.S, kLocateRegStations, cdiff != nullptr, [&](auto s, auto clk) {
            hipLaunchKernelGGL((k_locate_zoom_scores<decltype(s)::value, decltype(clk)::value>), grid, block, 0, st, Q, g, zg, table, cdiff,
                               static_cast<const int32_t *>(centre), zmap, ctx->zoom_part.as<ClosureCand>());
        });
        track_zoom_steps_dispatch(zg.side, [&](auto rows, auto cols) {
            hipLaunchKernelGGL((k_track_zoom_steps<decltype(rows)::value, decltype(cols)::value>), dim3(n_tracks), dim3(kTrackZoomThreads),
                               track_zoom_lds_bytes(zg.n_pos), st, zg, tg, static_cast<const int32_t *>(centre), static_cast<const long long *>(zmap), E,
                               total);
        });
        hipLaunchKernelGGL(k_track_zoom_finish, dim3(n_tracks), block, 0, st, Q, g, zg, tg, table, cdiff, roots, ctx->ctrack_roots.as<const double>(),
                           static_cast<const int32_t *>(centre), static_cast<const long long *>(zmap), static_cast<const signed char *>(E),
                           static_cast<const long long *>(total), ctx->tzoom_out.as<CellTrackOut>(), ctx->tzoom_cells.as<int32_t>(),
                           ctx->tzoom_own.as<long long>(), ctx->zoom_lags.as<int32_t>(), ctx->zoom_corr.as<double>());
    }
    int download(tdoa_ctx *ctx) const override
    {
        hipStream_t st = ctx->stream;
        const size_t n_sets = coarse.run.n_sets, n_tracks = coarse.run.n_tracks(), sp = n_sets * w.gf.P;
        if (int rc = coarse.download(ctx)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(o.track, ctx->tzoom_out.p, sizeof(CellTrackOut) * n_tracks, hipMemcpyDeviceToHost, st));
        if (o.cells) HIPCHK(ctx, hipMemcpyAsync(o.cells, ctx->tzoom_cells.p, sizeof(int32_t) * n_sets, hipMemcpyDeviceToHost, st));
        if (o.own) HIPCHK(ctx, hipMemcpyAsync(o.own, ctx->tzoom_own.p, sizeof(int64_t) * n_sets, hipMemcpyDeviceToHost, st));
        if (o.lags) HIPCHK(ctx, hipMemcpyAsync(o.lags, ctx->zoom_lags.p, sizeof(int32_t) * sp, hipMemcpyDeviceToHost, st));
        if (o.corr) HIPCHK(ctx, hipMemcpyAsync(o.corr, ctx->zoom_corr.p, sizeof(double) * sp, hipMemcpyDeviceToHost, st));
        if (o.map) HIPCHK(ctx, hipMemcpyAsync(o.map, ctx->zoom_map.p, sizeof(int64_t) * n_sets * w.z.n_pos, hipMemcpyDeviceToHost, st));
        if (o.total) HIPCHK(ctx, hipMemcpyAsync(o.total, ctx->tzoom_total.p, sizeof(int64_t) * n_tracks * w.z.n_pos, hipMemcpyDeviceToHost, st));
        return TDOA_OK;
    }
};

}  // namespace

extern "C" {

int tdoa_process_locate_track_zoom(tdoa_ctx *ctx, int windows_per_stack, int max_step, int min_separation, int Z, int H, int fine_step,
                                   int fine_separation, tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host, int32_t *lags_host,
                                   double *corr_host, int64_t *total_host, tdoa_cell_track *ztrack_host, int32_t *zcells_host,
                                   int64_t *zown_host, int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host, int64_t *ztotal_host)
{
    LocateTrackZoomSearch s(max_step, min_separation, Z, H, fine_step, fine_separation, track_host, cells_host, own_host, lags_host, corr_host,
                            total_host, LocateTrackZoomHost{ztrack_host, zcells_host, zown_host, zlags_host, zcorr_host, zmap_host, ztotal_host});
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_locate_track_zoom(tdoa_group *g, int windows_per_stack, int max_step, int min_separation, int Z, int H, int fine_step,
                                         int fine_separation, tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host,
                                         int32_t *lags_host, double *corr_host, int64_t *total_host, tdoa_cell_track *ztrack_host,
                                         int32_t *zcells_host, int64_t *zown_host, int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host,
                                         int64_t *ztotal_host)
{
    LocateTrackZoomSearch s(max_step, min_separation, Z, H, fine_step, fine_separation, track_host, cells_host, own_host, lags_host, corr_host,
                            total_host, LocateTrackZoomHost{ztrack_host, zcells_host, zown_host, zlags_host, zcorr_host, zmap_host, ztotal_host});
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_debug_locate_track_zoom_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int max_step,
                                        int min_separation, int Z, int H, int fine_step, int fine_separation, tdoa_cell_track *track,
                                        int32_t *cells, int64_t *own, int32_t *lags, double *corr, int64_t *total, tdoa_cell_track *ztrack,
                                        int32_t *zcells, int64_t *zown, int32_t *zlags, double *zcorr, int64_t *zmap, int64_t *ztotal)
{
    LocateTrackZoomSearch s(max_step, min_separation, Z, H, fine_step, fine_separation, track, cells, own, lags, corr, total,
                            LocateTrackZoomHost{ztrack, zcells, zown, zlags, zcorr, zmap, ztotal});
    return debug_search_from_q(ctx, q, n_sets, track_len, n_stations, n_w, s);
}

}  // extern "C"
