// sync_locate_api.inc -- from reference blocks to fix in one call (include/tdoa_mi355x.h: "clocks to fix in one call" and
// "free-running clocks to fix in one call"), host side.  A chain is a StackSearch (stack_search.inc) that holds a fine clock stage
// and a locate stage and puts k_line_mix (stack_line_mix.hpp) between their launches, so that the stacks' clocks go from the one to
// the other on the device, inside one step graph behind one accumulation of the stacks.  The locate stage runs under the call's
// own clock differences (LocateClocks, locate_run.inc): the context's clock table is neither read nor changed.  SyncChain states
// that once; what a chain's fine stage answers for it -- which device words the link reads, what an absent mix stands for, the
// bound on a row -- is a small description each:
//   ClockChain   the fine clock search (SyncFineSearch, sync_fine_api.inc) -> the zoom locate (LocateZoomSearch,
//                locate_zoom_api.inc); the link reads sfine_clock, no rates
//   LineChain    the fine clock lines (SyncLineFineSearch, sync_drift_fine_api.inc) -> the zoomed cell tracks
//                (LocateTrackZoomSearch, locate_track_zoom_api.inc); the link reads slfine_clock and slfine_rate
// The two held searches share no device buffer (the clock stages write sync_*, sfine_*, sline_* and slfine_*, the locate stages
// locate_*, ctrack_*, zoom_*, tzoom_* and the statistics' mstat_*); the link writes mix_*.  Also the host-only statements of the
// rule and the kernel alone on the caller's words.
// Included by tdoa_mi355x.hip after the four searches' files.

namespace {

static_assert(sizeof(LineMix) == sizeof(tdoa_line_mix) && sizeof(tdoa_line_mix) == 24, "tdoa_line_mix layout");
static_assert(sizeof(tdoa_clock_mix) == 16, "tdoa_clock_mix layout");
static_assert(kLocateDelayUnit * kSyncFineMaxCentre == 1ll << 31, "a clock in 1/16 sample below 2^31 is |centre| + margin below 2^27");

// an entry as the kernel takes it; what the check calls an entry's sources
LineMix widen(const tdoa_clock_mix &e) { return LineMix{e.a, 0, e.b, 0, e.wa, e.wb}; }
LineMix widen(const tdoa_line_mix &e) { return LineMix{e.a, e.xa, e.b, e.xb, e.wa, e.wb}; }
const char *mix_outside(const tdoa_clock_mix *) { return "a mix entry names a stack outside 0 .. n_stacks - 1"; }
const char *mix_outside(const tdoa_line_mix *) { return "a mix entry names a line outside 0 .. n_lines - 1"; }

// what every entry refuses of m mix entries over n sources; nullptr when they are in range
template <class Mix> const char *check_mix(const Mix *mix, int m, int n)
{
    for (int t = 0; mix && t < m; t++) {
        const LineMix e = widen(mix[t]);
        if (e.a < 0 || e.a >= n || e.b < 0 || e.b >= n) return mix_outside(mix);
        if (e.xa < -kLineMixMaxX || e.xa > kLineMixMaxX || e.xb < -kLineMixMaxX || e.xb > kLineMixMaxX) return "a mix entry's |xa| or |xb| above 65535";
        if (e.wa < 0 || e.wb < 0) return "a mix entry has a negative weight";
        if ((long long)e.wa + e.wb < 1 || (long long)e.wa + e.wb > kClockMixMaxDen) return "a mix entry's wa + wb outside 1 .. 65536";
    }
    return nullptr;
}

// the largest |x| of m checked entries, at least L - 1 (the lines' own positions)
template <class Mix> long long mix_reach(const Mix *mix, int m, int L)
{
    long long X = L - 1;
    for (int t = 0; mix && t < m; t++) X = std::max<long long>(X, std::max(std::abs(widen(mix[t]).xa), std::abs(widen(mix[t]).xb)));
    return X;
}

// whether a continued clock of the caller's words leaves int32
bool line_mix_overflows(const int32_t *clock16, const int32_t *fine_rate, int S, long long den, const tdoa_line_mix *mix, int m)
{
    for (int t = 0; t < m; t++)
        for (int s = 0; s < S; s++) {
            const size_t ia = (size_t)mix[t].a * S + s, ib = (size_t)mix[t].b * S + s;
            if (std::llabs(line_cont(clock16[ia], fine_rate[ia], mix[t].xa, den)) > INT32_MAX ||
                std::llabs(line_cont(clock16[ib], fine_rate[ib], mix[t].xb, den)) > INT32_MAX)
                return true;
        }
    return false;
}

// the rule on the host: the kernel's row, rate nullptr as there
template <class Mix> void mix_rows(const int32_t *c16, const int32_t *rate, int S, long long den, const Mix *mix, int n_rows, int32_t *rows)
{
    for (int t = 0; t < n_rows; t++)
        for (int s = 0; s < S; s++) {
            const LineMix e = widen(mix[t]);
            rows[(size_t)t * S + s] = clock_mix_row(line_mix_source(c16, rate, (size_t)e.a * S + s, e.xa, den),
                                                    line_mix_source(c16, rate, (size_t)e.b * S + s, e.xb, den), e.wa, e.wb);
        }
}

// the link's one launch on the entries in ctx->mix_in; rate nullptr: the clocks as they are (den is not read)
void launch_line_mix(tdoa_ctx *ctx, const int32_t *c16, const int32_t *rate, int n_sets, int S, long long den, int U_loc)
{
    hipLaunchKernelGGL(k_line_mix, dim3((unsigned)n_sets), dim3(kLineMixThreads), 0, ctx->stream, c16, rate, ctx->mix_in.as<const LineMix>(), S,
                       S * (S - 1) / 2, den, U_loc, ctx->mix_rows.as<int32_t>(), ctx->mix_cdiff.as<long long>(), ctx->mix_cdiff_up.as<long long>());
}

// the entries, the rows, the differences and U_loc x them for n_sets stacks of S stations
int ensure_line_mix(tdoa_ctx *ctx, size_t n_sets, int S)
{
    int rc;
    const size_t sp = n_sets * (size_t)(S * (S - 1) / 2);
    if ((rc = ensure(ctx, ctx->mix_in, sizeof(LineMix) * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->mix_rows, sizeof(int32_t) * n_sets * S))) return rc;
    if ((rc = ensure(ctx, ctx->mix_cdiff, sizeof(long long) * sp))) return rc;
    return ensure(ctx, ctx->mix_cdiff_up, sizeof(long long) * sp);
}

// ---- what the chains' fine stages answer ---------------------------------------------------------------------------------------
// the device words the link reads (buffers, not pointers: a reserve between bind and launch may move them) and the lines' U D
struct LinkWords {
    const DevBuf *clock, *rate;              // rate nullptr: none
    long long den;
};

struct ClockChain {
    using Fine = SyncFineSearch;
    using Locate = LocateZoomSearch;
    using Mix = tdoa_clock_mix;
    static constexpr StepProduct::Kind kind = StepProduct::SyncLocate;
    static constexpr const char *go_what = "clocks to fix in one call with TDOA_LAGS_GO";
    static constexpr const char *row_what = nullptr;         // |row| <= 16 (|centre| + gate + 1), which the fine stage has bounded
    static int stations(const Fine &f) { return f.coarse.g.S; }
    static LinkWords words(const tdoa_ctx *ctx, const Fine &) { return LinkWords{&ctx->sfine_clock, nullptr, 1}; }
    static int sources(int n_sets, int) { return n_sets; }
    static LineMix own(int t, int) { return LineMix{t, 0, t, 0, 1, 0}; }      // every stack its own clock
    static long long margin(const Fine &f, long long) { return f.coarse.G + 1; }
};

struct LineChain {
    using Fine = SyncLineFineSearch;
    using Locate = LocateTrackZoomSearch;
    using Mix = tdoa_line_mix;
    static constexpr StepProduct::Kind kind = StepProduct::SyncDriftLocate;
    static constexpr const char *go_what = "free-running clocks to fix in one call with TDOA_LAGS_GO";
    static constexpr const char *row_what = "|centre| + gate + 2 + ((max_drift + 1) X) div drift_den >= 2^27, X the larger of L - 1 and the mix's largest |x|: "
                                            "a row in 1/16 sample would not fit int32";
    static int stations(const Fine &f) { return f.fg.S; }
    static LinkWords words(const tdoa_ctx *ctx, const Fine &f) { return LinkWords{&ctx->slfine_clock, &ctx->slfine_rate, (long long)f.U * f.coarse.D}; }
    static int sources(int n_sets, int L) { return n_sets / L; }
    static LineMix own(int t, int L) { return LineMix{t / L, t % L, t / L, t % L, 1, 0}; }      // every stack its own line at its own position
    // |clock16| <= 16 (|centre| + gate + 1) and |fine_rate| <= U (max_drift + 1), so a line continued to |x| <= X stays below
    // 16 (|centre| + gate + 2 + ((max_drift + 1) X) div drift_den)
    static long long margin(const Fine &f, long long X) { return f.coarse.G + 2 + ((long long)f.coarse.H + 1) * X / f.coarse.D; }
};

// ---- the chain -------------------------------------------------------------------------------------------------------------------
// The checks' order is the fine stage, the mix and (where the description words one) the rows' size, the locate stage, then
// U_loc x a row, which must fit 32 bits like U_loc x a clock table's entry.  |row| <= 16 (|centre| + margin): a convex combination.
template <class D> struct SyncChain : StackSearch {
    typename D::Fine fine;
    typename D::Locate zoom;
    const typename D::Mix *mix;              // [set], NULL: D::own
    int32_t *rows;                           // [set][station], may be NULL
    std::vector<LineMix> mix_in;             // bind: the mix as it is uploaded

    SyncChain(const typename D::Fine &f, const typename D::Mix *mix, int32_t *rows_host, const typename D::Locate &z)
        : StackSearch(D::go_what, nullptr), fine(f), zoom(z), mix(mix), rows(rows_host)
    {
        zoom.coarse.own_clocks = true;       // before the checks: they ask nothing of the context's clock table
    }
    const char *check_args() const override
    {
        if (const char *bad = fine.check_args()) return bad;
        return zoom.check_args();
    }
    // whether scale x the rows' bound leaves 32 bits at one of S stations
    bool row_overflows(int n_sets, int L, int S, long long scale) const
    {
        const long long margin = D::margin(fine, mix_reach(mix, n_sets, L));
        for (int s = 0; s < S; s++)
            if (scale * kLocateDelayUnit * (std::llabs(fine.coarse.centre ? (long long)fine.coarse.centre[s] : 0ll) + margin) >= (1ll << 31)) return true;
        return false;
    }
    int check_rows(int n_sets, int L, int S, const char **what) const
    {
        if (const char *bad = check_mix(mix, n_sets, D::sources(n_sets, L))) return refuse_with(what, TDOA_ERR_INVALID, bad);
        if (D::row_what && row_overflows(n_sets, L, S, 1)) return refuse_with(what, TDOA_ERR_INVALID, D::row_what);
        return TDOA_OK;
    }
    int check_scaled(const tdoa_ctx *ctx, int n_sets, int L, int S, const char **what) const
    {
        if (ctx->locate_up > 1 && row_overflows(n_sets, L, S, ctx->locate_up))
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "a clock table entry times the upsampling factor does not fit 32 bits");
        return TDOA_OK;
    }
    int check_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what) const override
    {
        if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse_with(what, TDOA_ERR_UNSUPPORTED, go_what);
        if (const int rc = fine.check_state(ctx, windows_per_stack, what)) return rc;
        int wpb = 0;
        (void)tdoa_num_windows(ctx, &wpb, nullptr);
        const StackGeom sg = stack_geom(wpb, windows_per_stack);
        const int S = (int)ctx->caps.size();
        if (const int rc = check_rows(sg.n_stacks, sg.spb, S, what)) return rc;
        if (const int rc = zoom.check_state(ctx, windows_per_stack, what)) return rc;
        return check_scaled(ctx, sg.n_stacks, sg.spb, S, what);
    }
    int check_sets(const tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what) const override
    {
        if (const int rc = fine.check_sets(ctx, q, n_sets, track_len, n_stations, n_w, what)) return rc;
        if (const int rc = check_rows(n_sets, track_len, n_stations, what)) return rc;
        if (const int rc = zoom.check_sets(ctx, q, n_sets, track_len, n_stations, n_w, what)) return rc;
        return check_scaled(ctx, n_sets, track_len, n_stations, what);
    }
    // both stages on the same sets; a clock-mix entry is widened here and lives until the call has synchronised
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override
    {
        fine.bind(ctx, sh);
        zoom.coarse.clocks = LocateClocks{&ctx->mix_cdiff, &ctx->mix_cdiff_up};
        zoom.bind(ctx, sh);
        mix_in.resize((size_t)sh.n_sets);
        for (int t = 0; t < sh.n_sets; t++) mix_in[t] = mix ? widen(mix[t]) : D::own(t, sh.L);
    }
    // both held searches' words; the locate stage's clock flag is on (the mix is data)
    void key(std::vector<uint64_t> *key, int m) const override
    {
        key->push_back(D::kind);
        fine.key(key, m);
        zoom.key(key, m);
    }
    int reserve(tdoa_ctx *ctx) const override
    {
        if (int rc = fine.reserve(ctx)) return rc;
        if (int rc = ensure_line_mix(ctx, mix_in.size(), D::stations(fine))) return rc;
        return zoom.reserve(ctx);
    }
    // the fine stage's inputs, the mix, the locate stage's: a call that changes only them replays the same graph
    int refresh(tdoa_ctx *ctx) const override
    {
        if (int rc = fine.refresh(ctx)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->mix_in.p, mix_in.data(), sizeof(LineMix) * mix_in.size(), hipMemcpyHostToDevice, ctx->stream));
        return zoom.refresh(ctx);
    }
    // the fine stage, the rows and differences from the words it left on the device, the locate stage under them
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
    {
        fine.launch(ctx, Q, roots);
        const LinkWords w = D::words(ctx, fine);
        launch_line_mix(ctx, w.clock->as<const int32_t>(), w.rate ? w.rate->as<const int32_t>() : nullptr, (int)mix_in.size(),
                        D::stations(fine), w.den, zoom.coarse.run.U);
        zoom.launch(ctx, Q, roots);
    }
    int download(tdoa_ctx *ctx) const override
    {
        if (int rc = fine.download(ctx)) return rc;
        if (rows)
            HIPCHK(ctx, hipMemcpyAsync(rows, ctx->mix_rows.p, sizeof(int32_t) * mix_in.size() * D::stations(fine), hipMemcpyDeviceToHost, ctx->stream));
        return zoom.download(ctx);
    }
};

// k_line_mix alone on the caller's words (the clocks, then the rates if there are any, into mix_debug) and n_rows entries of
// LineMix's layout, with U_loc an argument (the context's setting is not read): the rows, the pairs' differences and U_loc x them
int debug_mix(tdoa_ctx *ctx, const int32_t *clock16, const int32_t *fine_rate, int n_sources, int n_stations, long long den, const void *mix,
              int n_rows, int U_loc, int32_t *rows, int64_t *cdiff, int64_t *cdiff_up)
{
    int rc;
    const size_t S = (size_t)n_stations, words = (size_t)n_sources * S, sp = (size_t)n_rows * (S * (S - 1) / 2);
    if ((rc = check_ctx(ctx))) return rc;
    if ((rc = ensure(ctx, ctx->mix_debug, (fine_rate ? 2 : 1) * sizeof(int32_t) * words))) return rc;
    if ((rc = ensure_line_mix(ctx, (size_t)n_rows, n_stations))) return rc;
    hipStream_t st = ctx->stream;
    int32_t *in = ctx->mix_debug.as<int32_t>();
    HIPCHK(ctx, hipMemcpyAsync(in, clock16, sizeof(int32_t) * words, hipMemcpyHostToDevice, st));
    if (fine_rate) HIPCHK(ctx, hipMemcpyAsync(in + words, fine_rate, sizeof(int32_t) * words, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->mix_in.p, mix, sizeof(LineMix) * (size_t)n_rows, hipMemcpyHostToDevice, st));
    launch_line_mix(ctx, in, fine_rate ? in + words : nullptr, n_rows, n_stations, den, U_loc);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(rows, ctx->mix_rows.p, sizeof(int32_t) * (size_t)n_rows * S, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(cdiff, ctx->mix_cdiff.p, sizeof(long long) * sp, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(cdiff_up, ctx->mix_cdiff_up.p, sizeof(long long) * sp, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return TDOA_OK;
}

}  // namespace

extern "C" {

// ---- clocks to fix in one call ------------------------------------------------------------------------------------------------
#define TDOA_SYNC_LOCATE_SEARCH(s)                                                                                               \
    SyncChain<ClockChain> s(SyncFineSearch(gate, rounds, U, fine_rounds, ref_delay, centre, SyncHost{sync_host, clock_host, lags_host, corr_host}, \
                                           SyncFineHost{fine_host, clock16_host, fine_lags_host, fine_corr_host}),              \
                            mix, rows_host,                                                                                      \
                            LocateZoomSearch(min_separation, Z, H, fine_separation, loc_host, loc_lags_host, loc_corr_host, map_host, \
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
    if (check_mix(mix, n_rows, n_stacks)) return TDOA_ERR_INVALID;
    mix_rows(clock16, nullptr, n_stations, 1, mix, n_rows, rows);
    return TDOA_OK;
}

// the kernel alone on the caller's clocks, of any size: no rates, so nothing is continued and nothing can leave int32
int tdoa_debug_clock_mix(tdoa_ctx *ctx, const int32_t *clock16, int n_stacks, int n_stations, const tdoa_clock_mix *mix, int n_rows, int U_loc,
                         int32_t *rows, int64_t *cdiff, int64_t *cdiff_up)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (!clock16 || !mix || !rows || !cdiff || !cdiff_up || n_stacks < 1 || n_stacks > kLocateMaxSets || n_rows < 1 || n_rows > kLocateMaxSets ||
        n_stations < 2 || n_stations > kLocateMaxStations || !upsample_factor_ok(U_loc))
        return fail(ctx, TDOA_ERR_INVALID, "a pointer is NULL, n_stacks or n_rows outside 1 .. 65535, n_stations outside 2 .. 64 or U_loc is not one of 1, 2, 4, 8, 16");
    if (const char *bad = check_mix(mix, n_rows, n_stacks)) return fail(ctx, TDOA_ERR_INVALID, bad);
    std::vector<LineMix> wide((size_t)n_rows);
    for (int t = 0; t < n_rows; t++) wide[t] = widen(mix[t]);
    return debug_mix(ctx, clock16, nullptr, n_stacks, n_stations, 1, wide.data(), n_rows, U_loc, rows, cdiff, cdiff_up);
}

// ---- free-running clocks to fix in one call -----------------------------------------------------------------------------------
#define TDOA_SYNC_DRIFT_LOCATE_SEARCH(s)                                                                                         \
    SyncChain<LineChain> s(SyncLineFineSearch(gate, max_drift, drift_den, rounds, U, fine_rounds, ref_delay, centre,             \
                                              SyncLineHost{line_host, clock_host, rate_host, rows_host, lags_host, corr_host},   \
                                              SyncLineFineHost{fine_host, clock16_host, fine_rate_host, fine_rows_host, fine_lags_host, fine_corr_host}), \
                           mix, mix_rows_host,                                                                                   \
                           LocateTrackZoomSearch(max_step, min_separation, Z, H, fine_step, fine_separation, track_host, cells_host, own_host, \
                                                 loc_lags_host, loc_corr_host, total_host,                                       \
                                                 LocateTrackZoomHost{ztrack_host, zcells_host, zown_host, zlags_host, zcorr_host, zmap_host, ztotal_host}))

int tdoa_process_sync_drift_locate(tdoa_ctx *ctx, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds, int U,
                                   int fine_rounds, const int32_t *ref_delay, const int32_t *centre, const tdoa_line_mix *mix, int max_step,
                                   int min_separation, int Z, int H, int fine_step, int fine_separation, tdoa_sync_line *line_host,
                                   int32_t *clock_host, int32_t *rate_host, int32_t *rows_host, int32_t *lags_host, double *corr_host,
                                   tdoa_sync_line *fine_host, int32_t *clock16_host, int32_t *fine_rate_host, int32_t *fine_rows_host,
                                   int32_t *fine_lags_host, double *fine_corr_host, int32_t *mix_rows_host, tdoa_cell_track *track_host,
                                   int32_t *cells_host, int64_t *own_host, int32_t *loc_lags_host, double *loc_corr_host, int64_t *total_host,
                                   tdoa_cell_track *ztrack_host, int32_t *zcells_host, int64_t *zown_host, int32_t *zlags_host,
                                   double *zcorr_host, int64_t *zmap_host, int64_t *ztotal_host)
{
    TDOA_SYNC_DRIFT_LOCATE_SEARCH(s);
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_sync_drift_locate(tdoa_group *g, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds, int U,
                                         int fine_rounds, const int32_t *ref_delay, const int32_t *centre, const tdoa_line_mix *mix,
                                         int max_step, int min_separation, int Z, int H, int fine_step, int fine_separation,
                                         tdoa_sync_line *line_host, int32_t *clock_host, int32_t *rate_host, int32_t *rows_host,
                                         int32_t *lags_host, double *corr_host, tdoa_sync_line *fine_host, int32_t *clock16_host,
                                         int32_t *fine_rate_host, int32_t *fine_rows_host, int32_t *fine_lags_host, double *fine_corr_host,
                                         int32_t *mix_rows_host, tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host,
                                         int32_t *loc_lags_host, double *loc_corr_host, int64_t *total_host, tdoa_cell_track *ztrack_host,
                                         int32_t *zcells_host, int64_t *zown_host, int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host,
                                         int64_t *ztotal_host)
{
    TDOA_SYNC_DRIFT_LOCATE_SEARCH(s);
    return group_process_search(g, windows_per_stack, s);
}

// set t * track_len + x is position x of line and track t
int tdoa_debug_sync_drift_locate_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int gate,
                                        int max_drift, int drift_den, int rounds, int U, int fine_rounds, const int32_t *ref_delay,
                                        const int32_t *centre, const tdoa_line_mix *mix, int max_step, int min_separation, int Z, int H,
                                        int fine_step, int fine_separation, tdoa_sync_line *line_host, int32_t *clock_host, int32_t *rate_host,
                                        int32_t *rows_host, int32_t *lags_host, double *corr_host, tdoa_sync_line *fine_host,
                                        int32_t *clock16_host, int32_t *fine_rate_host, int32_t *fine_rows_host, int32_t *fine_lags_host,
                                        double *fine_corr_host, int32_t *mix_rows_host, tdoa_cell_track *track_host, int32_t *cells_host,
                                        int64_t *own_host, int32_t *loc_lags_host, double *loc_corr_host, int64_t *total_host,
                                        tdoa_cell_track *ztrack_host, int32_t *zcells_host, int64_t *zown_host, int32_t *zlags_host,
                                        double *zcorr_host, int64_t *zmap_host, int64_t *ztotal_host)
{
    TDOA_SYNC_DRIFT_LOCATE_SEARCH(s);
    return debug_search_from_q(ctx, q, n_sets, track_len, n_stations, n_w, s);
}
#undef TDOA_SYNC_DRIFT_LOCATE_SEARCH

// Host only: the plain-C statement of the rule, tdoa_sync_line_clock16's with x of either sign and tdoa_clock_mix_rows' mean
int tdoa_line_mix_rows(const int32_t *clock16, const int32_t *fine_rate, int n_lines, int n_stations, int U, int drift_den,
                       const tdoa_line_mix *mix, int n_rows, int32_t *rows)
{
    if (!clock16 || !fine_rate || !mix || !rows || n_lines < 1 || n_stations < 1 || n_rows < 1 || !sync_fine_factor_ok(U) || drift_den < 1)
        return TDOA_ERR_INVALID;
    if (check_mix(mix, n_rows, n_lines)) return TDOA_ERR_INVALID;
    const long long den = (long long)U * drift_den;
    if (line_mix_overflows(clock16, fine_rate, n_stations, den, mix, n_rows)) return TDOA_ERR_INVALID;
    mix_rows(clock16, fine_rate, n_stations, den, mix, n_rows, rows);
    return TDOA_OK;
}

// the kernel alone on the caller's words: they are the caller's, so the host looks at every continued clock before the launch
int tdoa_debug_line_mix(tdoa_ctx *ctx, const int32_t *clock16, const int32_t *fine_rate, int n_lines, int n_stations, int U, int drift_den,
                        const tdoa_line_mix *mix, int n_rows, int U_loc, int32_t *rows, int64_t *cdiff, int64_t *cdiff_up)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (!clock16 || !fine_rate || !mix || !rows || !cdiff || !cdiff_up || n_lines < 1 || n_lines > kLocateMaxSets || n_rows < 1 ||
        n_rows > kLocateMaxSets || n_stations < 2 || n_stations > kLocateMaxStations || !sync_fine_factor_ok(U) || drift_den < 1 ||
        !upsample_factor_ok(U_loc))
        return fail(ctx, TDOA_ERR_INVALID, "a pointer is NULL, n_lines or n_rows outside 1 .. 65535, n_stations outside 2 .. 64, U not one of 2, 4, 8, 16, "
                                           "drift_den < 1 or U_loc is not one of 1, 2, 4, 8, 16");
    if (const char *bad = check_mix(mix, n_rows, n_lines)) return fail(ctx, TDOA_ERR_INVALID, bad);
    const long long den = (long long)U * drift_den;
    if (line_mix_overflows(clock16, fine_rate, n_stations, den, mix, n_rows)) return fail(ctx, TDOA_ERR_INVALID, "a continued clock does not fit int32");
    return debug_mix(ctx, clock16, fine_rate, n_lines, n_stations, den, mix, n_rows, U_loc, rows, cdiff, cdiff_up);
}

}  // extern "C"
