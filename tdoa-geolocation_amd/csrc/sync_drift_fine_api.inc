// sync_drift_fine_api.inc -- the fine clock lines (stack_sync_drift_fine.hpp), host side: the search as a StackSearch
// (stack_search.inc) that holds the clock-line search (SyncLineSearch, sync_drift_api.inc) for its coarse stage and adds the
// checks, the buffers, the one place the refinement's kernels are launched and the download; the search's three entries and
// tdoa_sync_line_clock16.  Included by tdoa_mi355x.hip after sync_drift_api.inc.

namespace {

// the outputs the refinement adds to SyncLineHost's (all but fine may be NULL)
struct SyncLineFineHost {
    tdoa_sync_line *fine = nullptr;          // [line]
    int32_t *clock16 = nullptr, *rate = nullptr;                 // [line][station]: 1/16 sample; 1/(U D) lag per position
    int32_t *rows = nullptr;                 // [stack][station], 1/16 sample
    int32_t *lags = nullptr;                 // [stack][pair], 1/U sample
    double *corr = nullptr;                  // [stack][pair]
};

struct SyncLineFineSearch : StackSearch {
    SyncLineSearch coarse;
    int U, Rf;                               // the factor, the fine sweeps
    SyncLineFineHost o;
    SyncLineFineGeom fg;                     // bind

    SyncLineFineSearch(int gate, int max_drift, int drift_den, int rounds, int factor, int fine_rounds, const int32_t *ref_delay,
                       const int32_t *centre, const SyncLineHost &host, const SyncLineFineHost &fine)
        : StackSearch("the fine clock lines with TDOA_LAGS_GO", "the fine clock lines' candidates and records"),
          coarse(gate, max_drift, drift_den, rounds, ref_delay, centre, host), U(factor), Rf(fine_rounds), o(fine)
    {
    }
    const char *check_args() const override { const char *bad = coarse.check_args(); return bad ? bad : SyncFineSearch::check_fine_args(U, Rf, o.fine); }
    // a fine row in 1/16 sample must fit int32: the offset's window, the slope's window over the line, the roundings
    bool row_too_large(int S, int L) const
    {
        const long long reach = coarse.G + 2 + ((long long)coarse.H + 1) * (L - 1) / coarse.D;
        for (int s = 0; s < S; s++)
            if (std::llabs(coarse.centre ? (long long)coarse.centre[s] : 0ll) + reach >= kSyncFineMaxCentre) return true;
        return false;
    }
    static constexpr const char *row_what = "|centre| + gate + 2 + ((max_drift + 1)(L - 1)) div drift_den >= 2^27: a fine row in 1/16 sample would not fit int32";
    // the clock-line search's checks, the tightened overflow bound on the line's windows, the rows
    int check_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what) const override
    {
        if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse_with(what, TDOA_ERR_UNSUPPORTED, go_what);
        if (const int rc = coarse.check_state(ctx, windows_per_stack, what)) return rc;
        const int S = (int)ctx->caps.size();
        int wpb = 0;
        (void)tdoa_num_windows(ctx, &wpb, nullptr);
        if (locate_overflows(S * (S - 1) / 2, wpb, U))
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "4 x pairs x windows per block > 2^17: the upsampled line's sum could overflow");
        if (row_too_large(S, stack_geom(wpb, windows_per_stack).spb)) return refuse_with(what, TDOA_ERR_INVALID, row_what);
        return TDOA_OK;
    }
    int check_sets(const tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what) const override
    {
        if (const int rc = coarse.check_sets(ctx, q, n_sets, track_len, n_stations, n_w, what)) return rc;
        if (locate_overflows(n_stations * (n_stations - 1) / 2, (long long)track_len * n_w, U))
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "4 x pairs x track_len x n_w > 2^17: the upsampled line's sum could overflow");
        if (row_too_large(n_stations, track_len)) return refuse_with(what, TDOA_ERR_INVALID, row_what);
        return TDOA_OK;
    }
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override
    {
        coarse.bind(ctx, sh);
        fg.S = coarse.g.S;
        fg.P = coarse.g.P;
        fg.n = coarse.g.n;
        fg.L = coarse.g.L;
        fg.U = U;
        fg.log_u = U == 2 ? 1 : U == 4 ? 2 : U == 8 ? 3 : 4;
        fg.W = 2 * U + 1;
        fg.D = coarse.D;
        fg.cands = fg.W * fg.W;
        fg.tiles = (fg.cands + kSyncLineFineThreads - 1) / kSyncLineFineThreads;
    }
    void key(std::vector<uint64_t> *key, int m) const override
    {
        key->insert(key->end(), {StepProduct::SyncDriftFine, (uint64_t)m, (uint64_t)coarse.G | ((uint64_t)coarse.H << 32),
                                 (uint64_t)coarse.D | ((uint64_t)coarse.R << 32), (uint64_t)U | ((uint64_t)Rf << 32)});
    }
    // the clock-line search's buffers, then the fine table, state, candidates and outputs
    int reserve(tdoa_ctx *ctx) const override
    {
        int rc;
        const size_t n_lines = coarse.n_lines, n_sets = n_lines * fg.L;
        if ((rc = coarse.reserve(ctx))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_cur, sizeof(long long) * n_lines * fg.S * fg.L))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_kappa, sizeof(long long) * n_lines * fg.S))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_eta, sizeof(long long) * n_lines * fg.S))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_part, sizeof(ClosureCand) * n_lines * fg.tiles))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_moved, sizeof(int32_t) * n_lines))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_start, sizeof(long long) * n_lines))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_out, sizeof(SyncLineOut) * n_lines))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_clock, sizeof(int32_t) * n_lines * fg.S))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_rate, sizeof(int32_t) * n_lines * fg.S))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_rows, sizeof(int32_t) * n_sets * fg.S))) return rc;
        if ((rc = ensure(ctx, ctx->slfine_lags, sizeof(int32_t) * n_sets * fg.P))) return rc;
        return ensure(ctx, ctx->slfine_corr, sizeof(double) * n_sets * fg.P);
    }
    int refresh(tdoa_ctx *ctx) const override { return coarse.refresh(ctx); }
    // the clock-line search's launches, then the refinement on its records, clocks and rates: the one place its kernels are
    // launched.  Two launches per step, Rf (S - 1) steps, the table's and the two finishes'.
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
    {
        coarse.launch(ctx, Q, roots);
        hipStream_t st = ctx->stream;
        const SyncLineFineDev d{ctx->sline_in.as<const int32_t>(), ctx->sline_k.as<const long long>(), ctx->sline_h.as<const int32_t>(),
                                ctx->sline_out.as<const SyncLineOut>(), ctx->slfine_cur.as<long long>(), ctx->slfine_kappa.as<long long>(),
                                ctx->slfine_eta.as<long long>(), ctx->slfine_part.as<ClosureCand>(), ctx->slfine_moved.as<int32_t>(),
                                ctx->slfine_start.as<long long>()};
        const dim3 lines((unsigned)coarse.n_lines), threads(kSyncLineFineThreads);
        const auto finish = [&](int pass) {
            hipLaunchKernelGGL(k_syncline_finish, lines, threads, 0, st, Q, SyncFineGrid{fg.n, fg.U, fg.log_u, nullptr}, fg, d,
                               d.kappa, d.eta, d.coarse, pass, roots, ctx->sline_roots.as<const double>(),
                               ctx->slfine_out.as<SyncLineOut>(), ctx->slfine_clock.as<int32_t>(), ctx->slfine_rate.as<int32_t>(),
                               ctx->slfine_rows.as<int32_t>(), ctx->slfine_lags.as<int32_t>(), ctx->slfine_corr.as<double>());
        };
        hipLaunchKernelGGL(k_synclinefine_init, lines, threads, 0, st, fg, d);
        finish(0);
        for (int r = 0; r < Rf; r++)
            for (int s = 1; s < fg.S; s++) {
                hipLaunchKernelGGL(k_synclinefine_step, dim3((unsigned)fg.tiles, (unsigned)coarse.n_lines), threads, 0, st, Q, fg, d, s);
                hipLaunchKernelGGL(k_synclinefine_commit, lines, threads, 0, st, fg, d, s, s == 1);
            }
        finish(1);
    }
    int download(tdoa_ctx *ctx) const override
    {
        hipStream_t st = ctx->stream;
        const size_t n_lines = coarse.n_lines, n_sets = n_lines * fg.L;
        if (int rc = coarse.download(ctx)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(o.fine, ctx->slfine_out.p, sizeof(SyncLineOut) * n_lines, hipMemcpyDeviceToHost, st));
        if (o.clock16) HIPCHK(ctx, hipMemcpyAsync(o.clock16, ctx->slfine_clock.p, sizeof(int32_t) * n_lines * fg.S, hipMemcpyDeviceToHost, st));
        if (o.rate) HIPCHK(ctx, hipMemcpyAsync(o.rate, ctx->slfine_rate.p, sizeof(int32_t) * n_lines * fg.S, hipMemcpyDeviceToHost, st));
        if (o.rows) HIPCHK(ctx, hipMemcpyAsync(o.rows, ctx->slfine_rows.p, sizeof(int32_t) * n_sets * fg.S, hipMemcpyDeviceToHost, st));
        if (o.lags) HIPCHK(ctx, hipMemcpyAsync(o.lags, ctx->slfine_lags.p, sizeof(int32_t) * n_sets * fg.P, hipMemcpyDeviceToHost, st));
        if (o.corr) HIPCHK(ctx, hipMemcpyAsync(o.corr, ctx->slfine_corr.p, sizeof(double) * n_sets * fg.P, hipMemcpyDeviceToHost, st));
        return TDOA_OK;
    }
};

}  // namespace

extern "C" {

int tdoa_process_sync_drift_fine(tdoa_ctx *ctx, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds, int U,
                                 int fine_rounds, const int32_t *ref_delay, const int32_t *centre, tdoa_sync_line *line_host,
                                 int32_t *clock_host, int32_t *rate_host, int32_t *rows_host, int32_t *lags_host, double *corr_host,
                                 tdoa_sync_line *fine_host, int32_t *clock16_host, int32_t *fine_rate_host, int32_t *fine_rows_host,
                                 int32_t *fine_lags_host, double *fine_corr_host)
{
    SyncLineFineSearch s(gate, max_drift, drift_den, rounds, U, fine_rounds, ref_delay, centre,
                         SyncLineHost{line_host, clock_host, rate_host, rows_host, lags_host, corr_host},
                         SyncLineFineHost{fine_host, clock16_host, fine_rate_host, fine_rows_host, fine_lags_host, fine_corr_host});
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_sync_drift_fine(tdoa_group *g, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds, int U,
                                       int fine_rounds, const int32_t *ref_delay, const int32_t *centre, tdoa_sync_line *line_host,
                                       int32_t *clock_host, int32_t *rate_host, int32_t *rows_host, int32_t *lags_host,
                                       double *corr_host, tdoa_sync_line *fine_host, int32_t *clock16_host, int32_t *fine_rate_host,
                                       int32_t *fine_rows_host, int32_t *fine_lags_host, double *fine_corr_host)
{
    SyncLineFineSearch s(gate, max_drift, drift_den, rounds, U, fine_rounds, ref_delay, centre,
                         SyncLineHost{line_host, clock_host, rate_host, rows_host, lags_host, corr_host},
                         SyncLineFineHost{fine_host, clock16_host, fine_rate_host, fine_rows_host, fine_lags_host, fine_corr_host});
    return group_process_search(g, windows_per_stack, s);
}

// set t * track_len + x is position x of line t
int tdoa_debug_sync_drift_fine_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int gate,
                                      int max_drift, int drift_den, int rounds, int U, int fine_rounds, const int32_t *ref_delay,
                                      const int32_t *centre, tdoa_sync_line *line, int32_t *clock, int32_t *rate, int32_t *rows,
                                      int32_t *lags, double *corr, tdoa_sync_line *fine, int32_t *clock16, int32_t *fine_rate,
                                      int32_t *fine_rows, int32_t *fine_lags, double *fine_corr)
{
    SyncLineFineSearch s(gate, max_drift, drift_den, rounds, U, fine_rounds, ref_delay, centre,
                         SyncLineHost{line, clock, rate, rows, lags, corr},
                         SyncLineFineHost{fine, clock16, fine_rate, fine_rows, fine_lags, fine_corr});
    return debug_search_from_q(ctx, q, n_sets, track_len, n_stations, n_w, s);
}

// The fine line continued past its block in 1/16 sample (host only): out[x - first][s] = clock16[s] + r(16 eta_s x, U D).
int tdoa_sync_line_clock16(const int32_t *clock16, const int32_t *fine_rate, int n_stations, int U, int drift_den, int first_position,
                           int n_positions, int32_t *out)
{
    if (!clock16 || !fine_rate || !out || n_stations < 1 || !sync_fine_factor_ok(U) || drift_den < 1 || first_position < 0 || n_positions < 1)
        return TDOA_ERR_INVALID;
    const long long den = (long long)U * drift_den;
    for (int x = 0; x < n_positions; x++)
        for (int s = 0; s < n_stations; s++)
            out[(size_t)x * n_stations + s] = (int32_t)line_cont(clock16[s], fine_rate[s], (long long)first_position + x, den);
    return TDOA_OK;
}

}  // extern "C"
