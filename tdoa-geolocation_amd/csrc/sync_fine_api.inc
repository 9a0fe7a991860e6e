// sync_fine_api.inc -- the fine clock search (stack_sync_fine.hpp), host side: the search as a StackSearch (stack_search.inc)
// that holds the clock search (SyncSearch, sync_api.inc) for its coarse stage and adds the one refinement kernel behind that
// search's launches, and the search's three entries.  Included by tdoa_mi355x.hip after sync_api.inc.

namespace {

// the outputs the refinement adds to SyncHost's (all but fine may be NULL)
struct SyncFineHost {
    tdoa_sync *fine = nullptr;               // [set]
    int32_t *clock16 = nullptr;              // [set][station], 1/16 sample
    int32_t *lags = nullptr;                 // [set][pair], 1/U sample
    double *corr = nullptr;                  // [set][pair]
};

struct SyncFineSearch : StackSearch {
    SyncSearch coarse;
    int U, Rf;                               // the factor, the fine sweeps
    SyncFineHost o;

    SyncFineSearch(int gate, int rounds, int factor, int fine_rounds, const int32_t *ref_delay, const int32_t *centre, const SyncHost &host,
                   const SyncFineHost &fine)
        : StackSearch("the fine clock search with TDOA_LAGS_GO", "the fine clock search's candidates and records"),
          coarse(gate, rounds, ref_delay, centre, host), U(factor), Rf(fine_rounds), o(fine)
    {
    }
    // what a refinement refuses of its own arguments; the fine clock lines' too (sync_drift_fine_api.inc)
    static const char *check_fine_args(int U, int Rf, const void *fine_host)
    {
        if (!sync_fine_factor_ok(U)) return "U is not 2, 4, 8 or 16";
        if (Rf < 0 || Rf > kSyncFineMaxRounds) return "fine_rounds outside 0 .. 16";
        return fine_host ? nullptr : "fine_host is NULL";
    }
    const char *check_args() const override { const char *bad = coarse.check_args(); return bad ? bad : check_fine_args(U, Rf, o.fine); }
    // the clock in 1/16 sample must fit int32
    bool centre_too_large(int S) const
    {
        for (int s = 0; coarse.centre && s < S; s++)
            if (std::llabs((long long)coarse.centre[s]) + coarse.G + 1 >= kSyncFineMaxCentre) return true;
        return false;
    }
    // the clock search's checks, the upsampled locate's tightened overflow bound, the centres
    int check_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what) const override
    {
        if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse_with(what, TDOA_ERR_UNSUPPORTED, go_what);
        if (const int rc = coarse.check_state(ctx, windows_per_stack, what)) return rc;
        const int S = (int)ctx->caps.size();
        int wpb = 0;
        (void)tdoa_num_windows(ctx, &wpb, nullptr);
        if (locate_overflows(S * (S - 1) / 2, stack_geom(wpb, windows_per_stack).mm, U))
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "4 x pairs x stack length > 2^17: the upsampled objective could overflow");
        if (centre_too_large(S)) return refuse_with(what, TDOA_ERR_INVALID, "|centre| + gate + 1 >= 2^27: the clock in 1/16 sample would not fit int32");
        return TDOA_OK;
    }
    int check_sets(const tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what) const override
    {
        if (const int rc = coarse.check_sets(ctx, q, n_sets, track_len, n_stations, n_w, what)) return rc;
        if (locate_overflows(n_stations * (n_stations - 1) / 2, n_w, U))
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "4 x pairs x n_w > 2^17: the upsampled objective could overflow");
        if (centre_too_large(n_stations)) return refuse_with(what, TDOA_ERR_INVALID, "|centre| + gate + 1 >= 2^27: the clock in 1/16 sample would not fit int32");
        return TDOA_OK;
    }
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override { coarse.bind(ctx, sh); }
    void key(std::vector<uint64_t> *key, int m) const override
    {
        key->insert(key->end(), {StepProduct::SyncFine, (uint64_t)m, (uint64_t)coarse.G, (uint64_t)coarse.R, (uint64_t)U, (uint64_t)Rf});
    }
    // the clock search's buffers, then the fine records, clocks, lags and correlations
    int reserve(tdoa_ctx *ctx) const override
    {
        int rc;
        const SyncGeom &g = coarse.g;
        if ((rc = coarse.reserve(ctx))) return rc;
        if ((rc = ensure(ctx, ctx->sfine_out, sizeof(SyncOut) * coarse.n_sets))) return rc;
        if ((rc = ensure(ctx, ctx->sfine_clock, sizeof(int32_t) * coarse.n_sets * g.S))) return rc;
        if ((rc = ensure(ctx, ctx->sfine_lags, sizeof(int32_t) * coarse.n_sets * g.P))) return rc;
        return ensure(ctx, ctx->sfine_corr, sizeof(double) * coarse.n_sets * g.P);
    }
    int refresh(tdoa_ctx *ctx) const override { return coarse.refresh(ctx); }
    // the clock search's launches, then the refinement on its records and clocks
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
    {
        coarse.launch(ctx, Q, roots);
        hipLaunchKernelGGL(k_sync_refine, dim3((unsigned)coarse.n_sets), dim3(kSyncThreads), 0, ctx->stream, Q, coarse.g, U, Rf,
                           ctx->sync_in.as<const int32_t>(), roots, ctx->sync_out.as<const SyncOut>(), ctx->sync_clock.as<const int32_t>(),
                           ctx->sfine_out.as<SyncOut>(), ctx->sfine_clock.as<int32_t>(), ctx->sfine_lags.as<int32_t>(),
                           ctx->sfine_corr.as<double>());
    }
    int download(tdoa_ctx *ctx) const override
    {
        hipStream_t st = ctx->stream;
        const SyncGeom &g = coarse.g;
        const size_t n_sets = coarse.n_sets;
        if (int rc = coarse.download(ctx)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(o.fine, ctx->sfine_out.p, sizeof(SyncOut) * n_sets, hipMemcpyDeviceToHost, st));
        if (o.clock16) HIPCHK(ctx, hipMemcpyAsync(o.clock16, ctx->sfine_clock.p, sizeof(int32_t) * n_sets * g.S, hipMemcpyDeviceToHost, st));
        if (o.lags) HIPCHK(ctx, hipMemcpyAsync(o.lags, ctx->sfine_lags.p, sizeof(int32_t) * n_sets * g.P, hipMemcpyDeviceToHost, st));
        if (o.corr) HIPCHK(ctx, hipMemcpyAsync(o.corr, ctx->sfine_corr.p, sizeof(double) * n_sets * g.P, hipMemcpyDeviceToHost, st));
        return TDOA_OK;
    }
};

}  // namespace

extern "C" {

int tdoa_process_sync_fine(tdoa_ctx *ctx, int windows_per_stack, int gate, int rounds, int U, int fine_rounds, const int32_t *ref_delay,
                           const int32_t *centre, tdoa_sync *sync_host, int32_t *clock_host, int32_t *lags_host, double *corr_host,
                           tdoa_sync *fine_host, int32_t *clock16_host, int32_t *fine_lags_host, double *fine_corr_host)
{
    SyncFineSearch s(gate, rounds, U, fine_rounds, ref_delay, centre, SyncHost{sync_host, clock_host, lags_host, corr_host},
                     SyncFineHost{fine_host, clock16_host, fine_lags_host, fine_corr_host});
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_sync_fine(tdoa_group *g, int windows_per_stack, int gate, int rounds, int U, int fine_rounds,
                                 const int32_t *ref_delay, const int32_t *centre, tdoa_sync *sync_host, int32_t *clock_host,
                                 int32_t *lags_host, double *corr_host, tdoa_sync *fine_host, int32_t *clock16_host,
                                 int32_t *fine_lags_host, double *fine_corr_host)
{
    SyncFineSearch s(gate, rounds, U, fine_rounds, ref_delay, centre, SyncHost{sync_host, clock_host, lags_host, corr_host},
                     SyncFineHost{fine_host, clock16_host, fine_lags_host, fine_corr_host});
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_debug_sync_fine_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int gate, int rounds, int U,
                                int fine_rounds, const int32_t *ref_delay, const int32_t *centre, tdoa_sync *sync, int32_t *clock,
                                int32_t *lags, double *corr, tdoa_sync *fine, int32_t *clock16, int32_t *fine_lags, double *fine_corr)
{
    SyncFineSearch s(gate, rounds, U, fine_rounds, ref_delay, centre, SyncHost{sync, clock, lags, corr},
                     SyncFineHost{fine, clock16, fine_lags, fine_corr});
    return debug_search_from_q(ctx, q, n_sets, 0, n_stations, n_w, s);
}

}  // extern "C"
