// sync_api.inc -- the clock search (stack_sync.hpp), host side: the search as a StackSearch (stack_search.inc) -- its checks,
// geometry, buffers, the one place its kernels are launched, its download -- and the search's three entries.
// Included by tdoa_mi355x.hip after stack_search.inc and locate_api.inc (locate_overflows) and before sync_drift_api.inc,
// which takes sync_inputs from here (declared in stack_search.inc).

namespace {

SyncGeom sync_geom(int S, int max_lag, int gate, int rounds)
{
    SyncGeom g;
    g.S = S;
    g.P = S * (S - 1) / 2;
    g.n = 2 * max_lag - 1;
    g.lag_lo = -(max_lag - 1);
    g.G = gate;
    g.R = rounds;
    g.W = 2 * gate + 1;
    g.tiles = S >= 3 ? (g.W * g.W + kSyncThreads - 1) / kSyncThreads : 0;
    return g;
}

// ref_delay, then centre (NULL: all 0), kSyncMaxStations words each: what the clock and the clock-line search upload
std::vector<int32_t> sync_inputs(const int32_t *ref_delay, const int32_t *centre, int S)
{
    std::vector<int32_t> in(2 * (size_t)kSyncMaxStations, 0);
    std::copy(ref_delay, ref_delay + S, in.begin());
    if (centre) std::copy(centre, centre + S, in.begin() + kSyncMaxStations);
    return in;
}

// the outputs of the three entries (all but sync may be NULL)
struct SyncHost {
    tdoa_sync *sync = nullptr;               // [set]
    int32_t *clock = nullptr;                // [set][station]
    int32_t *lags = nullptr;                 // [set][pair]
    double *corr = nullptr;                  // [set][pair]
};

struct SyncSearch : StackSearch {
    int G, R;                                // gate, rounds
    const int32_t *ref_delay, *centre;       // [stations]; centre NULL: all 0
    SyncHost o;
    SyncGeom g;                              // bind: the geometry, the sets and the inputs as they are uploaded
    size_t n_sets = 0;
    std::vector<int32_t> in;

    SyncSearch(int gate, int rounds, const int32_t *ref_delay, const int32_t *centre, const SyncHost &host)
        : StackSearch("the clock search with TDOA_LAGS_GO", "the clock search's candidates and records"), G(gate), R(rounds),
          ref_delay(ref_delay), centre(centre), o(host)
    {
    }
    const char *check_args() const override
    {
        if (G < 0 || G > kSyncMaxGate) return "gate outside 0 .. 1023";
        if (R < 0 || R > kSyncMaxRounds) return "rounds outside 0 .. 16";
        if (!ref_delay) return "ref_delay is NULL";
        if (!o.sync) return "sync_host is NULL";
        return nullptr;
    }
    // the lag mode, the captures, the station count, the overflow bound
    int check_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what) const override
    {
        if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse_with(what, TDOA_ERR_UNSUPPORTED, go_what);
        if (ctx->caps.empty()) return refuse_with(what, TDOA_ERR_STATE, "captures missing");
        const int S = (int)ctx->caps.size();
        if (S < 2 || S > kSyncMaxStations) return refuse_with(what, TDOA_ERR_UNSUPPORTED, "the clock search needs 2 .. 64 stations");
        int wpb = 0;
        if (tdoa_num_windows(ctx, &wpb, nullptr)) return refuse_with(what, TDOA_ERR_STATE, "captures missing or too small");
        if (locate_overflows(S * (S - 1) / 2, stack_geom(wpb, windows_per_stack).mm))
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "pairs x stack length > 2^17: the objective could overflow");
        if (3ll * wpb > kLocateMaxSets) return refuse_with(what, TDOA_ERR_UNSUPPORTED, "more than 65535 stacks");
        return TDOA_OK;
    }
    int check_sets(const tdoa_ctx *, const int64_t *q, int n_sets, int, int n_stations, int n_w, const char **what) const override
    {
        if (!q || n_sets < 1 || n_sets > kLocateMaxSets || n_w < 1 || n_stations < 2 || n_stations > kSyncMaxStations)
            return refuse_with(what, TDOA_ERR_INVALID, "q is NULL, n_sets outside 1 .. 65535, n_w < 1 or n_stations outside 2 .. 64");
        if (locate_overflows(n_stations * (n_stations - 1) / 2, n_w))
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "pairs x n_w > 2^17: the objective could overflow");
        return TDOA_OK;
    }
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override
    {
        g = sync_geom(sh.S, ctx->prm.max_lag, G, R);
        n_sets = (size_t)sh.n_sets;
        in = sync_inputs(ref_delay, centre, sh.S);
    }
    void key(std::vector<uint64_t> *key, int m) const override
    {
        key->insert(key->end(), {StepProduct::Sync, (uint64_t)m, (uint64_t)G, (uint64_t)R});
    }
    // the inputs, the start's tiles' candidates, the records, clocks, lags and correlations
    int reserve(tdoa_ctx *ctx) const override
    {
        int rc;
        if ((rc = ensure(ctx, ctx->sync_in, sizeof(int32_t) * 2 * kSyncMaxStations))) return rc;
        if ((rc = ensure(ctx, ctx->sync_part, sizeof(ClosureCand) * std::max<size_t>(n_sets * g.tiles, 1)))) return rc;
        if ((rc = ensure(ctx, ctx->sync_out, sizeof(SyncOut) * n_sets))) return rc;
        if ((rc = ensure(ctx, ctx->sync_clock, sizeof(int32_t) * n_sets * g.S))) return rc;
        if ((rc = ensure(ctx, ctx->sync_lags, sizeof(int32_t) * n_sets * g.P))) return rc;
        return ensure(ctx, ctx->sync_corr, sizeof(double) * n_sets * g.P);
    }
    // the delays and the centres: a call that changes only them replays the same graph
    int refresh(tdoa_ctx *ctx) const override
    {
        HIPCHK(ctx, hipMemcpyAsync(ctx->sync_in.p, in.data(), sizeof(int32_t) * in.size(), hipMemcpyHostToDevice, ctx->stream));
        return TDOA_OK;
    }
    // Q [n_sets][P][n] -> the records in ctx->sync_out, the clocks, lags and correlations: the one place the search is launched
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
    {
        hipStream_t st = ctx->stream;
        auto *d_in = ctx->sync_in.as<const int32_t>();
        auto *part = ctx->sync_part.as<ClosureCand>();
        if (g.tiles > 0)
            hipLaunchKernelGGL(k_sync_start, dim3((unsigned)g.tiles, (unsigned)n_sets), dim3(kSyncThreads), 0, st, Q, g, d_in, part);
        hipLaunchKernelGGL(k_sync_steps, dim3((unsigned)n_sets), dim3(kSyncThreads), 0, st, Q, g, d_in, roots,
                           static_cast<const ClosureCand *>(part), ctx->sync_out.as<SyncOut>(), ctx->sync_clock.as<int32_t>(),
                           ctx->sync_lags.as<int32_t>(), ctx->sync_corr.as<double>());
    }
    int download(tdoa_ctx *ctx) const override
    {
        hipStream_t st = ctx->stream;
        HIPCHK(ctx, hipMemcpyAsync(o.sync, ctx->sync_out.p, sizeof(SyncOut) * n_sets, hipMemcpyDeviceToHost, st));
        if (o.clock) HIPCHK(ctx, hipMemcpyAsync(o.clock, ctx->sync_clock.p, sizeof(int32_t) * n_sets * g.S, hipMemcpyDeviceToHost, st));
        if (o.lags) HIPCHK(ctx, hipMemcpyAsync(o.lags, ctx->sync_lags.p, sizeof(int32_t) * n_sets * g.P, hipMemcpyDeviceToHost, st));
        if (o.corr) HIPCHK(ctx, hipMemcpyAsync(o.corr, ctx->sync_corr.p, sizeof(double) * n_sets * g.P, hipMemcpyDeviceToHost, st));
        return TDOA_OK;
    }
};

}  // namespace

extern "C" {

int tdoa_process_sync(tdoa_ctx *ctx, int windows_per_stack, int gate, int rounds, const int32_t *ref_delay, const int32_t *centre,
                      tdoa_sync *sync_host, int32_t *clock_host, int32_t *lags_host, double *corr_host)
{
    SyncSearch s(gate, rounds, ref_delay, centre, SyncHost{sync_host, clock_host, lags_host, corr_host});
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_sync(tdoa_group *g, int windows_per_stack, int gate, int rounds, const int32_t *ref_delay, const int32_t *centre,
                            tdoa_sync *sync_host, int32_t *clock_host, int32_t *lags_host, double *corr_host)
{
    SyncSearch s(gate, rounds, ref_delay, centre, SyncHost{sync_host, clock_host, lags_host, corr_host});
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_debug_sync_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int gate, int rounds,
                           const int32_t *ref_delay, const int32_t *centre, tdoa_sync *sync, int32_t *clock, int32_t *lags,
                           double *corr)
{
    SyncSearch s(gate, rounds, ref_delay, centre, SyncHost{sync, clock, lags, corr});
    return debug_search_from_q(ctx, q, n_sets, 0, n_stations, n_w, s);
}

}  // extern "C"
