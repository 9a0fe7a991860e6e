// sync_api.inc -- the clock search, host side: its buffers, the kernels' launches (shared by a context's own step,
// step_products.inc, the group's merged sum and tdoa_debug_sync_from_q).
// Included by tdoa_mi355x.hip after locate_api.inc and locate_run.inc and before step_products.inc.

extern "C" {

static SyncGeom sync_geom(int S, int max_lag, int gate, int rounds)
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

// the arguments the three sync entries share; they need no device
static const char *check_sync_args(int gate, int rounds, const void *ref_delay, const void *sync)
{
    if (gate < 0 || gate > kSyncMaxGate) return "gate outside 0 .. 1023";
    if (rounds < 0 || rounds > kSyncMaxRounds) return "rounds outside 0 .. 16";
    if (!ref_delay) return "ref_delay is NULL";
    if (!sync) return "sync_host is NULL";
    return nullptr;
}

// ref_delay, then centre (NULL: all 0), kSyncMaxStations words each: what upload_sync_in sends
static std::vector<int32_t> sync_inputs(const int32_t *ref_delay, const int32_t *centre, int S)
{
    std::vector<int32_t> in(2 * (size_t)kSyncMaxStations, 0);
    std::copy(ref_delay, ref_delay + S, in.begin());
    if (centre) std::copy(centre, centre + S, in.begin() + kSyncMaxStations);
    return in;
}

// the buffers of the search for n_sets stacks: the inputs, the start's tiles' candidates, the records, clocks, lags and
// correlations
static int ensure_sync(tdoa_ctx *ctx, size_t n_sets, const SyncGeom &g)
{
    int rc;
    if ((rc = ensure(ctx, ctx->sync_in, sizeof(int32_t) * 2 * kSyncMaxStations))) return rc;
    if ((rc = ensure(ctx, ctx->sync_part, sizeof(ClosureCand) * std::max<size_t>(n_sets * g.tiles, 1)))) return rc;
    if ((rc = ensure(ctx, ctx->sync_out, sizeof(SyncOut) * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->sync_clock, sizeof(int32_t) * n_sets * g.S))) return rc;
    if ((rc = ensure(ctx, ctx->sync_lags, sizeof(int32_t) * n_sets * g.P))) return rc;
    return ensure(ctx, ctx->sync_corr, sizeof(double) * n_sets * g.P);
}

// the delays and the centres to the device, before the launch (asynchronous on ctx->stream; `in` lives until the caller has
// synchronised).  Data, not part of a step graph's key: a call that changes only them replays the same graph.
static int upload_sync_in(tdoa_ctx *ctx, const std::vector<int32_t> &in)
{
    HIPCHK(ctx, hipMemcpyAsync(ctx->sync_in.p, in.data(), sizeof(int32_t) * in.size(), hipMemcpyHostToDevice, ctx->stream));
    return TDOA_OK;
}

// Q [n_sets][P][n] -> the records in ctx->sync_out, the clocks, lags and correlations: the one place the search is launched.
// Kernel launches only (the step graph captures them).
static void launch_sync(tdoa_ctx *ctx, const long long *Q, const double *roots, int n_sets, const SyncGeom &g)
{
    hipStream_t st = ctx->stream;
    auto *in = ctx->sync_in.as<const int32_t>();
    auto *part = ctx->sync_part.as<ClosureCand>();
    if (g.tiles > 0)
        hipLaunchKernelGGL(k_sync_start, dim3((unsigned)g.tiles, (unsigned)n_sets), dim3(kSyncThreads), 0, st, Q, g, in, part);
    hipLaunchKernelGGL(k_sync_steps, dim3((unsigned)n_sets), dim3(kSyncThreads), 0, st, Q, g, in, roots,
                       static_cast<const ClosureCand *>(part), ctx->sync_out.as<SyncOut>(), ctx->sync_clock.as<int32_t>(),
                       ctx->sync_lags.as<int32_t>(), ctx->sync_corr.as<double>());
}

// the outputs to the host (all but sync may be NULL); asynchronous on ctx->stream
static int download_sync(tdoa_ctx *ctx, size_t n_sets, const SyncGeom &g, tdoa_sync *sync, int32_t *clock, int32_t *lags, double *corr)
{
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(sync, ctx->sync_out.p, sizeof(SyncOut) * n_sets, hipMemcpyDeviceToHost, st));
    if (clock) HIPCHK(ctx, hipMemcpyAsync(clock, ctx->sync_clock.p, sizeof(int32_t) * n_sets * g.S, hipMemcpyDeviceToHost, st));
    if (lags) HIPCHK(ctx, hipMemcpyAsync(lags, ctx->sync_lags.p, sizeof(int32_t) * n_sets * g.P, hipMemcpyDeviceToHost, st));
    if (corr) HIPCHK(ctx, hipMemcpyAsync(corr, ctx->sync_corr.p, sizeof(double) * n_sets * g.P, hipMemcpyDeviceToHost, st));
    return TDOA_OK;
}

// the clock search on a group's merged sum (finish_from_host, stacked_api.inc)
static int sync_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack, int gate, int rounds, const int32_t *ref_delay,
                          const int32_t *centre, tdoa_sync *sync, int32_t *clock, int32_t *lags, double *corr)
{
    const int S = (int)ctx->caps.size();
    const SyncGeom g = sync_geom(S, ctx->prm.max_lag, gate, rounds);
    const std::vector<int32_t> in = sync_inputs(ref_delay, centre, S);
    return finish_from_host(
        ctx, q_sum, windows_per_stack,
        [&](int n_stacks, const double *roots) -> int {
            int rc;
            if ((rc = ensure_sync(ctx, n_stacks, g))) return rc;
            if ((rc = upload_sync_in(ctx, in))) return rc;
            launch_sync(ctx, ctx->stack_q.as<const long long>(), roots, n_stacks, g);
            return TDOA_OK;
        },
        [&](int n_stacks) { return download_sync(ctx, n_stacks, g, sync, clock, lags, corr); });
}

// what tdoa_process_sync and the group's call refuse once the arguments are in range: the lag mode, the captures, the
// station count, the overflow bound.  *what receives the message.
static int check_sync_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what)
{
    const auto refuse = [&](int status, const char *why) {
        *what = why;
        return status;
    };
    if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse(TDOA_ERR_UNSUPPORTED, "the clock search with TDOA_LAGS_GO");
    if (ctx->caps.empty()) return refuse(TDOA_ERR_STATE, "captures missing");
    const int S = (int)ctx->caps.size();
    if (S < 2 || S > kSyncMaxStations) return refuse(TDOA_ERR_UNSUPPORTED, "the clock search needs 2 .. 64 stations");
    int wpb = 0;
    if (tdoa_num_windows(ctx, &wpb, nullptr)) return refuse(TDOA_ERR_STATE, "captures missing or too small");
    if (locate_overflows(S * (S - 1) / 2, stack_geom(wpb, windows_per_stack).mm))
        return refuse(TDOA_ERR_UNSUPPORTED, "pairs x stack length > 2^17: the objective could overflow");
    if (3ll * wpb > kLocateMaxSets) return refuse(TDOA_ERR_UNSUPPORTED, "more than 65535 stacks");
    return TDOA_OK;
}

}  // extern "C"
