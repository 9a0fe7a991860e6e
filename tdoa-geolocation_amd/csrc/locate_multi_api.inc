// locate_multi_api.inc -- several emitters per stack, host side: the rounds' buffers, the kernels' launches (shared by a
// context's own step, step_products.inc, the group's merged sum and tdoa_debug_locate_multi_from_q) and the checks the entries
// share.  The rounds' outputs are [round][set] planes of the delay-table search's own buffers, so round 0 is launch_locate
// (locate_api.inc) as it stands, on plane 0.
// Included by tdoa_mi355x.hip after locate_api.inc and before step_products.inc.

extern "C" {

// the arguments the three entries share; they need no device
static const char *check_locate_multi_args(int n_emitters, int guard, int min_separation, const void *loc)
{
    if (n_emitters < 1 || n_emitters > kLocateMaxEmitters) return "n_emitters outside 1 .. 8";
    if (guard < 0) return "guard < 0";
    return check_locate_args(min_separation, loc);
}

// the rounds' mask as the kernels take it: a guard of the range's length already excludes every lag of the range
static LocateMask locate_mask(int round, int guard, const LocateGeom &g) { return LocateMask{round, std::min(guard, g.n)}; }

// the buffers of K rounds for n_sets stacks: K planes of the search's buffers (the tiles' candidates and the cells serve one
// round at a time) and the centres [set][pair], kLocateMaxEmitters words each
static int ensure_locate_multi(tdoa_ctx *ctx, size_t n_sets, int K, const LocateGeom &g)
{
    int rc;
    if ((rc = ensure(ctx, ctx->locate_map, sizeof(long long) * K * n_sets * g.n_cells))) {
        char buf[256];
        snprintf(buf, sizeof(buf), "the delay-table search's map [%d rounds][%zu stacks][%d cells] (%.1f MB) does not fit in device memory: %s",
                 K, n_sets, (int)g.n_cells, 8.0 * (double)K * (double)n_sets * g.n_cells / 1e6, ctx->last_error.c_str());
        return fail(ctx, TDOA_ERR_NOMEM, buf);
    }
    if ((rc = ensure(ctx, ctx->locate_part, sizeof(ClosureCand) * n_sets * g.tiles))) return rc;
    if ((rc = ensure(ctx, ctx->locate_best, sizeof(int32_t) * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->locate_out, sizeof(LocateOut) * K * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->locate_lags, sizeof(int32_t) * K * n_sets * g.P))) return rc;
    if ((rc = ensure(ctx, ctx->locate_corr, sizeof(double) * K * n_sets * g.P))) return rc;
    if ((rc = ensure(ctx, ctx->locate_centres, sizeof(LocateCentres) * n_sets * g.P))) return rc;
    return ensure_map_stats(ctx, K * n_sets);
}

// Q [n_sets][P][n] -> K planes of records, maps, lags and correlations: the one place the rounds are launched.  Round 0 is
// launch_locate; every later round is the masked scores, the masked finish, and the runner-up's pass as the search runs it,
// on the round's planes.  The statistics of all K planes of maps follow the last round.  Kernel launches only (the step graph
// captures them).
static void launch_locate_multi(tdoa_ctx *ctx, const long long *Q, const double *roots, int n_sets, int K, int guard, const LocateGeom &g)
{
    launch_locate(ctx, Q, roots, n_sets, g, K == 1);
    if (K == 1) return;
    hipStream_t st = ctx->stream;
    const dim3 grid((unsigned)g.tiles, (unsigned)n_sets), one((unsigned)n_sets);
    auto *table = ctx->locate_table.as<const int32_t>();
    const long long *cdiff = ctx->clock_stacks ? ctx->locate_clock.as<const long long>() : nullptr;
    auto *part = ctx->locate_part.as<ClosureCand>();
    auto *best = ctx->locate_best.as<int32_t>();
    auto *centres = ctx->locate_centres.as<LocateCentres>();
    hipLaunchKernelGGL(k_locate_centres, one, dim3(kLocateThreads), 0, st, g, table, cdiff, static_cast<const int32_t *>(best), centres);
    for (int r = 1; r < K; r++) {
        const LocateMask mk = locate_mask(r, guard, g);
        auto *map = ctx->locate_map.as<long long>() + (size_t)r * n_sets * g.n_cells;
        auto *out = ctx->locate_out.as<LocateOut>() + (size_t)r * n_sets;
        auto *lags = ctx->locate_lags.as<int32_t>() + (size_t)r * n_sets * g.P;
        auto *corr = ctx->locate_corr.as<double>() + (size_t)r * n_sets * g.P;
        switch (g.S <= kLocateMaskedRegStations ? g.S : 0) {
#define TDOA_LOCATE_CASE(s)                                                                                                      \
    case s:                                                                                                                      \
        if (cdiff)                                                                                                               \
            hipLaunchKernelGGL((k_locate_scores_masked<s, true>), grid, dim3(kLocateThreads), 0, st, Q, g, table, cdiff,         \
                               static_cast<const LocateCentres *>(centres), mk, map, part);                                            \
        else                                                                                                                     \
            hipLaunchKernelGGL((k_locate_scores_masked<s, false>), grid, dim3(kLocateThreads), 0, st, Q, g, table, cdiff,        \
                               static_cast<const LocateCentres *>(centres), mk, map, part);                                            \
        break;
        TDOA_LOCATE_CASE(2) TDOA_LOCATE_CASE(3) TDOA_LOCATE_CASE(4) TDOA_LOCATE_CASE(5) TDOA_LOCATE_CASE(6) TDOA_LOCATE_CASE(7)
        TDOA_LOCATE_CASE(8) TDOA_LOCATE_CASE(9) TDOA_LOCATE_CASE(10) TDOA_LOCATE_CASE(11) TDOA_LOCATE_CASE(12) TDOA_LOCATE_CASE(13)
        TDOA_LOCATE_CASE(14) TDOA_LOCATE_CASE(15)
        default:
            TDOA_LOCATE_CASE(0)
        }
#undef TDOA_LOCATE_CASE
        hipLaunchKernelGGL(k_locate_finish_masked, one, dim3(kLocateThreads), 0, st, Q, g, table, cdiff, roots,
                           static_cast<const ClosureCand *>(part), mk, centres, best, out, lags, corr);
        hipLaunchKernelGGL(k_locate_runner, grid, dim3(kLocateThreads), 0, st, static_cast<const long long *>(map), g,
                           static_cast<const int32_t *>(best), part);
        hipLaunchKernelGGL(k_locate_finish, one, dim3(kLocateThreads), 0, st, Q, g, table, cdiff, roots, static_cast<const ClosureCand *>(part), 1,
                           best, out, lags, corr);
    }
    launch_map_stats(ctx, ctx->locate_map.as<const long long>(), (size_t)g.n_cells, K * n_sets, g, ctx->locate_out.p, roots, n_sets);
}

// the outputs to the host (all but loc may be NULL): the K planes lie one behind the other; asynchronous on ctx->stream
static int download_locate_multi(tdoa_ctx *ctx, size_t n_sets, int K, const LocateGeom &g, tdoa_location *loc, int32_t *lags, double *corr,
                                 int64_t *map)
{
    return download_locate(ctx, K * n_sets, g, loc, lags, corr, map);
}

// the rounds on a group's merged sum (finish_from_host, stacked_api.inc)
static int locate_multi_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack, int K, int guard, int min_separation,
                                  tdoa_location *loc, int32_t *lags, double *corr, int64_t *map)
{
    const LocateGeom g = locate_geom(ctx, min_separation);
    return finish_from_host(
        ctx, q_sum, windows_per_stack,
        [&](int n_stacks, const double *roots) -> int {
            if (int rc = ensure_locate_multi(ctx, n_stacks, K, g)) return rc;
            launch_locate_multi(ctx, ctx->stack_q.as<const long long>(), roots, n_stacks, K, guard, g);
            return TDOA_OK;
        },
        [&](int n_stacks) { return download_locate_multi(ctx, n_stacks, K, g, loc, lags, corr, map); });
}

}  // extern "C"
