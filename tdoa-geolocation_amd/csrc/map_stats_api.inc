// map_stats_api.inc -- map statistics, host side: the setting a context keeps (tdoa_locate_set_stats), the statistics' buffers,
// the one place the kernels of stack_map_stats.hpp are launched (called at the end of the delay-table family's launch,
// launch_locate_run, so a context's own step, the group's merged sum and the debug entries all get it), the download into the context
// and tdoa_locate_last_stats.  With the setting off nothing here allocates, launches or copies.
// Included by tdoa_mi355x.hip before locate_api.inc and locate_run.inc.

extern "C" {

static bool map_stats_on(const tdoa_ctx *ctx) { return ctx->mstat_n_ranks > 0; }

// the word the family's product appends to the step graph's key: the ranks' count and foot (the ranks themselves are data)
static uint64_t map_stats_key(const tdoa_ctx *ctx) { return (uint64_t)ctx->mstat_n_ranks | ((uint64_t)ctx->mstat_foot << 8); }

int tdoa_locate_set_stats(tdoa_ctx *ctx, const uint16_t *ranks, int n_ranks, int foot)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (n_ranks < 0 || n_ranks > kMapStatsMaxRanks || foot < 0 || foot > 65535)
        return fail(ctx, TDOA_ERR_INVALID, "n_ranks outside 0 .. 8 or foot outside 0 .. 65535");
    if (!ranks || n_ranks == 0) {            // off (the buffers stay: a cached step graph may still name them)
        ctx->mstat_n_ranks = ctx->mstat_foot = 0;
        return TDOA_OK;
    }
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    int32_t words[kMapStatsMaxRanks] = {0};
    for (int r = 0; r < n_ranks; r++) words[r] = ranks[r];
    if ((rc = ensure(ctx, ctx->mstat_ranks, sizeof(words)))) {       // (allocated once: every later setting fits)
        ctx->mstat_n_ranks = ctx->mstat_foot = 0;
        return rc;
    }
    ctx->mstat_n_ranks = n_ranks;
    ctx->mstat_foot = foot;
    HIPCHK(ctx, hipMemcpyAsync(ctx->mstat_ranks.p, words, sizeof(words), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));                  // words goes out of scope
    return TDOA_OK;
}

// the planes one round of launches takes: the bins are the statistics' only large buffer, 64 KB per plane at eight ranks
constexpr int kMapStatsGroup = 1024;

// the buffers for n_planes judged planes, when the setting is on: the records, and the bins and the state of one group of planes
static int ensure_map_stats(tdoa_ctx *ctx, size_t n_planes)
{
    if (!map_stats_on(ctx)) return TDOA_OK;
    int rc;
    const size_t group = std::min<size_t>(n_planes, kMapStatsGroup);
    if ((rc = ensure(ctx, ctx->mstat_hist, sizeof(uint32_t) * group * ctx->mstat_n_ranks * kMapBins))) return rc;
    if ((rc = ensure(ctx, ctx->mstat_state, sizeof(MapStatsState) * group))) return rc;
    return ensure(ctx, ctx->mstat_out, sizeof(MapStatsOut) * n_planes);
}

// n_planes planes of n_cells words, `stride` words apart, judged by records rec[n_planes] (tdoa_location and tdoa_cell_track
// share what is read: cell and score_q) on the scale of roots[(plane0 + p) mod n_roots] -> the statistics of planes plane0 ..
// plane0 + n_planes - 1 of the call in ctx->mstat_out: the one place the statistics' kernels are launched.  Does nothing with
// the setting off.  Kernel launches only (the step graph captures them).
static void launch_map_stats(tdoa_ctx *ctx, const long long *planes, size_t stride, int n_planes, const LocateGeom &lg, const void *rec,
                             const double *roots, int n_roots, int plane0 = 0)
{
    if (!map_stats_on(ctx)) return;
    hipStream_t st = ctx->stream;
    MapStatsGeom g;
    g.n_cells = lg.n_cells;
    g.n_cols = lg.n_cols;
    g.sep = lg.sep;
    g.n_ranks = ctx->mstat_n_ranks;
    g.foot = ctx->mstat_foot;
    g.n_roots = n_roots;
    g.chunks = (lg.n_cells + kMapChunk - 1) / kMapChunk;
    g.stride = stride;
    auto *hist = ctx->mstat_hist.as<uint32_t>();
    auto *state = ctx->mstat_state.as<MapStatsState>();
    auto *out = ctx->mstat_out.as<MapStatsOut>();
    auto *ranks = ctx->mstat_ranks.as<const int32_t>();
    const size_t lds = sizeof(uint32_t) * g.n_ranks * kMapBins;
    for (int p0 = 0; p0 < n_planes; p0 += kMapStatsGroup) {
        const unsigned n = (unsigned)std::min(kMapStatsGroup, n_planes - p0);
        const long long *pp = planes + (size_t)p0 * stride;
        const LocateOut *rr = static_cast<const LocateOut *>(rec) + p0;
        g.plane0 = plane0 + p0;
        const dim3 grid((unsigned)g.chunks, n), one(n);
        hipLaunchKernelGGL(k_map_begin, one, dim3(kMapThreads), 0, st, g, hist, state, out);
        for (int pass = 0; pass < kMapPasses; pass++) {
            hipLaunchKernelGGL(k_map_hist, grid, dim3(kMapThreads), lds, st, pp, g, rr, pass, static_cast<const MapStatsState *>(state), hist);
            hipLaunchKernelGGL(k_map_pick, one, dim3(kMapThreads), 0, st, g, rr, roots, ranks, pass, state, hist, out);
        }
        if (g.foot > 0) hipLaunchKernelGGL(k_map_foot, grid, dim3(kMapThreads), 0, st, pp, g, rr, out);
    }
}

// the last call's statistics to the context, with the call's other outputs; asynchronous on ctx->stream.  With the setting
// off the context forgets the ones it had.
static int download_map_stats(tdoa_ctx *ctx, size_t n_planes)
{
    if (!map_stats_on(ctx)) {
        ctx->mstat_host.clear();
        return TDOA_OK;
    }
    ctx->mstat_host.resize(n_planes);
    HIPCHK(ctx, hipMemcpyAsync(ctx->mstat_host.data(), ctx->mstat_out.p, sizeof(MapStatsOut) * n_planes, hipMemcpyDeviceToHost, ctx->stream));
    return TDOA_OK;
}

int tdoa_locate_last_stats(tdoa_ctx *ctx, tdoa_map_stats *out, int max_planes, int *n_planes)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (ctx->mstat_host.empty()) return fail(ctx, TDOA_ERR_STATE, "the last call of the delay-table family computed no statistics (tdoa_locate_set_stats)");
    if (n_planes) *n_planes = (int)ctx->mstat_host.size();
    if (!out || max_planes < (int)ctx->mstat_host.size()) return fail(ctx, TDOA_ERR_INVALID, "out is NULL or max_planes is less than the planes of the last call");
    std::memcpy(out, ctx->mstat_host.data(), sizeof(MapStatsOut) * ctx->mstat_host.size());
    return TDOA_OK;
}

}  // extern "C"
