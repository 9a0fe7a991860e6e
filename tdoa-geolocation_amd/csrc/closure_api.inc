// closure_api.inc -- the closure search, host side: its buffers, the kernels' launches (shared by a context's own step,
// step_products.inc, the group's merged sum and tdoa_debug_closure_from_q), tdoa_num_triples.
// Included by tdoa_mi355x.hip after stacked_api.inc and before step_products.inc.

extern "C" {

static int closure_triples(int S) { return S * (S - 1) * (S - 2) / 6; }

static ClosureGeom closure_geom(int S, int max_lag, int gate, int min_separation)
{
    ClosureGeom g;
    g.S = S;
    g.P = S * (S - 1) / 2;
    g.T = closure_triples(S);
    g.n = 2 * max_lag - 1;
    g.lag_lo = -(max_lag - 1);
    g.G = gate;
    g.sep = min_separation;
    g.tiles = (2 * gate + 1 + kClosureTileU - 1) / kClosureTileU;
    return g;
}

// the arguments the three closure entries share; they need no device
static const char *check_closure_args(int gate, int min_separation, const void *out)
{
    if (gate < 0 || gate > kClosureMaxGate) return "gate outside 0 .. 1023";
    if (min_separation < 1) return "min_separation < 1";
    if (!out) return "the output is NULL";
    return nullptr;
}

// the buffers of the search for n_sets stacks: centres, the tiles' candidates, (u*, v*) and the records
static int ensure_closure(tdoa_ctx *ctx, size_t n_sets, const ClosureGeom &g)
{
    int rc;
    const size_t n_st = n_sets * (size_t)g.T;
    if ((rc = ensure(ctx, ctx->closure_centre, sizeof(int32_t) * kClosureMaxStations))) return rc;
    if ((rc = ensure(ctx, ctx->closure_part, sizeof(ClosureCand) * n_st * g.tiles))) return rc;
    if ((rc = ensure(ctx, ctx->closure_best, sizeof(ClosureBest) * n_st))) return rc;
    return ensure(ctx, ctx->closure_out, sizeof(ClosureOut) * n_st);
}

// the stations' centres to the device, before the launch (asynchronous on ctx->stream; `centre` lives until the caller has
// synchronised).  Data, not part of a step graph's key: a call that changes only the centres replays the same graph.
static int upload_closure_centre(tdoa_ctx *ctx, const std::vector<int32_t> &centre)
{
    HIPCHK(ctx, hipMemcpyAsync(ctx->closure_centre.p, centre.data(), sizeof(int32_t) * centre.size(), hipMemcpyHostToDevice, ctx->stream));
    return TDOA_OK;
}

// Q [n_sets][P][n] -> the records in ctx->closure_out: the one place the search is launched.  Kernel launches only (the
// step graph captures them).
static void launch_closure(tdoa_ctx *ctx, const long long *Q, const double *roots, int n_sets, const ClosureGeom &g)
{
    hipStream_t st = ctx->stream;
    const dim3 grid((unsigned)(n_sets * g.T), (unsigned)g.tiles), one((unsigned)(n_sets * g.T));
    const size_t lds = closure_lds_bytes(g.G);
    auto *centre = ctx->closure_centre.as<const int32_t>();
    auto *part = ctx->closure_part.as<ClosureCand>();
    auto *best = ctx->closure_best.as<ClosureBest>();
    auto *out = ctx->closure_out.as<ClosureOut>();
    for (int pass = 0; pass < 2; pass++) {
        hipLaunchKernelGGL(k_closure_search, grid, dim3(kClosureThreads), lds, st, Q, g, centre,
                           pass ? static_cast<const ClosureBest *>(best) : nullptr, part);
        hipLaunchKernelGGL(k_closure_finish, one, dim3(kClosureThreads), 0, st, Q, g, centre, roots,
                           static_cast<const ClosureCand *>(part), pass, best, out);
    }
}

static int download_closure(tdoa_ctx *ctx, size_t n_sets, const ClosureGeom &g, tdoa_closure *out)
{
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->closure_out.p, sizeof(ClosureOut) * n_sets * g.T, hipMemcpyDeviceToHost, ctx->stream));
    return TDOA_OK;
}

static std::vector<int32_t> closure_centres(const int32_t *centre, int S)
{
    return centre ? std::vector<int32_t>(centre, centre + S) : std::vector<int32_t>((size_t)S, 0);
}

int tdoa_num_triples(const tdoa_ctx *ctx)
{
    if (!ctx) return 0;
    const int S = (int)ctx->caps.size();
    return S >= 3 && S <= kClosureMaxStations ? closure_triples(S) : 0;
}

// the closure search on a group's merged sum (finish_from_host, stacked_api.inc)
static int closure_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack, int gate, int min_separation,
                             const int32_t *centre, tdoa_closure *out)
{
    const int S = (int)ctx->caps.size();
    const ClosureGeom g = closure_geom(S, ctx->prm.max_lag, gate, min_separation);
    const std::vector<int32_t> c = closure_centres(centre, S);
    return finish_from_host(
        ctx, q_sum, windows_per_stack,
        [&](int n_stacks, const double *roots) -> int {
            int rc;
            if ((rc = ensure_closure(ctx, n_stacks, g))) return rc;
            if ((rc = upload_closure_centre(ctx, c))) return rc;
            launch_closure(ctx, ctx->stack_q.as<const long long>(), roots, n_stacks, g);
            return TDOA_OK;
        },
        [&](int n_stacks) { return download_closure(ctx, n_stacks, g, out); });
}

}  // extern "C"
