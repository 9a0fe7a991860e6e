// closure_api.inc -- the closure search (stack_closure.hpp), host side: the search as a StackSearch (stack_search.inc) -- its
// checks, geometry, buffers, the one place its kernels are launched, its download -- tdoa_num_triples and the search's three
// entries.  Included by tdoa_mi355x.hip after stack_search.inc.

namespace {

int closure_triples(int S) { return S * (S - 1) * (S - 2) / 6; }

ClosureGeom closure_geom(int S, int max_lag, int gate, int min_separation)
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

struct ClosureSearch : StackSearch {
    int G, sep;                              // gate, min_separation
    const int32_t *centre_in;                // [stations], NULL: all 0
    tdoa_closure *out;                       // [set][triple]
    ClosureGeom g;                           // bind: the geometry, the sets and the centres as they are uploaded
    size_t n_sets = 0;
    std::vector<int32_t> centre;

    ClosureSearch(int gate, int min_separation, const int32_t *centre, tdoa_closure *out)
        : StackSearch("the closure search with TDOA_LAGS_GO", "the closure search's candidates and records"), G(gate), sep(min_separation),
          centre_in(centre), out(out)
    {
    }
    const char *check_args() const override
    {
        if (G < 0 || G > kClosureMaxGate) return "gate outside 0 .. 1023";
        if (sep < 1) return "min_separation < 1";
        if (!out) return "the output is NULL";
        return nullptr;
    }
    int check_state(const tdoa_ctx *ctx, int, const char **what) const override
    {
        if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse_with(what, TDOA_ERR_UNSUPPORTED, go_what);
        if (ctx->caps.empty()) return refuse_with(what, TDOA_ERR_STATE, "captures missing");
        if (ctx->caps.size() < 3 || ctx->caps.size() > (size_t)kClosureMaxStations)
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "the closure search needs 3 .. 64 stations");
        return TDOA_OK;
    }
    int check_sets(const tdoa_ctx *, const int64_t *q, int n_sets, int, int n_stations, int n_w, const char **what) const override
    {
        if (!q || n_sets < 1 || n_w < 1 || n_stations < 3 || n_stations > kClosureMaxStations)
            return refuse_with(what, TDOA_ERR_INVALID, "q is NULL, n_sets < 1, n_w < 1 or n_stations outside 3 .. 64");
        if ((long long)n_sets * closure_triples(n_stations) > INT_MAX / 4) return refuse_with(what, TDOA_ERR_INVALID, "too many sets");
        return TDOA_OK;
    }
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override
    {
        g = closure_geom(sh.S, ctx->prm.max_lag, G, sep);
        n_sets = (size_t)sh.n_sets;
        centre = centre_in ? std::vector<int32_t>(centre_in, centre_in + sh.S) : std::vector<int32_t>((size_t)sh.S, 0);
    }
    void key(std::vector<uint64_t> *key, int m) const override
    {
        key->insert(key->end(), {StepProduct::Closure, (uint64_t)m, (uint64_t)G, (uint64_t)sep});
    }
    // centres, the tiles' candidates, (u*, v*) and the records
    int reserve(tdoa_ctx *ctx) const override
    {
        int rc;
        const size_t n_st = n_sets * (size_t)g.T;
        if ((rc = ensure(ctx, ctx->closure_centre, sizeof(int32_t) * kClosureMaxStations))) return rc;
        if ((rc = ensure(ctx, ctx->closure_part, sizeof(ClosureCand) * n_st * g.tiles))) return rc;
        if ((rc = ensure(ctx, ctx->closure_best, sizeof(ClosureBest) * n_st))) return rc;
        return ensure(ctx, ctx->closure_out, sizeof(ClosureOut) * n_st);
    }
    // the stations' centres: a call that changes only them replays the same graph
    int refresh(tdoa_ctx *ctx) const override
    {
        HIPCHK(ctx, hipMemcpyAsync(ctx->closure_centre.p, centre.data(), sizeof(int32_t) * centre.size(), hipMemcpyHostToDevice, ctx->stream));
        return TDOA_OK;
    }
    // Q [n_sets][P][n] -> the records in ctx->closure_out: the one place the search is launched
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
    {
        hipStream_t st = ctx->stream;
        const dim3 grid((unsigned)(n_sets * g.T), (unsigned)g.tiles), one((unsigned)(n_sets * g.T));
        const size_t lds = closure_lds_bytes(g.G);
        auto *centres = ctx->closure_centre.as<const int32_t>();
        auto *part = ctx->closure_part.as<ClosureCand>();
        auto *best = ctx->closure_best.as<ClosureBest>();
        auto *rec = ctx->closure_out.as<ClosureOut>();
        for (int pass = 0; pass < 2; pass++) {
            hipLaunchKernelGGL(k_closure_search, grid, dim3(kClosureThreads), lds, st, Q, g, centres,
                               pass ? static_cast<const ClosureBest *>(best) : nullptr, part);
            hipLaunchKernelGGL(k_closure_finish, one, dim3(kClosureThreads), 0, st, Q, g, centres, roots,
                               static_cast<const ClosureCand *>(part), pass, best, rec);
        }
    }
    int download(tdoa_ctx *ctx) const override
    {
        HIPCHK(ctx, hipMemcpyAsync(out, ctx->closure_out.p, sizeof(ClosureOut) * n_sets * g.T, hipMemcpyDeviceToHost, ctx->stream));
        return TDOA_OK;
    }
};

}  // namespace

extern "C" {

int tdoa_num_triples(const tdoa_ctx *ctx)
{
    if (!ctx) return 0;
    const int S = (int)ctx->caps.size();
    return S >= 3 && S <= kClosureMaxStations ? closure_triples(S) : 0;
}

int tdoa_process_closure(tdoa_ctx *ctx, int windows_per_stack, int gate, int min_separation, const int32_t *centre,
                         tdoa_closure *closure_host)
{
    ClosureSearch s(gate, min_separation, centre, closure_host);
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_closure(tdoa_group *g, int windows_per_stack, int gate, int min_separation, const int32_t *centre,
                               tdoa_closure *closure_host)
{
    ClosureSearch s(gate, min_separation, centre, closure_host);
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_debug_closure_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int gate, int min_separation,
                              const int32_t *centre, tdoa_closure *out)
{
    ClosureSearch s(gate, min_separation, centre, out);
    return debug_search_from_q(ctx, q, n_sets, 0, n_stations, n_w, s);
}

}  // extern "C"
