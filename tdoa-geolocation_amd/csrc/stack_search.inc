// stack_search.inc -- a search on the stacks' fixed-point sums Q ([stack][pair][2 max_lag - 1] int64) and the three routes
// that reach every such search, each written once:
//   own step     process_search: the search's kernels are nodes of the context's step graph, behind the stack's accumulation
//   merged sum   group_process_search: the members' partial Q added on the host, searched on member 0 (search_from_host)
//   caller's Q   debug_search_from_q: the caller's words in ctx->debug_q, sqrt(n_w) per set in ctx->debug_roots
// A search is a StackSearch: its checks, its geometry and host-side inputs for a shape (bind), its graph-key words, its
// buffers, its uploads, its launches and its download.  closure_api.inc, sync_api.inc, sync_drift_api.inc and locate_run.inc
// hold one each, with the extern "C" entries that build it from their arguments and call one of the drivers.  A search may
// hold others and compose their members: a refinement (sync_fine_api.inc, sync_drift_fine_api.inc, locate_zoom_api.inc,
// locate_track_zoom_api.inc) holds the search it refines and launches behind it; the one chain (SyncChain, sync_locate_api.inc)
// holds a fine clock stage and a locate stage and puts the clock link between their launches.
// Included by tdoa_mi355x.hip after group_api.inc (the drivers call process_impl and the group's helpers) and before the
// searches' files.

namespace {

// a helper of one search's file that another's uses, declared here so that neither depends on where the other is included
std::vector<int32_t> sync_inputs(const int32_t *ref_delay, const int32_t *centre, int S);      // sync_api.inc; sync_drift_api.inc

// what a search is bound to before its buffers are sized: a context's own stacks, or the caller's sets
struct SearchShape {
    int S, n_sets;                           // stations; stacks (sets) searched
    int L;                                   // the sets of a track or line: the stacks per block, or the caller's track_len
    double track_w;                          // the windows a track or line holds: the windows per block, or track_len x n_w
};

// a check's refusal: the message into *what, the status back
int refuse_with(const char **what, int status, const char *why)
{
    *what = why;
    return status;
}

struct StackSearch {
    const char *go_what;                     // the refusal of TDOA_LAGS_GO under the search's name
    const char *nomem_what;                  // what the step's no-memory message calls the buffers; nullptr: reserve words its own
    StackSearch(const char *go, const char *nomem) : go_what(go), nomem_what(nomem) {}

    // the entries' arguments; needs no device.  The message, or nullptr
    virtual const char *check_args() const = 0;
    // what a context's own call and the group's call refuse of the context's captures and state once the arguments are in range
    virtual int check_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what) const = 0;
    // what the debug entry refuses of the caller's sets
    virtual int check_sets(const tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what) const = 0;
    // geometry and host-side inputs for a shape; the inputs live in the object until the call has synchronised
    virtual void bind(const tdoa_ctx *ctx, const SearchShape &shape) = 0;
    // the words of the step graph's key, the Kind first: everything the launches depend on (m: windows_per_stack)
    virtual void key(std::vector<uint64_t> *key, int m) const = 0;
    virtual int reserve(tdoa_ctx *ctx) const = 0;            // the buffers
    virtual int refresh(tdoa_ctx *ctx) const = 0;            // the inputs to the device, asynchronous on ctx->stream: data, not in the key
    virtual void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const = 0;      // kernel launches only (a step graph captures them)
    virtual int download(tdoa_ctx *ctx) const = 0;           // the outputs to the host, asynchronous on ctx->stream
};

// ---- own step: the search on the stack's sums inside the step graph.  The stack has no output of its own, so no finishing
// kernels (k = min_sep = 1 are never read) -----------------------------------------------------------------------------------
struct SearchProduct : StackProduct {
    StackSearch *search = nullptr;

    int reserve(const StepView &v) override
    {
        if (int rc = StackProduct::reserve(v)) return rc;
        search->bind(v.ctx, SearchShape{(int)v.ctx->caps.size(), layout.n_stacks, layout.spb, (double)v.wpb});
        if (int rc = search->reserve(v.ctx)) return search->nomem_what ? surfaces_nomem(v, search->nomem_what, 1.0) : rc;
        return TDOA_OK;
    }
    void key(std::vector<uint64_t> *key) const override { search->key(key, m); }
    int refresh(const StepView &v) override { return search->refresh(v.ctx); }
    void enqueue(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        StackProduct::enqueue(v);
        search->launch(ctx, ctx->stack_q.as<const long long>(), stack_dev(ctx, layout.n_stacks, v.P).roots);
    }
    int download(const StepView &v) const override { return search->download(v.ctx); }
};

int process_search(tdoa_ctx *ctx, int windows_per_stack, StackSearch &search)
{
    if (int rc = refuse_stacked(ctx, windows_per_stack, search.check_args(), search.go_what, true)) return rc;
    const char *what = nullptr;
    if (const int rc = search.check_state(ctx, windows_per_stack, &what)) return fail(ctx, rc, what);
    SearchProduct prod;
    fill_stack(&prod, windows_per_stack);
    prod.search = &search;
    return process_impl(ctx, 0, 1, nullptr, nullptr, nullptr, 0.0, &prod);
}

// ---- merged sum: the search on a group's sum (finish_from_host, stacked_api.inc); a track or line spans a block --------------
int search_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack, StackSearch &search)
{
    int wpb = 0;
    if (int rc = tdoa_num_windows(ctx, &wpb, nullptr)) return fail(ctx, rc, "captures missing or too small");
    const StackGeom sg = stack_geom(wpb, windows_per_stack);
    search.bind(ctx, SearchShape{(int)ctx->caps.size(), sg.n_stacks, sg.spb, (double)wpb});
    return finish_from_host(
        ctx, q_sum, windows_per_stack,
        [&](int, const double *roots) -> int {
            int rc;
            if ((rc = search.reserve(ctx))) return rc;
            if ((rc = search.refresh(ctx))) return rc;
            search.launch(ctx, ctx->stack_q.as<const long long>(), roots);
            return TDOA_OK;
        },
        [&](int) { return search.download(ctx); });
}

// The search over the members: their shares of the fixed-point sums as in tdoa_group_process_stacked, added on the host;
// member 0 searches the merged Q with the kernels a single context's call ends with.
int group_process_search(tdoa_group *g, int windows_per_stack, StackSearch &search)
{
    if (!g) return TDOA_ERR_INVALID;
    if (windows_per_stack < 0) return group_fail(g, TDOA_ERR_INVALID, "windows_per_stack < 0");
    if (const char *bad = search.check_args()) return group_fail(g, TDOA_ERR_INVALID, bad);
    const int world = (int)g->members.size();
    tdoa_ctx *c0 = g->members[0];
    if (world == 1) {                        // no merge: the member's call writes the outputs
        const int rc = process_search(c0, windows_per_stack, search);
        return rc == TDOA_OK ? rc : member_fail(g, 0, rc);
    }
    const char *what = nullptr;
    if (const int rc = search.check_state(c0, windows_per_stack, &what)) return group_fail(g, rc, member_name(0, c0->device) + what);
    const int64_t *sum = nullptr;
    if (const int rc = group_merged_q(g, windows_per_stack, &sum)) return rc;
    const int rc = search_from_host(c0, sum, windows_per_stack, search);
    return rc == TDOA_OK ? rc : member_fail(g, 0, rc);
}

// ---- caller's Q: the search's kernels on the caller's words: n_sets sets of P = S (S-1) / 2 rows of 2 max_lag - 1 int64, every
// set a stack of n_w windows; set t * track_len + j is position j of track or line t.  The words and sqrt(n_w) per set go to
// buffers that are the debug entries' alone (ctx->debug_q, ctx->debug_roots): the stack's sums and a cached step graph's buffers
// stay as they are.  (A call that has to allocate or grow one of its buffers moves alloc_gen like every ensure(): the next step
// captures its graph again, with the same results.)  Needs the context for max_lag, its settings and the device only. ----------
int debug_search_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, StackSearch &search)
{
    int rc;
    if (!ctx) return TDOA_ERR_INVALID;
    if (const char *bad = search.check_args()) return fail(ctx, TDOA_ERR_INVALID, bad);
    const char *what = nullptr;
    if ((rc = search.check_sets(ctx, q, n_sets, track_len, n_stations, n_w, &what))) return fail(ctx, rc, what);
    search.bind(ctx, SearchShape{n_stations, n_sets, track_len, (double)track_len * (double)n_w});
    const size_t n_q = (size_t)n_sets * (n_stations * (n_stations - 1) / 2) * (size_t)(2 * ctx->prm.max_lag - 1);
    const std::vector<double> roots((size_t)n_sets, std::sqrt((double)n_w));      // (lives until the call has synchronised)
    if ((rc = check_ctx(ctx))) return rc;
    if ((rc = ensure(ctx, ctx->debug_q, sizeof(long long) * n_q))) return rc;
    if ((rc = ensure(ctx, ctx->debug_roots, sizeof(double) * n_sets))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->debug_q.p, q, sizeof(long long) * n_q, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->debug_roots.p, roots.data(), sizeof(double) * n_sets, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = search.reserve(ctx))) return rc;
    if ((rc = search.refresh(ctx))) return rc;
    search.launch(ctx, ctx->debug_q.as<const long long>(), ctx->debug_roots.as<const double>());
    return download_and_wait(ctx, [&] { return search.download(ctx); });
}

}  // namespace
