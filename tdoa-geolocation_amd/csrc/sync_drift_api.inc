// sync_drift_api.inc -- the clock-line search (stack_sync_drift.hpp), host side: its buffers, the kernels' launches (shared
// by a context's own step, the group's merged sum and tdoa_debug_sync_drift_from_q), its step product and its entries.
// Included by tdoa_mi355x.hip after group_api.inc.

namespace {

SyncLineGeom syncline_geom(int S, int max_lag, int gate, int max_drift, int L)
{
    SyncLineGeom g;
    g.S = S;
    g.P = S * (S - 1) / 2;
    g.n = 2 * max_lag - 1;
    g.lag_lo = -(max_lag - 1);
    g.W = 2 * gate + 1;
    g.V = 2 * max_drift + 1;
    g.L = L;
    g.cands = g.W * g.V;                     // <= 2047 x 1025
    g.tiles = (g.cands + kSyncLineThreads - 1) / kSyncLineThreads;
    return g;
}

// the arguments the three entries share; they need no device
const char *check_sync_drift_args(int gate, int max_drift, int drift_den, int rounds, const void *ref_delay, const void *line)
{
    if (gate < 0 || gate > kSyncMaxGate) return "gate outside 0 .. 1023";
    if (max_drift < 0 || max_drift > kSyncLineMaxDrift) return "max_drift outside 0 .. 512";
    if (drift_den < 1) return "drift_den < 1";
    if (rounds < 0 || rounds > kSyncMaxRounds) return "rounds outside 0 .. 16";
    if (!ref_delay) return "ref_delay is NULL";
    if (!line) return "line_host is NULL";
    return nullptr;
}

// What a call sends every time: ref_delay and centre (sync_inputs), shift(h, j) at [rank(h) * L + j], sqrt(N_w) per line.
// Data, not part of a step graph's key: the table depends on (H, D, L), which are, but the debug and the group's calls write
// the same buffer.
struct SyncLineInputs {
    std::vector<int32_t> in, tab;
    std::vector<double> line_roots;
};

SyncLineInputs syncline_inputs(const int32_t *ref_delay, const int32_t *centre, int S, int H, int D, int L, int n_lines, double n_w_line)
{
    SyncLineInputs x;
    x.in = sync_inputs(ref_delay, centre, S);
    x.tab.resize((size_t)(2 * H + 1) * L);
    for (int r = 0; r <= 2 * H; r++) {
        const int h = (r & 1) ? (r + 1) / 2 : -(r / 2);
        for (int j = 0; j < L; j++) x.tab[(size_t)r * L + j] = (int32_t)drift_shift(h, j, D);
    }
    x.line_roots.assign((size_t)n_lines, std::sqrt(n_w_line));
    return x;
}

// the outputs of the three entries (all but line may be NULL)
struct SyncLineHost {
    tdoa_sync_line *line = nullptr;          // [line]
    int32_t *clock = nullptr, *rate = nullptr;                   // [line][station]
    int32_t *rows = nullptr;                 // [stack][station]
    int32_t *lags = nullptr;                 // [stack][pair]
    double *corr = nullptr;                  // [stack][pair]
};

int ensure_syncline(tdoa_ctx *ctx, size_t n_lines, const SyncLineGeom &g)
{
    int rc;
    const size_t n_sets = n_lines * g.L;
    if ((rc = ensure(ctx, ctx->sline_in, sizeof(int32_t) * 2 * kSyncMaxStations))) return rc;
    if ((rc = ensure(ctx, ctx->sline_tab, sizeof(int32_t) * (size_t)g.V * g.L))) return rc;
    if ((rc = ensure(ctx, ctx->sline_roots, sizeof(double) * n_lines))) return rc;
    if ((rc = ensure(ctx, ctx->sline_cur, sizeof(long long) * n_lines * g.S * g.L))) return rc;
    if ((rc = ensure(ctx, ctx->sline_k, sizeof(long long) * n_lines * g.S))) return rc;
    if ((rc = ensure(ctx, ctx->sline_h, sizeof(int32_t) * n_lines * g.S))) return rc;
    if ((rc = ensure(ctx, ctx->sline_part, sizeof(ClosureCand) * n_lines * g.tiles))) return rc;
    if ((rc = ensure(ctx, ctx->sline_moved, sizeof(int32_t) * n_lines))) return rc;
    if ((rc = ensure(ctx, ctx->sline_start, sizeof(long long) * n_lines))) return rc;
    if ((rc = ensure(ctx, ctx->sline_out, sizeof(SyncLineOut) * n_lines))) return rc;
    if ((rc = ensure(ctx, ctx->sline_clock, sizeof(int32_t) * n_lines * g.S))) return rc;
    if ((rc = ensure(ctx, ctx->sline_rate, sizeof(int32_t) * n_lines * g.S))) return rc;
    if ((rc = ensure(ctx, ctx->sline_rows, sizeof(int32_t) * n_sets * g.S))) return rc;
    if ((rc = ensure(ctx, ctx->sline_lags, sizeof(int32_t) * n_sets * g.P))) return rc;
    return ensure(ctx, ctx->sline_corr, sizeof(double) * n_sets * g.P);
}

// asynchronous on ctx->stream; `x` lives until the caller has synchronised
int upload_syncline_inputs(tdoa_ctx *ctx, const SyncLineInputs &x)
{
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->sline_in.p, x.in.data(), sizeof(int32_t) * x.in.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->sline_tab.p, x.tab.data(), sizeof(int32_t) * x.tab.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->sline_roots.p, x.line_roots.data(), sizeof(double) * x.line_roots.size(), hipMemcpyHostToDevice, st));
    return TDOA_OK;
}

// Q [n_lines][L][P][n] -> the records, clocks, rates, rows, lags and correlations: the one place the search is launched.
// roots [set]: sqrt(n_w) of the positions' stacks.  Kernel launches only (the step graph captures them): two per step.
void launch_syncline(tdoa_ctx *ctx, const long long *Q, const double *roots, int n_lines, const SyncLineGeom &g, int rounds)
{
    hipStream_t st = ctx->stream;
    const SyncLineDev d{ctx->sline_in.as<const int32_t>(), ctx->sline_tab.as<const int32_t>(), ctx->sline_cur.as<long long>(),
                        ctx->sline_k.as<long long>(),      ctx->sline_h.as<int32_t>(),         ctx->sline_part.as<ClosureCand>(),
                        ctx->sline_moved.as<int32_t>(),    ctx->sline_start.as<long long>()};
    const dim3 lines((unsigned)n_lines), threads(kSyncLineThreads);
    const auto step = [&](int s, int hi, int first, int count) {
        hipLaunchKernelGGL(k_syncline_step, dim3((unsigned)g.tiles, (unsigned)n_lines), threads, 0, st, Q, g, d.in, d.tab,
                           static_cast<const long long *>(d.cur), s, hi, d.part);
        hipLaunchKernelGGL(k_syncline_commit, lines, threads, 0, st, g, d, s, first, count);
    };
    const auto finish = [&](int pass) {
        hipLaunchKernelGGL(k_syncline_finish, lines, threads, 0, st, Q, g, d, pass, roots, ctx->sline_roots.as<const double>(),
                           ctx->sline_out.as<SyncLineOut>(), ctx->sline_clock.as<int32_t>(), ctx->sline_rate.as<int32_t>(),
                           ctx->sline_rows.as<int32_t>(), ctx->sline_lags.as<int32_t>(), ctx->sline_corr.as<double>());
    };
    hipLaunchKernelGGL(k_syncline_init, lines, threads, 0, st, g, d);
    for (int s = 1; s < g.S; s++) step(s, s, 0, 0);
    finish(0);
    for (int r = 0; r < rounds; r++)
        for (int s = 1; s < g.S; s++) step(s, g.S, s == 1, 1);
    finish(1);
}

// the outputs to the host; asynchronous on ctx->stream
int download_syncline(tdoa_ctx *ctx, size_t n_lines, const SyncLineGeom &g, const SyncLineHost &o)
{
    hipStream_t st = ctx->stream;
    const size_t n_sets = n_lines * g.L;
    HIPCHK(ctx, hipMemcpyAsync(o.line, ctx->sline_out.p, sizeof(SyncLineOut) * n_lines, hipMemcpyDeviceToHost, st));
    if (o.clock) HIPCHK(ctx, hipMemcpyAsync(o.clock, ctx->sline_clock.p, sizeof(int32_t) * n_lines * g.S, hipMemcpyDeviceToHost, st));
    if (o.rate) HIPCHK(ctx, hipMemcpyAsync(o.rate, ctx->sline_rate.p, sizeof(int32_t) * n_lines * g.S, hipMemcpyDeviceToHost, st));
    if (o.rows) HIPCHK(ctx, hipMemcpyAsync(o.rows, ctx->sline_rows.p, sizeof(int32_t) * n_sets * g.S, hipMemcpyDeviceToHost, st));
    if (o.lags) HIPCHK(ctx, hipMemcpyAsync(o.lags, ctx->sline_lags.p, sizeof(int32_t) * n_sets * g.P, hipMemcpyDeviceToHost, st));
    if (o.corr) HIPCHK(ctx, hipMemcpyAsync(o.corr, ctx->sline_corr.p, sizeof(double) * n_sets * g.P, hipMemcpyDeviceToHost, st));
    return TDOA_OK;
}

// what tdoa_process_sync_drift and the group's call refuse once the arguments are in range: the lag mode, the captures, the
// station count, the overflow bound of a line's sums.  *what receives the message.
int check_sync_drift_state(const tdoa_ctx *ctx, const char **what)
{
    const auto refuse = [&](int status, const char *why) {
        *what = why;
        return status;
    };
    if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse(TDOA_ERR_UNSUPPORTED, "the clock-line search with TDOA_LAGS_GO");
    if (ctx->caps.empty()) return refuse(TDOA_ERR_STATE, "captures missing");
    const int S = (int)ctx->caps.size();
    if (S < 2 || S > kSyncMaxStations) return refuse(TDOA_ERR_UNSUPPORTED, "the clock-line search needs 2 .. 64 stations");
    int wpb = 0;
    if (tdoa_num_windows(ctx, &wpb, nullptr)) return refuse(TDOA_ERR_STATE, "captures missing or too small");
    if (locate_overflows(S * (S - 1) / 2, wpb))
        return refuse(TDOA_ERR_UNSUPPORTED, "pairs x windows per block > 2^17: a line's sum could overflow");
    if (3ll * wpb > kLocateMaxSets) return refuse(TDOA_ERR_UNSUPPORTED, "more than 65535 stacks");
    return TDOA_OK;
}

// ---- the clock-line search on the stacks' sums, inside the step graph.  Its stack has no output of its own. ---------------
struct SyncDriftProduct : StackProduct {
    int S = 0, G = 0, H = 0, D = 1, R = 0;   // stations, gate, max_drift, drift_den, rounds
    SyncLineInputs inputs;                   // data, not part of the key
    SyncLineHost host;

    SyncLineGeom geom(const tdoa_ctx *ctx) const { return syncline_geom(S, ctx->prm.max_lag, G, H, layout.spb); }
    int reserve(const StepView &v) override
    {
        if (int rc = StackProduct::reserve(v)) return rc;
        if (ensure_syncline(v.ctx, 3, geom(v.ctx))) return surfaces_nomem(v, "the clock-line search's candidates and records", 1.0);
        return TDOA_OK;
    }
    void key(std::vector<uint64_t> *key) const override
    {
        key->insert(key->end(), {SyncDrift, (uint64_t)m, (uint64_t)G | ((uint64_t)H << 32), (uint64_t)D | ((uint64_t)R << 32)});
    }
    int refresh(const StepView &v) override { return upload_syncline_inputs(v.ctx, inputs); }
    void enqueue(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        StackProduct::enqueue(v);
        launch_syncline(ctx, ctx->stack_q.as<const long long>(), stack_dev(ctx, layout.n_stacks, v.P).roots, 3, geom(ctx), R);
    }
    int download(const StepView &v) const override { return download_syncline(v.ctx, 3, geom(v.ctx), host); }
};

// the search on a group's merged sum (finish_from_host, stacked_api.inc)
int sync_drift_from_host(tdoa_ctx *ctx, const int64_t *q_sum, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds,
                         const int32_t *ref_delay, const int32_t *centre, const SyncLineHost &host)
{
    const int S = (int)ctx->caps.size();
    int wpb = 0;
    if (int rc = tdoa_num_windows(ctx, &wpb, nullptr)) return fail(ctx, rc, "captures missing or too small");
    const int L = stack_geom(wpb, windows_per_stack).spb;
    const SyncLineGeom g = syncline_geom(S, ctx->prm.max_lag, gate, max_drift, L);
    const SyncLineInputs x = syncline_inputs(ref_delay, centre, S, max_drift, drift_den, L, 3, (double)wpb);
    return finish_from_host(
        ctx, q_sum, windows_per_stack,
        [&](int, const double *roots) -> int {
            int rc;
            if ((rc = ensure_syncline(ctx, 3, g))) return rc;
            if ((rc = upload_syncline_inputs(ctx, x))) return rc;
            launch_syncline(ctx, ctx->stack_q.as<const long long>(), roots, 3, g, rounds);
            return TDOA_OK;
        },
        [&](int) { return download_syncline(ctx, 3, g, host); });
}

}  // namespace

extern "C" {

static_assert(sizeof(SyncLineOut) == sizeof(tdoa_sync_line) && sizeof(tdoa_sync_line) == 40, "tdoa_sync_line layout");

int tdoa_process_sync_drift(tdoa_ctx *ctx, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds,
                            const int32_t *ref_delay, const int32_t *centre, tdoa_sync_line *line_host, int32_t *clock_host,
                            int32_t *rate_host, int32_t *rows_host, int32_t *lags_host, double *corr_host)
{
    if (int rc = refuse_stacked(ctx, windows_per_stack, check_sync_drift_args(gate, max_drift, drift_den, rounds, ref_delay, line_host),
                                "the clock-line search with TDOA_LAGS_GO", true))
        return rc;
    const char *what = nullptr;              // (the station count, the overflow bound: shared with the group's call)
    if (const int rc = check_sync_drift_state(ctx, &what)) return fail(ctx, rc, what);
    SyncDriftProduct prod;
    fill_stack(&prod, windows_per_stack);
    prod.S = (int)ctx->caps.size();
    prod.G = gate;
    prod.H = max_drift;
    prod.D = drift_den;
    prod.R = rounds;
    int wpb = 0;
    if (int rc = tdoa_num_windows(ctx, &wpb, nullptr)) return fail(ctx, rc, "captures missing or too small");
    prod.inputs = syncline_inputs(ref_delay, centre, prod.S, max_drift, drift_den, stack_geom(wpb, windows_per_stack).spb, 3, (double)wpb);
    prod.host = SyncLineHost{line_host, clock_host, rate_host, rows_host, lags_host, corr_host};
    return process_impl(ctx, 0, 1, nullptr, nullptr, nullptr, 0.0, &prod);
}

// the search's kernels on the caller's words: n_sets sets of P = S (S-1) / 2 rows of 2 max_lag - 1 int64, every set a stack of
// n_w windows, set t * track_len + j position j of line t.  Needs the context for max_lag and the device only.
int tdoa_debug_sync_drift_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int gate,
                                 int max_drift, int drift_den, int rounds, const int32_t *ref_delay, const int32_t *centre,
                                 tdoa_sync_line *line, int32_t *clock, int32_t *rate, int32_t *rows, int32_t *lags, double *corr)
{
    int rc;
    if (!ctx) return TDOA_ERR_INVALID;
    if (const char *bad = check_sync_drift_args(gate, max_drift, drift_den, rounds, ref_delay, line)) return fail(ctx, TDOA_ERR_INVALID, bad);
    if (!q || n_sets < 1 || n_sets > kLocateMaxSets || n_w < 1 || n_stations < 2 || n_stations > kSyncMaxStations)
        return fail(ctx, TDOA_ERR_INVALID, "q is NULL, n_sets outside 1 .. 65535, n_w < 1 or n_stations outside 2 .. 64");
    if (track_len < 1 || n_sets % track_len != 0) return fail(ctx, TDOA_ERR_INVALID, "track_len < 1 or not a divisor of n_sets");
    const int n_lines = n_sets / track_len;
    const SyncLineGeom g = syncline_geom(n_stations, ctx->prm.max_lag, gate, max_drift, track_len);
    if (locate_overflows(g.P, (long long)track_len * n_w))
        return fail(ctx, TDOA_ERR_UNSUPPORTED, "pairs x track_len x n_w > 2^17: a line's sum could overflow");
    std::vector<double> roots;
    const SyncLineInputs x = syncline_inputs(ref_delay, centre, n_stations, max_drift, drift_den, track_len, n_lines, (double)track_len * (double)n_w);
    if ((rc = upload_debug_q(ctx, q, (size_t)n_sets * g.P * g.n, n_sets, n_w, &roots))) return rc;
    if ((rc = ensure_syncline(ctx, n_lines, g))) return rc;
    if ((rc = upload_syncline_inputs(ctx, x))) return rc;
    launch_syncline(ctx, ctx->debug_q.as<const long long>(), ctx->debug_roots.as<const double>(), n_lines, g, rounds);
    const SyncLineHost host{line, clock, rate, rows, lags, corr};
    return download_and_wait(ctx, [&] { return download_syncline(ctx, n_lines, g, host); });
}

// tdoa_process_sync_drift over the members: their shares of the fixed-point sums as in tdoa_group_process_stacked, added on
// the host; member 0 searches the merged Q with the kernels a single context's call ends with.
int tdoa_group_process_sync_drift(tdoa_group *g, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds,
                                  const int32_t *ref_delay, const int32_t *centre, tdoa_sync_line *line_host, int32_t *clock_host,
                                  int32_t *rate_host, int32_t *rows_host, int32_t *lags_host, double *corr_host)
{
    if (!g) return TDOA_ERR_INVALID;
    if (windows_per_stack < 0) return group_fail(g, TDOA_ERR_INVALID, "windows_per_stack < 0");
    if (const char *bad = check_sync_drift_args(gate, max_drift, drift_den, rounds, ref_delay, line_host)) return group_fail(g, TDOA_ERR_INVALID, bad);
    const int world = (int)g->members.size();
    tdoa_ctx *c0 = g->members[0];
    if (world == 1) {                        // no merge: the member's call writes the outputs
        const int rc = tdoa_process_sync_drift(c0, windows_per_stack, gate, max_drift, drift_den, rounds, ref_delay, centre, line_host,
                                               clock_host, rate_host, rows_host, lags_host, corr_host);
        return rc == TDOA_OK ? rc : member_fail(g, 0, rc);
    }
    const char *what = nullptr;
    if (const int rc = check_sync_drift_state(c0, &what)) return group_fail(g, rc, member_name(0, c0->device) + what);
    const int64_t *sum = nullptr;
    if (const int rc = group_merged_q(g, windows_per_stack, &sum)) return rc;
    const SyncLineHost host{line_host, clock_host, rate_host, rows_host, lags_host, corr_host};
    const int rc = sync_drift_from_host(c0, sum, windows_per_stack, gate, max_drift, drift_den, rounds, ref_delay, centre, host);
    return rc == TDOA_OK ? rc : member_fail(g, 0, rc);
}

// The line continued past its block at the table's 1/16 sample (host only): out[j - first][s] = 16 k_s + r(16 h_s j, D).
int tdoa_sync_line_clock(const int32_t *clock, const int32_t *rate, int n_stations, int drift_den, int first_position, int n_positions,
                         int32_t *out)
{
    if (!clock || !rate || !out || n_stations < 1 || drift_den < 1 || first_position < 0 || n_positions < 1) return TDOA_ERR_INVALID;
    for (int j = 0; j < n_positions; j++)
        for (int s = 0; s < n_stations; s++) {
            const long long num = (long long)kLocateDelayUnit * rate[s] * ((long long)first_position + j);
            const long long a = (2 * (num < 0 ? -num : num) + drift_den) / (2 * (long long)drift_den);
            out[(size_t)j * n_stations + s] = (int32_t)((long long)kLocateDelayUnit * clock[s] + (num < 0 ? -a : a));
        }
    return TDOA_OK;
}

}  // extern "C"
