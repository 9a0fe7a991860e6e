// sync_drift_api.inc -- the clock-line search (stack_sync_drift.hpp), host side: the search as a StackSearch (stack_search.inc)
// -- its checks, geometry, inputs, buffers, the one place its kernels are launched, its download -- the search's three entries
// and tdoa_sync_line_clock.  Included by tdoa_mi355x.hip after stack_search.inc, locate_api.inc (locate_overflows) and
// sync_api.inc (sync_inputs); drift_shift is step_products.inc's.

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

struct SyncLineSearch : StackSearch {
    int G, H, D, R;                          // gate, max_drift, drift_den, rounds
    const int32_t *ref_delay, *centre;       // [stations]; centre NULL: all 0
    SyncLineHost o;
    SyncLineGeom g;                          // bind: the geometry, the lines and the inputs as they are uploaded
    size_t n_lines = 0;
    SyncLineInputs x;

    SyncLineSearch(int gate, int max_drift, int drift_den, int rounds, const int32_t *ref_delay, const int32_t *centre, const SyncLineHost &host)
        : StackSearch("the clock-line search with TDOA_LAGS_GO", "the clock-line search's candidates and records"), G(gate), H(max_drift),
          D(drift_den), R(rounds), ref_delay(ref_delay), centre(centre), o(host)
    {
    }
    const char *check_args() const override
    {
        if (G < 0 || G > kSyncMaxGate) return "gate outside 0 .. 1023";
        if (H < 0 || H > kSyncLineMaxDrift) return "max_drift outside 0 .. 512";
        if (D < 1) return "drift_den < 1";
        if (R < 0 || R > kSyncMaxRounds) return "rounds outside 0 .. 16";
        if (!ref_delay) return "ref_delay is NULL";
        if (!o.line) return "line_host is NULL";
        return nullptr;
    }
    // the lag mode, the captures, the station count, the overflow bound of a line's sums
    int check_state(const tdoa_ctx *ctx, int, const char **what) const override
    {
        if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse_with(what, TDOA_ERR_UNSUPPORTED, go_what);
        if (ctx->caps.empty()) return refuse_with(what, TDOA_ERR_STATE, "captures missing");
        const int S = (int)ctx->caps.size();
        if (S < 2 || S > kSyncMaxStations) return refuse_with(what, TDOA_ERR_UNSUPPORTED, "the clock-line search needs 2 .. 64 stations");
        int wpb = 0;
        if (tdoa_num_windows(ctx, &wpb, nullptr)) return refuse_with(what, TDOA_ERR_STATE, "captures missing or too small");
        if (locate_overflows(S * (S - 1) / 2, wpb))
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "pairs x windows per block > 2^17: a line's sum could overflow");
        if (3ll * wpb > kLocateMaxSets) return refuse_with(what, TDOA_ERR_UNSUPPORTED, "more than 65535 stacks");
        return TDOA_OK;
    }
    int check_sets(const tdoa_ctx *, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what) const override
    {
        if (!q || n_sets < 1 || n_sets > kLocateMaxSets || n_w < 1 || n_stations < 2 || n_stations > kSyncMaxStations)
            return refuse_with(what, TDOA_ERR_INVALID, "q is NULL, n_sets outside 1 .. 65535, n_w < 1 or n_stations outside 2 .. 64");
        if (track_len < 1 || n_sets % track_len != 0) return refuse_with(what, TDOA_ERR_INVALID, "track_len < 1 or not a divisor of n_sets");
        if (locate_overflows(n_stations * (n_stations - 1) / 2, (long long)track_len * n_w))
            return refuse_with(what, TDOA_ERR_UNSUPPORTED, "pairs x track_len x n_w > 2^17: a line's sum could overflow");
        return TDOA_OK;
    }
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override
    {
        g = syncline_geom(sh.S, ctx->prm.max_lag, G, H, sh.L);
        n_lines = (size_t)(sh.n_sets / sh.L);
        x = syncline_inputs(ref_delay, centre, sh.S, H, D, sh.L, (int)n_lines, sh.track_w);
    }
    void key(std::vector<uint64_t> *key, int m) const override
    {
        key->insert(key->end(), {StepProduct::SyncDrift, (uint64_t)m, (uint64_t)G | ((uint64_t)H << 32), (uint64_t)D | ((uint64_t)R << 32)});
    }
    int reserve(tdoa_ctx *ctx) const override
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
    int refresh(tdoa_ctx *ctx) const override
    {
        hipStream_t st = ctx->stream;
        HIPCHK(ctx, hipMemcpyAsync(ctx->sline_in.p, x.in.data(), sizeof(int32_t) * x.in.size(), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->sline_tab.p, x.tab.data(), sizeof(int32_t) * x.tab.size(), hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->sline_roots.p, x.line_roots.data(), sizeof(double) * x.line_roots.size(), hipMemcpyHostToDevice, st));
        return TDOA_OK;
    }
    // Q [n_lines][L][P][n] -> the records, clocks, rates, rows, lags and correlations: the one place the search is launched.
    // roots [set]: sqrt(n_w) of the positions' stacks.  Two launches per step.
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override
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
            hipLaunchKernelGGL(k_syncline_finish, lines, threads, 0, st, Q, SyncGrid{g.n, g.lag_lo}, g, d, d.k, d.h, nullptr, pass, roots,
                               ctx->sline_roots.as<const double>(),
                               ctx->sline_out.as<SyncLineOut>(), ctx->sline_clock.as<int32_t>(), ctx->sline_rate.as<int32_t>(),
                               ctx->sline_rows.as<int32_t>(), ctx->sline_lags.as<int32_t>(), ctx->sline_corr.as<double>());
        };
        hipLaunchKernelGGL(k_syncline_init, lines, threads, 0, st, g, d);
        for (int s = 1; s < g.S; s++) step(s, s, 0, 0);
        finish(0);
        for (int r = 0; r < R; r++)
            for (int s = 1; s < g.S; s++) step(s, g.S, s == 1, 1);
        finish(1);
    }
    int download(tdoa_ctx *ctx) const override
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
};

}  // namespace

extern "C" {

static_assert(sizeof(SyncLineOut) == sizeof(tdoa_sync_line) && sizeof(tdoa_sync_line) == 40, "tdoa_sync_line layout");

int tdoa_process_sync_drift(tdoa_ctx *ctx, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds,
                            const int32_t *ref_delay, const int32_t *centre, tdoa_sync_line *line_host, int32_t *clock_host,
                            int32_t *rate_host, int32_t *rows_host, int32_t *lags_host, double *corr_host)
{
    SyncLineSearch s(gate, max_drift, drift_den, rounds, ref_delay, centre, SyncLineHost{line_host, clock_host, rate_host, rows_host, lags_host, corr_host});
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_group_process_sync_drift(tdoa_group *g, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds,
                                  const int32_t *ref_delay, const int32_t *centre, tdoa_sync_line *line_host, int32_t *clock_host,
                                  int32_t *rate_host, int32_t *rows_host, int32_t *lags_host, double *corr_host)
{
    SyncLineSearch s(gate, max_drift, drift_den, rounds, ref_delay, centre, SyncLineHost{line_host, clock_host, rate_host, rows_host, lags_host, corr_host});
    return group_process_search(g, windows_per_stack, s);
}

// set t * track_len + j is position j of line t
int tdoa_debug_sync_drift_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int gate,
                                 int max_drift, int drift_den, int rounds, const int32_t *ref_delay, const int32_t *centre,
                                 tdoa_sync_line *line, int32_t *clock, int32_t *rate, int32_t *rows, int32_t *lags, double *corr)
{
    SyncLineSearch s(gate, max_drift, drift_den, rounds, ref_delay, centre, SyncLineHost{line, clock, rate, rows, lags, corr});
    return debug_search_from_q(ctx, q, n_sets, track_len, n_stations, n_w, s);
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
