// locate_run.inc -- the delay-table family, host side: tdoa_process_locate, tdoa_process_locate_multi, tdoa_process_locate_track
// and tdoa_process_locate_track_multi are one computation with two switches (K rounds on masked lags; the recurrence over the L
// stacks of a track).  A LocateCall is what a caller of one of the four asks for, a LocateRun is the call on n_sets stacks; the
// checks the entries share and the run's buffers, launches and download exist once, here; LocateSearch hands them to the three
// routes of stack_search.inc, and the family's twelve entries and tdoa_debug_upsample_q are at the end.
// Included by tdoa_mi355x.hip after stack_search.inc, map_stats_api.inc and locate_api.inc.

namespace {

// what one of the four entries is asked for.  tracks and rounds say which entry it is: without rounds K = 1 and guard = 0, and
// only the entry with both reports the per-stack counts (pairs).  Of the outputs a search takes loc (required), lags, corr and
// map, the tracks take track (required), cells, own, pairs (with rounds), lags, corr and total.
struct LocateCall {
    bool tracks = false, rounds = false;
    int J = 0;                               // max_step
    int K = 1, guard = 0;                    // n_emitters, guard
    int sep = 1;                             // min_separation
    tdoa_location *loc = nullptr;            // [round][stack]
    tdoa_cell_track *track = nullptr;        // [round][track]
    int32_t *cells = nullptr;                // [round][track][L]
    int64_t *own = nullptr;                  // [round][track][L]
    int32_t *pairs = nullptr;                // [round][stack][2]: pairs_in, reserved
    int32_t *lags = nullptr;                 // [round][stack][pair]
    double *corr = nullptr;                  // [round][stack][pair]
    int64_t *map = nullptr;                  // [round][stack][cell]
    int64_t *total = nullptr;                // [round][track][cell]
};

// the two searches' and the two tracks' calls (n_emitters and guard are read with rounds only)
LocateCall locate_search_call(bool rounds, int n_emitters, int guard, int min_separation, tdoa_location *loc, int32_t *lags, double *corr,
                              int64_t *map)
{
    LocateCall c;
    c.rounds = rounds;
    c.K = rounds ? n_emitters : 1;
    c.guard = rounds ? guard : 0;
    c.sep = min_separation;
    c.loc = loc;
    c.lags = lags;
    c.corr = corr;
    c.map = map;
    return c;
}
LocateCall locate_track_call(bool rounds, int max_step, int n_emitters, int guard, int min_separation, tdoa_cell_track *track, int32_t *cells,
                             int64_t *own, int32_t *pairs, int32_t *lags, double *corr, int64_t *total)
{
    LocateCall c = locate_search_call(rounds, n_emitters, guard, min_separation, nullptr, lags, corr, nullptr);
    c.tracks = true;
    c.J = max_step;
    c.track = track;
    c.cells = cells;
    c.own = own;
    c.pairs = pairs;
    c.total = total;
    return c;
}

// a call on n_sets stacks.  With the setting U > 1 (tdoa_locate_set_upsample) the kernels run on the upsampled surfaces: g
// describes those -- n = (n_in - 1) U + 1 fine lags from lag_lo U -- and guard counts fine lags
struct LocateRun {
    LocateGeom g;
    int U, n_in;                             // the factor; the lags of a row of the Q the call is given
    int n_sets;
    int L;                                   // the stacks of a track, 0: no recurrence (the search alone)
    int J, K, guard;
    bool pairs;                              // the per-stack counts are produced (and with them the centres, even for K = 1)

    size_t n_tracks() const { return L ? (size_t)n_sets / L : 0; }
    size_t plane() const { return (size_t)n_sets * g.n_cells; }      // one round's maps, in words
};

LocateRun locate_run(const tdoa_ctx *ctx, const LocateCall &c, int n_sets, int L)
{
    LocateGeom g = locate_geom(ctx, c.sep);
    const int U = ctx->locate_up, n_in = g.n;
    g.n = (int32_t)upsample_len(n_in, U);                                    // (check_locate_upsample: it fits)
    g.lag_lo *= U;
    const int guard = (int)std::min<long long>((long long)c.guard * U, g.n);      // (a guard of the range's length excludes every lag)
    return LocateRun{g, U, n_in, n_sets, c.tracks ? L : 0, c.J, c.K, guard, c.tracks && c.rounds};
}

// What the setting U > 1 adds to the refusals of a call on n_sets stacks of P pairs, once the table and the clocks are known:
// nullptr, or the message and *status.  The fine lags of a row must fit 32 bits and U times every table and clock entry too
// (TDOA_ERR_UNSUPPORTED); the upsampled surfaces must not be larger than the device's memory (TDOA_ERR_NOMEM, by arithmetic:
// nothing is allocated here).
const char *check_locate_upsample(const tdoa_ctx *ctx, size_t n_sets, int P, int *status, bool ctx_clocks = true)
{
    thread_local char buf[320];
    const int U = ctx->locate_up;
    if (U == 1) return nullptr;
    *status = TDOA_ERR_UNSUPPORTED;
    const long long n_u = upsample_len(2ll * ctx->prm.max_lag - 1, U);
    if (n_u > INT_MAX) return "the upsampled lag range does not fit 32 bits";
    if (ctx->locate_table_max * U >= (1ll << 31)) return "a delay table entry times the upsampling factor does not fit 32 bits";
    if (ctx_clocks && ctx->clock_stacks && ctx->locate_clock_max * U >= (1ll << 31)) return "a clock table entry times the upsampling factor does not fit 32 bits";
    const double bytes = 8.0 * (double)n_sets * (double)P * (double)n_u;
    const size_t tiles = ((size_t)(2ll * ctx->prm.max_lag - 1) + kUpsampleThreads - 1) / kUpsampleThreads;
    if ((ctx->total_mem && bytes > (double)ctx->total_mem) || (double)n_sets * P * (double)tiles > (double)INT_MAX) {
        *status = TDOA_ERR_NOMEM;
        snprintf(buf, sizeof(buf), "the delay-table search's upsampled surfaces [%zu stacks][%d pairs][%lld lags of 1/%d sample] (%.1f MB) do not fit in device memory",
                 n_sets, P, n_u, U, bytes / 1e6);
        return buf;
    }
    return nullptr;
}

// the arguments of a call; they need no device
const char *check_locate_call(const LocateCall &c)
{
    if (c.rounds && (c.K < 1 || c.K > kLocateMaxEmitters)) return "n_emitters outside 1 .. 8";
    if (c.rounds && c.guard < 0) return "guard < 0";
    if (c.tracks && (c.J < 0 || c.J > kCellTrackMaxStep)) return "max_step outside 0 .. 16";
    if (c.sep < 1) return "min_separation < 1";
    if (c.tracks ? !c.track : !c.loc) return c.tracks ? "track_host is NULL" : "loc_host is NULL";
    return nullptr;
}

// what a search on S stations needs of the context's table; nullptr when it is there
const char *check_locate_table(const tdoa_ctx *ctx, int S)
{
    if (ctx->locate_cells == 0) return "no delay table (tdoa_locate_set_table)";
    if (ctx->locate_stations != S) return "the delay table's n_stations differs from the stations searched";
    return nullptr;
}

// what a search on n_sets stacks of S stations needs of the context's clock table, when there is one
const char *check_locate_clock(const tdoa_ctx *ctx, int n_sets, int S)
{
    if (ctx->clock_stacks == 0) return nullptr;
    if (ctx->clock_stacks != n_sets) return "the clock table's n_stacks differs from the stacks searched";
    if (ctx->clock_stations != S) return "the clock table's n_stations differs from the stations searched";
    return nullptr;
}

// what a context's own call and the group's call refuse once the arguments are in range: the lag mode, the captures, the
// station count, the table, the overflow bound, the clock table's shape; with tracks also a track's sum that could overflow
// and too many positions.  *what receives the message.  ctx_clocks: the run adds the context's clock table (LocateClocks);
// a run under clocks of its own asks nothing of that table.
int check_locate_state(const tdoa_ctx *ctx, int windows_per_stack, bool tracks, const char **what, bool ctx_clocks = true)
{
    const auto refuse = [&](int status, const char *why) {
        *what = why;
        return status;
    };
    if (ctx->prm.lag_mode == TDOA_LAGS_GO) return refuse(TDOA_ERR_UNSUPPORTED, "the delay-table search with TDOA_LAGS_GO");
    if (ctx->caps.empty()) return refuse(TDOA_ERR_STATE, "captures missing");
    const int S = (int)ctx->caps.size(), P = S * (S - 1) / 2;
    if (S < 2 || S > kLocateMaxStations) return refuse(TDOA_ERR_UNSUPPORTED, "the delay-table search needs 2 .. 64 stations");
    if (const char *bad = check_locate_table(ctx, S)) return refuse(TDOA_ERR_STATE, bad);
    int wpb = 0;
    if (tdoa_num_windows(ctx, &wpb, nullptr)) return refuse(TDOA_ERR_STATE, "captures missing or too small");
    const StackGeom sg = stack_geom(wpb, windows_per_stack);
    const int U = ctx->locate_up;
    if (locate_overflows(P, sg.mm, U))
        return refuse(TDOA_ERR_UNSUPPORTED, U > 1 ? "4 x pairs x stack length > 2^17 on upsampled surfaces: a cell's score could overflow"
                                                  : "pairs x stack length > 2^17: a cell's score could overflow");
    if (3ll * wpb > kLocateMaxSets) return refuse(TDOA_ERR_UNSUPPORTED, "more than 65535 stacks");
    if (ctx_clocks)
        if (const char *bad = check_locate_clock(ctx, sg.n_stacks, S)) return refuse(TDOA_ERR_STATE, bad);
    int status = TDOA_OK;
    if (const char *bad = check_locate_upsample(ctx, (size_t)sg.n_stacks, P, &status, ctx_clocks)) return refuse(status, bad);
    if (!tracks) return TDOA_OK;
    if (locate_overflows(P, wpb, U))
        return refuse(TDOA_ERR_UNSUPPORTED, U > 1 ? "4 x pairs x windows per block > 2^17 on upsampled surfaces: a track's sum could overflow"
                                                  : "pairs x windows per block > 2^17: a track's sum could overflow");
    if (sg.spb > kCellTrackMaxLen) return refuse(TDOA_ERR_UNSUPPORTED, "a track of more than 4096 stacks");
    return TDOA_OK;
}

// what the debug entries refuse of the caller's sets: the table, the clock table's shape, the overflow bounds, the track's length
int check_locate_sets(const tdoa_ctx *ctx, bool tracks, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what,
                      bool ctx_clocks = true)
{
    if (!q || n_sets < 1 || n_sets > kLocateMaxSets || n_w < 1 || n_stations < 2 || n_stations > kLocateMaxStations)
        return refuse_with(what, TDOA_ERR_INVALID, "q is NULL, n_sets outside 1 .. 65535, n_w < 1 or n_stations outside 2 .. 64");
    if (tracks && (track_len < 1 || n_sets % track_len != 0)) return refuse_with(what, TDOA_ERR_INVALID, "track_len < 1 or not a divisor of n_sets");
    if (const char *bad = check_locate_table(ctx, n_stations)) return refuse_with(what, TDOA_ERR_STATE, bad);
    if (ctx_clocks)
        if (const char *bad = check_locate_clock(ctx, n_sets, n_stations)) return refuse_with(what, TDOA_ERR_STATE, bad);
    const int P = n_stations * (n_stations - 1) / 2, U = ctx->locate_up;
    if (!tracks && locate_overflows(P, n_w, U))
        return refuse_with(what, TDOA_ERR_UNSUPPORTED, U > 1 ? "4 x pairs x n_w > 2^17 on upsampled surfaces: a cell's score could overflow"
                                                              : "pairs x n_w > 2^17: a cell's score could overflow");
    if (tracks && locate_overflows(P, (long long)track_len * n_w, U))
        return refuse_with(what, TDOA_ERR_UNSUPPORTED, U > 1 ? "4 x pairs x track_len x n_w > 2^17 on upsampled surfaces: a track's sum could overflow"
                                                              : "pairs x track_len x n_w > 2^17: a track's sum could overflow");
    int status = TDOA_OK;
    if (const char *bad = check_locate_upsample(ctx, (size_t)n_sets, P, &status, ctx_clocks)) return refuse_with(what, status, bad);
    if (tracks && track_len > kCellTrackMaxLen) return refuse_with(what, TDOA_ERR_UNSUPPORTED, "a track of more than 4096 stacks");
    return TDOA_OK;
}

// ---- where a round's planes lie -----------------------------------------------------------------------------------------------
// The buffers of a run, in units of one round's plane ([stack] or [track] records, [stack][pair] words, [stack][cell] or
// [track][cell] sums); "-" is not requested.  Round r's plane is plane r of its buffer, with two exceptions: locate_map with
// tracks of L > 1, and ctrack_t.
//
//   buffer          search (L = 0)   tracks, L = 1     tracks, L > 1   what a round keeps there
//   locate_map      K                K                 1               its scores.  L > 1: every round's scores overwrite the one
//                                                                      plane (the round's finish has read it by then); L = 1: a
//                                                                      track never leaves its map, which is T_0 and goes to the caller
//   locate_part     1                1                 1               the tiles' candidates, one round at a time: the search's, then
//   locate_best     1                1                 1               the tracks' (never more than the stacks), and the best cells
//   locate_out      K                1                 1               the search's records; with tracks only round 0 runs the
//                                                                      search's finish, and its records stay on the device
//   locate_lags     K                K                 K               the best cells' lags and correlations, or the positions' of
//   locate_corr     K                K                 K               the round's tracks (round 0's overwrite the search's)
//   locate_centres  1 (K > 1 only)   1 (K > 1 or the counts)           the excluded intervals' centres [stack][pair], all rounds' words
//   ctrack_d        -                -                 1               the steps D: a round's finish walks them before the next
//                                                                      round's steps write them
//   ctrack_t        -                -                 K + 1           [T_0 of round 0][the other half][T_0 of round 1] ... [T_0 of
//                                                                      round K - 1]: a round steps between its own T_0 and the shared
//                                                                      other half, so every round's T_0 is there for the download
//   ctrack_roots    -                1                 1               sqrt(N_w) per track (data: uploaded by every call)
//   ctrack_out      -                K                 K               the tracks' records
//   ctrack_cells    -                K                 K               the tracks' cells and own scores [stack]
//   ctrack_own      -                K                 K
//   ctrack_pairs    -                K (the counts)    K (the counts)  pairs_in and reserved [stack][2]
//   map statistics  K n_sets         the larger of n_sets and K n_tracks   one record per judged plane: the search judges its maps,
//                                                                      the tracks judge T_0
//   locate_qu       with U > 1: the upsampled surfaces [stack][pair][n], which every kernel above then reads as Q,
//   locate_table_up             U x the table [station][cell] and U x the clock differences [stack][pair]: state beside the table and
//   locate_clock_up             the clocks, remade when either or U changes (remake_locate_scaled), data of a replayed graph

// round r's scores [stack][cell]
long long *locate_run_map(const tdoa_ctx *ctx, const LocateRun &run, int r)
{
    return ctx->locate_map.as<long long>() + (run.L > 1 ? 0 : (size_t)r * run.plane());
}

// the planes round r's call judges and the caller of the tracks receives as `total`: T_0 of its tracks [track][cell], which for
// tracks of one stack -- and for the search, whose stacks are judged one by one -- are the round's maps
long long *locate_run_total(const tdoa_ctx *ctx, const LocateRun &run, int r)
{
    if (run.L <= 1) return locate_run_map(ctx, run, r);
    return ctx->ctrack_t.as<long long>() + (size_t)(r == 0 ? 0 : r + 1) * run.n_tracks() * run.g.n_cells;
}

// the ping-pong's other half (L > 1)
long long *locate_run_other(const tdoa_ctx *ctx, const LocateRun &run) { return ctx->ctrack_t.as<long long>() + run.n_tracks() * run.g.n_cells; }

// round r's planes of the per-stack and per-track buffers
struct LocateRound {
    LocateOut *out;            // the search's records
    int32_t *lags;
    double *corr;
    CellTrackOut *track;       // the tracks' records, cells, own scores and counts
    int32_t *cells;
    long long *own;
    int32_t *pairs;
};
LocateRound locate_run_round(const tdoa_ctx *ctx, const LocateRun &run, int r)
{
    const size_t set0 = (size_t)r * run.n_sets;
    return LocateRound{ctx->locate_out.as<LocateOut>() + set0,
                       ctx->locate_lags.as<int32_t>() + set0 * run.g.P,
                       ctx->locate_corr.as<double>() + set0 * run.g.P,
                       ctx->ctrack_out.as<CellTrackOut>() + (size_t)r * run.n_tracks(),
                       ctx->ctrack_cells.as<int32_t>() + set0,
                       ctx->ctrack_own.as<long long>() + set0,
                       ctx->ctrack_pairs.as<int32_t>() + 2 * set0};
}

// the planes the run's statistics judge
size_t locate_run_judged(const LocateRun &run) { return (size_t)run.K * (run.L ? run.n_tracks() : (size_t)run.n_sets); }

// the run's buffers (the table above)
int ensure_locate_run(tdoa_ctx *ctx, const LocateRun &run)
{
    int rc;
    const LocateGeom &g = run.g;
    const size_t n_sets = run.n_sets, n_tracks = run.n_tracks(), K = run.K, sp = n_sets * g.P;
    const size_t map_planes = run.L > 1 ? 1 : K, t_planes = run.L > 1 ? K + 1 : 0;
    if (run.U > 1) {
        if (ensure(ctx, ctx->locate_qu, sizeof(long long) * sp * (size_t)g.n)) {
            char buf[320];
            snprintf(buf, sizeof(buf), "the delay-table search's upsampled surfaces [%zu stacks][%d pairs][%d lags of 1/%d sample] (%.1f MB) do not fit in device memory: %s",
                     n_sets, (int)g.P, (int)g.n, run.U, 8.0 * (double)sp * (double)g.n / 1e6, ctx->last_error.c_str());
            return fail(ctx, TDOA_ERR_NOMEM, buf);
        }
    }
    if (ensure(ctx, ctx->locate_map, sizeof(long long) * map_planes * run.plane()) ||
        (run.L > 1 && (ensure(ctx, ctx->ctrack_d, 2 * run.plane()) || ensure(ctx, ctx->ctrack_t, sizeof(long long) * t_planes * n_tracks * g.n_cells)))) {
        char buf[320];
        snprintf(buf, sizeof(buf),
                 "the delay-table search's maps [%d rounds][%zu stacks][%d cells] (%.1f MB as %zu planes) and the cell tracks' steps (%.1f MB) "
                 "and sums [%zu][%zu tracks] (%.1f MB) do not fit in device memory: %s",
                 run.K, n_sets, (int)g.n_cells, 8.0 * (double)map_planes * (double)run.plane() / 1e6, map_planes,
                 run.L > 1 ? 2.0 * (double)run.plane() / 1e6 : 0.0, t_planes, n_tracks, 8.0 * (double)t_planes * (double)n_tracks * g.n_cells / 1e6,
                 ctx->last_error.c_str());
        return fail(ctx, TDOA_ERR_NOMEM, buf);
    }
    if ((rc = ensure(ctx, ctx->locate_part, sizeof(ClosureCand) * n_sets * g.tiles))) return rc;
    if ((rc = ensure(ctx, ctx->locate_best, sizeof(int32_t) * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->locate_out, sizeof(LocateOut) * (run.L ? 1 : K) * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->locate_lags, sizeof(int32_t) * K * sp))) return rc;
    if ((rc = ensure(ctx, ctx->locate_corr, sizeof(double) * K * sp))) return rc;
    if ((run.K > 1 || run.pairs) && (rc = ensure(ctx, ctx->locate_centres, sizeof(LocateCentres) * sp))) return rc;
    if (!run.L) return ensure_map_stats(ctx, locate_run_judged(run));
    if ((rc = ensure(ctx, ctx->ctrack_roots, sizeof(double) * n_tracks))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_out, sizeof(CellTrackOut) * K * n_tracks))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_cells, sizeof(int32_t) * K * n_sets))) return rc;
    if ((rc = ensure(ctx, ctx->ctrack_own, sizeof(long long) * K * n_sets))) return rc;
    if (run.pairs && (rc = ensure(ctx, ctx->ctrack_pairs, 2 * sizeof(int32_t) * K * n_sets))) return rc;
    return ensure_map_stats(ctx, std::max(n_sets, locate_run_judged(run)));
}

// ---- the launches' pieces -----------------------------------------------------------------------------------------------------
// The clock differences a run adds to its pairs' delays, [set][pair], and U x them for a run on upsampled surfaces; no buffers:
// no clocks.  The family's one place that picks them: the context's clock table (tdoa_locate_set_clock) for every call but the
// ones that make their stacks' clocks themselves (sync_locate_api.inc).  Buffers, not pointers: a reserve between bind and launch
// may move them.
struct LocateClocks {
    const DevBuf *diff = nullptr, *diff_up = nullptr;
    bool any() const { return diff != nullptr; }
    const long long *get(bool up) const { return diff ? (up ? diff_up : diff)->as<const long long>() : nullptr; }
};
LocateClocks locate_ctx_clocks(const tdoa_ctx *ctx)
{
    return ctx->clock_stacks ? LocateClocks{&ctx->locate_clock, &ctx->locate_clock_up} : LocateClocks{};
}

// what every launch of a run takes
struct LocateDev {
    hipStream_t st;
    const long long *Q;                      // [n_sets][P][n]: the call's words, with U > 1 the upsampled ones
    const double *roots, *track_roots;       // sqrt(N_w) per stack and per track
    const int32_t *table;
    const long long *cdiff;                  // the clock table's differences, nullptr without one
    ClosureCand *part;
    int32_t *best;
    LocateCentres *centres;
    signed char *D;
};

// The scores' kernel for a station count and the clock flag: the family's one station-count table.  `launch` is called with
// std::integral_constant<int, S_T> -- the stations kept in registers up to reg_stations, 0: the re-reading form -- and
// std::bool_constant<CLK>.
template <class Launch> void locate_scores_dispatch(int S, int reg_stations, bool clocked, Launch &&launch)
{
    switch (S <= reg_stations ? S : 0) {
#define TDOA_LOCATE_CASE(s)                                                                                                      \
    case s:                                                                                                                      \
        if (clocked)                                                                                                             \
            launch(std::integral_constant<int, s>{}, std::true_type{});                                                          \
        else                                                                                                                     \
            launch(std::integral_constant<int, s>{}, std::false_type{});                                                         \
        break;
    TDOA_LOCATE_CASE(2) TDOA_LOCATE_CASE(3) TDOA_LOCATE_CASE(4) TDOA_LOCATE_CASE(5) TDOA_LOCATE_CASE(6) TDOA_LOCATE_CASE(7)
    TDOA_LOCATE_CASE(8) TDOA_LOCATE_CASE(9) TDOA_LOCATE_CASE(10) TDOA_LOCATE_CASE(11) TDOA_LOCATE_CASE(12) TDOA_LOCATE_CASE(13)
    TDOA_LOCATE_CASE(14) TDOA_LOCATE_CASE(15) TDOA_LOCATE_CASE(16)
    default:
        TDOA_LOCATE_CASE(0)
    }
#undef TDOA_LOCATE_CASE
}

// rows [n_rows][n] -> [n_rows][(n - 1) U + 1], U in {2, 4, 8, 16}: the one place the upsampler is launched (n_rows x tiles fits
// the grid: check_locate_upsample, tdoa_debug_upsample_q)
void launch_stack_upsample(hipStream_t st, const long long *Q, size_t n_rows, int n, int U, long long *out)
{
    const int tiles = (n + kUpsampleThreads - 1) / kUpsampleThreads;
    const dim3 grid((unsigned)(n_rows * (size_t)tiles)), block(kUpsampleThreads);
    switch (U) {
    case 2: hipLaunchKernelGGL(k_stack_upsample<2>, grid, block, 0, st, Q, n, tiles, out); break;
    case 4: hipLaunchKernelGGL(k_stack_upsample<4>, grid, block, 0, st, Q, n, tiles, out); break;
    case 8: hipLaunchKernelGGL(k_stack_upsample<8>, grid, block, 0, st, Q, n, tiles, out); break;
    case 16: hipLaunchKernelGGL(k_stack_upsample<16>, grid, block, 0, st, Q, n, tiles, out); break;
    }
}

// the rounds' mask as the kernels take it: a guard of the range's length already excludes every lag of the range
LocateMask locate_mask(int round, int guard, const LocateGeom &g) { return LocateMask{round, std::min(guard, g.n)}; }

// round r's scores into its map and the tiles' candidates: unmasked in round 0, on the lags the earlier rounds left otherwise
void launch_locate_scores(const LocateDev &d, const LocateRun &run, int r, long long *map)
{
    const LocateGeom &g = run.g;
    const dim3 grid((unsigned)g.tiles, (unsigned)run.n_sets), block(kLocateThreads);
    if (r == 0) {
        locate_scores_dispatch(g.S, kLocateRegStations, d.cdiff != nullptr, [&](auto s, auto clk) {
            hipLaunchKernelGGL((k_locate_scores<decltype(s)::value, decltype(clk)::value>), grid, block, 0, d.st, d.Q, g, d.table, d.cdiff, map, d.part);
        });
        return;
    }
    const LocateMask mk = locate_mask(r, run.guard, g);
    locate_scores_dispatch(g.S, kLocateMaskedRegStations, d.cdiff != nullptr, [&](auto s, auto clk) {
        if constexpr (decltype(s)::value <= kLocateMaskedRegStations)      // (the table's last case is the unmasked kernel's alone)
            hipLaunchKernelGGL((k_locate_scores_masked<decltype(s)::value, decltype(clk)::value>), grid, block, 0, d.st, d.Q, g, d.table, d.cdiff,
                               static_cast<const LocateCentres *>(d.centres), mk, map, d.part);
    });
}

// the search's end of round r on its map: the best cell and its record (pass 0, in a later round with the mask's test and the
// round's centres), the runner-up's candidates, the record's runner-up (pass 1)
void launch_locate_finish(const LocateDev &d, const LocateRun &run, int r, const long long *map, const LocateRound &p)
{
    const LocateGeom &g = run.g;
    const dim3 grid((unsigned)g.tiles, (unsigned)run.n_sets), one((unsigned)run.n_sets), block(kLocateThreads);
    const ClosureCand *part = d.part;
    if (r == 0)
        hipLaunchKernelGGL(k_locate_finish, one, block, 0, d.st, d.Q, g, d.table, d.cdiff, d.roots, part, 0, d.best, p.out, p.lags, p.corr);
    else
        hipLaunchKernelGGL(k_locate_finish_masked, one, block, 0, d.st, d.Q, g, d.table, d.cdiff, d.roots, part, locate_mask(r, run.guard, g),
                           d.centres, d.best, p.out, p.lags, p.corr);
    hipLaunchKernelGGL(k_locate_runner, grid, block, 0, d.st, map, g, static_cast<const int32_t *>(d.best), d.part);
    hipLaunchKernelGGL(k_locate_finish, one, block, 0, d.st, d.Q, g, d.table, d.cdiff, d.roots, part, 1, d.best, p.out, p.lags, p.corr);
}

// the recurrence over the L stacks of every track, from the round's maps down to T_0 in t0: position L - 1 is the last stack's
// map as it stands; an even position writes t0, an odd one `other`, and each reads what the position above wrote.  (A track
// of one stack has no steps: its T_0 is its map.)
void launch_cell_track_steps(const LocateDev &d, const CellTrackGeom &g, unsigned n_tracks, const long long *map, long long *t0, long long *other)
{
    const int rows = (int)(((long long)g.n_cells + g.n_cols - 1) / g.n_cols);
    const dim3 tiles((unsigned)g.tiles_x * (unsigned)((rows + kCellTrackH - 1) / kCellTrackH), n_tracks);
    for (int j = g.L - 2; j >= 0; j--) {
        const long long *t_in = j == g.L - 2 ? map + (size_t)(g.L - 1) * g.n_cells : ((j + 1) & 1) ? other : t0;
        const size_t in_stride = j == g.L - 2 ? (size_t)g.L * g.n_cells : (size_t)g.n_cells;
        hipLaunchKernelGGL(k_cell_track_step, tiles, dim3(kCellTrackThreads), cell_track_lds_bytes(g.J), d.st, t_in, in_stride, map, g, j,
                           (j & 1) ? other : t0, d.D);
    }
}

// the tracks' end of round r on T_0: the tiles' candidates, the best track walked back through D and its record (pass 0, in a
// later round with the mask's test, the counts and the round's centres), the runner-up's candidates, the record's runner-up
void launch_cell_track_finish(const LocateDev &d, const LocateRun &run, const CellTrackGeom &g, int r, const long long *map, const long long *t0,
                              const LocateRound &p)
{
    const unsigned n_tracks = (unsigned)run.n_tracks();
    const dim3 grid((unsigned)run.g.tiles, n_tracks), one(n_tracks), block(kCellTrackThreads);
    const signed char *D = d.D;
    const ClosureCand *part = d.part;
    hipLaunchKernelGGL(k_cell_track_best, grid, block, 0, d.st, t0, g.n_cells, d.part);
    if (r == 0)
        hipLaunchKernelGGL(k_cell_track_finish, one, block, 0, d.st, d.Q, run.g, g, d.table, d.cdiff, d.roots, d.track_roots, map, D, part, 0, d.best,
                           p.track, p.cells, p.own, p.lags, p.corr);
    else
        hipLaunchKernelGGL(k_cell_track_finish_masked, one, block, 0, d.st, d.Q, run.g, g, d.table, d.cdiff, d.roots, d.track_roots, map, D, part,
                           locate_mask(r, run.guard, run.g), d.centres, d.best, p.track, p.cells, p.own, p.pairs, p.lags, p.corr);
    hipLaunchKernelGGL(k_locate_runner, grid, dim3(kLocateThreads), 0, d.st, t0, run.g, static_cast<const int32_t *>(d.best), d.part);
    hipLaunchKernelGGL(k_cell_track_finish, one, block, 0, d.st, d.Q, run.g, g, d.table, d.cdiff, d.roots, d.track_roots, map, D, part, 1, d.best,
                       p.track, p.cells, p.own, p.lags, p.corr);
}

CellTrackGeom cell_track_geom(const LocateGeom &lg, int L, int J)
{
    CellTrackGeom g;
    g.n_cells = lg.n_cells;
    g.n_cols = lg.n_cols;
    g.tiles_x = (std::min(lg.n_cols, lg.n_cells) + kCellTrackW - 1) / kCellTrackW;     // (a row holds at most n_cells cells)
    g.L = L;
    g.J = J;
    return g;
}

// Q [n_sets][P][n] -> the run's records, maps or T_0, cells, own scores, counts, lags and correlations, and the statistics of
// the planes it judges: the one place the family is launched.  Round 0 unmasked, the centres its cells give where a later round
// or the counts need them, rounds 1 .. K - 1 on masked lags, the statistics.  A round is the scores, then the search's end
// (every round of a search; with tracks round 0 only, whose best cells the search's records keep on the device), then with
// tracks the recurrence and the tracks' end.  With a clock table (its shape checked by the caller: n_sets stacks of g.S
// stations) the scores' clock instantiation runs and the finishes add the same differences.  With tracks their roots are in
// ctx->ctrack_roots (LocateSearch::refresh).  With U > 1 the run starts with the upsampler, and every launch behind it takes
// its output, the scaled table and the scaled clock differences: Q is [n_sets][P][n_in] then.  clocks: the run's clock
// differences (LocateSearch::bind).  Kernel launches only (the step graph captures them).
void launch_locate_run(tdoa_ctx *ctx, const long long *Q, const double *roots, const LocateRun &run, const LocateClocks &clocks)
{
    const LocateGeom &g = run.g;
    const int32_t *table = ctx->locate_table.as<const int32_t>();
    const long long *cdiff = clocks.get(run.U > 1);
    if (run.U > 1) {
        table = ctx->locate_table_up.as<const int32_t>();
        launch_stack_upsample(ctx->stream, Q, (size_t)run.n_sets * g.P, run.n_in, run.U, ctx->locate_qu.as<long long>());
        Q = ctx->locate_qu.as<const long long>();
    }
    const LocateDev d{ctx->stream, Q, roots, ctx->ctrack_roots.as<const double>(), table, cdiff, ctx->locate_part.as<ClosureCand>(),
                      ctx->locate_best.as<int32_t>(), ctx->locate_centres.as<LocateCentres>(), ctx->ctrack_d.as<signed char>()};
    const CellTrackGeom tg = cell_track_geom(g, run.L, run.J);
    const unsigned n_tracks = (unsigned)run.n_tracks();
    for (int r = 0; r < run.K; r++) {
        const LocateRound p = locate_run_round(ctx, run, r);
        long long *map = locate_run_map(ctx, run, r), *t0 = locate_run_total(ctx, run, r);
        launch_locate_scores(d, run, r, map);
        if (!run.L || r == 0) launch_locate_finish(d, run, r, map, p);
        if (run.L) {
            launch_cell_track_steps(d, tg, n_tracks, map, t0, locate_run_other(ctx, run));
            launch_cell_track_finish(d, run, tg, r, map, t0, p);
        }
        if (r > 0) continue;
        const dim3 sets((unsigned)run.n_sets), block(kLocateThreads);
        if (run.pairs)
            hipLaunchKernelGGL(k_track_centres, sets, block, 0, d.st, g, run.L, d.table, d.cdiff, static_cast<const int32_t *>(d.best),
                               static_cast<const int32_t *>(p.cells), d.centres, p.pairs);
        else if (run.K > 1 && !run.L)
            hipLaunchKernelGGL(k_locate_centres, sets, block, 0, d.st, g, d.table, d.cdiff, static_cast<const int32_t *>(d.best), d.centres);
    }
    // the statistics of the judged planes, in the records' order.  They lie one behind the other, but for T_0 of L > 1: round 0's
    // and then the K - 1 others' (none with K = 1), which lie behind the ping-pong's other half
    const size_t cells = (size_t)g.n_cells;
    const int n = run.L ? (int)n_tracks : run.n_sets;
    const void *rec = run.L ? ctx->ctrack_out.p : ctx->locate_out.p;
    const double *scale = run.L ? d.track_roots : roots;
    if (run.L <= 1) {
        launch_map_stats(ctx, locate_run_total(ctx, run, 0), cells, run.K * n, g, rec, scale, n);
    } else {
        launch_map_stats(ctx, locate_run_total(ctx, run, 0), cells, n, g, rec, scale, n);
        launch_map_stats(ctx, locate_run_total(ctx, run, 1), cells, (run.K - 1) * n, g, ctx->ctrack_out.as<CellTrackOut>() + n, scale, n, n);
    }
}

// the outputs to the host (all but the records may be NULL): the K planes lie one behind the other, but for T_0 of L > 1,
// which comes round by round; asynchronous on ctx->stream
int download_locate_run(tdoa_ctx *ctx, const LocateRun &run, const LocateCall &o)
{
    hipStream_t st = ctx->stream;
    const size_t K = run.K, n_sets = run.n_sets, n_tracks = run.n_tracks(), sp = n_sets * run.g.P, t_plane = n_tracks * run.g.n_cells;
    if (!run.L) {
        HIPCHK(ctx, hipMemcpyAsync(o.loc, ctx->locate_out.p, sizeof(LocateOut) * K * n_sets, hipMemcpyDeviceToHost, st));
    } else {
        HIPCHK(ctx, hipMemcpyAsync(o.track, ctx->ctrack_out.p, sizeof(CellTrackOut) * K * n_tracks, hipMemcpyDeviceToHost, st));
        if (o.cells) HIPCHK(ctx, hipMemcpyAsync(o.cells, ctx->ctrack_cells.p, sizeof(int32_t) * K * n_sets, hipMemcpyDeviceToHost, st));
        if (o.own) HIPCHK(ctx, hipMemcpyAsync(o.own, ctx->ctrack_own.p, sizeof(int64_t) * K * n_sets, hipMemcpyDeviceToHost, st));
        if (o.pairs && run.pairs)
            HIPCHK(ctx, hipMemcpyAsync(o.pairs, ctx->ctrack_pairs.p, 2 * sizeof(int32_t) * K * n_sets, hipMemcpyDeviceToHost, st));
    }
    if (o.lags) HIPCHK(ctx, hipMemcpyAsync(o.lags, ctx->locate_lags.p, sizeof(int32_t) * K * sp, hipMemcpyDeviceToHost, st));
    if (o.corr) HIPCHK(ctx, hipMemcpyAsync(o.corr, ctx->locate_corr.p, sizeof(double) * K * sp, hipMemcpyDeviceToHost, st));
    if (!run.L && o.map) HIPCHK(ctx, hipMemcpyAsync(o.map, ctx->locate_map.p, sizeof(int64_t) * K * run.plane(), hipMemcpyDeviceToHost, st));
    for (int r = 0; run.L && o.total && r < run.K; r++)
        HIPCHK(ctx, hipMemcpyAsync(o.total + (size_t)r * t_plane, locate_run_total(ctx, run, r), sizeof(int64_t) * t_plane, hipMemcpyDeviceToHost, st));
    return download_map_stats(ctx, locate_run_judged(run));
}

// ---- the family as a search on the stacks' sums (stack_search.inc) ----------------------------------------------------------------
struct LocateSearch : StackSearch {
    LocateCall call;                         // the entry's arguments and outputs
    LocateRun run{};                         // bind: the call on the shape's sets; a context's own tracks span a block
    bool own_clocks = false;                 // the run's clocks are its holder's (set before the checks and bind), not the context's table
    LocateClocks clocks;                     // bind: the context's clock table, if any; with own_clocks its holder's buffers
    bool clocked = false;                    // ... whether the run has clocks (another kernel; the clocks are data)
    uint64_t stats = 0;                      // ... and the map statistics' word (map_stats_key: more kernels; the ranks are data), 0: off
    std::vector<double> track_roots;         // sqrt(N_w) per track

    explicit LocateSearch(const LocateCall &c) : StackSearch("the delay-table search with TDOA_LAGS_GO", nullptr), call(c) {}
    const char *check_args() const override { return check_locate_call(call); }
    int check_state(const tdoa_ctx *ctx, int windows_per_stack, const char **what) const override
    {
        return check_locate_state(ctx, windows_per_stack, call.tracks, what, !own_clocks);
    }
    int check_sets(const tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, const char **what) const override
    {
        return check_locate_sets(ctx, call.tracks, q, n_sets, track_len, n_stations, n_w, what, !own_clocks);
    }
    void bind(const tdoa_ctx *ctx, const SearchShape &sh) override
    {
        run = locate_run(ctx, call, sh.n_sets, sh.L);
        if (!own_clocks) clocks = locate_ctx_clocks(ctx);
        clocked = clocks.any();
        stats = map_stats_key(ctx);
        track_roots.assign(run.n_tracks(), std::sqrt(sh.track_w));
    }
    // the rounds and the mask, the tracks' length (0: none) and step, whether the counts are produced (the centres are data), the
    // table's shape (the table itself is data), the clock flag, the upsampling factor (more kernels, another geometry), the statistics
    void key(std::vector<uint64_t> *key, int m) const override
    {
        key->insert(key->end(), {StepProduct::Locate, (uint64_t)m, (uint64_t)run.L | ((uint64_t)run.pairs << 32), (uint64_t)call.J, (uint64_t)call.K,
                                 (uint64_t)call.guard, (uint64_t)call.sep, (uint64_t)run.g.n_cells | ((uint64_t)run.g.n_cols << 32),
                                 (uint64_t)clocked | ((uint64_t)(run.U - 1) << 8), stats});
    }
    int reserve(tdoa_ctx *ctx) const override { return ensure_locate_run(ctx, run); }
    // the tracks' roots (every call: the three routes write their own there)
    int refresh(tdoa_ctx *ctx) const override
    {
        if (call.tracks)
            HIPCHK(ctx, hipMemcpyAsync(ctx->ctrack_roots.p, track_roots.data(), sizeof(double) * track_roots.size(), hipMemcpyHostToDevice, ctx->stream));
        return TDOA_OK;
    }
    void launch(tdoa_ctx *ctx, const long long *Q, const double *roots) const override { launch_locate_run(ctx, Q, roots, run, clocks); }
    int download(tdoa_ctx *ctx) const override { return download_locate_run(ctx, run, call); }
};

}  // namespace

extern "C" {

// ---- a context's own call ---------------------------------------------------------------------------------------------------------
int tdoa_process_locate(tdoa_ctx *ctx, int windows_per_stack, int min_separation, tdoa_location *loc_host, int32_t *lags_host,
                        double *corr_host, int64_t *map_host)
{
    LocateSearch s(locate_search_call(false, 1, 0, min_separation, loc_host, lags_host, corr_host, map_host));
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_process_locate_track(tdoa_ctx *ctx, int windows_per_stack, int max_step, int min_separation, tdoa_cell_track *track_host,
                              int32_t *cells_host, int64_t *own_host, int32_t *lags_host, double *corr_host, int64_t *total_host)
{
    LocateSearch s(locate_track_call(false, max_step, 1, 0, min_separation, track_host, cells_host, own_host, nullptr, lags_host, corr_host, total_host));
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_process_locate_multi(tdoa_ctx *ctx, int windows_per_stack, int n_emitters, int guard, int min_separation, tdoa_location *loc_host,
                              int32_t *lags_host, double *corr_host, int64_t *map_host)
{
    LocateSearch s(locate_search_call(true, n_emitters, guard, min_separation, loc_host, lags_host, corr_host, map_host));
    return process_search(ctx, windows_per_stack, s);
}

int tdoa_process_locate_track_multi(tdoa_ctx *ctx, int windows_per_stack, int max_step, int n_emitters, int guard, int min_separation,
                                    tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host, int32_t *pairs_host,
                                    int32_t *lags_host, double *corr_host, int64_t *total_host)
{
    LocateSearch s(locate_track_call(true, max_step, n_emitters, guard, min_separation, track_host, cells_host, own_host, pairs_host, lags_host,
                                     corr_host, total_host));
    return process_search(ctx, windows_per_stack, s);
}

// ---- over a group's members: member 0's table, clocks and settings are the ones a group of several searches with -------------------
int tdoa_group_process_locate(tdoa_group *g, int windows_per_stack, int min_separation, tdoa_location *loc_host, int32_t *lags_host,
                              double *corr_host, int64_t *map_host)
{
    LocateSearch s(locate_search_call(false, 1, 0, min_separation, loc_host, lags_host, corr_host, map_host));
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_group_process_locate_track(tdoa_group *g, int windows_per_stack, int max_step, int min_separation, tdoa_cell_track *track_host,
                                    int32_t *cells_host, int64_t *own_host, int32_t *lags_host, double *corr_host, int64_t *total_host)
{
    LocateSearch s(locate_track_call(false, max_step, 1, 0, min_separation, track_host, cells_host, own_host, nullptr, lags_host, corr_host, total_host));
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_group_process_locate_multi(tdoa_group *g, int windows_per_stack, int n_emitters, int guard, int min_separation,
                                    tdoa_location *loc_host, int32_t *lags_host, double *corr_host, int64_t *map_host)
{
    LocateSearch s(locate_search_call(true, n_emitters, guard, min_separation, loc_host, lags_host, corr_host, map_host));
    return group_process_search(g, windows_per_stack, s);
}

int tdoa_group_process_locate_track_multi(tdoa_group *g, int windows_per_stack, int max_step, int n_emitters, int guard, int min_separation,
                                          tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host, int32_t *pairs_host,
                                          int32_t *lags_host, double *corr_host, int64_t *total_host)
{
    LocateSearch s(locate_track_call(true, max_step, n_emitters, guard, min_separation, track_host, cells_host, own_host, pairs_host, lags_host,
                                     corr_host, total_host));
    return group_process_search(g, windows_per_stack, s);
}

// ---- on the caller's words, against the context's table and clocks; the outputs are [round] planes -----------------------------------
int tdoa_debug_locate_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int min_separation,
                             tdoa_location *loc, int32_t *lags, double *corr, int64_t *map)
{
    LocateSearch s(locate_search_call(false, 1, 0, min_separation, loc, lags, corr, map));
    return debug_search_from_q(ctx, q, n_sets, 0, n_stations, n_w, s);
}

int tdoa_debug_locate_multi_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int n_emitters, int guard,
                                   int min_separation, tdoa_location *loc, int32_t *lags, double *corr, int64_t *map)
{
    LocateSearch s(locate_search_call(true, n_emitters, guard, min_separation, loc, lags, corr, map));
    return debug_search_from_q(ctx, q, n_sets, 0, n_stations, n_w, s);
}

int tdoa_debug_locate_track_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int max_step,
                                   int min_separation, tdoa_cell_track *track, int32_t *cells, int64_t *own, int32_t *lags,
                                   double *corr, int64_t *total)
{
    LocateSearch s(locate_track_call(false, max_step, 1, 0, min_separation, track, cells, own, nullptr, lags, corr, total));
    return debug_search_from_q(ctx, q, n_sets, track_len, n_stations, n_w, s);
}

int tdoa_debug_locate_track_multi_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int max_step,
                                         int n_emitters, int guard, int min_separation, tdoa_cell_track *track, int32_t *cells,
                                         int64_t *own, int32_t *pairs, int32_t *lags, double *corr, int64_t *total)
{
    LocateSearch s(locate_track_call(true, max_step, n_emitters, guard, min_separation, track, cells, own, pairs, lags, corr, total));
    return debug_search_from_q(ctx, q, n_sets, track_len, n_stations, n_w, s);
}

// The upsampler (stack_upsample.hpp) on the caller's words: n_rows rows of 2 max_lag - 1 int64 -> n_rows rows of
// (2 max_lag - 2) U + 1.  Needs the context for max_lag and the device only; the setting of the context is not read.
int tdoa_debug_upsample_q(tdoa_ctx *ctx, const int64_t *q, int n_rows, int U, int64_t *out)
{
    int rc;
    if (!ctx) return TDOA_ERR_INVALID;
    if (!q || !out || n_rows < 1 || !upsample_factor_ok(U)) return fail(ctx, TDOA_ERR_INVALID, "q or out is NULL, n_rows < 1 or U is not one of 1, 2, 4, 8, 16");
    const long long n = 2ll * ctx->prm.max_lag - 1, n_u = upsample_len(n, U), tiles = (n + kUpsampleThreads - 1) / kUpsampleThreads;
    if (n_u > INT_MAX || (double)n_rows * (double)tiles > (double)INT_MAX) return fail(ctx, TDOA_ERR_UNSUPPORTED, "the upsampled rows do not fit the grid");
    if (U == 1) {
        std::memcpy(out, q, sizeof(int64_t) * (size_t)n_rows * (size_t)n);
        return TDOA_OK;
    }
    if ((rc = check_ctx(ctx))) return rc;
    if ((rc = ensure(ctx, ctx->debug_q, sizeof(long long) * (size_t)n_rows * (size_t)n))) return rc;
    if ((rc = ensure(ctx, ctx->locate_qu, sizeof(long long) * (size_t)n_rows * (size_t)n_u))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->debug_q.p, q, sizeof(long long) * (size_t)n_rows * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    launch_stack_upsample(ctx->stream, ctx->debug_q.as<const long long>(), (size_t)n_rows, (int)n, U, ctx->locate_qu.as<long long>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->locate_qu.p, sizeof(long long) * (size_t)n_rows * (size_t)n_u, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TDOA_OK;
}

}  // extern "C"
