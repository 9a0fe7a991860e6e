// debug_api.inc -- the tdoa_debug_* and tdoa_profile_* entry points (tests and measurements).
// Included by tdoa_mi355x.hip after its entries.  The searches' tdoa_debug_*_from_q entries are in the searches' own files
// (debug_search_from_q, stack_search.inc).

extern "C" {

int tdoa_debug_force_generic(tdoa_ctx *ctx, int on)
{
    if (!ctx) return TDOA_ERR_INVALID;
    ctx->knobs.force_generic = on != 0;
    return TDOA_OK;
}

int tdoa_debug_segment_quads(int n_stations, const int32_t *pairs, int n_pairs, int32_t *quads_out, int max_quads)
{
    if (n_stations < 2 || n_stations > kMaxQuadStations || n_pairs < 0 || (n_pairs && !pairs) || max_quads < 0 || (max_quads && !quads_out))
        return -TDOA_ERR_INVALID;
    std::vector<std::pair<int, int>> pr;
    for (int i = 0; i < n_pairs; i++) {
        const int a = pairs[2 * i], c = pairs[2 * i + 1];
        if (a < 0 || c < 0 || a >= n_stations || c >= n_stations || a == c) return -TDOA_ERR_INVALID;
        pr.emplace_back(a, c);
    }
    const std::vector<StationQuad> q = build_segment_quads(n_stations, pr);
    if ((int)q.size() > max_quads) return -TDOA_ERR_INVALID;
    for (size_t i = 0; i < q.size(); i++) {
        int32_t *o = quads_out + 8 * i;
        o[0] = q[i].a; o[1] = q[i].b; o[2] = q[i].c; o[3] = q[i].d;
        for (int k = 0; k < 4; k++) o[4 + k] = q[i].pair[k];
    }
    return (int)q.size();
}

int tdoa_debug_staged_groups(int n_stations, int max_pairs, uint32_t *masks_out, int32_t *counts_out, uint8_t *pairs_out, int max_groups)
{
    if (n_stations < 2 || n_stations > kStgMaxStations || max_pairs < 1 || max_pairs > kStgMaxWaves || max_groups < 0 ||
        (max_groups && (!masks_out || !counts_out || !pairs_out)))
        return -TDOA_ERR_INVALID;
    const std::vector<StgGroup> g = build_stg_groups(n_stations, max_pairs, max_pairs == kStgMaxWaves);      // (16: the folded form's table)
    if ((int)g.size() > max_groups) return -TDOA_ERR_INVALID;
    for (size_t i = 0; i < g.size(); i++) {
        masks_out[i] = g[i].mask;
        counts_out[i] = g[i].n;
        std::memcpy(pairs_out + 16 * i, g[i].pair, 16);
    }
    return (int)g.size();
}

int64_t tdoa_debug_stg_paired_index(int n2, int row, int col)
{
    if ((n2 != 256 && n2 != 512) || row < 0 || row >= n2 || col < 0 || col >= 4096) return -1;
    return (int64_t)tdoa::stg_paired_at(n2, row, col);
}

int tdoa_debug_k1_split_table(uint16_t *hi, uint8_t *lo)
{
    if (!hi || !lo) return TDOA_ERR_INVALID;
    std::vector<int32_t> tab, direct, quad;
    std::vector<uint8_t> split;
    k1_build_table_host(tab, direct, quad, &split);
    std::memcpy(lo, split.data(), kK1DirectEntries);
    std::memcpy(hi, split.data() + kK1DirectEntries, 2 * (size_t)kK1DirectEntries);
    return TDOA_OK;
}

int tdoa_debug_step_layout(int n_stations, int n_windows, int rank, int world, int max_per_batch, int32_t *pw_out, int max_pw,
                           int32_t *quads_out, int32_t *n_quads)
{
    if (n_stations < 2 || n_windows < 1 || world < 1 || rank < 0 || rank >= world || max_per_batch < 1 || max_pw < 0 ||
        (max_pw && (!pw_out || !quads_out)) || !n_quads)
        return -TDOA_ERR_INVALID;
    QuadCache cache;
    StepLayout L;
    if (int rc = build_step_layout(n_stations, n_windows, rank, world, max_per_batch, cache, &L)) return -rc;
    if ((int)L.pw.size() > max_pw) return -TDOA_ERR_INVALID;
    for (size_t wi = 0; wi < L.mine.size(); wi++) {
        const size_t batch = wi / L.per_batch, sw_base = L.sw_off[batch * L.per_batch];
        for (size_t k = L.pw_off[wi]; k < L.pw_off[wi + 1]; k++) {
            const PWDesc &d = L.pw[k];
            const int32_t rec[6] = {d.out_index, (int32_t)batch, d.sw_a, d.sw_b, L.sw_station[sw_base + d.sw_a], L.sw_station[sw_base + d.sw_b]};
            std::memcpy(pw_out + 6 * k, rec, sizeof(rec));
        }
        for (size_t k = L.q_off[wi]; k < L.q_off[wi + 1]; k++) {      // at most one quad per pair-window
            const QuadDesc &q = L.quads[k];
            const int32_t rec[9] = {(int32_t)batch, q.sw_ta, q.sw_tb, q.sw_sc, q.sw_sd, q.pw[0], q.pw[1], q.pw[2], q.pw[3]};
            std::memcpy(quads_out + 9 * k, rec, sizeof(rec));
        }
    }
    *n_quads = (int32_t)L.quads.size();
    return (int)L.pw.size();
}

int tdoa_debug_graph_info(tdoa_ctx *ctx, int32_t info[4], const char *dot_path)
{
    if (!ctx || !info) return TDOA_ERR_INVALID;
    if (!ctx->graph) return fail(ctx, TDOA_ERR_STATE, "no captured step");
    info[0] = ctx->graph_nodes;
    info[1] = ctx->graph_edges;
    info[2] = ctx->graph_roots;
    info[3] = ctx->graph_memsets;
    if (dot_path && dot_path[0]) {
        HIPCHK(ctx, hipGraphDebugDotPrint(ctx->graph, dot_path, hipGraphDebugDotFlagsVerbose));
        // the parameters of the memset nodes (probe builds only), read back from the graph itself: <dot_path>.memsets
        size_t n_nodes = 0;
        HIPCHK(ctx, hipGraphGetNodes(ctx->graph, nullptr, &n_nodes));
        std::vector<hipGraphNode_t> nodes(n_nodes);
        if (n_nodes) HIPCHK(ctx, hipGraphGetNodes(ctx->graph, nodes.data(), &n_nodes));
        const std::string mp = std::string(dot_path) + ".memsets";
        if (FILE *f = std::fopen(mp.c_str(), "w")) {
            for (hipGraphNode_t nd : nodes) {
                hipGraphNodeType ty;
                hipMemsetParams mpz;
                if (hipGraphNodeGetType(nd, &ty) == hipSuccess && ty == hipGraphNodeTypeMemset &&
                    hipGraphMemsetNodeGetParams(nd, &mpz) == hipSuccess)
                    std::fprintf(f, "memset node: dst %p elementSize %u width %zu height %zu pitch %zu value %u\n", mpz.dst,
                                 mpz.elementSize, mpz.width, mpz.height, mpz.pitch, mpz.value);
            }
            std::fclose(f);
        }
    }
    return TDOA_OK;
}

int tdoa_debug_poison_workspace(tdoa_ctx *ctx)
{
    if (!ctx) return TDOA_ERR_INVALID;
    // floats only: no kernel derives an index from a value in these buffers (peak lags come from the keys, which are not
    // poisoned), so a NaN can end up in a result but never in an address.  (stack_q holds integers: the pattern is a large
    // number there, and every element is written before it is read like the floats; so does track_t, the sums of
    // tdoa_process_track -- its steps, track_d, are added to lag indices and stay as they are; the closure search's
    // candidates, cells and records are compared and copied, never added to an address; the delay-table search's map,
    // candidates and records likewise -- a cell taken from a candidate is checked against the table's size -- and its table,
    // which is state, is left alone; the clock-line search's clocks only enter lags that are checked against the range, and a
    // candidate's number taken from its tiles is clamped to the candidates there are; the upsampled surfaces are integers like
    // stack_q, every word written by the upsampler before a search reads it; the zoom locate's window maps, candidates and
    // records are the delay-table search's again, and its fine table is state; the fine clock lines' table and candidates are
    // the clock-line search's again; the zoomed cell tracks' sums, records, cells and own scores are compared and copied -- their
    // centres and steps E, which are added to window positions, stay as they are; the mixed clock rows and their differences
    // only enter lags that are checked against the range, every word written by k_line_mix before the locate stage reads it;
    // the zoomed rounds' counts are copied, and the rounds' records they take their windows' centres from are written by the
    // rounds before them, a cell checked against the table's size)
    for (DevBuf *b : {&ctx->mix_rows, &ctx->mix_cdiff, &ctx->mix_cdiff_up, &ctx->tzoom_total, &ctx->tzoom_out, &ctx->tzoom_cells, &ctx->tzoom_own, &ctx->v, &ctx->tz, &ctx->fine_raw, &ctx->once_edges, &ctx->surf, &ctx->surf_out, &ctx->stack_q, &ctx->stack_surf,
                      &ctx->track_t, &ctx->closure_part, &ctx->closure_best, &ctx->closure_out, &ctx->locate_map, &ctx->locate_part,
                      &ctx->locate_best, &ctx->locate_out, &ctx->locate_lags, &ctx->locate_corr, &ctx->sline_cur, &ctx->sline_part,
                      &ctx->sline_out, &ctx->sline_rows, &ctx->sline_lags, &ctx->sline_corr, &ctx->locate_qu, &ctx->zoom_map, &ctx->zoom_part,
                      &ctx->zoom_out, &ctx->zoom_lags, &ctx->zoom_corr, &ctx->mzoom_pairs, &ctx->slfine_cur, &ctx->slfine_part, &ctx->slfine_out,
                      &ctx->slfine_rows, &ctx->slfine_lags, &ctx->slfine_corr})
        if (b->p && b->cap >= 4) HIPCHK(ctx, hipMemsetD32Async(static_cast<hipDeviceptr_t>(b->p), 0x7FC00000, b->cap / 4, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TDOA_OK;
}

int tdoa_debug_last_route(const tdoa_ctx *ctx, int32_t info[16])
{
    if (!ctx || !info) return TDOA_ERR_INVALID;
    if (!ctx->route_set) return TDOA_ERR_STATE;
    std::memcpy(info, ctx->route, sizeof(ctx->route));
    return TDOA_OK;
}

int tdoa_debug_flags(tdoa_ctx *ctx, unsigned flags)
{
    if (!ctx) return TDOA_ERR_INVALID;
    knobs_from_debug_flags(ctx->knobs, flags);
    return TDOA_OK;
}

int tdoa_debug_last_k1(tdoa_ctx *ctx, int sw_index, tdoa_fm_stats *stats, int32_t *single_look)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (sw_index < 0 || (size_t)(sw_index + 1) * sizeof(FmStats) > ctx->stats.cap) return fail(ctx, TDOA_ERR_INVALID, "no such station-window");
    if (stats) HIPCHK(ctx, hipMemcpy(stats, ctx->stats.as<FmStats>() + sw_index, sizeof(FmStats), hipMemcpyDeviceToHost));
    if (single_look) *single_look = ctx->once_active ? 1 : 0;
    return TDOA_OK;
}

int tdoa_profile_enable(tdoa_ctx *ctx, int on)
{
    if (!ctx) return TDOA_ERR_INVALID;
    ctx->profiling = on == 1;
    ctx->graph_prof = on == 2;
    return TDOA_OK;
}

int tdoa_profile_select(tdoa_ctx *ctx, unsigned int scope_mask)
{
    if (!ctx) return TDOA_ERR_INVALID;
    ctx->prof_mask = scope_mask;
    return TDOA_OK;
}

int tdoa_profile_reset(tdoa_ctx *ctx)
{
    if (!ctx) return TDOA_ERR_INVALID;
    prof_collect(ctx);
    for (int k = 0; k < TDOA_K_COUNT; k++) {
        ctx->prof_ms[k] = 0;
        ctx->prof_launches[k] = 0;
        ctx->prof_bytes[k] = 0;
    }
    return TDOA_OK;
}

int tdoa_profile_get(tdoa_ctx *ctx, int kernel, double *total_ms, int64_t *launches, double *algorithmic_bytes)
{
    if (!ctx || kernel < 0 || kernel >= TDOA_K_COUNT) return TDOA_ERR_INVALID;
    if (total_ms) *total_ms = ctx->prof_ms[kernel];
    if (launches) *launches = ctx->prof_launches[kernel];
    if (algorithmic_bytes) *algorithmic_bytes = ctx->prof_bytes[kernel];
    return TDOA_OK;
}

int tdoa_debug_select_peaks(tdoa_ctx *ctx, const float *surface, int n_lags, int lag_lo, int k, int min_separation,
                            tdoa_peak *peaks, int32_t *count)
{
    int rc;
    if (!ctx) return TDOA_ERR_INVALID;
    if (check_k_sep(k, min_separation) || !peaks || !surface || n_lags < 1 ||
        (long long)lag_lo + n_lags - 1 > INT_MAX / 2 || lag_lo < -(INT_MAX / 2))
        return fail(ctx, TDOA_ERR_INVALID, "bad argument");
    if ((rc = check_ctx(ctx))) return rc;
    if ((rc = ensure(ctx, ctx->lagdump, sizeof(float) * (size_t)n_lags))) return rc;
    if ((rc = ensure(ctx, ctx->scales, sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->sel_peaks, sizeof(PeakOut) * k))) return rc;
    if ((rc = ensure(ctx, ctx->sel_count, sizeof(int32_t)))) return rc;
    const double one = 1.0;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->lagdump.p, surface, sizeof(float) * (size_t)n_lags, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->scales.p, &one, sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_select_peaks, dim3(1), dim3(kSelThreads), 0, st, ctx->lagdump.as<const float>(), (size_t)0,
                       n_lags, lag_lo, static_cast<const PWDesc *>(nullptr), static_cast<const unsigned long long *>(nullptr),
                       ctx->scales.as<const double>(), static_cast<const double *>(nullptr), k, min_separation,
                       ctx->sel_peaks.as<PeakOut>(), ctx->sel_count.as<int32_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(peaks, ctx->sel_peaks.p, sizeof(PeakOut) * k, hipMemcpyDeviceToHost, st));
    if (count) HIPCHK(ctx, hipMemcpyAsync(count, ctx->sel_count.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));       // `one` is a stack object
    return TDOA_OK;
}

#ifdef TDOA_STG_TIMING
// measurement build only: read and clear the staged walk's wave-cycle counters (dec_staged.hpp)
int tdoa_debug_stg_prof(unsigned long long *out8)
{
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(tdoa::g_stg_prof), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long z[8] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(tdoa::g_stg_prof), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"
