// step_graph.inc -- tdoa_process's step: which units a rank runs in which launch groups (StepLayout), and the whole-step
// hipGraph that is captured once and replayed while its key holds.
// Included by tdoa_mi355x.hip after fm_route.inc.

namespace {

// Which (window, pair) units of a step one rank runs, in which launch groups, and the descriptors' indices -- plain
// numbers, no device state.  Window wi of the rank (mine[wi]) owns station-windows [sw_off[wi], sw_off[wi+1]) and likewise
// pw and quads; every slot and pair-window index is relative to the first window of its launch group.
struct StepLayout {
    std::vector<int> mine;                   // owned windows, ascending
    int per_batch = 1;                       // windows per launch group
    std::vector<int> sw_station;             // station of each station-window
    std::vector<PWDesc> pw;                  // len_a is the caller's
    std::vector<QuadDesc> quads;
    std::vector<size_t> sw_off, pw_off, q_off;
};

// The rank of `world` that runs pair p of window wid in a job of W windows and P pairs -- the one statement of the sharding
// rule (SURVEY section 8e) that the step layout, the multi-device group's merge and its file ingest all use.  Window-major:
// rank r owns the windows wid = r (mod world), so a station-window is transformed once and reused by all its pairs.  With
// fewer windows than ranks that would leave ranks idle: then the (window, pair) units u = wid*P + p are dealt
// u = r (mod world) and a rank transforms only the stations its pairs need (station spectra are duplicated across ranks).
// tdoa_amd/sharding.py unit_owner states the same rule.
int unit_owner(int wid, int p, int W, int P, int world)
{
    return W < world ? (int)(((long long)wid * P + p) % world) : wid % world;
}

// max_per_batch: the caller's bound (tdoa_params.windows_per_batch, workspace).  TDOA_ERR_UNSUPPORTED: a window's station
// or pair count alone exceeds the grid limit.
int build_step_layout(int S, int W, int rank, int world, int max_per_batch, QuadCache &quad_cache, StepLayout *out)
{
    const int P = S * (S - 1) / 2;
    StepLayout &L = *out;
    L = StepLayout{};
    auto owns = [&](int wid, int p) { return unit_owner(wid, p, W, P, world) == rank; };
    for (int w = 0; w < W; w++) {
        bool any = false;
        for (int p = 0; p < P && !any; p++) any = owns(w, p);
        if (any) L.mine.push_back(w);
    }
    // default: every window of this rank in one launch group (launch tails cost more than cache residency gains)
    L.per_batch = std::min(max_per_batch, (int)std::max<size_t>(L.mine.size(), 1));
    // per_batch * S and per_batch * P become gridDim.y of the FFT kernels (HIP limit 65535)
    if (std::max(S, P) > 65535) return TDOA_ERR_UNSUPPORTED;
    L.per_batch = std::max(1, std::min(L.per_batch, 65535 / std::max(S, P)));
    if (!L.mine.empty()) {                   // groups of equal size (99 windows at most 85 at a time: 50 + 49, not 85 + 14)
        const int groups = ((int)L.mine.size() + L.per_batch - 1) / L.per_batch;
        L.per_batch = ((int)L.mine.size() + groups - 1) / groups;
    }

    const size_t nm = L.mine.size(), pb = (size_t)L.per_batch;
    L.sw_off.assign(nm + 1, 0);
    L.pw_off.assign(nm + 1, 0);
    L.q_off.assign(nm + 1, 0);
    for (size_t wi = 0; wi < nm; wi++) {
        const int wid = L.mine[wi];
        const size_t batch_base = L.sw_off[wi - wi % pb];
        std::vector<int> slot(S, -1), owned;
        std::vector<std::pair<int, int>> st_pairs;
        int p = 0;
        for (int i = 0; i < S; i++)
            for (int j = i + 1; j < S; j++, p++) {
                if (!owns(wid, p)) continue;
                for (int s : {i, j})
                    if (slot[s] < 0) {
                        slot[s] = (int)(L.sw_station.size() - batch_base);
                        L.sw_station.push_back(s);
                    }
                L.pw.push_back(PWDesc{slot[i], slot[j], wid * P + p, 0});
                owned.push_back(p);
                st_pairs.emplace_back(i, j);
            }
        L.sw_off[wi + 1] = L.sw_station.size();
        L.pw_off[wi + 1] = L.pw.size();
        // segment form: the quad cover of this window's pairs (the same for every window under window-major sharding).
        // Every pair-window of the rank is in exactly one quad; run_fm_batch takes the quads of a batch or none of them.
        // (the greedy cover costs O(P S^2) per quad: beyond kMaxQuadStations stations the segment form stays pair by pair)
        if (!owned.empty() && S <= kMaxQuadStations) {
            auto it = quad_cache.find(owned);
            if (it == quad_cache.end()) it = quad_cache.emplace(owned, build_segment_quads(S, st_pairs)).first;
            const int pw_base = (int)(L.pw_off[wi] - L.pw_off[wi - wi % pb]);
            for (const StationQuad &q : it->second) {
                QuadDesc d{slot[q.a], q.b >= 0 ? slot[q.b] : -1, slot[q.c], q.d >= 0 ? slot[q.d] : -1, {-1, -1, -1, -1}};
                for (int o = 0; o < 4; o++)
                    if (q.pair[o] >= 0) d.pw[o] = pw_base + q.pair[o];
                L.quads.push_back(d);
            }
        }
        L.q_off[wi + 1] = L.quads.size();
    }
    return TDOA_OK;
}

// Upper bound on windows per launch group: tdoa_params.windows_per_batch, and a third of the device's memory for the
// workspace (96 GB of an MI355X's 288: cfg4's 99 windows x 36 spectra are one group of 30 GB; round 3 stopped at 24 GiB and
// ran them as 85 + 14).  one_window: the launch group of one window as run_fm_batch sees it.
// (ADVICE r05 asks to evaluate this once per shape and to count every buffer in `held`: a change of grouping, its own PR)
int batch_bound(tdoa_ctx *ctx, const FftPlan &pl, int lag_lo, int lag_hi, const FmBatchShape &one_window)
{
    // what reserve_fm_batch asks for per window (+ 1/8: ensure() rounds every buffer up): TZ, the V workspace in the form this
    // plan's pair step uses, code rows where K1 is materialised
    const FmBytes by = plan_fm_batch(ctx->knobs, ctx->stg, ctx->n_cu, pl, lag_lo, lag_hi, one_window).bytes;
    const double bytes_per_window = 1.125 * ((double)by.tz + (double)by.v + (double)by.codes + (double)by.codes_lp);
    // the bound: a third of the device (tdoa_create), and not more than is FREE now plus what this context already holds of it
    // (captures attached by the caller, other contexts, other ranks on the same card all count against the device)
    double limit = ctx->workspace_limit;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        // (the surface outputs' buffers too: whether an earlier call allocated them must not change the grouping)
        const double held = (double)ctx->tz.cap + (double)ctx->v.cap + (double)ctx->codes.cap + (double)ctx->codes_lp.cap +
                            (double)ctx->surf.cap + (double)ctx->surf_out.cap + (double)ctx->stack_q.cap + (double)ctx->stack_surf.cap +
                            (double)ctx->drift_keys.cap + (double)ctx->drift_prof.cap + (double)ctx->track_t.cap + (double)ctx->track_d.cap +
                            (double)ctx->locate_table.cap + (double)ctx->locate_map.cap + (double)ctx->ctrack_d.cap + (double)ctx->ctrack_t.cap +
                            (double)ctx->mstat_hist.cap;
        limit = std::min(limit, std::max(0.0, (double)free_b + held - 1073741824.0));      // 1 GiB stays free: descriptors, edges, the runtime
    } else {
        (void)hipGetLastError();
    }
    const int asked = ctx->prm.windows_per_batch > 0 ? ctx->prm.windows_per_batch : INT_MAX;
    return (int)std::max(1.0, std::min<double>(asked, limit / bytes_per_window));
}

// Everything a step's launches depend on: same key => the captured graph can be replayed as is
// (the step's product appends its own words: step_products.inc, key_*)
std::vector<uint64_t> step_graph_key(const tdoa_ctx *ctx, int rank, int world, int per_batch, long long wlen, long long block,
                                     bool go, bool fine, double gate)
{
    std::vector<uint64_t> key = {(uint64_t)ctx->caps.size(), (uint64_t)rank, (uint64_t)world, (uint64_t)per_batch, (uint64_t)wlen,
                                 (uint64_t)ctx->prm.max_lag | ((uint64_t)ctx->prm.k1_smooth << 32) | ((uint64_t)(ctx->prm.k1_gate != 0) << 62) |
                                     ((uint64_t)go << 61), (uint64_t)block,
                                 ctx->alloc_gen, (uint64_t)fine, 0};
    std::memcpy(&key.back(), &gate, sizeof(double));
    for (const KnobVar &kv : kKnobVars) key.push_back(kv.flag ? (uint64_t)(ctx->knobs.*kv.flag) : (uint64_t)(ctx->knobs.*kv.num));
    for (auto &c : ctx->caps) {
        key.push_back((uint64_t)(uintptr_t)c.dev);
        key.push_back((uint64_t)c.n);
    }
    key.push_back(ctx->graph_prof ? 0x100000000ull | ctx->prof_mask : 0ull);      // an instrumented step is a different graph
    return key;
}

bool step_graph_on(const tdoa_ctx *ctx) { return ctx->knobs.use_graph && !ctx->profiling; }

// the step graph captured under `key` is there: run_step_graph will replay it (its descriptors are still on the device)
bool step_graph_replays(const tdoa_ctx *ctx, const std::vector<uint64_t> &key)
{
    return step_graph_on(ctx) && ctx->graph_exec && key == ctx->graph_key;
}

// after -> [record ev] -> after's successors
hipError_t splice_event_record(hipGraph_t g, hipGraphNode_t after, hipEvent_t ev)
{
    size_t nd = 0;
    hipError_t r = hipGraphNodeGetDependentNodes(after, nullptr, &nd);
    if (r != hipSuccess) return r;
    std::vector<hipGraphNode_t> succ(nd);
    if (nd && (r = hipGraphNodeGetDependentNodes(after, succ.data(), &nd)) != hipSuccess) return r;
    hipGraphNode_t rec = nullptr;
    for (hipGraphNode_t sn : succ)
        if ((r = hipGraphRemoveDependencies(g, &after, &sn, 1)) != hipSuccess) return r;
    if ((r = hipGraphAddEventRecordNode(&rec, g, &after, 1, ev)) != hipSuccess) return r;
    for (hipGraphNode_t sn : succ)
        if ((r = hipGraphAddDependencies(g, &rec, &sn, 1)) != hipSuccess) return r;
    return hipSuccess;
}

// Enqueues one step on ctx->stream: replays the cached step graph when `key` is its key, else captures enqueue() into a
// new one and launches that, or -- graphs off, or the profiling path -- runs enqueue() directly.
int run_step_graph(tdoa_ctx *ctx, const std::vector<uint64_t> &key, const std::function<int()> &enqueue)
{
    hipStream_t st = ctx->stream;
    if (step_graph_replays(ctx, key)) {
        ctx->once_active = ctx->graph_once;
        std::memcpy(ctx->route, ctx->graph_route, sizeof(ctx->route));
        HIPCHK(ctx, hipGraphLaunch(ctx->graph_exec, st));
        return TDOA_OK;
    }
    if (!step_graph_on(ctx)) return enqueue();
    if (ctx->graph_exec) { (void)hipGraphExecDestroy(ctx->graph_exec); ctx->graph_exec = nullptr; }
    if (ctx->graph) { (void)hipGraphDestroy(ctx->graph); ctx->graph = nullptr; }
    ctx->graph_key.clear();
    HIPCHK(ctx, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    clear_graph_marks(ctx);
    ctx->capturing = true;
    const int rc = enqueue();
    ctx->capturing = false;
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(st, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return fail(ctx, TDOA_ERR_HIP, "hipStreamEndCapture", e);
    ctx->graph = g;
    // the step was captured from ONE stream: it must come out as one dependency chain -- every node but the first has
    // a predecessor (a node without one would replay unordered against the kernels that feed or consume it)
    size_t n_nodes = 0, n_edges = 0, n_roots = 0;
    HIPCHK(ctx, hipGraphGetNodes(g, nullptr, &n_nodes));
    HIPCHK(ctx, hipGraphGetEdges(g, nullptr, nullptr, &n_edges));
    HIPCHK(ctx, hipGraphGetRootNodes(g, nullptr, &n_roots));
    std::vector<hipGraphNode_t> nodes(n_nodes);
    if (n_nodes) HIPCHK(ctx, hipGraphGetNodes(g, nodes.data(), &n_nodes));
    int memsets = 0;
    for (hipGraphNode_t nd : nodes) {
        hipGraphNodeType ty;
        if (hipGraphNodeGetType(nd, &ty) == hipSuccess && ty == hipGraphNodeTypeMemset) memsets++;
    }
    ctx->graph_nodes = (int)n_nodes;
    ctx->graph_edges = (int)n_edges;
    ctx->graph_roots = (int)n_roots;
    ctx->graph_memsets = memsets;
    if (n_nodes && (n_roots != 1 || n_edges + 1 < n_nodes))
        return fail(ctx, TDOA_ERR_STATE, "captured step is not one dependency chain");
    if (memsets && !ctx->knobs.memset_nodes) return fail(ctx, TDOA_ERR_STATE, "captured step holds a memset node");
    // graph-mode profiling: an event-record node before the first and after the last kernel of every marked scope
    for (auto &m : ctx->graph_marks) {
        if (!m.before || !m.last || m.last == m.before) { m.e0 = m.e1 = nullptr; continue; }
        HIPCHK(ctx, hipEventCreate(&m.e0));
        HIPCHK(ctx, hipEventCreate(&m.e1));
        HIPCHK(ctx, splice_event_record(g, m.last, m.e1));       // (the later place first: `before` keeps its successor until then)
        HIPCHK(ctx, splice_event_record(g, m.before, m.e0));
    }
    HIPCHK(ctx, hipGraphInstantiate(&ctx->graph_exec, g, nullptr, nullptr, 0));
    ctx->graph_key = key;
    ctx->graph_once = ctx->once_active;
    std::memcpy(ctx->graph_route, ctx->route, sizeof(ctx->route));
    HIPCHK(ctx, hipGraphLaunch(ctx->graph_exec, st));
    return TDOA_OK;
}

// after the step has synchronised: add the times of the event-record nodes the step graph holds
void collect_step_graph_marks(tdoa_ctx *ctx)
{
    if (!step_graph_on(ctx) || !ctx->graph_prof) return;
    for (auto &m : ctx->graph_marks) {
        float ms = 0;
        if (m.e0 && m.e1 && hipEventElapsedTime(&ms, m.e0, m.e1) == hipSuccess) {
            ctx->prof_ms[m.kernel] += ms;
            ctx->prof_launches[m.kernel] += 1;
            ctx->prof_bytes[m.kernel] += m.bytes;
        }
    }
}

}  // namespace
