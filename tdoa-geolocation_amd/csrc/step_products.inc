// step_products.inc -- what a step (process_impl) can write besides its peak records: the correlation surfaces
// (tdoa_process_lags), the K strongest peaks per pair-window (tdoa_process_peaks), the stacked surfaces of a block's windows
// (tdoa_process_stacked), the same stacks taken along the best of 2H+1 lag slopes (tdoa_process_stacked_drift), the best
// delay track through a stack's windows (tdoa_process_track), one consistent lag set per station triple of a stack
// (tdoa_process_closure), a table of candidate positions scored on all pairs' stacks (tdoa_process_locate).  Every product is four functions next to each other, called by process_impl in this order:
//   reserve_*   its buffers, after the step's grouping is fixed (batch_bound counts them as held, so a later call groups as
//               this one did); no allocation may happen once the step is being captured
//   key_*       the words it appends to the step graph's key: everything its launches depend on
//   (upload_stack, upload_stack_drift, upload_stack_track: the products with descriptors of their own send them with the
//   step's, when the step is not replayed; refresh_closure: data a call may change under the same key, sent every time)
//   enqueue_*   its kernels, after the step's decode -- unscoped launches, kernel nodes only: the step stays one chain
//   download_*  its asynchronous copies out on ctx->stream
// All of them read the K5 kernels' lag arrays in ctx->surf, pair-window i of the rank at i * n_lags.
// Included by tdoa_mi355x.hip after step_graph.inc and stacked_api.inc.

namespace {

// What the stages see of the step (read-only)
struct StepView {
    tdoa_ctx *ctx;
    const StepLayout *lay;
    size_t slots;                            // W x P records of the job
    int n_lags, lag_lo, P, wpb;
    const PWDesc *d_pw;                      // the rank's pair-windows, the slots' keys and scales on the device
    const unsigned long long *d_keys;
    const double *d_scales;
    const double *slot_gain;                 // enqueue_* only: the single-look path's gains, nullptr on every other path

    size_t n_owned() const { return lay->pw.size(); }
    size_t surf_n() const { return (size_t)n_lags * slots; }
};

struct LagsProduct {
    float *lags_host = nullptr;
    void *lags_dev = nullptr;
};
struct PeaksProduct {
    int k = 0, min_sep = 0;
    tdoa_peak *peaks_host = nullptr;         // [slot][k]
    int32_t *count_host = nullptr;           // [slot]
};
struct StackProduct {
    int m = 0;                               // windows per stack, 0: the whole block
    int k = 0, min_sep = 0;
    double gate = 0.0;
    tdoa_peak *peaks_host = nullptr;         // [stack][pair][k]
    int32_t *count_host = nullptr;           // [stack][pair]
    tdoa_fine_peak *fine_host = nullptr;
    float *surface_host = nullptr;
    int64_t *partial_host = nullptr;         // the rank's fixed-point sums Q
    StackLayout layout;                      // filled by reserve_stack
    std::vector<double> ones;                // upload_stack's host copy of the unit scales (lives until the step's upload has synchronised)
    // the finishing kernels run when one of their outputs is asked for (a group member returns its partial sums only)
    bool finish() const { return peaks_host || count_host || fine_host || surface_host; }
};

struct StackDriftProduct {
    StackProduct stack;                      // the stack's own arguments and outputs, computed on Q_{h*}
    int H = 0, D = 1;                        // hypotheses -H .. H, slope h / D lags per window
    int32_t *drift_host = nullptr;           // [stack][pair]: h*
    tdoa_peak *profile_host = nullptr;       // [stack][pair][2H+1]
    int mm = 0, hb = 1;                      // filled by reserve_stack_drift: the stack length, hypotheses per workgroup
    std::vector<int32_t> tab;                // ... and shift(h, j) at [(h + H) * mm + j]
};

struct StackTrackProduct {
    int m = 0, J = 0;                        // windows per stack (0: the whole block), the largest step between two windows
    tdoa_peak *score_host = nullptr;         // [stack][pair]
    int32_t *lags_host = nullptr;            // [stack][pair][mm]
    double *values_host = nullptr;           // [stack][pair][mm]
    float *surface_host = nullptr;           // [stack][pair][n_lags]
    int64_t *total_host = nullptr;           // [stack][pair][n_lags]
    int mm = 0;                              // filled by reserve_stack_track: the stack length,
    StackLayout layout;                      // the stacks (their roots are what the finish reads),
    std::vector<int32_t> table;              // pos [stack-pair][mm], then n_w [stack-pair] (stack_track.hpp, TrackTable)
    std::vector<double> ones;                // upload_stack_desc's host copy of the unit scales
};

struct ClosureProduct {
    StackProduct stack;                      // the stack whose sums Q are searched: no output of its own, so no finishing kernels
    int G = 0, sep = 1;                      // gate, min_separation
    std::vector<int32_t> centre;             // [stations]: data, not part of the key
    tdoa_closure *out_host = nullptr;        // [stack][triple]
};

struct LocateProduct {
    StackProduct stack;                      // the stack whose sums Q are searched: no output of its own, so no finishing kernels
    int sep = 1;                             // min_separation
    int n_cells = 0, n_cols = 0;             // the shape of the context's table: in the key (the table itself is data)
    tdoa_location *loc_host = nullptr;       // [stack]
    int32_t *lags_host = nullptr;            // [stack][pair]
    double *corr_host = nullptr;             // [stack][pair]
    int64_t *map_host = nullptr;             // [stack][cell]
};

// the product of one step; the numbers are the first word a product appends to the graph key
struct StepProduct {
    enum Kind { None = 0, Lags = 1, Peaks = 2, Stack = 3, StackDrift = 4, StackTrack = 5, Closure = 6, Locate = 7 } kind = None;
    LagsProduct lags;
    PeaksProduct peaks;
    StackProduct stack;
    StackDriftProduct drift;
    StackTrackProduct track;
    ClosureProduct closure;
    LocateProduct locate;
};

// ctx->surf for the rank's pair-windows; `copies`: float surfaces of the step the product holds in all (the message's size)
int surfaces_nomem(const StepView &v, const char *what, double copies)
{
    char buf[256];
    snprintf(buf, sizeof(buf), "%s (%.1f MB) does not fit in device memory: %s", what,
             copies * 4.0 * (double)v.n_lags * (double)std::max(v.n_owned(), v.slots) / 1e6, v.ctx->last_error.c_str());
    return fail(v.ctx, TDOA_ERR_NOMEM, buf);
}
int reserve_surf(const StepView &v, double copies)
{
    if (ensure(v.ctx, v.ctx->surf, sizeof(float) * std::max<size_t>(v.n_owned() * v.n_lags, 1)))
        return surfaces_nomem(v, "correlation surfaces", copies);
    return TDOA_OK;
}

// ---- the surfaces in the caller's layout [slot][n_lags] (ctx->surf_out) ----------------------------------------------
int reserve_lags(const StepView &v, const LagsProduct &)
{
    if (int rc = reserve_surf(v, 2.0)) return rc;
    if (ensure(v.ctx, v.ctx->surf_out, sizeof(float) * (v.surf_n() + 1))) return surfaces_nomem(v, "correlation surfaces, caller's layout", 2.0);
    return TDOA_OK;
}
void key_lags(const LagsProduct &, std::vector<uint64_t> *key) { key->insert(key->end(), {StepProduct::Lags, 0, 0, 0}); }
void enqueue_lags(const StepView &v, const LagsProduct &)
{
    hipStream_t st = v.ctx->stream;
    hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((v.surf_n() / 2 + 256) / 256)), dim3(256), 0, st,
                       v.ctx->surf_out.as<unsigned long long>(), (v.surf_n() + 1) / 2);
    if (v.n_owned())
        hipLaunchKernelGGL(k_surface_out, dim3((unsigned)v.n_owned(), (unsigned)((v.n_lags + 1023) / 1024)), dim3(256), 0, st,
                           v.ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.d_pw, v.d_scales, v.slot_gain,
                           v.ctx->surf_out.as<float>());
}
int download_lags(const StepView &v, const LagsProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    if (p.lags_dev)
        HIPCHK(ctx, hipMemcpyAsync(p.lags_dev, ctx->surf_out.p, sizeof(float) * v.surf_n(), hipMemcpyDeviceToDevice, ctx->stream));
    if (p.lags_host)
        HIPCHK(ctx, hipMemcpyAsync(p.lags_host, ctx->surf_out.p, sizeof(float) * v.surf_n(), hipMemcpyDeviceToHost, ctx->stream));
    return TDOA_OK;
}

// ---- k peaks [slot][k] and their counts [slot] (ctx->sel_peaks, ctx->sel_count) ----------------------------------------
int reserve_peaks(const StepView &v, const PeaksProduct &p)
{
    if (int rc = reserve_surf(v, 1.0)) return rc;
    if (ensure(v.ctx, v.ctx->sel_peaks, sizeof(PeakOut) * v.slots * p.k) || ensure(v.ctx, v.ctx->sel_count, sizeof(int32_t) * (v.slots + 1)))
        return surfaces_nomem(v, "selected peaks", 1.0);
    return TDOA_OK;
}
void key_peaks(const PeaksProduct &p, std::vector<uint64_t> *key)
{
    key->insert(key->end(), {StepProduct::Peaks, (uint64_t)p.k, (uint64_t)p.min_sep, 0});
}
void enqueue_peaks(const StepView &v, const PeaksProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    hipStream_t st = ctx->stream;
    const size_t rec_words = v.slots * (size_t)p.k * (sizeof(PeakOut) / 8);
    hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((rec_words + 255) / 256)), dim3(256), 0, st, ctx->sel_peaks.as<unsigned long long>(),
                       rec_words);
    hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((v.slots / 2 + 256) / 256)), dim3(256), 0, st,
                       ctx->sel_count.as<unsigned long long>(), (v.slots + 1) / 2);
    if (v.n_owned())
        hipLaunchKernelGGL(k_select_peaks, dim3((unsigned)v.n_owned()), dim3(kSelThreads), 0, st, ctx->surf.as<const float>(),
                           (size_t)v.n_lags, v.n_lags, v.lag_lo, v.d_pw, v.d_keys, v.d_scales, v.slot_gain, p.k, p.min_sep,
                           ctx->sel_peaks.as<PeakOut>(), ctx->sel_count.as<int32_t>());
}
int download_peaks(const StepView &v, const PeaksProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    if (p.peaks_host)
        HIPCHK(ctx, hipMemcpyAsync(p.peaks_host, ctx->sel_peaks.p, sizeof(PeakOut) * v.slots * p.k, hipMemcpyDeviceToHost, ctx->stream));
    if (p.count_host)
        HIPCHK(ctx, hipMemcpyAsync(p.count_host, ctx->sel_count.p, sizeof(int32_t) * v.slots, hipMemcpyDeviceToHost, ctx->stream));
    return TDOA_OK;
}

// ---- the stacks' fixed-point sums (ctx->stack_q) and, finished, their surfaces and peaks (stacked_api.inc) ------------
int reserve_stack(const StepView &v, StackProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    if (int rc = reserve_surf(v, 1.0)) return rc;
    p.layout = build_stack_layout(v.lay->pw, v.wpb, v.P, p.m);
    const size_t n_sp = (size_t)p.layout.n_stacks * v.P;
    if (ensure(ctx, ctx->stack_q, sizeof(long long) * n_sp * v.n_lags) ||
        ensure(ctx, ctx->stack_desc, stack_desc_bytes(p.layout.n_stacks, v.P, v.n_owned())) ||
        (p.finish() && ensure_stack_finish(ctx, n_sp, v.n_lags, p.k)))
        return surfaces_nomem(v, "correlation surfaces and their stacked sums", 1.0);
    return TDOA_OK;
}
void key_stack(const StackProduct &p, std::vector<uint64_t> *key)
{
    key->insert(key->end(), {StepProduct::Stack, (uint64_t)p.k, (uint64_t)p.min_sep, (uint64_t)p.m | ((uint64_t)p.finish() << 32)});
}
int upload_stack(const StepView &v, StackProduct &p) { return upload_stack_desc(v.ctx, p.layout, v.P, &p.ones, true); }
void enqueue_stack(const StepView &v, const StackProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    const int n_stacks = p.layout.n_stacks;
    const StackDev sd = stack_dev(ctx, n_stacks, v.P);
    hipLaunchKernelGGL(k_stack_accumulate, dim3((unsigned)(n_stacks * v.P), (unsigned)((v.n_lags + kStackTile - 1) / kStackTile)),
                       dim3(kStackThreads), 0, ctx->stream, ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.d_pw, sd.desc, sd.list,
                       v.d_scales, v.slot_gain, ctx->stack_q.as<long long>());
    if (p.finish()) launch_stack_finish(ctx, n_stacks, v.P, v.n_lags, v.lag_lo, p.k, p.min_sep, p.gate);
}
int download_stack_product(const StepView &v, const StackProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    const size_t n_sp = (size_t)p.layout.n_stacks * v.P;
    if (int rc = download_stack(ctx, n_sp, v.n_lags, p.k, p.peaks_host, p.count_host, p.fine_host, p.surface_host)) return rc;
    if (p.partial_host)
        HIPCHK(ctx, hipMemcpyAsync(p.partial_host, ctx->stack_q.p, sizeof(int64_t) * n_sp * v.n_lags, hipMemcpyDeviceToHost, ctx->stream));
    return TDOA_OK;
}

// ---- the stacks along the best lag slope (stack_drift.hpp): the per-slope keys, h* and the profile, then the stack's own --
// shift(h, j) = sgn(h) ((2 |h| j + D) div (2 D)): the nearest integer to h j / D, halves away from zero
long long drift_shift(int h, long long j, long long D)
{
    const long long a = (2 * (long long)std::abs(h) * j + D) / (2 * D);
    return h < 0 ? -a : a;
}
// the stack length a call with windows_per_stack = m uses
int stack_length(int wpb, int m) { return m > 0 ? std::min(m, wpb) : wpb; }

int reserve_stack_drift(const StepView &v, StackDriftProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    if (int rc = reserve_stack(v, p.stack)) return rc;
    p.mm = stack_length(v.wpb, p.stack.m);
    const int n_hyp = 2 * p.H + 1;
    p.tab.resize((size_t)n_hyp * p.mm);
    for (int h = -p.H; h <= p.H; h++)
        for (int j = 0; j < p.mm; j++) p.tab[(size_t)(h + p.H) * p.mm + j] = (int32_t)drift_shift(h, j, p.D);
    // hypotheses per workgroup: the most whose shifts spread over no more than the staged span holds beyond its tile, for
    // every window position (one hypothesis has no spread); not more than twice the hypotheses there are
    for (p.hb = kShearHyp; p.hb > 1; p.hb /= 2) {
        bool fits = p.hb / 2 < n_hyp;
        for (int z0 = 0; fits && z0 < n_hyp; z0 += p.hb)
            for (int j = 0; fits && j < p.mm; j++)
                fits = p.tab[(size_t)std::min(z0 + p.hb - 1, n_hyp - 1) * p.mm + j] - p.tab[(size_t)z0 * p.mm + j] <= kShearSpread;
        if (fits) break;
    }
    const size_t n_sp = (size_t)p.stack.layout.n_stacks * v.P;
    if (ensure(ctx, ctx->drift_tab, sizeof(int32_t) * p.tab.size()) ||
        ensure(ctx, ctx->drift_keys, sizeof(unsigned long long) * n_sp * n_hyp) ||
        ensure(ctx, ctx->drift_h, sizeof(int32_t) * std::max<size_t>(n_sp, 1)) ||
        ensure(ctx, ctx->drift_prof, sizeof(PeakOut) * n_sp * n_hyp))
        return surfaces_nomem(v, "the slope search's keys and profile", 1.0);
    return TDOA_OK;
}
void key_stack_drift(const StackDriftProduct &p, std::vector<uint64_t> *key)
{
    const StackProduct &s = p.stack;
    key->insert(key->end(), {StepProduct::StackDrift, (uint64_t)s.k, (uint64_t)s.min_sep, (uint64_t)s.m | ((uint64_t)s.finish() << 32),
                             (uint64_t)p.H, (uint64_t)p.D});
}
int upload_stack_drift(const StepView &v, StackDriftProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    if (int rc = upload_stack(v, p.stack)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->drift_tab.p, p.tab.data(), sizeof(int32_t) * p.tab.size(), hipMemcpyHostToDevice, ctx->stream));
    return TDOA_OK;
}
template <int HB>
void launch_shear_search(const StepView &v, const StackDriftProduct &p, const StackDev &sd, const ShearGeom &g)
{
    tdoa_ctx *ctx = v.ctx;
    const int n_stacks = p.stack.layout.n_stacks, n_hyp = 2 * p.H + 1;
    hipLaunchKernelGGL(k_stack_shear_search<HB>,
                       dim3((unsigned)(n_stacks * v.P), (unsigned)((v.n_lags + kShearTile - 1) / kShearTile), (unsigned)((n_hyp + HB - 1) / HB)),
                       dim3(kStackThreads), 0, ctx->stream, ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.lag_lo, v.d_pw,
                       sd.desc, sd.list, v.d_scales, v.slot_gain, sd.roots, ctx->drift_tab.as<const int32_t>(), g,
                       ctx->drift_keys.as<unsigned long long>());
}
void enqueue_stack_drift(const StepView &v, const StackDriftProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    hipStream_t st = ctx->stream;
    const StackProduct &s = p.stack;
    const int n_stacks = s.layout.n_stacks, n_hyp = 2 * p.H + 1;
    const unsigned n_sp = (unsigned)(n_stacks * v.P);
    const StackDev sd = stack_dev(ctx, n_stacks, v.P);
    const ShearGeom g{p.H, p.mm, v.wpb, v.P};
    const size_t n_keys = (size_t)n_sp * n_hyp;
    hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, st, ctx->drift_keys.as<unsigned long long>(), n_keys);
    switch (p.hb) {
    case 8: launch_shear_search<8>(v, p, sd, g); break;
    case 4: launch_shear_search<4>(v, p, sd, g); break;
    case 2: launch_shear_search<2>(v, p, sd, g); break;
    default: launch_shear_search<1>(v, p, sd, g);
    }
    hipLaunchKernelGGL(k_stack_pick_drift, dim3(n_sp), dim3(kWave), 0, st, ctx->drift_keys.as<const unsigned long long>(), p.H,
                       ctx->drift_h.as<int32_t>(), ctx->drift_prof.as<PeakOut>());
    hipLaunchKernelGGL(k_stack_accumulate_sheared, dim3(n_sp, (unsigned)((v.n_lags + kStackTile - 1) / kStackTile)), dim3(kStackThreads), 0,
                       st, ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.d_pw, sd.desc, sd.list, v.d_scales, v.slot_gain,
                       ctx->drift_tab.as<const int32_t>(), ctx->drift_h.as<const int32_t>(), g, ctx->stack_q.as<long long>());
    if (s.finish()) launch_stack_finish(ctx, n_stacks, v.P, v.n_lags, v.lag_lo, s.k, s.min_sep, s.gate);
}
int download_stack_drift(const StepView &v, const StackDriftProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    const size_t n_sp = (size_t)p.stack.layout.n_stacks * v.P;
    if (int rc = download_stack_product(v, p.stack)) return rc;
    if (p.drift_host) HIPCHK(ctx, hipMemcpyAsync(p.drift_host, ctx->drift_h.p, sizeof(int32_t) * n_sp, hipMemcpyDeviceToHost, ctx->stream));
    if (p.profile_host)
        HIPCHK(ctx, hipMemcpyAsync(p.profile_host, ctx->drift_prof.p, sizeof(PeakOut) * n_sp * (2 * p.H + 1), hipMemcpyDeviceToHost, ctx->stream));
    return TDOA_OK;
}

// ---- the best delay track through every stack-pair's windows (stack_track.hpp) ------------------------------------------
// T (ctx->track_t): two halves [stack-pair][n_lags] TrackPair, position j writes half j & 1 and reads the other, so T_0 ends
// in the first; D (ctx->track_d): [stack-pair][mm][n_lags][2] int8; total and the float surface go where the plain stack
// keeps Q and its surface (ctx->stack_q, ctx->stack_surf)
int reserve_stack_track(const StepView &v, StackTrackProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    if (int rc = reserve_surf(v, 1.0)) return rc;
    p.layout = build_stack_layout(v.lay->pw, v.wpb, v.P, p.m);
    p.mm = stack_length(v.wpb, p.m);
    const size_t n_sp = (size_t)p.layout.n_stacks * v.P;
    p.table.assign(n_sp * p.mm + n_sp, -1);
    std::fill(p.table.begin() + n_sp * p.mm, p.table.end(), 0);
    for (size_t i = 0; i < v.lay->pw.size(); i++) {
        const int wid = v.lay->pw[i].out_index / v.P, pair = v.lay->pw[i].out_index % v.P;
        const size_t sp = (size_t)((wid / v.wpb) * p.layout.spb + (wid % v.wpb) / p.mm) * v.P + pair;
        p.table[sp * p.mm + (wid % v.wpb) % p.mm] = (int32_t)i;
        p.table[n_sp * p.mm + sp]++;
    }
    if (ensure(ctx, ctx->stack_desc, stack_desc_bytes(p.layout.n_stacks, v.P, v.n_owned())) ||
        ensure(ctx, ctx->track_tab, sizeof(int32_t) * p.table.size()) ||
        ensure(ctx, ctx->track_t, 2 * sizeof(TrackPair) * n_sp * v.n_lags) ||
        ensure(ctx, ctx->track_d, 2 * n_sp * p.mm * v.n_lags) ||
        ensure(ctx, ctx->stack_q, sizeof(long long) * n_sp * v.n_lags) ||
        ensure(ctx, ctx->stack_surf, sizeof(float) * n_sp * v.n_lags) ||
        ensure(ctx, ctx->track_score, sizeof(PeakOut) * n_sp) ||
        ensure(ctx, ctx->track_lags, sizeof(int32_t) * n_sp * p.mm) ||
        ensure(ctx, ctx->track_values, sizeof(double) * n_sp * p.mm))
        return surfaces_nomem(v, "correlation surfaces and the track's sums and steps", 1.0 + 0.5 * p.mm);
    return TDOA_OK;
}
void key_stack_track(const StackTrackProduct &p, std::vector<uint64_t> *key)
{
    key->insert(key->end(), {StepProduct::StackTrack, (uint64_t)p.m, (uint64_t)p.J, 0});
}
int upload_stack_track(const StepView &v, StackTrackProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    if (int rc = upload_stack_desc(ctx, p.layout, v.P, &p.ones, true)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->track_tab.p, p.table.data(), sizeof(int32_t) * p.table.size(), hipMemcpyHostToDevice, ctx->stream));
    return TDOA_OK;
}
void enqueue_stack_track(const StepView &v, const StackTrackProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    hipStream_t st = ctx->stream;
    const int n_stacks = p.layout.n_stacks;
    const unsigned n_sp = (unsigned)(n_stacks * v.P);
    const StackDev sd = stack_dev(ctx, n_stacks, v.P);
    const int32_t *tab = ctx->track_tab.as<const int32_t>();
    const TrackTable tt{tab, tab + (size_t)n_sp * p.mm, p.mm};
    TrackPair *half[2] = {ctx->track_t.as<TrackPair>(), ctx->track_t.as<TrackPair>() + (size_t)n_sp * v.n_lags};
    const dim3 grid(n_sp, (unsigned)((v.n_lags + kTrackTile - 1) / kTrackTile));
    {
        ProfScope ps(ctx, TDOA_K_TRACK_STEP, (4.0 + 2.0 * sizeof(TrackPair) + 2.0) * (double)v.n_lags * (double)v.n_owned());
        for (int j = p.mm - 1; j >= 0; j--)
            hipLaunchKernelGGL(k_track_step, grid, dim3(kTrackThreads), 0, st, ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags,
                               v.d_pw, v.d_scales, v.slot_gain, tt, j, p.J, static_cast<const TrackPair *>(half[(j + 1) & 1]),
                               half[j & 1], ctx->track_d.as<signed char>());
    }
    ProfScope ps(ctx, TDOA_K_TRACK_FINISH, (2.0 * sizeof(TrackPair) + 12.0) * (double)v.n_lags * n_sp);
    hipLaunchKernelGGL(k_track_finish, dim3(n_sp), dim3(kTrackThreads), 0, st, static_cast<const TrackPair *>(half[0]),
                       ctx->track_d.as<const signed char>(), ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.lag_lo, v.P,
                       v.d_pw, v.d_scales, v.slot_gain, sd.roots, tt, ctx->track_score.as<PeakOut>(), ctx->track_lags.as<int32_t>(),
                       ctx->track_values.as<double>(), ctx->stack_q.as<long long>(), ctx->stack_surf.as<float>());
}
int download_stack_track(const StepView &v, const StackTrackProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    hipStream_t st = ctx->stream;
    const size_t n_sp = (size_t)p.layout.n_stacks * v.P;
    if (p.score_host) HIPCHK(ctx, hipMemcpyAsync(p.score_host, ctx->track_score.p, sizeof(PeakOut) * n_sp, hipMemcpyDeviceToHost, st));
    if (p.lags_host) HIPCHK(ctx, hipMemcpyAsync(p.lags_host, ctx->track_lags.p, sizeof(int32_t) * n_sp * p.mm, hipMemcpyDeviceToHost, st));
    if (p.values_host) HIPCHK(ctx, hipMemcpyAsync(p.values_host, ctx->track_values.p, sizeof(double) * n_sp * p.mm, hipMemcpyDeviceToHost, st));
    if (p.surface_host)
        HIPCHK(ctx, hipMemcpyAsync(p.surface_host, ctx->stack_surf.p, sizeof(float) * n_sp * v.n_lags, hipMemcpyDeviceToHost, st));
    if (p.total_host)
        HIPCHK(ctx, hipMemcpyAsync(p.total_host, ctx->stack_q.p, sizeof(int64_t) * n_sp * v.n_lags, hipMemcpyDeviceToHost, st));
    return TDOA_OK;
}

// ---- the closure search on the stacks' sums (stack_closure.hpp, closure_api.inc) ---------------------------------------
int reserve_closure(const StepView &v, ClosureProduct &p)
{
    if (int rc = reserve_stack(v, p.stack)) return rc;
    const ClosureGeom g = closure_geom((int)p.centre.size(), v.ctx->prm.max_lag, p.G, p.sep);
    if (ensure_closure(v.ctx, p.stack.layout.n_stacks, g)) return surfaces_nomem(v, "the closure search's candidates and records", 1.0);
    return TDOA_OK;
}
void key_closure(const ClosureProduct &p, std::vector<uint64_t> *key)
{
    key->insert(key->end(), {StepProduct::Closure, (uint64_t)p.stack.m, (uint64_t)p.G, (uint64_t)p.sep});
}
int refresh_closure(const StepView &v, const ClosureProduct &p) { return upload_closure_centre(v.ctx, p.centre); }
void enqueue_closure(const StepView &v, const ClosureProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    enqueue_stack(v, p.stack);
    const int n_stacks = p.stack.layout.n_stacks;
    launch_closure(ctx, ctx->stack_q.as<const long long>(), stack_dev(ctx, n_stacks, v.P).roots, n_stacks,
                   closure_geom((int)p.centre.size(), ctx->prm.max_lag, p.G, p.sep));
}
int download_closure_product(const StepView &v, const ClosureProduct &p)
{
    return download_closure(v.ctx, p.stack.layout.n_stacks, closure_geom((int)p.centre.size(), v.ctx->prm.max_lag, p.G, p.sep), p.out_host);
}

// ---- the delay-table search on the stacks' sums (stack_locate.hpp, locate_api.inc) -------------------------------------
int reserve_locate(const StepView &v, LocateProduct &p)
{
    if (int rc = reserve_stack(v, p.stack)) return rc;
    return ensure_locate(v.ctx, p.stack.layout.n_stacks, locate_geom(v.ctx, p.sep));
}
void key_locate(const LocateProduct &p, std::vector<uint64_t> *key)
{
    key->insert(key->end(), {StepProduct::Locate, (uint64_t)p.stack.m, (uint64_t)p.sep, (uint64_t)p.n_cells | ((uint64_t)p.n_cols << 32)});
}
void enqueue_locate(const StepView &v, const LocateProduct &p)
{
    tdoa_ctx *ctx = v.ctx;
    enqueue_stack(v, p.stack);
    const int n_stacks = p.stack.layout.n_stacks;
    launch_locate(ctx, ctx->stack_q.as<const long long>(), stack_dev(ctx, n_stacks, v.P).roots, n_stacks, locate_geom(ctx, p.sep));
}
int download_locate_product(const StepView &v, const LocateProduct &p)
{
    return download_locate(v.ctx, p.stack.layout.n_stacks, locate_geom(v.ctx, p.sep), p.loc_host, p.lags_host, p.corr_host, p.map_host);
}

// ---- process_impl's one dispatch per stage ---------------------------------------------------------------------------
int reserve_product(const StepView &v, StepProduct &p)
{
    switch (p.kind) {
    case StepProduct::Lags: return reserve_lags(v, p.lags);
    case StepProduct::Peaks: return reserve_peaks(v, p.peaks);
    case StepProduct::Stack: return reserve_stack(v, p.stack);
    case StepProduct::StackDrift: return reserve_stack_drift(v, p.drift);
    case StepProduct::StackTrack: return reserve_stack_track(v, p.track);
    case StepProduct::Closure: return reserve_closure(v, p.closure);
    case StepProduct::Locate: return reserve_locate(v, p.locate);
    default: return TDOA_OK;
    }
}
void key_product(const StepProduct &p, std::vector<uint64_t> *key)
{
    switch (p.kind) {
    case StepProduct::Lags: return key_lags(p.lags, key);
    case StepProduct::Peaks: return key_peaks(p.peaks, key);
    case StepProduct::Stack: return key_stack(p.stack, key);
    case StepProduct::StackDrift: return key_stack_drift(p.drift, key);
    case StepProduct::StackTrack: return key_stack_track(p.track, key);
    case StepProduct::Closure: return key_closure(p.closure, key);
    case StepProduct::Locate: return key_locate(p.locate, key);
    default: key->insert(key->end(), {StepProduct::None, 0, 0, 0});
    }
}
int upload_product(const StepView &v, StepProduct &p)
{
    switch (p.kind) {
    case StepProduct::Stack: return upload_stack(v, p.stack);
    case StepProduct::StackDrift: return upload_stack_drift(v, p.drift);
    case StepProduct::StackTrack: return upload_stack_track(v, p.track);
    case StepProduct::Closure: return upload_stack(v, p.closure.stack);
    case StepProduct::Locate: return upload_stack(v, p.locate.stack);
    default: return TDOA_OK;
    }
}
// every call, replayed or not, before the step is launched
int refresh_product(const StepView &v, const StepProduct &p)
{
    return p.kind == StepProduct::Closure ? refresh_closure(v, p.closure) : TDOA_OK;
}
void enqueue_product(const StepView &v, const StepProduct &p)
{
    if (p.kind != StepProduct::None) v.ctx->prof_last = -1;    // unscoped launches
    switch (p.kind) {
    case StepProduct::Lags: return enqueue_lags(v, p.lags);
    case StepProduct::Peaks: return enqueue_peaks(v, p.peaks);
    case StepProduct::Stack: return enqueue_stack(v, p.stack);
    case StepProduct::StackDrift: return enqueue_stack_drift(v, p.drift);
    case StepProduct::StackTrack: return enqueue_stack_track(v, p.track);
    case StepProduct::Closure: return enqueue_closure(v, p.closure);
    case StepProduct::Locate: return enqueue_locate(v, p.locate);
    default: return;
    }
}
int download_product(const StepView &v, const StepProduct &p)
{
    switch (p.kind) {
    case StepProduct::Lags: return download_lags(v, p.lags);
    case StepProduct::Peaks: return download_peaks(v, p.peaks);
    case StepProduct::Stack: return download_stack_product(v, p.stack);
    case StepProduct::StackDrift: return download_stack_drift(v, p.drift);
    case StepProduct::StackTrack: return download_stack_track(v, p.track);
    case StepProduct::Closure: return download_closure_product(v, p.closure);
    case StepProduct::Locate: return download_locate_product(v, p.locate);
    default: return TDOA_OK;
    }
}

}  // namespace
