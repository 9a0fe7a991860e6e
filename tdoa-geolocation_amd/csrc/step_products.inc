// step_products.inc -- what a step (process_impl) can write besides its peak records: the correlation surfaces
// (tdoa_process_lags), the K strongest peaks per pair-window (tdoa_process_peaks), the stacked surfaces of a block's windows
// (tdoa_process_stacked), the same stacks taken along the best of 2H+1 lag slopes (tdoa_process_stacked_drift), the best
// delay track through a stack's windows (tdoa_process_track), and a search on the stacks' sums (SearchProduct,
// stack_search.inc: the closure, clock, clock-line and delay-table searches).  Every product
// is a struct derived from StepProduct: the entry point fills it, process_impl calls its six hooks in this order (a product
// overrides the ones it needs; process_impl without a product writes the peak records only):
//   reserve   its buffers, after the step's grouping is fixed (batch_bound counts them as held, so a later call groups as
//             this one did); no allocation may happen once the step is being captured
//   key       the words it appends to the step graph's key: everything its launches depend on
//   upload    descriptors of its own, sent with the step's when the step is not replayed
//   refresh   data a call may change under the same key, sent every time
//   enqueue   its kernels, after the step's decode -- unscoped launches, kernel nodes only: the step stays one chain
//   download  its asynchronous copies out on ctx->stream
// StackDriftProduct and SearchProduct derive from StackProduct and call its hooks from theirs.
// All of them read the K5 kernels' lag arrays in ctx->surf, pair-window i of the rank at i * n_lags.
// Here: StepProduct, LagsProduct, PeaksProduct, StackProduct, StackDriftProduct, StackTrackProduct.
// Included by tdoa_mi355x.hip after step_graph.inc and stacked_api.inc, before process_impl.

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

// the product of one step; the numbers are the first word a product appends to the graph key
struct StepProduct {
    enum Kind { None = 0, Lags = 1, Peaks = 2, Stack = 3, StackDrift = 4, StackTrack = 5, Closure = 6, Locate = 7, Sync = 8, SyncDrift = 9, SyncFine = 10, LocateZoom = 11, SyncDriftFine = 12, LocateTrackZoom = 13, SyncLocate = 14, SyncDriftLocate = 15, LocateMultiZoom = 16 };
    virtual int reserve(const StepView &v) = 0;
    virtual void key(std::vector<uint64_t> *key) const = 0;
    virtual int upload(const StepView &) { return TDOA_OK; }
    virtual int refresh(const StepView &) { return TDOA_OK; }
    virtual void enqueue(const StepView &v) const = 0;
    virtual int download(const StepView &v) const = 0;
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
struct LagsProduct : StepProduct {
    float *lags_host = nullptr;
    void *lags_dev = nullptr;

    int reserve(const StepView &v) override
    {
        if (int rc = reserve_surf(v, 2.0)) return rc;
        if (ensure(v.ctx, v.ctx->surf_out, sizeof(float) * (v.surf_n() + 1))) return surfaces_nomem(v, "correlation surfaces, caller's layout", 2.0);
        return TDOA_OK;
    }
    void key(std::vector<uint64_t> *key) const override { key->insert(key->end(), {Lags, 0, 0, 0}); }
    void enqueue(const StepView &v) const override
    {
        hipStream_t st = v.ctx->stream;
        hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((v.surf_n() / 2 + 256) / 256)), dim3(256), 0, st,
                           v.ctx->surf_out.as<unsigned long long>(), (v.surf_n() + 1) / 2);
        if (v.n_owned())
            hipLaunchKernelGGL(k_surface_out, dim3((unsigned)v.n_owned(), (unsigned)((v.n_lags + 1023) / 1024)), dim3(256), 0, st,
                               v.ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.d_pw, v.d_scales, v.slot_gain,
                               v.ctx->surf_out.as<float>());
    }
    int download(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        if (lags_dev)
            HIPCHK(ctx, hipMemcpyAsync(lags_dev, ctx->surf_out.p, sizeof(float) * v.surf_n(), hipMemcpyDeviceToDevice, ctx->stream));
        if (lags_host)
            HIPCHK(ctx, hipMemcpyAsync(lags_host, ctx->surf_out.p, sizeof(float) * v.surf_n(), hipMemcpyDeviceToHost, ctx->stream));
        return TDOA_OK;
    }
};

// ---- k peaks [slot][k] and their counts [slot] (ctx->sel_peaks, ctx->sel_count) ----------------------------------------
struct PeaksProduct : StepProduct {
    int k = 0, min_sep = 0;
    tdoa_peak *peaks_host = nullptr;         // [slot][k]
    int32_t *count_host = nullptr;           // [slot]

    int reserve(const StepView &v) override
    {
        if (int rc = reserve_surf(v, 1.0)) return rc;
        if (ensure(v.ctx, v.ctx->sel_peaks, sizeof(PeakOut) * v.slots * k) || ensure(v.ctx, v.ctx->sel_count, sizeof(int32_t) * (v.slots + 1)))
            return surfaces_nomem(v, "selected peaks", 1.0);
        return TDOA_OK;
    }
    void key(std::vector<uint64_t> *key) const override { key->insert(key->end(), {Peaks, (uint64_t)k, (uint64_t)min_sep, 0}); }
    void enqueue(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        hipStream_t st = ctx->stream;
        const size_t rec_words = v.slots * (size_t)k * (sizeof(PeakOut) / 8);
        hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((rec_words + 255) / 256)), dim3(256), 0, st, ctx->sel_peaks.as<unsigned long long>(),
                           rec_words);
        hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((v.slots / 2 + 256) / 256)), dim3(256), 0, st,
                           ctx->sel_count.as<unsigned long long>(), (v.slots + 1) / 2);
        if (v.n_owned())
            hipLaunchKernelGGL(k_select_peaks, dim3((unsigned)v.n_owned()), dim3(kSelThreads), 0, st, ctx->surf.as<const float>(),
                               (size_t)v.n_lags, v.n_lags, v.lag_lo, v.d_pw, v.d_keys, v.d_scales, v.slot_gain, k, min_sep,
                               ctx->sel_peaks.as<PeakOut>(), ctx->sel_count.as<int32_t>());
    }
    int download(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        if (peaks_host)
            HIPCHK(ctx, hipMemcpyAsync(peaks_host, ctx->sel_peaks.p, sizeof(PeakOut) * v.slots * k, hipMemcpyDeviceToHost, ctx->stream));
        if (count_host)
            HIPCHK(ctx, hipMemcpyAsync(count_host, ctx->sel_count.p, sizeof(int32_t) * v.slots, hipMemcpyDeviceToHost, ctx->stream));
        return TDOA_OK;
    }
};

// ---- the stacks' fixed-point sums (ctx->stack_q) and, finished, their surfaces and peaks (stacked_api.inc) ------------
struct StackProduct : StepProduct {
    int m = 0;                               // windows per stack, 0: the whole block
    int k = 0, min_sep = 0;
    double gate = 0.0;
    tdoa_peak *peaks_host = nullptr;         // [stack][pair][k]
    int32_t *count_host = nullptr;           // [stack][pair]
    tdoa_fine_peak *fine_host = nullptr;
    float *surface_host = nullptr;
    int64_t *partial_host = nullptr;         // the rank's fixed-point sums Q
    StackLayout layout;                      // filled by reserve
    std::vector<double> ones;                // upload's host copy of the unit scales (lives until the step's upload has synchronised)

    // the finishing kernels run when one of their outputs is asked for (a group member returns its partial sums only)
    bool finish() const { return peaks_host || count_host || fine_host || surface_host; }
    uint64_t m_word() const { return (uint64_t)m | ((uint64_t)finish() << 32); }
    size_t n_sp(const StepView &v) const { return (size_t)layout.n_stacks * v.P; }

    int reserve(const StepView &v) override
    {
        tdoa_ctx *ctx = v.ctx;
        if (int rc = reserve_surf(v, 1.0)) return rc;
        layout = build_stack_layout(v.lay->pw, stack_geom(v.wpb, m), v.P);
        if (ensure(ctx, ctx->stack_q, sizeof(long long) * n_sp(v) * v.n_lags) ||
            ensure(ctx, ctx->stack_desc, stack_desc_bytes(layout.n_stacks, v.P, v.n_owned())) ||
            (finish() && ensure_stack_finish(ctx, n_sp(v), v.n_lags, k)))
            return surfaces_nomem(v, "correlation surfaces and their stacked sums", 1.0);
        return TDOA_OK;
    }
    void key(std::vector<uint64_t> *key) const override { key->insert(key->end(), {Stack, (uint64_t)k, (uint64_t)min_sep, m_word()}); }
    int upload(const StepView &v) override { return upload_stack_desc(v.ctx, layout, v.P, &ones, true); }
    void enqueue(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        const int n_stacks = layout.n_stacks;
        const StackDev sd = stack_dev(ctx, n_stacks, v.P);
        hipLaunchKernelGGL(k_stack_accumulate, dim3((unsigned)(n_stacks * v.P), (unsigned)((v.n_lags + kStackTile - 1) / kStackTile)),
                           dim3(kStackThreads), 0, ctx->stream, ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.d_pw, sd.desc, sd.list,
                           v.d_scales, v.slot_gain, ctx->stack_q.as<long long>());
        if (finish()) launch_stack_finish(ctx, n_stacks, v.P, v.n_lags, v.lag_lo, k, min_sep, gate);
    }
    int download(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        if (int rc = download_stack(ctx, n_sp(v), v.n_lags, k, peaks_host, count_host, fine_host, surface_host)) return rc;
        if (partial_host)
            HIPCHK(ctx, hipMemcpyAsync(partial_host, ctx->stack_q.p, sizeof(int64_t) * n_sp(v) * v.n_lags, hipMemcpyDeviceToHost, ctx->stream));
        return TDOA_OK;
    }
};

// ---- the stacks along the best lag slope (stack_drift.hpp): the per-slope keys, h* and the profile, then the stack's own --
// shift(h, j) = sgn(h) ((2 |h| j + D) div (2 D)): the nearest integer to h j / D, halves away from zero
long long drift_shift(int h, long long j, long long D)
{
    const long long a = (2 * (long long)std::abs(h) * j + D) / (2 * D);
    return h < 0 ? -a : a;
}

struct StackDriftProduct : StackProduct {    // the stack's own arguments and outputs, computed on Q_{h*}
    int H = 0, D = 1;                        // hypotheses -H .. H, slope h / D lags per window
    int32_t *drift_host = nullptr;           // [stack][pair]: h*
    tdoa_peak *profile_host = nullptr;       // [stack][pair][2H+1]
    int hb = 1;                              // filled by reserve: hypotheses per workgroup
    std::vector<int32_t> tab;                // ... and shift(h, j) at [(h + H) * mm + j]

    int reserve(const StepView &v) override
    {
        tdoa_ctx *ctx = v.ctx;
        if (int rc = StackProduct::reserve(v)) return rc;
        const int mm = layout.mm, n_hyp = 2 * H + 1;
        tab.resize((size_t)n_hyp * mm);
        for (int h = -H; h <= H; h++)
            for (int j = 0; j < mm; j++) tab[(size_t)(h + H) * mm + j] = (int32_t)drift_shift(h, j, D);
        // hypotheses per workgroup: the most whose shifts spread over no more than the staged span holds beyond its tile, for
        // every window position (one hypothesis has no spread); not more than twice the hypotheses there are
        for (hb = kShearHyp; hb > 1; hb /= 2) {
            bool fits = hb / 2 < n_hyp;
            for (int z0 = 0; fits && z0 < n_hyp; z0 += hb)
                for (int j = 0; fits && j < mm; j++)
                    fits = tab[(size_t)std::min(z0 + hb - 1, n_hyp - 1) * mm + j] - tab[(size_t)z0 * mm + j] <= kShearSpread;
            if (fits) break;
        }
        if (ensure(ctx, ctx->drift_tab, sizeof(int32_t) * tab.size()) ||
            ensure(ctx, ctx->drift_keys, sizeof(unsigned long long) * n_sp(v) * n_hyp) ||
            ensure(ctx, ctx->drift_h, sizeof(int32_t) * std::max<size_t>(n_sp(v), 1)) ||
            ensure(ctx, ctx->drift_prof, sizeof(PeakOut) * n_sp(v) * n_hyp))
            return surfaces_nomem(v, "the slope search's keys and profile", 1.0);
        return TDOA_OK;
    }
    void key(std::vector<uint64_t> *key) const override
    {
        key->insert(key->end(), {StackDrift, (uint64_t)k, (uint64_t)min_sep, m_word(), (uint64_t)H, (uint64_t)D});
    }
    int upload(const StepView &v) override
    {
        tdoa_ctx *ctx = v.ctx;
        if (int rc = StackProduct::upload(v)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->drift_tab.p, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
        return TDOA_OK;
    }
    template <int HB>
    void launch_shear_search(const StepView &v, const StackDev &sd, const ShearGeom &g) const
    {
        tdoa_ctx *ctx = v.ctx;
        const int n_stacks = layout.n_stacks, n_hyp = 2 * H + 1;
        hipLaunchKernelGGL(k_stack_shear_search<HB>,
                           dim3((unsigned)(n_stacks * v.P), (unsigned)((v.n_lags + kShearTile - 1) / kShearTile), (unsigned)((n_hyp + HB - 1) / HB)),
                           dim3(kStackThreads), 0, ctx->stream, ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.lag_lo, v.d_pw,
                           sd.desc, sd.list, v.d_scales, v.slot_gain, sd.roots, ctx->drift_tab.as<const int32_t>(), g,
                           ctx->drift_keys.as<unsigned long long>());
    }
    void enqueue(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        hipStream_t st = ctx->stream;
        const int n_stacks = layout.n_stacks, n_hyp = 2 * H + 1;
        const unsigned n_sp = (unsigned)(n_stacks * v.P);
        const StackDev sd = stack_dev(ctx, n_stacks, v.P);
        const ShearGeom g{H, layout.mm, v.wpb, v.P};
        const size_t n_keys = (size_t)n_sp * n_hyp;
        hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, st, ctx->drift_keys.as<unsigned long long>(), n_keys);
        switch (hb) {
        case 8: launch_shear_search<8>(v, sd, g); break;
        case 4: launch_shear_search<4>(v, sd, g); break;
        case 2: launch_shear_search<2>(v, sd, g); break;
        default: launch_shear_search<1>(v, sd, g);
        }
        hipLaunchKernelGGL(k_stack_pick_drift, dim3(n_sp), dim3(kWave), 0, st, ctx->drift_keys.as<const unsigned long long>(), H,
                           ctx->drift_h.as<int32_t>(), ctx->drift_prof.as<PeakOut>());
        hipLaunchKernelGGL(k_stack_accumulate_sheared, dim3(n_sp, (unsigned)((v.n_lags + kStackTile - 1) / kStackTile)), dim3(kStackThreads), 0,
                           st, ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.d_pw, sd.desc, sd.list, v.d_scales, v.slot_gain,
                           ctx->drift_tab.as<const int32_t>(), ctx->drift_h.as<const int32_t>(), g, ctx->stack_q.as<long long>());
        if (finish()) launch_stack_finish(ctx, n_stacks, v.P, v.n_lags, v.lag_lo, k, min_sep, gate);
    }
    int download(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        if (int rc = StackProduct::download(v)) return rc;
        if (drift_host) HIPCHK(ctx, hipMemcpyAsync(drift_host, ctx->drift_h.p, sizeof(int32_t) * n_sp(v), hipMemcpyDeviceToHost, ctx->stream));
        if (profile_host)
            HIPCHK(ctx, hipMemcpyAsync(profile_host, ctx->drift_prof.p, sizeof(PeakOut) * n_sp(v) * (2 * H + 1), hipMemcpyDeviceToHost, ctx->stream));
        return TDOA_OK;
    }
};

// ---- the best delay track through every stack-pair's windows (stack_track.hpp) ------------------------------------------
// T (ctx->track_t): two halves [stack-pair][n_lags] TrackPair, position j writes half j & 1 and reads the other, so T_0 ends
// in the first; D (ctx->track_d): [stack-pair][mm][n_lags][2] int8; total and the float surface go where the plain stack
// keeps Q and its surface (ctx->stack_q, ctx->stack_surf)
struct StackTrackProduct : StepProduct {
    int m = 0, J = 0;                        // windows per stack (0: the whole block), the largest step between two windows
    tdoa_peak *score_host = nullptr;         // [stack][pair]
    int32_t *lags_host = nullptr;            // [stack][pair][mm]
    double *values_host = nullptr;           // [stack][pair][mm]
    float *surface_host = nullptr;           // [stack][pair][n_lags]
    int64_t *total_host = nullptr;           // [stack][pair][n_lags]
    StackLayout layout;                      // filled by reserve: the stacks (their roots are what the finish reads),
    std::vector<int32_t> table;              // pos [stack-pair][mm], then n_w [stack-pair] (stack_track.hpp, TrackTable)
    std::vector<double> ones;                // upload_stack_desc's host copy of the unit scales

    int reserve(const StepView &v) override
    {
        tdoa_ctx *ctx = v.ctx;
        if (int rc = reserve_surf(v, 1.0)) return rc;
        layout = build_stack_layout(v.lay->pw, stack_geom(v.wpb, m), v.P);
        const int mm = layout.mm;
        const size_t n_sp = (size_t)layout.n_stacks * v.P;
        table.assign(n_sp * mm + n_sp, -1);
        std::fill(table.begin() + n_sp * mm, table.end(), 0);
        for (size_t i = 0; i < v.lay->pw.size(); i++) {
            const int wid = v.lay->pw[i].out_index / v.P, pair = v.lay->pw[i].out_index % v.P;
            const size_t sp = (size_t)layout.stack_of(wid) * v.P + pair;
            table[sp * mm + layout.pos_of(wid)] = (int32_t)i;
            table[n_sp * mm + sp]++;
        }
        if (ensure(ctx, ctx->stack_desc, stack_desc_bytes(layout.n_stacks, v.P, v.n_owned())) ||
            ensure(ctx, ctx->track_tab, sizeof(int32_t) * table.size()) ||
            ensure(ctx, ctx->track_t, 2 * sizeof(TrackPair) * n_sp * v.n_lags) ||
            ensure(ctx, ctx->track_d, 2 * n_sp * mm * v.n_lags) ||
            ensure(ctx, ctx->stack_q, sizeof(long long) * n_sp * v.n_lags) ||
            ensure(ctx, ctx->stack_surf, sizeof(float) * n_sp * v.n_lags) ||
            ensure(ctx, ctx->track_score, sizeof(PeakOut) * n_sp) ||
            ensure(ctx, ctx->track_lags, sizeof(int32_t) * n_sp * mm) ||
            ensure(ctx, ctx->track_values, sizeof(double) * n_sp * mm))
            return surfaces_nomem(v, "correlation surfaces and the track's sums and steps", 1.0 + 0.5 * mm);
        return TDOA_OK;
    }
    void key(std::vector<uint64_t> *key) const override { key->insert(key->end(), {StackTrack, (uint64_t)m, (uint64_t)J, 0}); }
    int upload(const StepView &v) override
    {
        tdoa_ctx *ctx = v.ctx;
        if (int rc = upload_stack_desc(ctx, layout, v.P, &ones, true)) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->track_tab.p, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice, ctx->stream));
        return TDOA_OK;
    }
    void enqueue(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        hipStream_t st = ctx->stream;
        const int n_stacks = layout.n_stacks, mm = layout.mm;
        const unsigned n_sp = (unsigned)(n_stacks * v.P);
        const StackDev sd = stack_dev(ctx, n_stacks, v.P);
        const int32_t *tab = ctx->track_tab.as<const int32_t>();
        const TrackTable tt{tab, tab + (size_t)n_sp * mm, mm};
        TrackPair *half[2] = {ctx->track_t.as<TrackPair>(), ctx->track_t.as<TrackPair>() + (size_t)n_sp * v.n_lags};
        const dim3 grid(n_sp, (unsigned)((v.n_lags + kTrackTile - 1) / kTrackTile));
        {
            ProfScope ps(ctx, TDOA_K_TRACK_STEP, (4.0 + 2.0 * sizeof(TrackPair) + 2.0) * (double)v.n_lags * (double)v.n_owned());
            for (int j = mm - 1; j >= 0; j--)
                hipLaunchKernelGGL(k_track_step, grid, dim3(kTrackThreads), 0, st, ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags,
                                   v.d_pw, v.d_scales, v.slot_gain, tt, j, J, static_cast<const TrackPair *>(half[(j + 1) & 1]),
                                   half[j & 1], ctx->track_d.as<signed char>());
        }
        ProfScope ps(ctx, TDOA_K_TRACK_FINISH, (2.0 * sizeof(TrackPair) + 12.0) * (double)v.n_lags * n_sp);
        hipLaunchKernelGGL(k_track_finish, dim3(n_sp), dim3(kTrackThreads), 0, st, static_cast<const TrackPair *>(half[0]),
                           ctx->track_d.as<const signed char>(), ctx->surf.as<const float>(), (size_t)v.n_lags, v.n_lags, v.lag_lo, v.P,
                           v.d_pw, v.d_scales, v.slot_gain, sd.roots, tt, ctx->track_score.as<PeakOut>(), ctx->track_lags.as<int32_t>(),
                           ctx->track_values.as<double>(), ctx->stack_q.as<long long>(), ctx->stack_surf.as<float>());
    }
    int download(const StepView &v) const override
    {
        tdoa_ctx *ctx = v.ctx;
        hipStream_t st = ctx->stream;
        const int mm = layout.mm;
        const size_t n_sp = (size_t)layout.n_stacks * v.P;
        if (score_host) HIPCHK(ctx, hipMemcpyAsync(score_host, ctx->track_score.p, sizeof(PeakOut) * n_sp, hipMemcpyDeviceToHost, st));
        if (lags_host) HIPCHK(ctx, hipMemcpyAsync(lags_host, ctx->track_lags.p, sizeof(int32_t) * n_sp * mm, hipMemcpyDeviceToHost, st));
        if (values_host) HIPCHK(ctx, hipMemcpyAsync(values_host, ctx->track_values.p, sizeof(double) * n_sp * mm, hipMemcpyDeviceToHost, st));
        if (surface_host)
            HIPCHK(ctx, hipMemcpyAsync(surface_host, ctx->stack_surf.p, sizeof(float) * n_sp * v.n_lags, hipMemcpyDeviceToHost, st));
        if (total_host)
            HIPCHK(ctx, hipMemcpyAsync(total_host, ctx->stack_q.p, sizeof(int64_t) * n_sp * v.n_lags, hipMemcpyDeviceToHost, st));
        return TDOA_OK;
    }
};

}  // namespace
