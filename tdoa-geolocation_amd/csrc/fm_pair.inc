// fm_pair.inc -- the pair call: two host windows through one batch of two station-windows and one pair-window.
// Included by tdoa_mi355x.hip after fm_route.inc.

namespace {

// copy two host IQ windows into scratch and build 2 sw + 1 pw descriptors
// (corr_len1: samples of the first window the transforms see, <= n1; the descriptors with the full lengths follow at
// d_sw + 2 for K1 and its statistics)
int stage_pair_u8(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2,
                  SWDesc **d_sw, PWDesc **d_pw, size_t corr_len1)
{
    int rc;
    size_t b1 = (2 * n1 + 15) & ~(size_t)15;
    if ((rc = ensure(ctx, ctx->scratch_a, b1 + 2 * n2 + 16))) return rc;
    auto *base = ctx->scratch_a.as<uint8_t>();
    if (n1) HIPCHK(ctx, hipMemcpyAsync(base, iq1, 2 * n1, hipMemcpyHostToDevice, ctx->stream));
    if (n2) HIPCHK(ctx, hipMemcpyAsync(base + b1, iq2, 2 * n2, hipMemcpyHostToDevice, ctx->stream));
    SWDesc sw[4] = {{base, (int32_t)corr_len1, 0}, {base + b1, (int32_t)n2, 0}, {base, (int32_t)n1, 0}, {base + b1, (int32_t)n2, 0}};
    PWDesc pw = {0, 1, 0, (int32_t)corr_len1};
    if ((rc = ensure(ctx, ctx->sw_desc, sizeof(sw)))) return rc;
    if ((rc = ensure(ctx, ctx->pw_desc, sizeof(pw)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->sw_desc.p, sw, sizeof(sw), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->pw_desc.p, &pw, sizeof(pw), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // sw/pw are stack objects
    *d_sw = ctx->sw_desc.as<SWDesc>();
    *d_pw = ctx->pw_desc.as<PWDesc>();
    return TDOA_OK;
}

// What a pair call returns; every pointer may be nullptr, at least one output must be asked for.
struct PairOut {
    tdoa_peak *peak = nullptr;
    double *lags = nullptr;                  // [2 max_lag - 1]: lag d at d + max_lag - 1
    tdoa_fine_peak *fine = nullptr;          // with `gate`
    double gate = 0.0;
    int sel_k = 0, sel_sep = 0;              // sel_k > 0: also the sel_k strongest separate peaks of the lag array (peak_select.hpp)
    tdoa_peak *sel_peaks = nullptr;
    int32_t *sel_count = nullptr;
};

int fm_pair(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2, int max_lag, const PairOut &o)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (max_lag < 1 || (!o.peak && !o.lags && !o.fine && !o.sel_k)) return fail(ctx, TDOA_ERR_INVALID, "bad argument");
    if (n1 == 0 || n2 == 0) {   // processor.go:622-625 behaviour: (0, 0.0)
        if (o.sel_k) std::fill(o.sel_peaks, o.sel_peaks + o.sel_k, tdoa_peak{0, 0.0f, 0.0});
        if (o.sel_k && o.sel_count) *o.sel_count = 0;
        if (o.peak) *o.peak = tdoa_peak{0, 0.0f, 0.0};
        if (o.fine) *o.fine = tdoa_fine_peak{0.0, 0.0f, {0.0f, 0.0f, 0.0f}, o.gate >= 0.0 ? 1 : 0, 0};
        if (o.lags) std::fill(o.lags, o.lags + (2 * max_lag - 1), 0.0);
        return TDOA_OK;
    }
    if (n1 > 0x7fffffff / 2 || n2 > 0x7fffffff / 2) return fail(ctx, TDOA_ERR_UNSUPPORTED, "window too long");
    // TDOA_LAGS_GO: template = the shorter input (ties: the first), its first B corr_block samples, lags [0, eff)
    const bool go = ctx->prm.lag_mode == TDOA_LAGS_GO;
    if (go && o.fine) return fail(ctx, TDOA_ERR_UNSUPPORTED, "sub-sample refinement with TDOA_LAGS_GO");
    if (go && n2 < n1) {                                      // processor.go:650-655
        std::swap(iq1, iq2);
        std::swap(n1, n2);
    }
    const int nl = 2 * max_lag - 1;
    size_t corr_len = n1;
    int lag_lo = -(max_lag - 1), lag_hi = max_lag - 1;
    if (go) {
        const long long blocks = go_blocks((long long)n1, ctx->prm.corr_block);
        if (blocks == 0) {                                    // processor.go:708-717: no block, (0, 0.0)
            if (o.peak) *o.peak = tdoa_peak{0, 0.0f, 0.0};
            if (o.lags) std::fill(o.lags, o.lags + nl, 0.0);
            return TDOA_OK;
        }
        corr_len = (size_t)(blocks * ctx->prm.corr_block);
        const long long eff = std::max<long long>(1, std::min<long long>(max_lag, (long long)n2 - (long long)n1));   // :668-678
        lag_lo = 0;
        lag_hi = (int)eff - 1;
    }
    FftPlan pl;
    const long long n = choose_fft_size(ctx, (long long)std::max(n1, n2) + max_lag, lag_lo, lag_hi, ctx->knobs.zpad, &pl, &rc);
    if (rc) return fail(ctx, rc, "FFT size unsupported");
    ctx->plan = pl;            // tdoa_plan_info reports the plan of the last call, pair calls included
    ctx->plan_n = n;
    SWDesc *d_sw;
    PWDesc *d_pw;
    if ((rc = stage_pair_u8(ctx, iq1, n1, iq2, n2, &d_sw, &d_pw, corr_len))) return rc;
    if ((rc = ensure(ctx, ctx->keys, sizeof(unsigned long long)))) return rc;
    if ((rc = ensure(ctx, ctx->scales, sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->peaks, sizeof(PeakOut)))) return rc;
    if ((rc = ensure(ctx, ctx->slot_gain, sizeof(double)))) return rc;
    if (o.fine) {
        if ((rc = ensure(ctx, ctx->fine_raw, 3 * sizeof(float)))) return rc;
        if ((rc = ensure(ctx, ctx->fine, sizeof(FineOut)))) return rc;
    }
    const int n_dump = lag_hi - lag_lo + 1;                   // the kernels write lag d at dump[d - lag_lo]
    float *dump = nullptr;
    if (o.sel_k) {
        if ((rc = ensure(ctx, ctx->sel_peaks, sizeof(PeakOut) * o.sel_k))) return rc;
        if ((rc = ensure(ctx, ctx->sel_count, sizeof(int32_t)))) return rc;
    }
    if (o.lags || o.sel_k) {
        if ((rc = ensure(ctx, ctx->lagdump, sizeof(float) * (size_t)n_dump))) return rc;
        dump = ctx->lagdump.as<float>();
        HIPCHK(ctx, hipMemsetAsync(dump, 0, sizeof(float) * (size_t)n_dump, ctx->stream));
    }
    auto *keys = ctx->keys.as<unsigned long long>();
    const auto *scales = ctx->scales.as<const double>();
    float *fine_raw = o.fine ? ctx->fine_raw.as<float>() : nullptr;
    double scale = 1.0 / (4.0 * (double)n * std::sqrt((double)corr_len));
    HIPCHK(ctx, hipMemsetAsync(keys, 0, sizeof(unsigned long long), ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->scales.p, &scale, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ctx->prof_last = -1;
    FmBatchShape shape = batch_shape(ctx);
    shape.n_sw = 2;
    shape.n_pw = 1;
    shape.maxlen = (int)std::max(n1, n2);
    shape.allow_fused_k1 = n1 >= 2 && n2 >= 2 && corr_len >= 2;
    shape.separate_stats = corr_len != n1;
    shape.equal_len = n1 == n2 && corr_len == n1;
    shape.fine = o.fine != nullptr;
    const FmBufs bf{d_sw, shape.separate_stats ? d_sw + 2 : nullptr, d_pw, nullptr, keys, dump, 1.0f, (double)(n1 + n2), fine_raw};
    rc = run_fm_batch(ctx, shape, pl, lag_lo, lag_hi, bf);
    if (rc) return rc;
    launch_decode(ctx, keys, scales, 1, fine_raw, o.gate);
    const double *slot_gain = ctx->once_active ? ctx->slot_gain.as<const double>() : nullptr;
    tdoa_peak pk;
    HIPCHK(ctx, hipMemcpyAsync(&pk, ctx->peaks.p, sizeof(pk), hipMemcpyDeviceToHost, ctx->stream));
    tdoa_fine_peak fk;
    if (o.fine) HIPCHK(ctx, hipMemcpyAsync(&fk, ctx->fine.p, sizeof(fk), hipMemcpyDeviceToHost, ctx->stream));
    if (o.sel_k) {
        hipLaunchKernelGGL(k_select_peaks, dim3(1), dim3(kSelThreads), 0, ctx->stream, dump, (size_t)0, n_dump, lag_lo,
                           static_cast<const PWDesc *>(nullptr), keys, scales, slot_gain, o.sel_k, o.sel_sep,
                           ctx->sel_peaks.as<PeakOut>(), ctx->sel_count.as<int32_t>());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(o.sel_peaks, ctx->sel_peaks.p, sizeof(PeakOut) * o.sel_k, hipMemcpyDeviceToHost, ctx->stream));
        if (o.sel_count) HIPCHK(ctx, hipMemcpyAsync(o.sel_count, ctx->sel_count.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    double pair_gain = 1.0;                                   // single-look K1: the lag array lacks g_t g_s like the key does
    if (o.lags && slot_gain)
        HIPCHK(ctx, hipMemcpyAsync(&pair_gain, slot_gain, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float> hl;
    if (o.lags) {
        hl.resize(n_dump);
        HIPCHK(ctx, hipMemcpyAsync(hl.data(), dump, sizeof(float) * (size_t)n_dump, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    prof_collect(ctx);
    if (o.peak) *o.peak = pk;
    if (o.fine) *o.fine = fk;
    if (o.lags) {                                             // layout [2 max_lag - 1]: lag d at d + max_lag - 1
        std::fill(o.lags, o.lags + nl, 0.0);
        for (int i = 0; i < n_dump; i++) o.lags[i + lag_lo + (max_lag - 1)] = (double)hl[i] * scale * pair_gain;
    }
    return TDOA_OK;
}

}  // namespace

extern "C" {

int tdoa_fm_xcorr_u8(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2, int max_lag,
                     tdoa_peak *peak)
{
    if (!peak) return fail(ctx, TDOA_ERR_INVALID, "peak is NULL");
    PairOut o;
    o.peak = peak;
    return fm_pair(ctx, iq1, n1, iq2, n2, max_lag, o);
}

int tdoa_fm_xcorr_lags_u8(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2, int max_lag,
                          double *lags_out)
{
    if (!lags_out) return fail(ctx, TDOA_ERR_INVALID, "lags_out is NULL");
    PairOut o;
    o.lags = lags_out;
    return fm_pair(ctx, iq1, n1, iq2, n2, max_lag, o);
}

int tdoa_fm_xcorr_fine_u8(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2, int max_lag,
                          double gate_samples, tdoa_peak *peak, tdoa_fine_peak *fine)
{
    if (!fine || !(gate_samples >= 0.0)) return fail(ctx, TDOA_ERR_INVALID, "fine is NULL or gate < 0");
    PairOut o;
    o.peak = peak;
    o.fine = fine;
    o.gate = gate_samples;
    return fm_pair(ctx, iq1, n1, iq2, n2, max_lag, o);
}

int tdoa_fm_xcorr_peaks_u8(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2, int max_lag, int k,
                           int min_separation, tdoa_peak *peaks, int32_t *count)
{
    int rc;
    if ((rc = check_selection(ctx, k, min_separation, peaks))) return rc;
    PairOut o;
    o.sel_k = k;
    o.sel_sep = min_separation;
    o.sel_peaks = peaks;
    o.sel_count = count;
    return fm_pair(ctx, iq1, n1, iq2, n2, max_lag, o);
}

}  // extern "C"
