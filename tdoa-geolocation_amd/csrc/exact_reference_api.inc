// exact_reference_api.inc -- mode A entry points (host side of exact_reference.hpp).
// Included at the end of tdoa_mi355x.hip; uses its helpers (fail, ensure, HIPCHK, check_ctx).

namespace {

// processor.go:400-406: int(sampleRate / (2*cutoff)) clamped to [3, 1000]
int ex_cutoff_window(double cutoff, double fs)
{
    double w = fs / (2 * cutoff);
    int window = (w < 2147483647.0) ? (int)w : 2147483647;
    if (window < 3) window = 3;
    if (window > 1000) window = 1000;
    return window;
}

inline unsigned ex_grid(size_t n, unsigned per = 256) { return (unsigned)std::max<size_t>(1, (n + per - 1) / per); }

// applyLowPassFilter (mode 0) / applyHighPassFilter body (mode 1); in != out
int ex_moving_average(tdoa_ctx *ctx, const float2 *in, float2 *out, size_t n, int window, int mode)
{
    if (n == 0) return TDOA_OK;
    if (window <= 1) {   // processor.go:271-273 returns the input itself
        if (mode == 0) {
            HIPCHK(ctx, hipMemcpyAsync(out, in, n * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            HIPCHK(ctx, hipMemsetAsync(out, 0, n * sizeof(float2), ctx->stream));
        }
        return TDOA_OK;
    }
    const int half = window / 2;
    const int span = kMaTile + 2 * half;
    const size_t lds = sizeof(float2) * (size_t)(span + (span >> 3) + 2);
    hipLaunchKernelGGL(k_ex_moving_average, dim3(ex_grid(n, kMaTile)), dim3(kMaThreads), lds, ctx->stream, in,
                       (long long)n, half, out, mode);
    return TDOA_OK;
}

// applyBandpassFilter (processor.go:354-381): in -> out, tmp is scratch; in untouched
int ex_bandpass(tdoa_ctx *ctx, const float2 *in, float2 *out, float2 *tmp, size_t n, double lo, double hi, double fs)
{
    int rc;
    const bool hp = lo > 0, lp = hi < fs / 2;
    if (hp && lp) {
        if ((rc = ex_moving_average(ctx, in, tmp, n, ex_cutoff_window(lo, fs), 1))) return rc;
        return ex_moving_average(ctx, tmp, out, n, ex_cutoff_window(hi, fs), 0);
    }
    if (hp) return ex_moving_average(ctx, in, out, n, ex_cutoff_window(lo, fs), 1);
    if (lp) return ex_moving_average(ctx, in, out, n, ex_cutoff_window(hi, fs), 0);
    HIPCHK(ctx, hipMemcpyAsync(out, in, n * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
    return TDOA_OK;
}

// applyNotchFilter (processor.go:412-434): in -> out; t1, t2 scratch
int ex_notch(tdoa_ctx *ctx, const float2 *in, float2 *out, float2 *t1, float2 *t2, size_t n, double f0, double bw,
             double fs)
{
    double lo = f0 - bw / 2, hi = f0 + bw / 2;
    if (lo < 0) lo = 0;
    if (hi > fs / 2) hi = fs / 2;
    int rc = ex_bandpass(ctx, in, t2, t1, n, lo, hi, fs);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ex_notch_combine, dim3(ex_grid(n)), dim3(256), 0, ctx->stream, in, t2, n, out);
    return TDOA_OK;
}

// calculateSignalPower -> *d_power (device double)
int ex_power(tdoa_ctx *ctx, const float2 *sig, size_t n, double *d_partials, double *d_power)
{
    const int chunks = (int)std::max<size_t>(1, (n + kPowChunk - 1) / kPowChunk);
    hipLaunchKernelGGL(k_ex_power_partial, dim3(chunks), dim3(256), 0, ctx->stream, sig, n, d_partials);
    hipLaunchKernelGGL(k_ex_power_final, dim3(1), dim3(256), 0, ctx->stream, d_partials, chunks, n, d_power);
    return TDOA_OK;
}

struct ExWork {
    float2 *a, *b, *c, *d;
    double *partials, *power;
    float2 *mean;
};

int ex_prepare(tdoa_ctx *ctx, size_t n, ExWork *w)
{
    int rc;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(float2);
    if ((rc = ensure(ctx, ctx->ex_a, bytes))) return rc;
    if ((rc = ensure(ctx, ctx->ex_b, bytes))) return rc;
    if ((rc = ensure(ctx, ctx->ex_c, bytes))) return rc;
    if ((rc = ensure(ctx, ctx->ex_d, bytes))) return rc;
    const size_t chunks = (n + kPowChunk - 1) / kPowChunk + 1;
    if ((rc = ensure(ctx, ctx->ex_part, sizeof(double) * (chunks + 8)))) return rc;
    w->a = ctx->ex_a.as<float2>();
    w->b = ctx->ex_b.as<float2>();
    w->c = ctx->ex_c.as<float2>();
    w->d = ctx->ex_d.as<float2>();
    w->power = ctx->ex_part.as<double>();
    w->mean = reinterpret_cast<float2 *>(w->power + 2);
    w->partials = w->power + 8;
    return TDOA_OK;
}

// preprocessSignal (processor.go:469-499) on device data: src -> dst (both n complex64)
// mean_ready: device pointer to the DC mean of src when the caller has already run k_ex_seq_sum (the two
// signals of a crossCorrelate run their sequential chains side by side), else nullptr
int ex_preprocess(tdoa_ctx *ctx, const float2 *src, float2 *dst, size_t n, int *weak_out,
                  const float2 *mean_ready = nullptr)
{
    int rc;
    ExWork w;
    if ((rc = ex_prepare(ctx, n, &w))) return rc;
    hipStream_t st = ctx->stream;
    const double fs = ctx->prm.sample_rate;
    double p0 = 0.0;
    if (n) {
        if ((rc = ex_power(ctx, src, n, w.partials, w.power))) return rc;
        HIPCHK(ctx, hipMemcpyAsync(&p0, w.power, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    const bool weak = p0 < ctx->prm.weak_threshold;          // :476
    if (weak_out) *weak_out = weak ? 1 : 0;
    if (n == 0) return TDOA_OK;
    // removeDCBias: src -> a
    if (!mean_ready) {
        const SeqSumJob job{src, n, w.mean};
        hipLaunchKernelGGL(k_ex_seq_sum, dim3(1), dim3(64), 0, st, job, job);
        mean_ready = w.mean;
    }
    hipLaunchKernelGGL(k_ex_sub_const, dim3(ex_grid(n)), dim3(256), 0, st, src, n, mean_ready, w.a);
    float2 *last;
    if (weak) {                                              // enhanceWeakSignal :437-466
        if ((rc = ex_notch(ctx, w.a, w.b, w.c, w.d, n, 60, 5, fs))) return rc;               // :446
        if ((rc = ex_notch(ctx, w.b, w.a, w.c, w.d, n, 120, 5, fs))) return rc;              // :447
        if ((rc = ex_notch(ctx, w.a, w.b, w.c, w.d, n, 1000000, 50000, fs))) return rc;      // :448
        if ((rc = ex_bandpass(ctx, w.b, w.a, w.c, n, 100.0, 40000.0, fs))) return rc;        // :453-457
        if ((rc = ex_moving_average(ctx, w.a, w.b, n, 50, 0))) return rc;                    // :460
        last = w.b;
    } else {                                                 // :484-497
        if ((rc = ex_bandpass(ctx, w.a, w.b, w.c, n, 500, 50000, fs))) return rc;            // :489
        if ((rc = ex_moving_average(ctx, w.b, w.a, n, 100, 0))) return rc;                   // :492
        last = w.a;
    }
    if ((rc = ex_power(ctx, last, n, w.partials, w.power))) return rc;                       // normalizeSignal
    hipLaunchKernelGGL(k_ex_scale, dim3(ex_grid(n)), dim3(256), 0, st, last, n, w.power, dst);
    HIPCHK(ctx, hipGetLastError());
    return TDOA_OK;
}

// timeDomainCorrelation (processor.go:646-736) on device data
int ex_tdc(tdoa_ctx *ctx, const float2 *d1, size_t n1, const float2 *d2, size_t n2, int max_lag, int32_t *delay,
           double *corr)
{
    int rc;
    const float2 *tpl = d1, *sig = d2;
    long long tl = (long long)n1, sl = (long long)n2;
    if (n1 > n2) { tpl = d2; tl = (long long)n2; sig = d1; sl = (long long)n1; }   // :650-655
    long long ml = max_lag;
    if (ml > sl - tl) ml = sl - tl;                                                // :668-670
    if (ml < 1) ml = 1;                                                            // :673-675
    const int block = ctx->prm.corr_block;                                         // :682
    const long long nb = tl > block ? (tl - block + block - 1) / block : 0;        // blockStart < tl - block
    *delay = 0;
    *corr = 0.0;
    if (nb == 0) return TDOA_OK;                                                   // numBlocks == 0 for every lag
    if (nb > 0x7fffffff / 4 || (size_t)block * sizeof(float2) * 2 + kTdcLags * sizeof(float2) > 60000)
        return fail(ctx, TDOA_ERR_UNSUPPORTED, "correlation geometry unsupported");
    if ((rc = ensure(ctx, ctx->scratch_b, sizeof(double) * (size_t)nb * (size_t)ml))) return rc;
    if ((rc = ensure(ctx, ctx->lagdump, sizeof(double) * (size_t)ml + sizeof(ExPeak)))) return rc;
    auto *bc = ctx->scratch_b.as<double>();
    auto *cv = ctx->lagdump.as<double>();
    auto *pk = reinterpret_cast<ExPeak *>(cv + ml);
    hipStream_t st = ctx->stream;
    if (ml >= 64) {
        const size_t lds = sizeof(float2) * (size_t)(2 * block + kTdcLags);
        hipLaunchKernelGGL(k_ex_tdc_blocks, dim3((unsigned)((ml + kTdcLags - 1) / kTdcLags), (unsigned)nb),
                           dim3(kTdcLags), lds, st, tpl, sig, sl, block, (int)ml, bc);
    } else {
        const long long waves = nb * ml;
        hipLaunchKernelGGL(k_ex_tdc_blocks_few, dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0, st, tpl, sig,
                           block, (int)ml, (int)nb, bc);
    }
    hipLaunchKernelGGL(k_ex_tdc_finalize, dim3((unsigned)((ml + 255) / 256)), dim3(256), 0, st, bc, (int)nb, (int)ml,
                       block, cv);
    hipLaunchKernelGGL(k_ex_first_max, dim3(1), dim3(256), 0, st, cv, (int)ml, pk);
    HIPCHK(ctx, hipGetLastError());
    ExPeak h;
    HIPCHK(ctx, hipMemcpyAsync(&h, pk, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    *delay = h.delay;
    *corr = h.corr;
    return TDOA_OK;
}

int ex_upload_c64(tdoa_ctx *ctx, DevBuf &buf, const float *host, size_t n, float2 **dev)
{
    int rc = ensure(ctx, buf, std::max<size_t>(n, 1) * sizeof(float2));
    if (rc) return rc;
    if (n) HIPCHK(ctx, hipMemcpyAsync(buf.p, host, n * sizeof(float2), hipMemcpyHostToDevice, ctx->stream));
    *dev = static_cast<float2 *>(buf.p);
    return TDOA_OK;
}

}  // namespace

extern "C" {

int tdoa_load_iq_u8(tdoa_ctx *ctx, const uint8_t *raw, size_t n, float *out_c64)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if ((!raw || !out_c64) && n) return fail(ctx, TDOA_ERR_INVALID, "NULL buffer");
    if (n == 0) return TDOA_OK;
    if ((rc = ensure(ctx, ctx->scratch_a, 2 * n))) return rc;
    if ((rc = ensure(ctx, ctx->tz, n * sizeof(float2)))) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->scratch_a.p, raw, 2 * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ex_u8_to_c64, dim3(ex_grid(n)), dim3(256), 0, st, ctx->scratch_a.as<uint8_t>(), n,
                       ctx->tz.as<float2>());
    HIPCHK(ctx, hipMemcpyAsync(out_c64, ctx->tz.p, n * sizeof(float2), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return TDOA_OK;
}

int tdoa_preprocess_c64(tdoa_ctx *ctx, const float *sig, size_t n, float *out_c64, int *weak_chain)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if ((!sig || !out_c64) && n) return fail(ctx, TDOA_ERR_INVALID, "NULL buffer");
    float2 *src, *dst;
    if ((rc = ex_upload_c64(ctx, ctx->scratch_a, sig, n, &src))) return rc;
    if ((rc = ensure(ctx, ctx->tz, std::max<size_t>(n, 1) * sizeof(float2)))) return rc;
    dst = ctx->tz.as<float2>();
    if ((rc = ex_preprocess(ctx, src, dst, n, weak_chain))) return rc;
    if (n) HIPCHK(ctx, hipMemcpyAsync(out_c64, dst, n * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TDOA_OK;
}

int tdoa_time_domain_correlation_c64(tdoa_ctx *ctx, const float *s1, size_t n1, const float *s2, size_t n2,
                                     int max_lag, int32_t *delay, double *corr)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!delay || !corr || (!s1 && n1) || (!s2 && n2)) return fail(ctx, TDOA_ERR_INVALID, "NULL buffer");
    float2 *d1, *d2;
    if ((rc = ex_upload_c64(ctx, ctx->tz, s1, n1, &d1))) return rc;
    if ((rc = ex_upload_c64(ctx, ctx->v, s2, n2, &d2))) return rc;
    return ex_tdc(ctx, d1, n1, d2, n2, max_lag, delay, corr);
}

int tdoa_cross_correlate_c64(tdoa_ctx *ctx, const float *s1, size_t n1, const float *s2, size_t n2, int32_t *delay,
                             double *corr)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!delay || !corr || (!s1 && n1) || (!s2 && n2)) return fail(ctx, TDOA_ERR_INVALID, "NULL buffer");
    *delay = 0;
    *corr = 0.0;
    if (n1 == 0 || n2 == 0) return TDOA_OK;                  // processor.go:622-625
    float2 *src, *p1, *p2;
    if ((rc = ensure(ctx, ctx->tz, n1 * sizeof(float2)))) return rc;
    if ((rc = ensure(ctx, ctx->v, n2 * sizeof(float2)))) return rc;
    p1 = ctx->tz.as<float2>();
    p2 = ctx->v.as<float2>();
    float2 *src2;
    if ((rc = ex_upload_c64(ctx, ctx->scratch_a, s1, n1, &src))) return rc;
    if ((rc = ex_upload_c64(ctx, ctx->scratch_b, s2, n2, &src2))) return rc;
    // removeDCBias of both signals: two independent sequential chains, one wave each, side by side
    ExWork w;
    if ((rc = ex_prepare(ctx, std::max(n1, n2), &w))) return rc;         // sized once: the mean slots must not move
    hipLaunchKernelGGL(k_ex_seq_sum, dim3(2), dim3(64), 0, ctx->stream, SeqSumJob{src, n1, w.mean},
                       SeqSumJob{src2, n2, w.mean + 1});
    if ((rc = ex_preprocess(ctx, src, p1, n1, nullptr, w.mean))) return rc;        // :629
    if ((rc = ex_preprocess(ctx, src2, p2, n2, nullptr, w.mean + 1))) return rc;   // :630
    return ex_tdc(ctx, p1, n1, p2, n2, ctx->prm.max_lag, delay, corr);   // :633-636
}

// The reference's pair loop (processor.go:816-830 for the reference blocks, :836-850 for the target blocks) in one call.
// crossCorrelate preprocesses BOTH its inputs on every call (:629-630), so a station's signal goes through the O(N W)
// filter chain once per pair it is in -- 12 times for 3 stations x 2 signal kinds where 6 are different.  Here every
// signal is preprocessed once and kept in HBM, then each pair i < j is correlated: same kernels on the same data, so
// (delay, corr) are bit-identical to tdoa_cross_correlate_c64 pair by pair.
int tdoa_cross_correlate_batch_c64(tdoa_ctx *ctx, const float *const *signals, const size_t *n, int n_signals,
                                   int32_t *delay, double *corr)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!signals || !n || n_signals < 2 || n_signals > 64 || !delay || !corr) return fail(ctx, TDOA_ERR_INVALID, "bad argument");
    size_t total = 0, nmax = 0;
    std::vector<size_t> off(n_signals);
    for (int s = 0; s < n_signals; s++) {
        if (!signals[s] && n[s]) return fail(ctx, TDOA_ERR_INVALID, "NULL signal");
        off[s] = total;
        total += n[s];
        nmax = std::max(nmax, n[s]);
    }
    const int P = n_signals * (n_signals - 1) / 2;
    for (int p = 0; p < P; p++) { delay[p] = 0; corr[p] = 0.0; }
    if (total == 0) return TDOA_OK;
    // raw signals in tz, preprocessed ones in v, one DC-mean slot per signal behind them
    if ((rc = ensure(ctx, ctx->tz, total * sizeof(float2)))) return rc;
    if ((rc = ensure(ctx, ctx->v, (total + (size_t)n_signals + 2) * sizeof(float2)))) return rc;
    float2 *raw = ctx->tz.as<float2>(), *pre = ctx->v.as<float2>();
    float2 *means = pre + total;
    for (int s = 0; s < n_signals; s++)
        if (n[s])
            HIPCHK(ctx, hipMemcpyAsync(raw + off[s], signals[s], n[s] * sizeof(float2), hipMemcpyHostToDevice, ctx->stream));
    ExWork w;
    if ((rc = ex_prepare(ctx, nmax, &w))) return rc;                     // sized once: nothing may move below
    // removeDCBias: the sequential chains of two signals run side by side (one wave each)
    for (int s = 0; s < n_signals; s += 2) {
        const int t = s + 1 < n_signals ? s + 1 : s;
        hipLaunchKernelGGL(k_ex_seq_sum, dim3(t == s ? 1 : 2), dim3(64), 0, ctx->stream, SeqSumJob{raw + off[s], n[s], means + s},
                           SeqSumJob{raw + off[t], n[t], means + t});
    }
    for (int s = 0; s < n_signals; s++)
        if (n[s] && (rc = ex_preprocess(ctx, raw + off[s], pre + off[s], n[s], nullptr, means + s))) return rc;
    int p = 0;
    for (int i = 0; i < n_signals; i++)
        for (int j = i + 1; j < n_signals; j++, p++) {
            if (n[i] == 0 || n[j] == 0) continue;                       // processor.go:622-625: (0, 0.0)
            if ((rc = ex_tdc(ctx, pre + off[i], n[i], pre + off[j], n[j], ctx->prm.max_lag, &delay[p], &corr[p]))) return rc;
        }
    return TDOA_OK;
}

int tdoa_simple_correlate_c64(tdoa_ctx *ctx, const float *s1, size_t n1, const float *s2, size_t n2, int32_t *delay,
                              float *corr)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!delay || !corr || (!s1 && n1) || (!s2 && n2)) return fail(ctx, TDOA_ERR_INVALID, "NULL buffer");
    *delay = 0;
    *corr = 0.0f;
    if (n1 == 0 || n2 == 0) return TDOA_OK;                  // simple_corr.go:84-86
    float2 *d1, *d2;
    if ((rc = ex_upload_c64(ctx, ctx->tz, s1, n1, &d1))) return rc;
    if ((rc = ex_upload_c64(ctx, ctx->v, s2, n2, &d2))) return rc;
    const float2 *tpl = d1, *sig = d2;
    long long tl = (long long)n1, sl = (long long)n2;
    if (n1 > n2) { tpl = d2; tl = (long long)n2; sig = d1; sl = (long long)n1; }
    long long ml = 1000;                                      // simple_corr.go:96
    if (ml > sl - tl) ml = sl - tl;
    if (ml < 1) ml = 1;
    if ((rc = ensure(ctx, ctx->lagdump, sizeof(SimpleLag) * (size_t)ml + 16))) return rc;
    auto *lags = ctx->lagdump.as<SimpleLag>();
    auto *tp = reinterpret_cast<float *>(lags + ml);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_ex_seq_power_f32, dim3(1), dim3(64), 0, st, tpl, (size_t)tl, tp);
    hipLaunchKernelGGL(k_ex_simple_corr, dim3((unsigned)((ml + 255) / 256)), dim3(256), 0, st, tpl, tl, sig, sl, (int)ml,
                       lags);
    HIPCHK(ctx, hipGetLastError());
    std::vector<SimpleLag> h((size_t)ml);
    float tpow = 0.0f;
    HIPCHK(ctx, hipMemcpyAsync(h.data(), lags, sizeof(SimpleLag) * (size_t)ml, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(&tpow, tp, sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    int best_delay = 0;
    float best = 0.0f;
    for (long long d = 0; d < ml; d++) {                     // simple_corr.go:145-156
        const float sp = h[(size_t)d].spow;
        if (tpow > 0 && sp > 0) {
            const float a = (float)std::sqrt((double)tpow);
            const float b = (float)std::sqrt((double)sp);
            const float den = a * b;
            const float nc = h[(size_t)d].corr / den;
            if (std::fabs((double)nc) > std::fabs((double)best)) {
                best = nc;
                best_delay = (int)d;
            }
        }
    }
    *delay = best_delay;
    *corr = best;
    return TDOA_OK;
}

int tdoa_fast_snr_u8(tdoa_ctx *ctx, const uint8_t *samples, int total, double *snr_db)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!snr_db || (!samples && total > 0)) return fail(ctx, TDOA_ERR_INVALID, "NULL buffer");
    *snr_db = -20.0;                                         // fast_analyzer.go:226
    int asz = 8192;                                          // :165
    if (total < asz) asz = total;
    if (asz <= 0) return TDOA_OK;
    const int start = (total - asz) / 2;                     // :171
    const uint8_t *ab = samples + (size_t)start * 2;
    std::vector<double> x((size_t)asz * 2), tw((size_t)asz * 2), ft((size_t)asz * 2);
    for (int i = 0; i < asz; i++) {                          // :176-186 conversion + Hann window
        const double re = ((double)ab[2 * i] - 127.5) / 127.5;
        const double im = ((double)ab[2 * i + 1] - 127.5) / 127.5;
        const double w = 0.5 - 0.5 * std::cos(2 * geo::kPi * (double)i / (double)(asz - 1));
        const double zr = 0.0 * im, zi = 0.0 * re;
        x[2 * i] = w * re - zr;
        x[2 * i + 1] = w * im + zi;
    }
    for (int k = 0; k < asz; k++) {                          // :239-242 twiddle table
        const double angle = -2 * geo::kPi * (double)k / (double)asz;
        volatile double angle_s = angle;   // keep cos() and sin() separate libm calls (no sincos merge)
        tw[2 * k] = std::cos(angle);
        tw[2 * k + 1] = std::sin(angle_s);
    }
    const size_t bytes = sizeof(double) * 2 * (size_t)asz;
    if ((rc = ensure(ctx, ctx->ex_a, bytes))) return rc;
    if ((rc = ensure(ctx, ctx->ex_b, bytes))) return rc;
    if ((rc = ensure(ctx, ctx->ex_c, bytes))) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->ex_a.p, x.data(), bytes, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->ex_b.p, tw.data(), bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ex_fast_dft, dim3((asz + 255) / 256), dim3(256), 0, st, ctx->ex_a.as<double2>(),
                       ctx->ex_b.as<double2>(), asz, ctx->ex_c.as<double2>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ft.data(), ctx->ex_c.p, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    std::vector<double> psd((size_t)asz), sorted;
    for (int i = 0; i < asz; i++) {                          // :192-195 |X|^2 via hypot
        double p = std::fabs(ft[2 * i]), q = std::fabs(ft[2 * i + 1]);
        if (p < q) std::swap(p, q);
        double a = 0.0;
        if (p != 0) {
            q = q / p;
            a = p * std::sqrt(1 + q * q);
        }
        psd[(size_t)i] = a * a;
    }
    sorted = psd;
    std::sort(sorted.begin(), sorted.end(), [](double u, double v) { return u < v; });
    const double sig_thr = sorted[(size_t)(int)(0.9 * (double)asz)];      // :203-204
    const double noise_thr = sorted[(size_t)(int)(0.4 * (double)asz)];
    double sp = 0, np = 0;
    int sc = 0, nc = 0;
    for (int i = 0; i < asz; i++) {
        if (psd[(size_t)i] >= sig_thr) { sp += psd[(size_t)i]; sc++; }
        else if (psd[(size_t)i] <= noise_thr) { np += psd[(size_t)i]; nc++; }
    }
    if (sc > 0) sp /= (double)sc;
    if (nc > 0) np /= (double)nc;
    if (np > 0 && sp > np) *snr_db = 10 * std::log10(sp / np);
    return TDOA_OK;
}

int tdoa_fast_analyze_u8(tdoa_ctx *ctx, const uint8_t *s, int total, tdoa_fast_analysis *out)
{
    if (!out || (!s && total > 0) || total < 0) return fail(ctx, TDOA_ERR_INVALID, "bad argument");
    std::memset(out, 0, sizeof(*out));
    out->total_samples = total;
    // fast_analyzer.go:117-155: the byte statistics come from the device pass (exact integer sums, the same
    // float64 values as the reference's running sums), the few f64 operations after them from finalize_quality
    if (total == 0) {   // 0/0 in the reference: NaN averages, no flags from extremes
        out->i_avg = out->q_avg = out->i_std = out->q_std = std::nan("");
        out->power_level = 20 * std::log10(std::nan(""));
        return tdoa_fast_snr_u8(ctx, s, total, &out->snr_estimate);
    }
    tdoa_window_quality wq;
    if (int rc = tdoa_window_quality_u8(ctx, s, (size_t)total, &wq)) return rc;
    out->i_avg = wq.i_avg;
    out->q_avg = wq.q_avg;
    out->i_std = wq.i_std;
    out->q_std = wq.q_std;
    out->power_level = wq.power_level;                                                    // :146-151
    out->has_clipping = wq.has_clipping;                                                  // :154
    out->has_overload = wq.has_overload;                                                  // :155
    return tdoa_fast_snr_u8(ctx, s, total, &out->snr_estimate);                           // :158
}

int tdoa_fast_analyze_capture_u8(tdoa_ctx *ctx, const uint8_t *raw, size_t n_bytes, tdoa_fast_analysis *ref,
                                 tdoa_fast_analysis *tgt)
{
    if (!raw || !ref || !tgt) return fail(ctx, TDOA_ERR_INVALID, "NULL buffer");
    const long long total = (long long)(n_bytes / 2), bs = total / 3;      // :66-71
    if (bs == 0) return fail(ctx, TDOA_ERR_INVALID, "file too small for dual-frequency analysis");
    const long long asz = std::min<long long>(32768, bs);                  // :77-81
    std::vector<uint8_t> rb((size_t)asz * 4), tb((size_t)asz * 2);
    std::memcpy(rb.data(), raw, (size_t)asz * 2);                                          // block 1
    std::memcpy(rb.data() + asz * 2, raw + bs * 2 * 2, (size_t)asz * 2);                   // block 3
    std::memcpy(tb.data(), raw + bs * 2, (size_t)asz * 2);                                 // block 2
    int rc = tdoa_fast_analyze_u8(ctx, rb.data(), (int)(asz * 2), ref);                    // :106
    if (rc) return rc;
    return tdoa_fast_analyze_u8(ctx, tb.data(), (int)asz, tgt);                            // :107
}

}  // extern "C"
