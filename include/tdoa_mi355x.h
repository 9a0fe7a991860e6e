/*
 * tdoa_mi355x.h -- C ABI of the MI355X-native TDOA correlation processor.
 *
 * Drop-in boundary for the correlation hot path of KX0U-Jim/tdoa-geolocation
 * (processor.go / simple_corr.go / fast_analyzer.go).  The reference has no FFI
 * today: every entry point below replaces a Go function that a cgo shim would
 * forward to (INTEGRATION.md shows the shim).  Citations are file:line in the
 * reference.  Plain pointers and sizes only; no C++/torch types.
 *
 * Data layouts (identical to the reference's):
 *   complex64 signal  = n x {float re, float im} interleaved   (Go []complex64)
 *   IQ capture bytes  = n x {uint8 I, uint8 Q} centred at 127.5 (.dat files,
 *                       librtlsdr-2freq/src/rtl_sdr.c:103-146), three equal
 *                       blocks [f1 | f2 | f1]
 *   delay             = samples, relative to the shorter input as template
 *
 * Ownership: the caller owns every pointer it passes; the library copies what
 * it needs during the call and keeps no host pointer afterwards (cgo rule).
 * A context is single-caller; use one context per GPU.  Every function
 * returns a status code (0 = TDOA_OK) and never aborts the host process.
 */
#ifndef TDOA_MI355X_H
#define TDOA_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDOA_ABI_VERSION 4

typedef struct tdoa_ctx tdoa_ctx;

enum {
    TDOA_OK = 0,
    TDOA_ERR_INVALID = 1,     /* bad argument                                  */
    TDOA_ERR_NO_DEVICE = 2,   /* no usable HIP device (no CPU fallback exists) */
    TDOA_ERR_HIP = 3,         /* a HIP runtime call failed (tdoa_last_error)   */
    TDOA_ERR_NOMEM = 4,
    TDOA_ERR_UNSUPPORTED = 5, /* size outside the supported range              */
    TDOA_ERR_STATE = 6,       /* call order (e.g. process before upload)       */
    TDOA_ERR_SINGULAR = 7     /* solver: singular Jacobian (processor.go:997-999) */
};

/* The constants the reference hard-codes, as parameters. */
typedef struct {
    double  sample_rate;     /* 2e6     processor.go:440,488,821,841            */
    int32_t max_lag;         /* 20000   processor.go:633                        */
    int32_t corr_block;      /* 1000    processor.go:682                        */
    double  weak_threshold;  /* 0.001   processor.go:476                        */
    int64_t window_len;      /* 2000000 processor.go:772 (testChunkSize)        */
    int32_t device;          /* HIP device ordinal                              */
    int32_t windows_per_batch; /* station-windows processed per launch group; 0 = auto */
    int32_t k1_smooth;       /* 0 (default): none.  W > 1: centred moving average of W samples (half-window W/2, edges
                                truncated: applyLowPassFilter, processor.go:270-296) on the discriminator output before
                                it is normalised -- the prebuilt reference binary's strong-signal chain is discriminator
                                -> removeDCBias -> applyLowPassFilter(10) -> normalizeSignal */
    int32_t k1_gate;         /* 0 (default): every window through the discriminator (the north-star pipeline).
                                1: the prebuilt reference binary's power gate (preprocessSignal):
                                a station-window whose mean power, mean |(b - 127.5)/127.5|^2, is <= 0.01 takes
                                envelope |x| -> removeDCBias -> normalizeSignal instead of the discriminator chain (and is
                                not smoothed).  The binary's third branch (<= 0.001: band-passed complex samples) has no
                                mode-B counterpart; such windows take the envelope too -- tdoa_window_quality_all
                                reports every window's mean power */
    int32_t lag_mode;        /* which lags mode B searches (K5):
                                TDOA_LAGS_SIGNED (0, default): -max_lag < lag < max_lag, template = the first input, peak =
                                largest |corr|, ties -> smaller |lag|, then the positive lag;
                                TDOA_LAGS_GO (1): the lag set and peak rule of timeDomainCorrelation (processor.go:646-736):
                                template = the SHORTER input (ties: the first, :650-655), only its first B corr_block samples
                                count (B = number of block starts 0, corr_block, ... below Lt - corr_block, :691; B = 0 gives
                                (0, 0.0)), lags 0 <= lag < max(1, min(max_lag, Ls - Lt)) (:668-678), first strictly larger
                                |corr| wins = the lowest lag among equals (:722-725), corr scaled by 1/sqrt(B corr_block)
                                (:719-720).  Windows of tdoa_process have equal lengths: lag 0 only, as in the reference's
                                own call pattern.  Not available with the sub-sample refinement (TDOA_ERR_UNSUPPORTED). */
    int32_t reserved;        /* 0 */
} tdoa_params;

enum { TDOA_LAGS_SIGNED = 0, TDOA_LAGS_GO = 1 };

/* One correlation peak.  lag > 0: the second station of the pair lags the first. */
typedef struct {
    int32_t lag;        /* samples                                           */
    float   abs_corr;   /* |corr| as float (sort/weight key)                 */
    double  corr;       /* signed, reference scale sum/sqrt(n_template)      */
} tdoa_peak;

/* Exact statistics of one FM-discriminated window (mode B preprocessing).  The discriminator output is held as an
 * integer phase code in units of pi/2^23 (-2^23 < code <= 2^23: exact in a float). */
typedef struct {
    int64_t  s1;              /* sum of the codes                                              */
    uint64_t s2_lo, s2_hi;    /* sum of code^2 (128 bits: code^2 < 2^46 per sample)             */
    float    mean, scale;     /* f32(s1 / n); f32(1 / sqrt(variance)), 1 if the variance is 0   */
} tdoa_fm_stats;

/* ---- lifecycle ------------------------------------------------------------ */
void        tdoa_default_params(tdoa_params *p);
int         tdoa_create(const tdoa_params *p, tdoa_ctx **out);
void        tdoa_destroy(tdoa_ctx *ctx);
const char *tdoa_strerror(int status);
const char *tdoa_last_error(const tdoa_ctx *ctx);   /* detail of the last failure */
int         tdoa_abi_version(void);
int         tdoa_device_count(void);

/* ---- mode A: the reference's executed call surface -------------------------
 * Bit-faithful GPU evaluation of the Go functions (same filters, same
 * accumulation order where the Go order is observable).                      */

/* processor.go:166-205 loadIQData conversion: (float32(b)-127.5)/127.5 */
int tdoa_load_iq_u8(tdoa_ctx *ctx, const uint8_t *raw, size_t n_samples, float *out_c64);

/* processor.go:469-499 preprocessSignal (power gate, filter chains, normalise);
 * *weak_chain receives 1 if enhanceWeakSignal (:437) was taken. */
int tdoa_preprocess_c64(tdoa_ctx *ctx, const float *sig, size_t n, float *out_c64, int *weak_chain);

/* processor.go:646-736 timeDomainCorrelation(signal1, signal2, maxLag) -> (delay, corr) */
int tdoa_time_domain_correlation_c64(tdoa_ctx *ctx, const float *s1, size_t n1,
                                     const float *s2, size_t n2, int max_lag,
                                     int32_t *delay, double *corr);

/* processor.go:619-643 crossCorrelate(signal1, signal2) -> (delay, corr):
 * the station-pair call surface (callers :818, :838, correlation_sanity.go:50,55).
 * Empty input returns TDOA_OK with (0, 0.0) like the reference (:622-625). */
int tdoa_cross_correlate_c64(tdoa_ctx *ctx, const float *s1, size_t n1,
                             const float *s2, size_t n2,
                             int32_t *delay, double *corr);
/* the reference's pair loop (processor.go:816-830, :836-850) in one call: every signal goes through
 * preprocessSignal ONCE (crossCorrelate re-does it for every pair a station is in, :629-630), then each pair
 * i < j is correlated; delay[p], corr[p] in the reference's pair order, bit-identical to per-pair calls */
int tdoa_cross_correlate_batch_c64(tdoa_ctx *ctx, const float *const *signals, const size_t *n_samples, int n_signals,
                                   int32_t *delay, double *corr);

/* simple_corr.go:83-160 simpleCorrelate -> (delay, float32 corr) */
int tdoa_simple_correlate_c64(tdoa_ctx *ctx, const float *s1, size_t n1,
                              const float *s2, size_t n2,
                              int32_t *delay, float *corr);

/* fast_analyzer.go:163-227 fastSNRCalculation(samples, totalSamples) -> dB */
int tdoa_fast_snr_u8(tdoa_ctx *ctx, const uint8_t *samples, int total_samples, double *snr_db);

/* fast_analyzer.go:15-24 FastAnalysis / :113-161 fastAnalyzeSamples */
typedef struct {
    int32_t total_samples;
    int32_t has_clipping;     /* any I or Q byte equal to 0 or 255 (:154) */
    int32_t has_overload;     /* I or Q standard deviation below 2 (:155)  */
    int32_t reserved;
    double  i_avg, q_avg, i_std, q_std;
    double  snr_estimate;     /* dB, fastSNRCalculation                    */
    double  power_level;      /* 20*log10(sqrt(i_std^2+q_std^2)), floor -100 (:146-151) */
} tdoa_fast_analysis;
int tdoa_fast_analyze_u8(tdoa_ctx *ctx, const uint8_t *samples, int total_samples, tdoa_fast_analysis *out);
/* fast_analyzer.go:53-111 fastAnalyzeDualFrequencyFile on capture bytes in memory: the first 32768
 * samples of blocks 1 and 3 -> ref, of block 2 -> tgt; TDOA_ERR_INVALID if the capture has < 3 samples */
int tdoa_fast_analyze_capture_u8(tdoa_ctx *ctx, const uint8_t *raw, size_t n_bytes,
                                 tdoa_fast_analysis *ref, tdoa_fast_analysis *tgt);

/* ---- mode B: the north-star pipeline ---------------------------------------
 * u8 IQ -> FM discriminator -> Stockham FFT -> conj-multiply -> inverse FFT
 * -> argmax, batched over (station, window) and (pair, window).
 *
 * A capture is 3 blocks of n = floor(total/3) samples (each capture its own
 * n, as processor.go:214 does per file).  Windows of window_len samples tile
 * each block from its start; the window grid comes from the shortest capture:
 * windows_per_block = max(1, n_min / window_len) (a block shorter than
 * window_len is one window of n_min samples).
 * Window id wid = block * windows_per_block + w; block 1 is the target
 * frequency, blocks 0 and 2 the reference frequency (processor.go:211-233).
 * Pairs are ordered i<j as in processor.go:816-850.                          */

/* copy one station's capture into HBM (ctx-owned).  A few host threads stage the bytes through pinned
 * buffers onto their own copy streams (about 40 GB/s from pageable memory against 15 GB/s for one
 * hipMemcpy); a station's previous buffer is reused when the new capture fits, so repeated
 * uploads of equal-sized captures keep their device addresses (TDOA_UPLOAD_THREADS overrides 4). */
int tdoa_capture_upload(tdoa_ctx *ctx, int station, const uint8_t *iq, size_t n_samples);
/* sharded ingest: upload only samples [first_sample, first_sample + n_samples) of a capture of total_samples -- a rank
 * of a multi-GPU job calls it once per run of windows it owns (tdoa_process(rank, world) reads nothing else), so the
 * host-to-device traffic of a G-rank job is 1/G of the capture per rank instead of all of it */
int tdoa_capture_upload_range(tdoa_ctx *ctx, int station, size_t total_samples, size_t first_sample, const uint8_t *iq,
                              size_t n_samples);
/* the same from a .dat file (collector.go:61 naming, raw u8 I,Q; any size, > 1 GiB safe): the threads
 * pread their chunks straight into the pinned buffers;
 * *n_samples (may be NULL) receives size/2 like processor.go:182 */
int tdoa_capture_upload_file(tdoa_ctx *ctx, int station, const char *path, size_t *n_samples);
/* or attach a buffer that is already in this device's memory (not copied, not freed) */
int tdoa_capture_attach_device(tdoa_ctx *ctx, int station, const void *dev_iq, size_t n_samples);
int tdoa_capture_clear(tdoa_ctx *ctx);
/* synthesise a simulator.go-style capture (tones + uniform noise, carrier-phase delay,
 * [ref | target | ref] blocks of block_samples; simulator.go:100-161) directly in HBM */
int tdoa_synth_capture(tdoa_ctx *ctx, int station, size_t block_samples, double ref_freq, double tgt_freq,
                       double noise_level, const double station_lle[3], const double tx_lle[3],
                       double tx_power, uint64_t seed);
/* the same for weak_signal_simulator.go (BASELINE config 3; weak_signal_simulator.go:89-257): weak reference blocks
 * (Gaussian noise 0.8 A, impulses p = 1e-3 at 5 A, phase drift 0.05 rad/s, DC 0.1 A), strong target block */
int tdoa_synth_weak_capture(tdoa_ctx *ctx, int station, size_t block_samples, double ref_freq, double tgt_freq,
                            const double station_lle[3], const double tx_lle[3], double ref_power, double tgt_power,
                            uint64_t seed);
/* read back part of a capture that lives in HBM */
int tdoa_capture_download(tdoa_ctx *ctx, int station, size_t first_sample, size_t n_samples, uint8_t *out);

int tdoa_num_windows(const tdoa_ctx *ctx, int *windows_per_block, int *n_windows_total);
int tdoa_num_pairs(const tdoa_ctx *ctx);

/* Correlate every pair on every window wid with wid % world == rank (with fewer windows than
 * ranks: every unit u = wid * n_pairs + pair with u % world == rank, so no rank idles).
 * out_host (may be NULL): [n_windows_total][n_pairs] tdoa_peak, entries of
 *   windows owned by other ranks are zero-filled;
 * out_dev (may be NULL): same array in device memory (for an RCCL all-gather
 *   of the per-pair peaks without a host round trip).
 * Search ranges below 4095 lags (params.max_lag) take a shorter inverse that never
 * materialises the full correlation array: about 15 % faster at max_lag <= 2047. */
int tdoa_process(tdoa_ctx *ctx, int rank, int world, tdoa_peak *out_host, void *out_dev);

/* upload + process in one call (host pointers in, host peaks out) */
int tdoa_process_u8(tdoa_ctx *ctx, const uint8_t *const *station_iq, const size_t *n_samples,
                    int n_stations, tdoa_peak *out);

/* single pair of raw IQ windows -> peak (lags -(max_lag-1) .. max_lag-1) */
int tdoa_fm_xcorr_u8(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2,
                     int max_lag, tdoa_peak *peak);

/* Sub-sample refinement and physical-plausibility gate (SURVEY section 8 row (f)-4;
 * PROJECT_NOTES.md:29-32: one sample is 500 ns = 150 m of range, max |TDOA| of the
 * deployed stations about 57 us = 114 samples).  Around the integer peak lag d:
 * y_q = s*c[d-1+q], s = sign(c[d]); frac = vertex of the parabola through the three
 * points, (y_m - y_p) / (2 (y_m - 2 y_0 + y_p)) when that curvature is negative, clamped to
 * [-1/2, 1/2], else 0.  The integer peak of tdoa_process is untouched (index parity). */
typedef struct {
    double  delay;      /* lag + frac, samples                               */
    float   frac;       /* vertex offset in [-1/2, 1/2]                      */
    float   y[3];       /* s*c[lag-1], s*c[lag], s*c[lag+1], reference scale */
    int32_t plausible;  /* |delay| <= gate_samples                           */
    int32_t reserved;
} tdoa_fine_peak;
/* tdoa_process + refinement: fine_host [n_windows_total][n_pairs] (zero delay, plausible
 * for windows of other ranks), out_host may be NULL */
int tdoa_process_fine(tdoa_ctx *ctx, int rank, int world, double gate_samples, tdoa_peak *out_host,
                      tdoa_fine_peak *fine_host);
int tdoa_fm_xcorr_fine_u8(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2,
                          int max_lag, double gate_samples, tdoa_peak *peak /* may be NULL */,
                          tdoa_fine_peak *fine);

/* The whole correlation of every pair-window, and its K strongest separate peaks (multipath, several emitters on the
 * channel, peak-to-sidelobe confidence).  Same layouts as tdoa_process: windows of other ranks are zero-filled, pairs
 * are i < j.  Both run inside the step graph; TDOA_LAGS_GO returns TDOA_ERR_UNSUPPORTED.
 *
 * tdoa_process_lags: [n_windows_total][n_pairs][2*max_lag-1] float, reference scale (lag d at d + max_lag - 1), the
 * values the peak search compared.  Either pointer may be NULL, not both.
 *
 * tdoa_process_peaks: [n_windows_total][n_pairs][k] peaks, 1 <= k <= 16, min_separation >= 1.  Peak 1 is tdoa_process's
 * peak.  Each next peak is the largest |c[l]| over the lags l that are a local maximum of |c| (|c[l]| >= |c[l-1]| and
 * >= |c[l+1]|, a neighbour outside the searched range counting as smaller), lie more than min_separation lags from
 * every peak already chosen, and hold neither NaN nor 0.  Ties go to the smaller |lag|, then the positive lag.  The
 * selection stops after k peaks or when no lag qualifies; unused records are zero.  count_host
 * [n_windows_total][n_pairs] (may be NULL): the records written. */
int tdoa_process_lags(tdoa_ctx *ctx, int rank, int world, float *lags_host, void *lags_dev);
int tdoa_process_peaks(tdoa_ctx *ctx, int rank, int world, int k, int min_separation, tdoa_peak *peaks_host,
                       int32_t *count_host);
/* the same selection for one pair of host windows (count may be NULL) */
int tdoa_fm_xcorr_peaks_u8(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2, int max_lag,
                           int k, int min_separation, tdoa_peak *peaks, int32_t *count);

/* Stacked correlation: the surfaces of a run of windows of one block added lag by lag -- one peak set per (stack, pair)
 * instead of one per pair-window.  The stations' clocks do not move within a block, so the windows' lags line up and the
 * sum keeps its maximum at the true delay where a single window's argmax is already lost in noise (coherent processing
 * gain, processor.go:770-782), on the plan of the short window.  (That holds for receivers on one clock and for the
 * synthetic captures.  Two free-running receivers differ in sample rate, the lag slides from window to window and this
 * sum smears: tdoa_process_stacked_drift below searches the slope and stacks along it.)
 *
 * A stack is a run of windows_per_stack consecutive windows of ONE block (0: the whole block; the last stack of a block
 * may be shorter; stacks never cross a block boundary, block 1 being another frequency).  With m = windows_per_stack,
 * stacks_per_block = ceil(windows_per_block / m), and stack j of block b has the id sid = b * stacks_per_block + j.
 * For stack sid, pair p, lag l, with c_w[l] the value tdoa_process_lags returns for window w as a double before its
 * rounding to float:
 *     q_w[l] = llrint(c_w[l] * 2^32)                     (int64, round to nearest even)
 *     Q[l]   = sum of q_w[l] over the stack's windows     (int64, exact, any order)
 *     C[l]   = (double)Q[l] * 2^-32 / sqrt(n_w)           n_w = windows in the stack
 * C is on the reference's scale for a template of n_w * window_len samples, so stacks and single windows compare.  The
 * fixed-point sum is associative: the result does not depend on the launch grouping or on which rank owned which window,
 * and a group's result is byte-identical to one context's.  |c| <= sqrt(window_len) <= 2^13 and a few thousand windows
 * stay far inside int64; the quantum is 2.3e-10.  Captures are bytes, so every c_w is finite; a non-finite term is not
 * defined behaviour of this call.
 *
 * peaks_host [n_stacks_total][n_pairs][k]: the selection rule of tdoa_process_peaks applied to (float)C (1 <= k <= 16,
 * min_separation >= 1; peak 1 = the argmax of |C|, ties to the smaller |lag|, then the positive lag).  corr of a record is
 * the double C[l], abs_corr its float magnitude.  count_host [n_stacks_total][n_pairs]: the records written.
 * fine_host [n_stacks_total][n_pairs]: peak 1 refined by the parabola and gate of tdoa_process_fine on C[d-1], C[d],
 * C[d+1] in double (a neighbour outside the searched range is reported as 0 and leaves frac at 0).
 * surface_host [n_stacks_total][n_pairs][2*max_lag-1]: (float)C.  partial_host, same shape: Q as the rank summed it.
 * Any of the five may be NULL, not all.
 * world > 1: a rank sums the windows (pair-major deal: the pair-windows) it owns; partial_host is then its share of Q --
 * zero where it owns nothing -- and the only output that means anything alone: the sum of the ranks' partials is the Q of
 * world = 1, word for word.  The other outputs of a rank are computed from its own partial, with n_w of the whole stack.
 * Runs inside the step graph.  TDOA_LAGS_GO: TDOA_ERR_UNSUPPORTED.  k, min_separation, a negative windows_per_stack or
 * gate_samples < 0: TDOA_ERR_INVALID. */
int tdoa_num_stacks(const tdoa_ctx *ctx, int windows_per_stack, int *stacks_per_block, int *n_stacks_total);
int tdoa_process_stacked(tdoa_ctx *ctx, int rank, int world, int windows_per_stack, int k, int min_separation,
                         double gate_samples, tdoa_peak *peaks_host, int32_t *count_host, tdoa_fine_peak *fine_host,
                         float *surface_host, int64_t *partial_host);

/* Drift-compensated stacking: the stacks of tdoa_process_stacked taken along a lag slope, the slope searched per
 * (stack, pair).  Two receivers whose sample rates differ by r (1 ppm: 1e-6) see their relative delay slide by
 * r * window_len lags per window; the plain stack then adds windows that do not line up.  Stacks, pairs, q_w[l], n_w and
 * C = Q * 2^-32 / sqrt(n_w) are exactly those of tdoa_process_stacked; window w of a stack has the position j = 0, 1, ...
 * in it, counted by window id.
 * Hypothesis h in -H .. H (H = max_drift) stands for a slope of h / D lags per window (D = drift_den).  Its shift is
 *     shift(h, j) = sgn(h) * ((2 |h| j + D) div (2 D))      the nearest integer to h j / D, halves away from zero;
 *                                                            integers only, shift(-h, j) = -shift(h, j)
 *     Q_h[L]      = sum over j of q_j[L + shift(h, j)]       a term whose lag falls outside -max_lag < lag < max_lag
 *                                                            contributes 0
 * and C_h is derived from Q_h as C from Q.  A pair whose lag is d0 + rho j in window j peaks at L = d0 under the hypothesis
 * nearest rho: the reported lag is the lag at the stack's first window.
 * profile_host [n_stacks_total][n_pairs][2H+1]: entry h + H is the peak of hypothesis h, the largest peak key of
 * (float)C_h[L] over L (the floats and the tie rule of tdoa_process_stacked's peak 1): lag, abs_corr the float magnitude,
 * corr the signed float as a double; no peak (every value 0): the zero record.
 * drift_host [n_stacks_total][n_pairs]: h*, the hypothesis with the largest abs_corr; ties go to the smaller |h|, then to
 * the positive h (the lag takes no part); no peak at all: 0.  The pair's relative clock rate is
 * h* / (D * window_len), times 1e6 in ppm.
 * peaks_host, count_host, fine_host, surface_host: those of tdoa_process_stacked computed on Q_{h*} in place of Q;
 * partial_host: Q_{h*}.  So profile[h* + H].lag == peaks[0].lag with the same abs_corr, and with H = 0 every output is
 * byte-identical to tdoa_process_stacked(ctx, 0, 1, ...) and drift_host all zero.  Any of the seven may be NULL, not all.
 * No rank / world and no group entry: the ranks' per-hypothesis maxima cannot be merged, and their per-hypothesis sums
 * would be 2H+1 surfaces each; one context sums all its windows.
 * Limit: a slope also smears the peak inside one window.  The search repairs the alignment between windows only; it is
 * meant for slopes up to about the peak's width per window.  One slope per stack: a delay that moves between windows
 * but not along a line is tdoa_process_track's, below.
 * Runs inside the step graph.  TDOA_ERR_INVALID: what tdoa_process_stacked refuses, drift_den < 1, max_drift < 0 or > 512,
 * a search whose largest shift, shift(H, m_eff - 1) with m_eff the stack length in use, exceeds max_lag - 1, all seven
 * outputs NULL.  TDOA_LAGS_GO: TDOA_ERR_UNSUPPORTED.  Before captures exist: TDOA_ERR_STATE. */
int tdoa_process_stacked_drift(tdoa_ctx *ctx, int windows_per_stack, int k, int min_separation, double gate_samples,
                               int max_drift /* H */, int drift_den /* D */,
                               tdoa_peak *peaks_host, int32_t *count_host, tdoa_fine_peak *fine_host,
                               float *surface_host, int64_t *partial_host,
                               int32_t *drift_host   /* [n_stacks_total][n_pairs]          */,
                               tdoa_peak *profile_host /* [n_stacks_total][n_pairs][2H+1]  */);

/* Delay tracks: one lag per window of a stack, for a delay that moves between windows but not along a line (a crystal
 * that is still warming up, a slope that changes sign inside a block, windows that carry no peak at all).  Consecutive
 * lags differ by at most J = max_step, and the track is the one along which the sum of the windows' correlation values is
 * largest: dynamic programming (Viterbi) over the surfaces of the step.
 * Stacks, pairs, q_w[l] = llrint(c_w[l] * 2^32), n_w and C = Q * 2^-32 / sqrt(n_w) are exactly those of
 * tdoa_process_stacked.  Window w of a stack has position j = 0 ... n_w-1 by window id.  Lags run over
 * -max_lag < l < max_lag.  J = max_step >= 0.
 * For a polarity σ in {+1, -1}, computed from the stack's last window back to its first:
 *     T_{n_w-1}[l] = σ q_{n_w-1}[l]
 *     T_j[l]       = σ q_j[l] + max over |δ| <= J, l+δ inside the range, of T_{j+1}[l+δ]
 *     D_j[l]       = the δ of that maximum; equal maxima: the smaller |δ|, then the positive δ
 *     L_0          = the l with the largest T_0[l]; equal maxima: the smaller |l|, then the positive l
 *     L_{j+1}      = L_j + D_j[L_j]
 * Polarity: the polarity with the larger max T_0 is taken, +1 on a tie: the track with the largest |sum over j of
 * q_j[L_j]|.  Every lag: T_0[l] is the best sum over all tracks that start at lag l in the stack's first window, so the
 * results are indexed by the lag at the first window, as the slope search reports its lag.  No track: if max T_0 = 0
 * (nothing but zeros) the score is the zero record and all lags and values are 0.  J = 0: σ T_0 = Q, and the score and
 * the surface are tdoa_process_stacked's peak 1 and surface, byte for byte.
 * mm is the stack length: windows_per_block when windows_per_stack is 0 or larger than it, otherwise windows_per_stack;
 * positions j >= n_w of a shorter last stack hold 0.
 * score_host:   lag = L_0; corr the double (σ max T_0) * 2^-32 / sqrt(n_w), the signed sum along the track on C's scale;
 *               abs_corr its float magnitude.
 * lags_host:    lags[j] = L_j.
 * values_host:  values[j] = (double)q_j[L_j] * 2^-32, the window's own correlation on the track: where the signal fades.
 * total_host:   σ T_0 of the chosen polarity, exact.
 * surface_host: (float)(total * 2^-32 / sqrt(n_w)).  More paths raise the score of noise alone (it grows with J): judge a
 *               score against the rest of this surface, not against a plain stack's.
 * Any of the five may be NULL, not all.
 * There is no rank / world and no group entry: a track crosses every window of its stack, so one context holds them all
 * (as for the slope search above, whose per-hypothesis maxima cannot be merged either).
 * Runs inside the step graph, one kernel per window position of a stack.  TDOA_ERR_INVALID: a NULL context (checked
 * before anything needs a device), windows_per_stack < 0, max_step < 0 or > 64, a stack length in use above 4096, all
 * five outputs NULL.  TDOA_LAGS_GO: TDOA_ERR_UNSUPPORTED.  Before captures exist: TDOA_ERR_STATE.  Too little device memory
 * (the steps D take 2 bytes per lag, window and pair): TDOA_ERR_NOMEM. */
int tdoa_process_track(tdoa_ctx *ctx, int windows_per_stack, int max_step /* J */,
                       tdoa_peak *score_host   /* [n_stacks_total][n_pairs]      */,
                       int32_t   *lags_host    /* [n_stacks_total][n_pairs][mm]  */,
                       double    *values_host  /* [n_stacks_total][n_pairs][mm]  */,
                       float     *surface_host /* [n_stacks_total][n_pairs][2*max_lag-1] */,
                       int64_t   *total_host   /* same shape                      */);

/* Closure search: one consistent lag set per station triple of a stack.  Everything above works on one station pair at a
 * time, but the delays of three stations i < j < k close: lag(i,j) + lag(j,k) = lag(i,k).  When noise, multipath or a second
 * emitter moves one pair's argmax the three lags contradict each other; the third surface usually holds what repairs them.
 * The search is exact integer work on Q: no station coordinates, no geometry, no floating point.
 * S stations with S >= 3.
 * Pairs are i < j in the library's order, p(i,j) = i*S - i(i+1)/2 + (j-i-1).
 * Triples are i < j < k in lexicographic order.  There are T = S(S-1)(S-2)/6 of them, returned by tdoa_num_triples.
 * Stacks, n_w and the int64 Q_p[l] over -max_lag < l < max_lag are exactly those of tdoa_process_stacked.
 * windows_per_stack has the same meaning, and stacks never cross a block.
 *   M_p[l] = |Q_p[l]|, an int64.
 *   centre[s] is an int32 per station.  NULL means all 0.  The centre of a pair is c_p(i,j) = centre[j] - centre[i], so
 *     centres close by construction.
 *   G = gate, 0 <= G <= 1023.  A pair's gated window is the lags c_p + x with |x| <= G that lie inside the searched range.
 *   A cell (u, v) of triple (i,j,k) has |u| <= G, |v| <= G and |v-u| <= G.  Its lags are a = c_ij + u, b = c_ik + v and
 *     e = b - a = c_jk + (v-u).  All three must lie inside -max_lag < . < max_lag; a cell with a lag outside does not exist.
 *   score_q(u,v) = M_ij[a] + M_ik[b] + M_jk[e].  This is an int64, and at most 3 * 2^57 here.
 *   The joint cell (u*, v*) is the largest score_q.  Among equal maxima the smaller |u| wins, then the positive u, then the
 *     smaller |v|, then the positive v.
 *   The zero record (all bytes 0) is returned when no cell exists or the maximum is 0.
 *   Independent peaks: for each of the three pairs, x*_p is the argmax of M_p over its gated window.  Equal maxima go to the
 *     smaller |x|, then the positive x.  Then own_q is the sum of the three maxima, and
 *     residual = (c_ij+x*_ij) + (c_jk+x*_jk) - (c_ik+x*_ik).
 *     So score_q <= own_q, and residual == 0 implies score_q == own_q.
 *   Runner-up: runner_q is the largest score_q over the cells with max(|u-u*|, |v-v*|) > min_separation
 *     (min_separation >= 1).  It is 0 when there is none.  A score is judged against it.
 * The record, 80 bytes, no padding: */
typedef struct {
    int32_t lag_ij, lag_ik, lag_jk, residual;      /* a, b, e of the joint cell; the independent peaks' closure residual */
    int64_t score_q, own_q, runner_q;
    double corr_ij, corr_ik, corr_jk;              /* the signed C = Q * 2^-32 / sqrt(n_w) at the three joint lags */
    double score, runner_up;                       /* (double)score_q * 2^-32 / sqrt(n_w) and the same of runner_q */
} tdoa_closure;

/* S(S-1)(S-2)/6 for the context's stations; 0 for a NULL context, fewer than 3 or more than 64 stations */
int tdoa_num_triples(const tdoa_ctx *ctx);

/* closure_host: [n_stacks_total][n_triples] (tdoa_num_stacks, tdoa_num_triples).  A centre that puts a whole window outside
 * the range is legal: it gives zero records.  One context sums all its windows; tdoa_group_process_closure is the group
 * form (the search is a function of the complete stacked Q only, so the members' partial sums merge).
 * Runs inside the step graph, behind the stack's accumulation: two launches of the search kernel (the joint cell, the
 * runner-up) and two of the finishing kernel.  (windows_per_stack, gate, min_separation) are part of the graph's key;
 * the centres are data in a device buffer, so a call that changes only the centres replays the same graph.
 * TDOA_ERR_INVALID: a NULL context (checked before anything needs a device), windows_per_stack < 0, gate < 0 or > 1023,
 * min_separation < 1, a NULL output.  TDOA_ERR_UNSUPPORTED: fewer than three stations (or more than 64), TDOA_LAGS_GO.
 * Before captures exist: TDOA_ERR_STATE. */
int tdoa_process_closure(tdoa_ctx *ctx, int windows_per_stack, int gate /* G */, int min_separation,
                         const int32_t *centre /* [n_stations] or NULL */,
                         tdoa_closure *closure_host /* [n_stacks_total][n_triples] */);

/* tests only: the same kernels on the caller's words q [n_sets][P][2*max_lag-1], P = n_stations (n_stations-1) / 2 rows in
 * the library's pair order, every set a stack of n_w windows; out [n_sets][T].  Needs a context for max_lag and the device,
 * and no captures.  TDOA_ERR_INVALID: what tdoa_process_closure refuses, q NULL, n_sets < 1, n_w < 1, n_stations outside
 * 3 .. 64. */
int tdoa_debug_closure_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int gate,
                              int min_separation, const int32_t *centre, tdoa_closure *out);

/* Delay-table search: a grid of candidate positions scored on all pairs' stacks.  Peaks, drift and tracks look at one
 * station pair, the closure search at one station triple, and a position is found afterwards from one picked lag per pair
 * (tdoa_solve_nstation, tdoa_solve_surface) -- a single wrong argmax pulls the fix kilometres off.  S stations have S - 1 free
 * delays; a transmitter position is the two-parameter family that makes a joint search of all of them tractable.  Every
 * candidate position ("cell") fixes one delay per station, hence one lag per pair, and its score is the sum of all pairs'
 * stacked magnitudes at those lags.  The best cell uses every pair at once and needs no peak to be picked.
 * The search is exact integer work on Q: the library knows nothing about the earth here, the delays are data.
 * Stacks, windows_per_stack, n_w, pairs i < j in the library's order and the int64 Q_p[l] over -max_lag < l < max_lag are
 * exactly those of tdoa_process_stacked.  M_p[l] = |Q_p[l]|.
 *   The table: delay[n_cells][n_stations] is int32, in units of 1/16 sample (TDOA_DELAY_UNIT).  1 <= n_cells <= 2^22.
 *     Entry t[c][s] is the propagation delay from candidate c to station s.  Only differences matter.
 *     n_cols >= 1 gives cells their coordinates, row = c div n_cols and col = c mod n_cols.  The last row may be short.
 *     n_cols = n_cells is a plain list.
 *   A cell's lags: for pair (i, j), d = t[c][j] - t[c][i], taken in 64 bits.  Then
 *     lag_p(c) = sgn(d) * ((2|d| + 16) div 32).
 *     This is the nearest integer to d/16, halves away from zero, integers only (the rule of shift(h, j) in the slope search).
 *     The sign is tdoa_peak's: lag > 0 means the second station lags the first.  It is also the sign of the closure search's
 *     centre[j] - centre[i].
 *   A cell's score: score_q(c) is the sum over all P pairs of M_p[lag_p(c)].  A pair whose lag falls outside the searched
 *     range contributes 0 and is not counted in pairs_in(c).
 *   The location is the cell with the largest score_q.  Among equal maxima the smaller cell index wins.
 *     If the largest score is 0, the zero record and zero lags and correlations are returned.
 *   The runner-up is the largest score_q over cells with max(|row - row*|, |col - col*|) > min_separation (>= 1).  Ties are
 *     broken the same way.  runner_q and runner_cell are 0 when there is none (a cell that exists and scores 0 gives
 *     runner_q 0 and its own index).  A score is judged against the runner-up.
 *   Overflow: |Q| <= n_w * 2^45.  The call returns TDOA_ERR_UNSUPPORTED when P * (stack length in use) > 2^17, so every sum
 *     stays below 2^62.
 * The record, 48 bytes, no padding: */
#define TDOA_DELAY_UNIT 16
typedef struct {
    int32_t cell, runner_cell, pairs_in, reserved;   /* pairs_in of the best cell */
    int64_t score_q, runner_q;
    double  score, runner_up;                        /* (double)x_q * 2^-32 / sqrt(n_w) */
} tdoa_location;

/* The table is context state: it needs no captures, is uploaded once and kept on the device (station-major).  It is data,
 * not part of a step graph's key -- only n_cells and n_cols are, so a call after a new table of the same shape replays the
 * same graph.  delay == NULL or n_cells == 0: forget the table.
 * TDOA_ERR_INVALID: a NULL context, n_cells outside 1 .. 2^22, n_cols < 1, n_stations outside 2 .. 64. */
int tdoa_locate_set_table(tdoa_ctx *ctx, const int32_t *delay /* [n_cells][n_stations] */, int n_cells, int n_cols, int n_stations);

/* lags_host and corr_host are what a caller hands to tdoa_solve_surface (range difference lag / sample_rate * c, weight
 * |C|).  They are the best cell's own table differences, rounded to the lag grid: they hold no measurement below one lag, so
 * the solver's fix is the cell's position again, and a table finer than one lag of range difference only produces plateaus
 * of equal scores (the smaller cell wins).  A fix finer than one lag needs the finer lag grid of tdoa_locate_set_upsample
 * ("sub-sample locate", below).  Runs inside the step graph, behind the stack's accumulation: the scores, the
 * runner-up's pass over the map and two launches of the finishing kernel.  (windows_per_stack, min_separation, n_cells,
 * n_cols) are part of the graph's key.  tdoa_group_process_locate is the group form (the search is a function of the
 * complete stacked Q only, so the members' partial sums merge).
 * TDOA_ERR_INVALID: a NULL context (checked before anything needs a device), a NULL loc_host, windows_per_stack < 0,
 * min_separation < 1.  TDOA_ERR_STATE: no captures, no table, or a table whose n_stations differs from the captures'.
 * TDOA_ERR_UNSUPPORTED: fewer than 2 or more than 64 stations, TDOA_LAGS_GO, the overflow bound (and more than 65535
 * stacks).  TDOA_ERR_NOMEM: the map [n_stacks_total][n_cells] does not fit; tdoa_last_error says so.
 * With station clocks (tdoa_locate_set_clock, below): whether a clock table is present is one more word of the graph's key,
 * and a clock table of another n_stacks or n_stations is TDOA_ERR_STATE. */
int tdoa_process_locate(tdoa_ctx *ctx, int windows_per_stack, int min_separation,
                        tdoa_location *loc_host /* [n_stacks_total], required */,
                        int32_t *lags_host      /* [n_stacks_total][n_pairs]: lag_p(cell*), 0 where outside / no location; may be NULL */,
                        double  *corr_host      /* same shape: signed C = Q * 2^-32 / sqrt(n_w) there; may be NULL */,
                        int64_t *map_host       /* [n_stacks_total][n_cells]: score_q of every cell; may be NULL */);

/* Station clocks for the delay-table search.  A table entry is pure propagation delay: the search above assumes that all
 * stations share one clock.  Stations that start their captures samples apart add clock[j] - clock[i] to every lag of pair
 * (i, j).  The clock table gives every stack its own station clocks (from tdoa_process_sync, below).
 *   clock[n_stacks][n_stations] is int32, in units of 1/16 sample (TDOA_DELAY_UNIT), like the delay table.  Only differences
 *     matter.  A caller can therefore give the block between two reference blocks the exact midpoint 8 * (k_before + k_after)
 *     of their clocks in samples.
 *   With a clock table set, tdoa_process_locate, tdoa_debug_locate_from_q and the group form use, for stack sid,
 *     d = (t[c][j] - t[c][i]) + (clock[sid][j] - clock[sid][i]), taken in 64 bits, and then the rule of lag_p(c) above.
 *     Everything else is unchanged.
 *   Without a clock table, and with an all-zero one, every output is byte-identical.
 * The clock table is context state, like the delay table: it needs no captures and is kept on the device.  Its contents are
 * data; whether one is present is part of a step graph's key, so new clocks of the same shape replay the same graph.
 * clock == NULL or n_stacks == 0: forget the clocks.  A search whose stacks (n_stacks_total; n_sets for the debug call) or
 * stations differ from the clock table's n_stacks or n_stations returns TDOA_ERR_STATE.
 * TDOA_ERR_INVALID: a NULL context, n_stacks outside 1 .. 65535, n_stations outside 2 .. 64. */
int tdoa_locate_set_clock(tdoa_ctx *ctx, const int32_t *clock /* [n_stacks][n_stations] */, int n_stacks, int n_stations);

/* tests only: the same kernels on the caller's words q [n_sets][P][2*max_lag-1], P = n_stations (n_stations-1) / 2 rows in
 * the library's pair order, every set a stack of n_w windows, with the context's table; outputs as tdoa_process_locate's
 * with n_sets for n_stacks_total.  Needs no captures.  Precondition: |q| <= 2^62 div P.  TDOA_ERR_INVALID: what
 * tdoa_process_locate refuses, q NULL, n_sets outside 1 .. 65535, n_w < 1, n_stations outside 2 .. 64.  TDOA_ERR_STATE: no
 * table, or one of another n_stations.  TDOA_ERR_UNSUPPORTED: P * n_w > 2^17. */
int tdoa_debug_locate_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int min_separation,
                             tdoa_location *loc, int32_t *lags, double *corr, int64_t *map);

/* Host only, no device: the table of a latitude / longitude grid at one height.  Cell r*cols + c lies at
 * (lat0 + r*dlat, lon0 + c*dlon, height_m), degrees and metres; stations_lle is [n_stations][3] like tdoa_solve_nstation's.
 * delay = llrint(16 * sample_rate * |ecef(cell) - ecef(station)| / c), through tdoa_latlon_to_ecef, c = 299 792 458 m/s.
 * TDOA_ERR_INVALID: NULL pointers, n_stations < 1, rows*cols outside 1 .. 2^22, non-finite input, sample_rate <= 0, a delay
 * that does not fit int32. */
int tdoa_locate_grid_table(const double *stations_lle, int n_stations, double lat0, double lon0, double dlat, double dlon,
                           int rows, int cols, double height_m, double sample_rate, int32_t *delay /* [rows*cols][n_stations] */);

/* Clock search: the stations' clock offsets from a block whose emitter is known.  Collector stations are synchronised by
 * reference signals, not by disciplined oscillators: every capture is [reference | target | reference] blocks for that
 * reason.  A reference block's emitter position is known, so the lag each pair would have from propagation alone is known;
 * what is left of the pair's peak is the difference of the two stations' clocks.  S stations have S - 1 free clocks, and all
 * P pairs' stacks are searched for them together: no peak is picked.
 * The search is exact integer work on Q.  Stacks, windows_per_stack, n_w, pairs i < j in the library's order and the int64
 * Q_p[l] over -max_lag < l < max_lag are exactly those of tdoa_process_locate.  M_p[l] = |Q_p[l]|.
 *   ref_delay[n_stations] is int32, in units of 1/16 sample (TDOA_DELAY_UNIT): the propagation delays from the known emitter,
 *     one row of a delay table (tdoa_locate_grid_table with rows = cols = 1, for example).
 *     e_ij = sgn(d) * ((2|d| + 16) div 32) with d = ref_delay[j] - ref_delay[i], taken in 64 bits: the rule of lag_p(c).
 *   centre[n_stations] is int32, in samples.  NULL means all 0.
 *   G = gate, 0 <= G <= 1023.  R = rounds, 0 <= R <= 16.
 *   The unknowns are k_s = centre[s] + x_s with |x_s| <= G, in samples.  x_0 = 0: station 0 is the gauge.
 *   The objective is F(k) = sum over i < j of M_ij[e_ij + k_j - k_i].  A lag outside the searched range adds 0 to F and is
 *     not counted in pairs_in.
 *   Order of candidates everywhere: rank(x) = 2|x| - (x > 0), so the smaller |x| comes first, then the positive x.  "Largest"
 *     always means the first of equal maxima in rank order.
 *   Start.  S = 2: x_1 is the largest M_01[e_01 + centre[1] - centre[0] + x].  S >= 3: (x_1, x_2) jointly over the whole
 *     square [-G, G]^2, the largest M_01[e_01 + k_1 - k_0] + M_02[e_02 + k_2 - k_0] + M_12[e_12 + k_2 - k_1].  Among equal
 *     maxima the smaller rank(x_1) wins, then the smaller rank(x_2).  There is no |x_2 - x_1| constraint, unlike the closure
 *     search; a lag outside the range just adds 0.
 *   Placing, for s = 3 .. S-1 in order: x_s is the largest sum over i < s of M_is[e_is + (centre[s] + x) - k_i].
 *   Sweeps, R times: for s = 1 .. S-1 in order (Gauss-Seidel, k_0 fixed) x_s is the largest sum over all S - 1 partners
 *     i != s of M at the pair's lag: e_is + (centre[s] + x) - k_i for a partner i < s, e_si + k_i - (centre[s] + x) for a
 *     partner i > s.  F never decreases over a sweep, and a sweep that moves nothing makes all later sweeps no-ops.
 *   If F at the final k is 0, the record, the clocks, the lags and the correlations are all zero.
 *   Overflow: the call returns TDOA_ERR_UNSUPPORTED when P * (stack length in use) > 2^17, as tdoa_process_locate does.
 * The record, 32 bytes, no padding: */
typedef struct {
    int32_t moved, pairs_in;   /* stations the last sweep changed (0: converged; 0 when R = 0); pairs inside the range at the final k */
    int64_t score_q, start_q;  /* F at the final k; F after placing, so score_q >= start_q */
    double  score;             /* (double)score_q * 2^-32 / sqrt(n_w) */
} tdoa_sync;

/* Runs on every stack of all three blocks, as the other stack products do; the caller reads the stacks of the block whose
 * emitter it described.  clock_host times TDOA_DELAY_UNIT is what tdoa_locate_set_clock takes.  Runs inside the step graph,
 * behind the stack's accumulation: the joint start over (2G+1)^2 cells (three or more stations) and one workgroup per stack
 * for the placing, the sweeps and the outputs.  (windows_per_stack, gate, rounds) are part of the graph's key; ref_delay and
 * centre are data in a device buffer, so a call that changes only them replays the same graph.  tdoa_group_process_sync is
 * the group form (the search is a function of the complete stacked Q only, so the members' partial sums merge).
 * TDOA_ERR_INVALID: a NULL context (checked before anything needs a device), windows_per_stack < 0, gate < 0 or > 1023,
 * rounds < 0 or > 16, a NULL ref_delay, a NULL sync_host.  TDOA_ERR_UNSUPPORTED: fewer than 2 or more than 64 stations,
 * TDOA_LAGS_GO, the overflow bound (and more than 65535 stacks).  Before captures exist: TDOA_ERR_STATE. */
int tdoa_process_sync(tdoa_ctx *ctx, int windows_per_stack, int gate /* G */, int rounds /* R */,
                      const int32_t *ref_delay /* [n_stations] */, const int32_t *centre /* [n_stations] or NULL */,
                      tdoa_sync *sync_host    /* [n_stacks_total], required */,
                      int32_t   *clock_host   /* [n_stacks_total][n_stations]: k_s in samples; may be NULL */,
                      int32_t   *lags_host    /* [n_stacks_total][n_pairs]: e_ij + k_j - k_i, 0 where outside; may be NULL */,
                      double    *corr_host    /* same shape: signed C = Q * 2^-32 / sqrt(n_w) there; may be NULL */);

/* tests only: the same kernels on the caller's words q [n_sets][P][2*max_lag-1], P = n_stations (n_stations-1) / 2 rows in
 * the library's pair order, every set a stack of n_w windows; outputs as tdoa_process_sync's with n_sets for
 * n_stacks_total.  Needs a context for max_lag and the device, and no captures.  Precondition: |q| <= 2^62 div P.
 * TDOA_ERR_INVALID: what tdoa_process_sync refuses, q NULL, n_sets outside 1 .. 65535, n_w < 1, n_stations outside 2 .. 64.
 * TDOA_ERR_UNSUPPORTED: P * n_w > 2^17. */
int tdoa_debug_sync_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int gate, int rounds,
                           const int32_t *ref_delay, const int32_t *centre, tdoa_sync *sync, int32_t *clock, int32_t *lags,
                           double *corr);

/* Fine clock search: the clock search's clocks refined to 1/U sample.  tdoa_process_sync works on whole lags: its clocks are up
 * to half a sample off, and it rounds e_ij to whole lags before it searches.  tdoa_locate_set_upsample scores cells on surfaces
 * of 1/U sample and tdoa_locate_set_clock takes clocks in 1/16 sample, so the refinement gives the locate clocks on its own grid.
 * U is one of 2, 4, 8, 16.  Rf = fine_rounds, 0 <= Rf <= 16.
 *   Coarse stage.  Exactly tdoa_process_sync(windows_per_stack, gate, rounds, ref_delay, centre, ...): sync_host, clock_host,
 *     lags_host and corr_host receive that call's bytes, and k are its clocks.
 *   The fine word.  n = 2 max_lag - 1.  A fine lag lam, in 1/U sample, is inside when |lam| <= (max_lag - 1) U.  Its word is
 *     Q_U[lam + (max_lag - 1) U] of the pair's row, Q_U exactly as tdoa_locate_set_upsample defines it (the committed taps, Q
 *     outside the row counting 0, phase 0 the word itself).  M_p(lam) is the word's magnitude.  An outside lag adds 0 and is not
 *     counted.  No Q_U is materialised: the words that are needed are evaluated from Q.
 *   The pair delays.  e^U_ij = sgn(d) * ((2|d| U + 16) div 32) with d = ref_delay[j] - ref_delay[i], taken in 64 bits: the
 *     upsampled locate's lag rule, so clock and locate agree on the grid.
 *   The search.  kappa_s = U k_s + y_s in 1/U sample, |y_s| <= U, y_0 = 0.  F_U(kappa) = sum over i < j of
 *     M_ij(e^U_ij + kappa_j - kappa_i).  start_q = F_U(U k).  Rf Gauss-Seidel sweeps over stations 1 .. S-1: station s takes the y
 *     of the largest sum over i != s of M with the others where they stand.  Candidates compete in the order
 *     rank(y) = 2|y| - (y > 0); the first of equal maxima wins.  The window stays centred on U k_s in every sweep, so the
 *     standing value is always a candidate and F_U never decreases.
 *   Outputs per stack.  fine_host is a second tdoa_sync record: moved is that of the last fine sweep (0 with Rf = 0), pairs_in
 *     the pairs inside at the final kappa, score_q = F_U(kappa), start_q, and score on the stack's scale.
 *     clock16_host[s] = kappa_s * (16 / U): the row tdoa_locate_set_clock takes.  fine_lags_host[p] = e^U + kappa_j - kappa_i
 *     in 1/U sample; fine_corr_host[p] the signed value of the word there; 0 and 0.0 for a pair outside.  If the coarse record
 *     is the zero record, or the final F_U is 0, every fine output is zero.  With Rf = 0, clock16 = 16 * clock.
 * The call does not read the context's tdoa_locate_set_upsample setting: its U is its own argument.  One more kernel behind
 * the clock search's in the step graph, one workgroup per stack; (windows_per_stack, gate, rounds, U, fine_rounds) are part of
 * the graph's key, ref_delay and centre stay data.  tdoa_group_process_sync_fine is the group form, same bytes.
 * TDOA_ERR_INVALID: what tdoa_process_sync refuses, U not in {2, 4, 8, 16}, fine_rounds < 0 or > 16, a NULL fine_host (all
 * checked before anything needs a device), |centre[s]| + gate + 1 >= 2^27 (the clock in 1/16 sample must fit int32).
 * TDOA_ERR_UNSUPPORTED: what tdoa_process_sync refuses, and the upsampled locate's tightened overflow bound,
 * 4 * P * (stack length in use) > 2^17. */
int tdoa_process_sync_fine(tdoa_ctx *ctx, int windows_per_stack, int gate /* G */, int rounds /* R */, int U, int fine_rounds /* Rf */,
                           const int32_t *ref_delay /* [n_stations] */, const int32_t *centre /* [n_stations] or NULL */,
                           tdoa_sync *sync_host      /* [n_stacks_total], required: tdoa_process_sync's */,
                           int32_t   *clock_host     /* [n_stacks_total][n_stations]: tdoa_process_sync's; may be NULL */,
                           int32_t   *lags_host      /* [n_stacks_total][n_pairs]: tdoa_process_sync's; may be NULL */,
                           double    *corr_host      /* same shape: tdoa_process_sync's; may be NULL */,
                           tdoa_sync *fine_host      /* [n_stacks_total], required */,
                           int32_t   *clock16_host   /* [n_stacks_total][n_stations]: kappa_s * (16 / U), 1/16 sample; may be NULL */,
                           int32_t   *fine_lags_host /* [n_stacks_total][n_pairs]: 1/U sample, 0 where outside; may be NULL */,
                           double    *fine_corr_host /* same shape: the signed word * 2^-32 / sqrt(n_w) there; may be NULL */);

/* tests only: the same kernels on the caller's words, as tdoa_debug_sync_from_q.  Precondition: |q| <= 2^60 div P.
 * TDOA_ERR_INVALID: what tdoa_process_sync_fine and tdoa_debug_sync_from_q refuse.  TDOA_ERR_UNSUPPORTED: 4 * P * n_w > 2^17. */
int tdoa_debug_sync_fine_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int gate, int rounds, int U,
                                int fine_rounds, const int32_t *ref_delay, const int32_t *centre, tdoa_sync *sync, int32_t *clock,
                                int32_t *lags, double *corr, tdoa_sync *fine, int32_t *clock16, int32_t *fine_lags,
                                double *fine_corr);

/* Clock lines: the stations' clock offsets and rates from a reference block.  tdoa_process_sync finds one offset per station
 * per stack and assumes the clocks stand still inside that stack; free-running receivers drift by lags per second, so the
 * whole-block stack smears along the drift and a one-window stack is where the noise wins.  This search takes the S - 1 clock
 * rates together with the S - 1 clock offsets, over all pairs and all stacks of a block at once: the station-consistent form
 * of tdoa_process_stacked_drift's slope search, as the clock search is of the per-pair argmax.
 * Lines and positions.
 *   Stacks, windows_per_stack, pairs i < j in the library's order, the int64 words Q_{sid,p}[l], e_ij from ref_delay, and
 *     rank(x) = 2|x| - (x > 0) are those of tdoa_process_sync.
 *   A line is one block.  Its positions are j = 0 .. L-1, the block's stacks in order (L = stacks_per_block).
 *   The debug entry takes n_sets and track_len as tdoa_debug_locate_track_from_q does.
 *   N_w is the number of windows of the whole line.
 * Unknowns.
 *   Per station s: k_s = centre[s] + x_s, |x_s| <= G (0 <= G <= 1023).
 *   Per station s: a slope h_s, |h_s| <= H (0 <= H <= 512), of h_s / D lags per position (D >= 1).
 *   Station 0 is the gauge: x_0 = 0, h_0 = 0.
 *   Clock of s at position j: k_s(j) = k_s + shift(h_s, j), with shift(h, j) = sgn(h) * ((2|h|j + D) div (2D)), the slope
 *     search's rule.
 * Objective.
 *   A_ij = sum over j of Q_{j,ij}[e_ij + k_j(j) - k_i(j)], the signed words summed along the line.
 *   A term outside -max_lag < lag < max_lag adds 0 and is not counted in terms_in.
 *   F = sum over i < j of |A_ij|.
 * Candidates.
 *   The candidates of a station are the (h, x) pairs in the order r = rank(h) * (2G+1) + rank(x).
 *   "Largest" means the first of equal maxima in that order: smaller |h|, then the positive h, then smaller |x|, then the
 *     positive x.
 * Search.
 *   Placing, for s = 1 .. S-1 in order: (x_s, h_s) is the largest sum over i < s of |A_is|, with the earlier stations where
 *     they were put.
 *   Sweeps, R times (0 <= R <= 16), for s = 1 .. S-1: (x_s, h_s) is the largest sum over i != s of |A_pair(i,s)|, with the sign
 *     convention of the clock search's sweeps.
 *   start_q is F after placing, and score_q is F at the end, so score_q >= start_q.
 *   moved counts the stations whose (k, h) the last sweep changed.
 *   If F = 0 at the end, every output of the line is zero.
 * Overflow.  P * N_w > 2^17 returns TDOA_ERR_UNSUPPORTED.  The debug entry's precondition is |q| <= 2^62 div (P * L).
 * The record, 40 bytes, no padding: */
typedef struct {
    int32_t moved, terms_in, positions, reserved;  /* stations the last sweep changed (0 when R = 0); terms inside the range at the end; L; 0 */
    int64_t score_q, start_q;  /* F at the end; F after placing */
    double  score;             /* (double)score_q * 2^-32 / sqrt(N_w) */
} tdoa_sync_line;

/* Outputs.  Per line (the three blocks in order): the record, clock[S] (k_s, in samples) and rate[S] (h_s).  Per stack:
 * rows[n_stacks_total][S] = 16 * k_s(j), what tdoa_locate_set_clock takes for that block.  Per stack and pair: the lag along
 * the line and the signed C of that stack there (0 and 0.0 outside the range).
 * Runs on all three blocks, as the other stack products do; the caller reads the line of the block whose emitter it
 * described.  Runs inside the step graph, behind the stack's accumulation: per step of a station one launch over tiles of 256
 * candidates and one that commits the tiles' best, then the outputs.  (windows_per_stack, gate, max_drift, drift_den, rounds)
 * are part of the graph's key; ref_delay, centre and the shift table are data in device buffers, so a call that changes only
 * the delays and centres replays the same graph.
 * TDOA_ERR_INVALID: what tdoa_process_sync refuses (line_host in the place of sync_host), max_drift < 0 or > 512, drift_den
 * < 1.  TDOA_ERR_STATE and TDOA_ERR_UNSUPPORTED: as its sibling, the overflow bound taken on the block's windows. */
int tdoa_process_sync_drift(tdoa_ctx *ctx, int windows_per_stack, int gate /* G */, int max_drift /* H */, int drift_den /* D */,
                            int rounds /* R */, const int32_t *ref_delay /* [n_stations] */,
                            const int32_t *centre /* [n_stations] or NULL */,
                            tdoa_sync_line *line_host /* [3], required */,
                            int32_t   *clock_host /* [3][n_stations]: k_s in samples; may be NULL */,
                            int32_t   *rate_host  /* [3][n_stations]: h_s; may be NULL */,
                            int32_t   *rows_host  /* [n_stacks_total][n_stations]: 16 k_s(j); may be NULL */,
                            int32_t   *lags_host  /* [n_stacks_total][n_pairs]; may be NULL */,
                            double    *corr_host  /* same shape; may be NULL */);

/* tests only: the same kernels on the caller's words q [n_sets][P][2*max_lag-1], every set a stack of n_w windows, set
 * t * track_len + j position j of line t, so N_w = track_len * n_w; outputs as tdoa_process_sync_drift's with n_sets /
 * track_len lines and n_sets stacks.  Needs a context for max_lag and the device, and no captures.
 * TDOA_ERR_INVALID: what tdoa_process_sync_drift refuses, q NULL, n_sets outside 1 .. 65535, n_w < 1, n_stations outside
 * 2 .. 64, track_len < 1 or not a divisor of n_sets.  TDOA_ERR_UNSUPPORTED: P * track_len * n_w > 2^17. */
int tdoa_debug_sync_drift_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int gate,
                                 int max_drift, int drift_den, int rounds, const int32_t *ref_delay, const int32_t *centre,
                                 tdoa_sync_line *line, int32_t *clock, int32_t *rate, int32_t *rows, int32_t *lags,
                                 double *corr);

/* Host helper, no device: writes out[j - first_position][s] = 16 * k_s + r(16 * h_s * j, D) for j = first_position ..
 * first_position + n_positions - 1.  Here r is the nearest integer, halves away from zero, in integers only.  This is the
 * line continued past its block at the table's 1/16 sample.  It assumes, as the ramp between two reference blocks does, that
 * the blocks follow one another without a gap.  TDOA_ERR_INVALID: a NULL pointer, n_stations < 1, drift_den < 1,
 * first_position < 0, n_positions < 1. */
int tdoa_sync_line_clock(const int32_t *clock, const int32_t *rate, int n_stations, int drift_den, int first_position,
                         int n_positions, int32_t *out /* [n_positions][n_stations] */);

/* Fine clock lines: the clock lines' offsets and rates refined to 1/U sample.  tdoa_process_sync_drift returns offsets in
 * whole samples and slopes in steps of 1/D lag per position; after L positions a slope that is half a step off has put
 * L/(2D) lags into every pair of the block the line is continued over, more than the upsampled locate gains.
 * tdoa_process_sync_drift_fine runs that search unchanged and, behind it in the same step graph, refines every line's S - 1
 * offsets and S - 1 rates on the 1/U-sample grid.
 *   Arguments.  (windows_per_stack, gate G, max_drift H, drift_den D, rounds R, U, fine_rounds Rf, ref_delay, centre,
 *     outputs).  U is one of 2, 4, 8, 16.  0 <= Rf <= 16.  The call does not read the context's tdoa_locate_set_upsample
 *     setting.
 *   Coarse stage.  Exactly tdoa_process_sync_drift(windows_per_stack, gate, max_drift, drift_den, rounds, ref_delay, centre,
 *     ...).  The first six outputs are that call's bytes.  k_s and h_s are its clocks and rates.
 *   The fine word.  It is as in tdoa_process_sync_fine.  A fine lag lam is inside when |lam| <= (max_lag - 1) U.  Its word is
 *     Q_U[lam + (max_lag - 1) U] of that (position, pair) row, with Q_U exactly as tdoa_locate_set_upsample defines it.  An
 *     outside term adds 0 and is not counted.  No Q_U is materialised.  e^U_ij = sgn(d) * ((2|d| U + 16) div 32) with
 *     d = ref_delay[j] - ref_delay[i], taken in 64 bits.
 *   Unknowns.  Per station s: kappa_s = U k_s + y_s in 1/U sample, |y_s| <= U, and eta_s = U h_s + g_s, |g_s| <= U, in units
 *     of 1/(U D) lag per position.  Station 0 is the gauge: y_0 = g_0 = 0.
 *   Clock at position x.  kappa_s(x) = kappa_s + shift(eta_s, x), in 1/U sample.  shift(h, x) = sgn(h) * ((2|h|x + D) div (2D))
 *     is the slope search's rule with the same D.
 *   Objective.  A^U_ij = sum over x of Q_U,x,ij[e^U_ij + kappa_j(x) - kappa_i(x)], the signed words summed along the line.
 *     F_U = sum over i < j of |A^U_ij|.
 *   Start.  start_q = F_U at y = g = 0.  Because of rounding (e^U and shift are rounded on the finer grid) this is not the
 *     coarse line's F.
 *   Search.  Rf Gauss-Seidel sweeps over stations 1 .. S-1.  There is no placing.  Station s takes the (g, y) of the largest
 *     sum over i != s of |A^U_pair(i,s)|, with the others where they stand.  Candidates compete in the order
 *     r = rank(g) * (2U + 1) + rank(y), with rank(x) = 2|x| - (x > 0).  The first of equal maxima wins.  The window stays
 *     centred on (U k_s, U h_s) in every sweep.  The standing value is therefore always a candidate and F_U never decreases.
 *   Outputs.  Per line: fine is a second tdoa_sync_line record: moved is that of the last fine sweep, 0 with Rf = 0; terms_in
 *     counts the terms inside at the end; positions = L; score_q = F_U, and start_q is as defined above;
 *     score = score_q * 2^-32 / sqrt(N_w).  Per line: clock16[S] = kappa_s * (16 / U).  Per line: fine_rate[S] = eta_s.  Per
 *     stack: fine_rows[S] = kappa_s(x) * (16 / U), the row tdoa_locate_set_clock takes.  Per stack and pair: fine_lags in 1/U
 *     sample and fine_corr, the signed word on that stack's scale.  Both are 0 and 0.0 for a term outside.  If the coarse
 *     record is the zero record or the final F_U is 0, every fine output of that line is zero.  With Rf = 0:
 *     clock16 = 16 * clock and fine_rate = U * rate.
 * Behind the clock-line search's launches: one launch that sets the fine table, per step of a station one launch over groups
 * of fine slopes and one that commits the groups' best, and two that write start_q and the outputs.  (windows_per_stack, gate,
 * max_drift, drift_den, rounds, U, fine_rounds) are part of the graph's key; ref_delay and centre stay data, so a call that
 * changes only them replays the graph.  tdoa_group_process_sync_drift_fine is the group form, same bytes.
 * TDOA_ERR_INVALID: what tdoa_process_sync_drift refuses, U not in {2, 4, 8, 16}, fine_rounds < 0 or > 16, a NULL fine_host
 * (all checked before anything needs a device), |centre[s]| + G + 2 + ((H + 1)(L - 1)) div D >= 2^27 (a fine row in 1/16
 * sample must fit int32).  TDOA_ERR_STATE and TDOA_ERR_UNSUPPORTED: what tdoa_process_sync_drift refuses, and the tightened
 * overflow bound 4 * P * N_w > 2^17, N_w the windows of a line. */
int tdoa_process_sync_drift_fine(tdoa_ctx *ctx, int windows_per_stack, int gate /* G */, int max_drift /* H */, int drift_den /* D */,
                                 int rounds /* R */, int U, int fine_rounds /* Rf */, const int32_t *ref_delay /* [n_stations] */,
                                 const int32_t *centre /* [n_stations] or NULL */,
                                 tdoa_sync_line *line_host /* [3], required: tdoa_process_sync_drift's */,
                                 int32_t   *clock_host /* [3][n_stations]: tdoa_process_sync_drift's; may be NULL */,
                                 int32_t   *rate_host  /* [3][n_stations]: tdoa_process_sync_drift's; may be NULL */,
                                 int32_t   *rows_host  /* [n_stacks_total][n_stations]: tdoa_process_sync_drift's; may be NULL */,
                                 int32_t   *lags_host  /* [n_stacks_total][n_pairs]: tdoa_process_sync_drift's; may be NULL */,
                                 double    *corr_host  /* same shape: tdoa_process_sync_drift's; may be NULL */,
                                 tdoa_sync_line *fine_host /* [3], required */,
                                 int32_t   *clock16_host   /* [3][n_stations]: kappa_s * (16 / U), 1/16 sample; may be NULL */,
                                 int32_t   *fine_rate_host /* [3][n_stations]: eta_s; may be NULL */,
                                 int32_t   *fine_rows_host /* [n_stacks_total][n_stations]: kappa_s(x) * (16 / U); may be NULL */,
                                 int32_t   *fine_lags_host /* [n_stacks_total][n_pairs]: 1/U sample, 0 where outside; may be NULL */,
                                 double    *fine_corr_host /* same shape: the signed word * 2^-32 / sqrt(n_w) there; may be NULL */);

/* tests only: the same kernels on the caller's words, as tdoa_debug_sync_drift_from_q.  Precondition: |q| <= 2^60 div (P * L).
 * TDOA_ERR_INVALID: what tdoa_process_sync_drift_fine and tdoa_debug_sync_drift_from_q refuse.  TDOA_ERR_UNSUPPORTED:
 * 4 * P * track_len * n_w > 2^17. */
int tdoa_debug_sync_drift_fine_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int gate,
                                      int max_drift, int drift_den, int rounds, int U, int fine_rounds, const int32_t *ref_delay,
                                      const int32_t *centre, tdoa_sync_line *line, int32_t *clock, int32_t *rate, int32_t *rows,
                                      int32_t *lags, double *corr, tdoa_sync_line *fine, int32_t *clock16, int32_t *fine_rate,
                                      int32_t *fine_rows, int32_t *fine_lags, double *fine_corr);

/* Host helper, no device: writes out[x - first_position][s] = clock16[s] + r(16 * eta_s * x, U * D), eta_s = fine_rate[s], for
 * x = first_position .. first_position + n_positions - 1.  Here r is the nearest integer, halves away from zero, in 64-bit
 * integers only.  This is the fine line continued past its block, in the 1/16 sample tdoa_locate_set_clock takes; blocks that
 * follow one another without a gap are assumed, as by tdoa_sync_line_clock.  TDOA_ERR_INVALID: a NULL pointer,
 * n_stations < 1, U not a factor (2, 4, 8, 16), drift_den < 1, first_position < 0, n_positions < 1. */
int tdoa_sync_line_clock16(const int32_t *clock16, const int32_t *fine_rate, int n_stations, int U, int drift_den,
                           int first_position, int n_positions, int32_t *out /* [n_positions][n_stations] */);

/* Cell tracks: follow an emitter from stack to stack through the delay-table search's maps.  tdoa_process_locate locates
 * every stack alone.  Stations with free-running clocks give every stack of a target block its own clock row, so the block's
 * windows cannot be summed lag by lag; their maps can be added cell by cell, because every map is in the emitter's
 * coordinates with that stack's clocks applied.  A position that moves between stacks (a vehicle, residual clock error) is
 * the 2-D analogue of tdoa_process_track's lag, and the same recurrence answers it.
 * Stacks, windows_per_stack, n_w, the table, the clocks and score_q(sid, c) are exactly tdoa_process_locate's.
 *   A track spans the stacks of one block: block b has positions j = 0 .. L-1, L = stacks_per_block (tdoa_num_stacks),
 *     stack sid = b L + j.  n_tracks = n_stacks_total / L.  s_j[c] = score_q(b L + j, c), with clocks when a clock table is set.
 *   Cells have row = c div n_cols and col = c mod n_cols.  A neighbour (row + dr, col + dc) exists when row + dr >= 0,
 *     0 <= col + dc < n_cols and its index is < n_cells (the last row may be short; n_cols = n_cells is a list, where tracks
 *     move along the index).
 *   J = max_step, 0 <= J <= 16.  The recurrence runs from the last position back to the first:
 *     T_{L-1}[c] = s_{L-1}[c]
 *     T_j[c]     = s_j[c] + max over |dr| <= J, |dc| <= J, neighbour exists, of T_{j+1}[neighbour]
 *     D_j[c]     = the (dr, dc) of that maximum
 *   Ties in D_j: the smaller rank(dr), then the smaller rank(dc), rank(x) = 2|x| - (x > 0) as in the clock search.  This is
 *     what a row maximum followed by a column maximum produces.  (0, 0) always exists.
 *   L_0 is the cell with the largest T_0; among equal maxima the smaller cell wins, which is the location's rule.
 *     L_{j+1} = L_j + D_j[L_j].
 *   If max T_0 = 0, the zero record is returned and every per-position output is 0.
 *   The runner-up is the largest T_0 over cells with max(|row - row_0|, |col - col_0|) > min_separation from L_0; ties and
 *     the case that there is none are as in tdoa_process_locate.
 *   There is no polarity: scores are sums of magnitudes.
 *   Overflow: the call returns TDOA_ERR_UNSUPPORTED when P * windows_per_block > 2^17; a track's sum is then below 2^62 by
 *     the argument tdoa_process_locate uses per stack.
 * Identities (held by the tests):
 *   L = 1 (windows_per_stack = 0): cell, runner_cell, score_q, runner_q, score, runner_up, lags, corr and total are
 *     tdoa_process_locate's bytes; total is its map.
 *   J = 0: total = the sum over j of the stacks' maps, word for word.
 *   score_q = total[cell] = the sum over j of own[j].
 *   Consecutive cells are at most J rows and columns apart.
 * The record, 48 bytes, no padding: */
typedef struct {
    int32_t cell, runner_cell;   /* L_0; the runner-up's cell */
    int32_t positions, steps;    /* L; the number of positions after which the track moves to another cell */
    int64_t score_q, runner_q;   /* max T_0; the runner-up's T_0 */
    double  score, runner_up;    /* (double)x_q * 2^-32 / sqrt(N_w), N_w = the windows of the track (L = 1: the location's scale) */
} tdoa_cell_track;

/* Runs inside the step graph, behind the stack's accumulation and the delay-table search: one launch per position
 * j = L-2 .. 0 of the recurrence's kernel, then the best cell, the walk and the runner-up's pass over T_0.
 * (windows_per_stack, max_step, min_separation, n_cells, n_cols, whether a clock table is present) are part of the graph's
 * key; the table and the clocks are data.  Every position's row of lags_host / corr_host can go to tdoa_solve_surface.
 * tdoa_group_process_locate_track is the group form.
 * TDOA_ERR_INVALID: a NULL context (checked before anything needs a device), a NULL track_host, windows_per_stack < 0,
 * max_step outside 0 .. 16, min_separation < 1.  TDOA_ERR_STATE: no captures, no table, or a table or clock table whose
 * shape does not match.  TDOA_ERR_UNSUPPORTED: TDOA_LAGS_GO, fewer than 2 or more than 64 stations, the overflow bound
 * above, more than 65535 stacks, L > 4096.  TDOA_ERR_NOMEM: besides the map the call needs 2 bytes per (stack, cell) for D
 * and 16 per (track, cell) for the two halves of T; tdoa_last_error says which did not fit. */
int tdoa_process_locate_track(tdoa_ctx *ctx, int windows_per_stack, int max_step /* J */, int min_separation,
                              tdoa_cell_track *track_host /* [n_tracks], required */,
                              int32_t *cells_host /* [n_tracks][L]: L_j; may be NULL */,
                              int64_t *own_host   /* [n_tracks][L]: s_j[L_j] (where the signal fades); may be NULL */,
                              int32_t *lags_host  /* [n_stacks_total][n_pairs]: lag_p(L_j) of stack b L + j, clocks included, 0 where outside; may be NULL */,
                              double  *corr_host  /* same shape: the signed C there on that stack's own scale; may be NULL */,
                              int64_t *total_host /* [n_tracks][n_cells]: T_0; may be NULL */);

/* tests only: the same kernels on the caller's words q [n_sets][P][2*max_lag-1] as tdoa_debug_locate_from_q takes them, with
 * the context's table and clocks.  n_sets is a multiple of track_len; set t * track_len + j is position j of track t, every
 * set a stack of n_w windows, N_w = track_len * n_w.  Needs no captures.  Precondition: |q| <= 2^62 div (P * track_len).
 * TDOA_ERR_INVALID: what tdoa_process_locate_track and tdoa_debug_locate_from_q refuse, track_len < 1 or not a divisor of
 * n_sets.  TDOA_ERR_STATE: as tdoa_debug_locate_from_q.  TDOA_ERR_UNSUPPORTED: P * track_len * n_w > 2^17, track_len > 4096. */
int tdoa_debug_locate_track_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w,
                                   int max_step, int min_separation, tdoa_cell_track *track, int32_t *cells, int64_t *own,
                                   int32_t *lags, double *corr, int64_t *total);

/* Several emitters per stack: mask the found lags and search again.  The peak of an emitter A in pair p's stack raises every
 * cell whose lag_p equals A's -- a whole hyperbola on the map -- and where three of A's pairs coincide a ridge, far more than
 * min_separation from A.  A weaker emitter B on the same channel lies under those ridges, so tdoa_process_locate's runner-up
 * is not a second emitter.  Taking A's lags out of every pair's stack and searching again finds B.
 * Stacks, windows_per_stack, n_w, the table, the clocks, lag_p(c), Q and the record are exactly tdoa_process_locate's.
 * K = n_emitters, 1 <= K <= TDOA_LOCATE_MAX_EMITTERS.  Per stack, rounds r = 0 .. K-1:
 *   E_p(r) is the set of excluded lags of pair p.  E_p(0) is empty.
 *     E_p(r+1) = E_p(r) united with { l : |l - lag_p(cell*_r)| <= guard } if round r found a cell and lag_p(cell*_r) lies
 *     inside the searched range; otherwise E_p(r+1) = E_p(r).  Intervals are clipped at the range edges.  They may overlap.
 *   M_p^r[l] = 0 for l in E_p(r) or outside the range, else |Q_p[l]|.
 *   score_q^r(c) = the sum over all P pairs of M_p^r[lag_p(c)].
 *   Round r's record: the largest score_q^r, equal maxima going to the smaller cell; the runner-up of that round's map beyond
 *     min_separation of that round's cell; pairs_in counts the pairs inside the range and not excluded at the cell; reserved
 *     carries the number of pairs inside the range but excluded at the cell.
 *   Per pair: a pair outside the range reports lag 0 and 0.0.  An excluded pair reports its lag and 0.0, so
 *     tdoa_solve_surface gives it no weight.
 *   If the largest score of a round is 0, the result is the zero record, zero lags and zero correlations, and nothing is
 *     added to E.  Every later round is then the zero record too.
 *   Q is never written.
 * Identity (held by the tests): round 0, and therefore the whole call with K = 1, returns tdoa_process_locate's bytes --
 *   record, lags, correlations, map.  reserved is 0 there.
 * The outputs are laid out [round][stack][...].  It joins nothing across stacks: combining it with tdoa_process_locate_track
 * is out of scope.  tdoa_process_locate_track_multi below is the call that runs the rounds on a block's tracks.
 * Runs inside the step graph, behind the stack's accumulation: round 0 as tdoa_process_locate launches it, then per further
 * round the masked scores, the runner-up's pass and two finishing launches.  (windows_per_stack, K, guard, min_separation,
 * n_cells, n_cols, whether a clock table is present) are part of the graph's key; the table, the clocks and the excluded
 * intervals are data.  tdoa_group_process_locate_multi is the group form.
 * TDOA_ERR_INVALID (no device needed): what tdoa_process_locate refuses, n_emitters outside 1 .. 8, guard < 0.  Every other
 * refusal is tdoa_process_locate's.  TDOA_ERR_NOMEM: the map [K][n_stacks_total][n_cells] does not fit; tdoa_last_error says
 * so. */
#define TDOA_LOCATE_MAX_EMITTERS 8
int tdoa_process_locate_multi(tdoa_ctx *ctx, int windows_per_stack, int n_emitters /* K */, int guard /* >= 0 lags */,
                              int min_separation,
                              tdoa_location *loc_host /* [K][n_stacks_total], required */,
                              int32_t *lags_host      /* [K][n_stacks_total][n_pairs]; may be NULL */,
                              double  *corr_host      /* same shape; may be NULL */,
                              int64_t *map_host       /* [K][n_stacks_total][n_cells]: score_q^r of every cell; may be NULL */);

/* tests only: the same kernels on the caller's words q [n_sets][P][2*max_lag-1] as tdoa_debug_locate_from_q takes them, with
 * the context's table and clocks; outputs [K][n_sets][...].  Needs no captures.  Errors as tdoa_debug_locate_from_q's, plus
 * n_emitters outside 1 .. 8 and guard < 0 (TDOA_ERR_INVALID). */
int tdoa_debug_locate_multi_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int n_emitters,
                                   int guard, int min_separation, tdoa_location *loc, int32_t *lags, double *corr, int64_t *map);

/* Several emitters per block: mask a found track's lags and track again.  tdoa_process_locate_multi finds a second emitter
 * only where a single stack shows it, and the runner-up of tdoa_process_locate_track is no second emitter, because emitter
 * A's ridges survive the sum over stacks.  Taking the lags of A's track out of every stack's pairs and tracking again finds
 * a weaker emitter B that no single stack shows, and lets both move.
 * Stacks, windows_per_stack, n_w, tracks (one per block, L = stacks per block), the table, the clocks, lag_p(c) with the
 * stack's clocks, Q, the recurrence T_j[c] = s_j[c] + max T_{j+1}[neighbour] with its tie order, and the record
 * tdoa_cell_track are exactly tdoa_process_locate_track's.
 * K = n_emitters, 1 <= K <= TDOA_LOCATE_MAX_EMITTERS.  Per track, rounds r = 0 .. K-1:
 *   E_p^j(r) is the set of excluded lags of pair p in stack j of the track.  E_p^j(0) is empty.
 *   M_p^{j,r}[l] = 0 for l in E_p^j(r) or outside the range, else |Q_p^j[l]|.
 *   s_j^r(c) = the sum over all P pairs of M_p^{j,r}[lag_p^j(c)].
 *   Round r's track is the cell track on the maps s_0^r .. s_{L-1}^r: T^r, D^r, L_0^r the cell of the largest T_0^r, equal
 *     maxima going to the smaller cell.  The walk is L_{j+1}^r = L_j^r + D_j^r[L_j^r].  The runner-up is the largest T_0^r
 *     beyond min_separation of L_0^r.  own_j^r = s_j^r[L_j^r].
 *   If max T_0^r > 0: E_p^j(r+1) = E_p^j(r) united with { l : |l - lag_p^j(L_j^r)| <= guard } for every stack j and every
 *     pair whose lag there lies inside the range.  Intervals are clipped at the range edges and may overlap.  Otherwise
 *     E(r+1) = E(r): the round returns the zero record and zero per-position outputs, and so does every later round.
 *   Per (round, stack): pairs_in counts the pairs inside the range and not excluded at L_j^r, reserved the pairs inside but
 *     excluded there.  An excluded pair reports its lag and 0.0; a pair outside reports 0 and 0.0.
 *   Q is never written.
 * Identities (held by the tests):
 *   Round 0 is tdoa_process_locate_track's bytes: record, cells, own, lags, corr, total.  So is the whole call with K = 1.
 *     There pairs_in is the count of pairs inside and reserved is 0.
 *   With one stack per track (L = 1), every round equals tdoa_process_locate_multi's round in cell, runner_cell, score_q,
 *     runner_q, score, runner_up, the lags and correlations byte for byte, pairs_in and reserved, and the map as total;
 *     positions = 1 and steps = 0.
 * Outputs are laid out [round][...].  A round is judged by its own runner-up; there is no stop rule.
 * Runs inside the step graph, behind the stack's accumulation: round 0 as tdoa_process_locate_track launches it and one
 * launch for the centres its track gives, then per further round the masked scores, the recurrence's L-1 launches, the best
 * cell, the runner-up's pass and two finishing launches.  (windows_per_stack, max_step, K, guard, min_separation, n_cells,
 * n_cols, whether a clock table is present) are part of the graph's key; the table, the clocks and the excluded intervals
 * are data.  tdoa_group_process_locate_track_multi is the group form.
 * TDOA_ERR_INVALID (no device needed): what tdoa_process_locate_track refuses, n_emitters outside 1 .. 8, guard < 0.  Every
 * other refusal is tdoa_process_locate_track's.  TDOA_ERR_NOMEM: besides what tdoa_process_locate_track needs, the call holds
 * 8 bytes per (track, cell) for every round's T_0 (L = 1: the map of every round); tdoa_last_error names what did not fit,
 * the rounds included. */
int tdoa_process_locate_track_multi(tdoa_ctx *ctx, int windows_per_stack, int max_step /* J */, int n_emitters /* K */,
                                    int guard /* >= 0 lags */, int min_separation,
                                    tdoa_cell_track *track_host /* [K][n_tracks], required */,
                                    int32_t *cells_host /* [K][n_tracks][L]; may be NULL */,
                                    int64_t *own_host   /* [K][n_tracks][L]; may be NULL */,
                                    int32_t *pairs_host /* [K][n_stacks_total][2]: pairs_in, reserved; may be NULL */,
                                    int32_t *lags_host  /* [K][n_stacks_total][n_pairs]; may be NULL */,
                                    double  *corr_host  /* same shape; may be NULL */,
                                    int64_t *total_host /* [K][n_tracks][n_cells]: T_0^r; may be NULL */);

/* tests only: the same kernels on the caller's words q [n_sets][P][2*max_lag-1] as tdoa_debug_locate_track_from_q takes them,
 * with its preconditions and the context's table and clocks; outputs [K][...] with n_sets for n_stacks_total.  Needs no
 * captures.  Errors as tdoa_debug_locate_track_from_q's, plus n_emitters outside 1 .. 8 and guard < 0 (TDOA_ERR_INVALID). */
int tdoa_debug_locate_track_multi_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w,
                                         int max_step, int n_emitters, int guard, int min_separation, tdoa_cell_track *track,
                                         int32_t *cells, int64_t *own, int32_t *pairs, int32_t *lags, double *corr,
                                         int64_t *total);

/* Map statistics: exact quantiles and the peak's footprint of every judged plane, computed where the plane lives.  The four
 * calls of the delay-table family return a best cell and a runner-up on noise alone too, and the runner-up is one far cell
 * on the first emitter's hyperbolae: it does not measure the noise.  The plane's own distribution does, and downloading the
 * plane to get it costs an order of magnitude more than the call.
 * The setting is context state, like the clock table.  While it is on, tdoa_process_locate, tdoa_process_locate_multi,
 * tdoa_process_locate_track and tdoa_process_locate_track_multi, their tdoa_debug_*_from_q and tdoa_group_* forms also
 * compute one tdoa_map_stats per judged plane -- the int64 plane whose largest word the record reports as score_q: the map
 * [round][stack] of the two searches (and of tracks of one stack), T_0 [round][track] of the two track calls -- in the
 * records' order.  The call's own outputs keep their bytes.  Off is the default, and with the setting off every call returns
 * its bytes and captures its graph as before.
 *   Per plane of n_cells words v[c] >= 0, best = the record's score_q, b = the record's cell, sep = the call's min_separation:
 *   n_live = #{c : v[c] > 0}.  A cell with no pair inside the range scores 0 and is not noise.
 *   quantile_q[i], i < n_ranks, is the word at index (ranks[i] * (n_live - 1)) div 65535 of the live words sorted ascending:
 *     rank 0 is the smallest live word, rank 65535 is best, equal ranks give equal words.  quantile[i] is that word as the
 *     call converts score_q to score: (double)q * 2^-32 / sqrt(n_w), n_w of the plane's stack or track.
 *   foot > 0: with q0 = quantile_q[0] and d = best - q0, level_q = q0 + (d >> 16) * foot + (((d & 0xffff) * foot) >> 16), which
 *     is q0 + (d * foot) div 65536 without overflow.  foot_cells = #{c : v[c] > 0 and v[c] >= level_q}; foot_near of those lie
 *     within sep rows and columns of b; row_lo .. row_hi and col_lo .. col_hi is their bounding box (row = c div n_cols).
 *     foot == 0 leaves level_q and the footprint's fields 0.
 *   A zero record (score_q == 0) gives the all-zero statistics.  Unused words of the two arrays are 0.
 * The selection is exact and the same in every run (integer histograms; a radix selection over six 11-bit digits).
 * The record, 168 bytes, no padding: */
#define TDOA_MAP_STATS_MAX_RANKS 8
typedef struct {
    int64_t quantile_q[TDOA_MAP_STATS_MAX_RANKS];
    double  quantile[TDOA_MAP_STATS_MAX_RANKS];
    int64_t level_q;
    int32_t n_live, foot_cells, foot_near;
    int32_t row_lo, row_hi, col_lo, col_hi, reserved;
} tdoa_map_stats;

/* ranks [n_ranks], each 0 .. 65535 (32768: the median); n_ranks == 0 or ranks == NULL switches the setting off.  The ranks'
 * count and foot are one more word of a step graph's key; the ranks themselves are data, so new ranks of the same count
 * replay the captured step.  TDOA_ERR_INVALID: a NULL context, n_ranks outside 0 .. 8, foot outside 0 .. 65535. */
int tdoa_locate_set_stats(tdoa_ctx *ctx, const uint16_t *ranks /* [n_ranks] */, int n_ranks /* 0 .. 8 */, int foot /* 0 .. 65535 */);

/* The statistics of the last call of the family on this context, which downloaded them with its other outputs: out
 * [*n_planes] in the records' order.  n_planes (may be NULL) receives the count whenever there are statistics.
 * TDOA_ERR_STATE: that call computed none (the setting was off).  TDOA_ERR_INVALID: a NULL context, a NULL out, max_planes
 * less than the count. */
int tdoa_locate_last_stats(tdoa_ctx *ctx, tdoa_map_stats *out, int max_planes, int *n_planes);

/* Sub-sample locate: band-limited upsampling of the stacked surfaces.  The delay table and the clock rows carry 1/16 sample,
 * the surfaces Q exist at whole lags only: lag_p(c) rounds d / 16 to a whole lag, so no cell is told from its neighbour below
 * one lag (150 m of range difference at 2 Msps).  With the setting U in {2, 4, 8, 16}, the four calls of the delay-table
 * family, their tdoa_debug_*_from_q and tdoa_group_* forms score the cells on Q upsampled to 1/U sample.  U = 1 is the default
 * and off: every call returns its bytes and captures its graph as before.
 *   The upsampled row: for a row Q[l], -max_lag < l < max_lag, of n = 2 max_lag - 1 lags, n_U = (n - 1) U + 1 words; index u
 *     stands for lag u / U - (max_lag - 1).
 *       Q_U[U l + r] = floor((sum over k = 0 .. 15 of h_r[k] Q[l + k - 7] + 2^14) / 2^15),  r = 0 .. U - 1, Q outside the range = 0
 *     h_r = h16[r 16 / U] of a committed table h16[16][16] of int32 at scale 2^15,
 *       h16[rho][k] = rint(2^15 sinc(x) kaiser_6(x / 8)),  x = k - 7 - rho / 16    (a 16-tap Kaiser-windowed sinc, beta = 6).
 *     The table is normative: the same 256 literals in csrc/stack_upsample.hpp and tdoa_amd/upsample.py
 *     (tdoa_locate_upsample_taps returns them); nothing computes a tap at run time.  Phase 0 is the delta: Q_U[U l] = Q[l].
 *     The sum is exact integer arithmetic, rounded half up by the floor; defined for |Q| <= 2^60.
 *   The search: the family's calls as documented, on Q_U, U * table, U * clock, U * guard, with n_U lags from -(max_lag - 1) U.
 *     The lag rule on d' = U d is sgn(d) * ((2|d| U + 16) div 32): the nearest 1/U lag, halves away from zero.
 *     min_separation, max_step and the map statistics are in cells and do not change.
 *   The outputs keep their layouts.  lags are in units of 1/U sample: a range difference is lag / (U * sample_rate) * c.
 *     corr is the signed C of Q_U there.  The excluded intervals of the _multi calls are guard * U fine lags around the fine
 *     centres.  A pair counts in pairs_in when its fine lag is inside the fine range.
 *   Overflow: |Q_U| <= 2.04 |Q| + 1.  With U > 1 the calls return TDOA_ERR_UNSUPPORTED when 4 * P * (stack length in use)
 *     > 2^17 (the tracks' bound on the windows of a track is tightened by the same factor 4), and when a table or clock entry
 *     has |t| * U >= 2^31.  TDOA_ERR_NOMEM when the upsampled surfaces [n_stacks_total][n_pairs][n_U] do not fit;
 *     tdoa_last_error says so.  Surfaces larger than the device's whole memory are refused by arithmetic, before anything is
 *     allocated; a size between the free and the whole memory is refused when its allocation fails, with the same message.
 *   The group's searches run on the merged sum: upsampling comes after the merge (the rounding is not linear).
 * U is one more word of a step graph's key; table, clocks and taps are data.  U * table and U * clock differences are kept
 * on the device beside the originals and remade when the table, the clocks or U change (here, in tdoa_locate_set_table and
 * in tdoa_locate_set_clock), so this call needs the device when U > 1 and a table or clocks are set.
 * TDOA_ERR_INVALID: a NULL context, U not one of 1, 2, 4, 8, 16. */
int tdoa_locate_set_upsample(tdoa_ctx *ctx, int U);

/* Host only, no device: the U phases' taps, taps[r][k] = h16[r 16 / U][k].  TDOA_ERR_INVALID: NULL taps, a bad U. */
int tdoa_locate_upsample_taps(int U, int32_t *taps /* [U][16] */);

/* tests only: the upsampler on the caller's rows q [n_rows][2*max_lag-1] -> out [n_rows][(2*max_lag-2)*U+1].  Needs a context
 * for max_lag and the device, and no captures; the context's own setting is not read.  Precondition: |q| <= 2^60.
 * TDOA_ERR_INVALID: a NULL context, q or out NULL, n_rows < 1, a bad U. */
int tdoa_debug_upsample_q(tdoa_ctx *ctx, const int64_t *q, int n_rows, int U, int64_t *out);

/* Zoom locate: a fine table searched around each stack's best cell.  The family finds an emitter in two steps: the best cell
 * of a coarse grid, then a finer grid around that cell, on whole lags or on the upsampled surfaces.  A context holds one table
 * and every stack of a call has another best cell, so the second step used to be one table upload and one call per stack.
 * Interpolating the coarse table on the device is no substitute: near a station range is a cone, and a bilinear table is
 * wrong by more than a sample there.  The fine delays are data, like everything else the family is given.
 *   The fine table: a second table of the context, delay[n_cells_f][n_stations] in n_cols_f columns, that covers the whole area
 *     at Z cells per coarse cell: fine cell (Z r, Z c) is meant to be coarse cell (r, c).  The library does not check that; it
 *     is the caller's table.  Units, limits, the station-major upload and the "forget" form are tdoa_locate_set_table's.  With
 *     the setting U > 1 it gets its U-scaled copy wherever the table gets one.  Its shape (n_cells_f, n_cols_f) is part of a
 *     step graph's key; its contents are data.  The last row may be short.
 *   The coarse stage is tdoa_process_locate on the context's table, clocks, upsample setting and statistics setting: the first
 *     four outputs are its bytes, and tdoa_locate_last_stats returns what it returns after that call.  The zoom's own map is
 *     not judged.
 *   The window: stack s has the location cell* = (r*, c*) in the coarse table's coordinates.  Its window is the positions
 *     (wa, wb), 0 <= wa, wb <= 2H; a position's fine row is Z r* - H + wa and its fine column is Z c* - H + wb.  A position
 *     competes when its row is >= 0, its column is in 0 .. n_cols_f - 1 and its fine cell index row * n_cols_f + col is
 *     < n_cells_f.  The centre is read on the device, so one captured graph serves every block.
 *   The score of a competing position is score_q of its fine cell exactly as the family defines it: the lag rule on the fine
 *     table's differences, plus the stack's clock differences where a clock table is set; with U > 1 the rule
 *     sgn(d) * ((2|d| U + 16) div 32) on Q_U.  A pair outside the searched range counts 0.  The words of Q are the same, and
 *     so is the overflow bound.
 *   The zoom's cell is the competing position with the largest score.  Among equal maxima the smaller fine cell index wins.
 *   The zero record: a stack with no location (the zero coarse record) gets the zero tdoa_zoom, zero lags and correlations and
 *     a zmap of -1 throughout.  A stack whose window's largest score is 0, or whose window has no competing position, also
 *     gets the zero record and zero lags and correlations; its zmap still holds its scores.
 * The record, 64 bytes, no padding: */
typedef struct {
    int32_t cell, runner_cell, pairs_in, n_best;     /* cell: the fine cell index; pairs_in there; n_best: the competing
                                                        positions with exactly score_q */
    int32_t row_lo, row_hi, col_lo, col_hi;          /* the smallest and largest fine row and column among those positions */
    int64_t score_q, runner_q;
    double  score, runner_up;                        /* (double)x_q * 2^-32 / sqrt(n_w) */
} tdoa_zoom;
/*   The runner-up is the largest score over competing positions with max(|row - row_z|, |col - col_z|) > fine_separation,
 *     with the same tie rule; runner_q, runner_up and runner_cell are 0 where there is none.
 *   With whole lags the best score is a plateau of many fine cells and the smaller index is a corner of it: n_best and the box
 *     let a caller take the plateau's middle and see the fix's real resolution.
 *   zlags and zcorr hold lag_p(cell) in 1/U sample and the signed correlation there, 0 and 0.0 for a pair outside the range:
 *     what tdoa_solve_surface takes.  zmap[s][wa * (2H + 1) + wb] is the position's score, or -1 where it does not compete.
 *   What follows: with the fine table equal to the table and Z = 1, the zoom's cell, score_q, lags and correlations are the
 *     location's.  Whenever the brute-force best cell of the whole fine table (tdoa_process_locate with the fine table as the
 *     table) lies inside a stack's window, it is the zoom's cell, with the same score, lags and correlations.
 *   Scope: the rounds (tdoa_process_locate_multi) and the cell tracks are not zoomed by this call; the cell tracks have
 *     tdoa_process_locate_track_zoom.  The rounds have tdoa_process_locate_multi_zoom.
 * Two kernels behind the locate's launches, in the same step graph: nothing goes through the host.  The graph's key is the
 * locate's words plus (Z, H, fine_separation, n_cells_f, n_cols_f).
 * TDOA_ERR_INVALID (tdoa_locate_set_fine_table): what tdoa_locate_set_table refuses. */
int tdoa_locate_set_fine_table(tdoa_ctx *ctx, const int32_t *delay /* [n_cells][n_stations] */, int n_cells, int n_cols, int n_stations);

/* The refusals are the locate's, and: TDOA_ERR_INVALID: Z outside 1 .. 64, H outside 0 .. 64, fine_separation < 1, a NULL
 * zoom_host.  TDOA_ERR_STATE: no fine table, or one of another n_stations.  TDOA_ERR_UNSUPPORTED: with U > 1, a fine table
 * entry with |t| * U >= 2^31.  TDOA_ERR_NOMEM: the window maps [n_stacks_total][(2H+1)^2] do not fit; tdoa_last_error gives
 * the sizes. */
int tdoa_process_locate_zoom(tdoa_ctx *ctx, int windows_per_stack, int min_separation, int Z, int H, int fine_separation,
                             tdoa_location *loc_host, int32_t *lags_host, double *corr_host, int64_t *map_host /* tdoa_process_locate's */,
                             tdoa_zoom *zoom_host   /* [n_stacks_total], required */,
                             int32_t *zlags_host    /* [n_stacks_total][n_pairs], may be NULL */,
                             double  *zcorr_host    /* same shape, may be NULL */,
                             int64_t *zmap_host     /* [n_stacks_total][(2H+1)^2], may be NULL */);

/* tests only: the same kernels on the caller's words, as tdoa_debug_locate_from_q, with the context's table, fine table, clocks
 * and settings; outputs as tdoa_process_locate_zoom's with n_sets for n_stacks_total.  Refuses what that call and
 * tdoa_debug_locate_from_q refuse. */
int tdoa_debug_locate_zoom_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int min_separation, int Z, int H,
                                  int fine_separation, tdoa_location *loc, int32_t *lags, double *corr, int64_t *map, tdoa_zoom *zoom,
                                  int32_t *zlags, double *zcorr, int64_t *zmap);

/* Zoomed rounds: every emitter round refined on the fine table.  tdoa_process_locate_multi finds a weaker second or third
 * emitter of a stack, but only to a coarse cell; the zoom locate refines a stack's first emitter only.  This call runs the
 * rounds and, behind them in the same step graph, searches every round's best cell again on the context's fine table, under
 * the mask that round ran under.  No table upload, no second call, nothing through the host.
 *   The coarse stage is tdoa_process_locate_multi(windows_per_stack, n_emitters, guard, min_separation) unchanged, on the
 *     context's table, clocks, upsample setting and statistics setting: the first four outputs are its bytes, and
 *     tdoa_locate_last_stats returns what it returns after that call.  The zoom's maps are not judged.
 *   The window of round r of stack s is the zoom locate's window of (2H + 1)^2 positions around Z x that round's coarse cell,
 *     with the zoom's geometry and competing rule.
 *   The mask is M_p^r, the one round r's coarse scores ran under: the score of a competing position is the sum over the pairs
 *     of M_p^r[lag_p(fine cell)], so a pair whose lag lies within guard of a centre left by rounds 0 .. r - 1 counts 0, and so
 *     does a pair outside the searched range.  The centres stay the coarse cells' lags: a round's fine cell adds nothing to E.
 *     With the setting U > 1 everything runs on Q_U, U x the fine table, U x the clocks and U x guard, as the rounds do.
 *     Round 0 has no mask: its outputs are tdoa_process_locate_zoom's.
 *   The outputs are [round][stack][...].  zoom: the round's tdoa_zoom; pairs_in counts the pairs inside the range and not
 *     excluded at the fine cell; n_best, the box and the runner-up are taken on the round's masked window scores.  zpairs:
 *     (pairs_in, reserved), reserved the pairs inside the range but excluded at the fine cell.  zlags and zcorr: the fine
 *     cell's lags in 1/U sample and signed correlations; a pair outside the range reports 0 and 0.0, an excluded pair reports
 *     its lag and 0.0 (all bytes zero), so tdoa_solve_surface gives it no weight.  zmap: the window's masked scores, -1 where
 *     a position does not compete.
 *   The zero record: a round with the zero coarse record gets the zero tdoa_zoom, zero zpairs, zero lags and correlations and
 *     a zmap of -1 throughout.  A window with no competing position, or whose largest masked score is 0, also gets the zero
 *     record, zero zpairs, lags and correlations; its zmap still holds its scores.
 *   What follows: n_emitters = 1 returns tdoa_process_locate_zoom's eight outputs and zpairs = (pairs_in, 0); round 0 of every
 *     n_emitters is that call's.  With the fine table equal to the table and Z = 1, every round's fine cell, score_q,
 *     pairs_in, reserved, lags and correlations are that round's coarse record's.
 *   Scope: the track rounds (tdoa_process_locate_track_multi) are not zoomed, nor are rounds part of the two one-call chains
 *     (tdoa_process_sync_locate, tdoa_process_sync_drift_locate); the masks come from the coarse cells, never from the fine
 *     ones; there is no stop rule: every call runs n_emitters rounds.
 * Two kernels behind the rounds' launches for any n_emitters, the round a grid dimension.  The graph's key is the rounds'
 * words plus (Z, H, fine_separation, n_cells_f, n_cols_f) under a kind of its own.
 * The refusals are tdoa_process_locate_multi's and tdoa_process_locate_zoom's, with their messages, and a NULL zoom_host
 * (TDOA_ERR_INVALID).  TDOA_ERR_NOMEM: the window maps [n_emitters][n_stacks_total][(2H+1)^2] do not fit (they can reach
 * 70 GB); tdoa_last_error gives the sizes. */
int tdoa_process_locate_multi_zoom(tdoa_ctx *ctx, int windows_per_stack, int n_emitters, int guard, int min_separation, int Z, int H,
                                   int fine_separation, tdoa_location *loc_host, int32_t *lags_host, double *corr_host,
                                   int64_t *map_host /* tdoa_process_locate_multi's */,
                                   tdoa_zoom *zoom_host   /* [n_emitters][n_stacks_total], required */,
                                   int32_t *zpairs_host   /* [n_emitters][n_stacks_total][2], may be NULL */,
                                   int32_t *zlags_host    /* [n_emitters][n_stacks_total][n_pairs], may be NULL */,
                                   double  *zcorr_host    /* same shape, may be NULL */,
                                   int64_t *zmap_host     /* [n_emitters][n_stacks_total][(2H+1)^2], may be NULL */);

/* tests only: the same kernels on the caller's words, as tdoa_debug_locate_multi_from_q, with the context's table, fine table,
 * clocks and settings; outputs as tdoa_process_locate_multi_zoom's with n_sets for n_stacks_total.  Refuses what that call and
 * tdoa_debug_locate_multi_from_q refuse. */
int tdoa_debug_locate_multi_zoom_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int n_emitters, int guard,
                                        int min_separation, int Z, int H, int fine_separation, tdoa_location *loc, int32_t *lags,
                                        double *corr, int64_t *map, tdoa_zoom *zoom, int32_t *zpairs, int32_t *zlags, double *zcorr,
                                        int64_t *zmap);

/* Zoomed cell tracks: a block's track refined on the fine table.  The cell track exists for free-running receivers: every
 * stack of a block has its own clock row, so the block's windows can be summed map by map only, never lag by lag.  The zoom
 * locate refines one stack; this call refines a whole track in the same step graph, with no table upload and no second call
 * per block.
 *   The coarse stage is tdoa_process_locate_track(windows_per_stack, max_step, min_separation) unchanged, on the context's
 *     table, clocks, upsample setting and statistics setting.  The first six outputs are that call's bytes, and
 *     tdoa_locate_last_stats returns what it returns after that call.  The fine planes are not judged.
 *   The windows: position j of track t is stack sid = t L + j.  Its window is the zoom's window around the track's coarse cell
 *     cells[t][j] = (r, c): position (wa, wb), 0 <= wa, wb <= 2H, has the fine row Z r - H + wa and the fine column
 *     Z c - H + wb, and competes under the zoom's rule.  w_j[pos] is score_q of that fine cell under stack sid's clock row,
 *     with the zoom's lag rule and the scaled fine table where U > 1, and -1 where the position does not compete.  w_j is zmap.
 *   The recurrence runs in fine coordinates, from the last position back, with Jf = fine_step:
 *     F_{L-1}[pos] = w_{L-1}[pos].  F_j[pos] = -1 where w_j[pos] = -1.  Otherwise let m be the largest F_{j+1}[pos'] over
 *     |dr|, |dc| <= Jf, where pos' is the position of window j + 1 whose fine row and column are (row + dr, col + dc); it
 *     must lie inside that window (0 <= wa', wb' <= 2H), and a -1 there does not count.  F_j[pos] = w_j[pos] + m.  If no such
 *     position exists, F_j[pos] = -1: no continuation.  E_j[pos] is the (dr, dc) of the maximum; ties go to the smaller
 *     rank(dr), then the smaller rank(dc), rank(x) = 2|x| - (x > 0), as in the coarse recurrence.
 *     Consecutive windows are offset by Z (C_{j+1} - C_j).  With Z J > 2H + Jf they need not touch; that is the caller's
 *     choice of H and is not refused.
 *   The track: f_0 is the position with the largest F_0, equal maxima: the smaller fine cell.  f_{j+1} = f_j + E_j[f_j].
 *     zcells holds the fine cells of f_j, zown holds w_j there.  zlags and zcorr hold the fine cell's lags (1/U sample) and
 *     signed correlations under that stack's clocks, 0 and 0.0 outside the range: what tdoa_solve_surface takes.  ztotal is
 *     F_0 in the coordinates of window 0.
 *   The record is a tdoa_cell_track: cell = f_0's fine cell, positions = L, steps = the number of j with f_{j+1} != f_j,
 *     score_q = max F_0; score and runner_up are on the coarse track's scale, 2^-32 / sqrt(N_w).  The runner-up is the largest
 *     F_0 >= 0 over positions with max(|row - row_0|, |col - col_0|) > fine_separation from f_0, with the same tie rule;
 *     runner_q, runner_up and runner_cell are 0 where there is none.
 *   Zero records: a track with the zero coarse record gets the zero ztrack and zero zcells, zown, zlags and zcorr; its zmap
 *     and ztotal are -1 throughout.  A track whose largest F_0 is <= 0 gets the same zeros; its zmap and ztotal keep their
 *     words.
 *   What follows:
 *     1. L = 1: ztrack's cell, runner_cell, score_q, runner_q, score and runner_up are tdoa_process_locate_zoom's tdoa_zoom
 *        fields; zlags, zcorr and zmap are its bytes; ztotal = zmap.
 *     2. J = 0 and Jf = 0: all windows of a track coincide and ztotal = the sum over j of zmap_j word for word, -1 where a
 *        position does not compete.
 *     3. score_q = ztotal[pos(f_0)] = the sum over j of zown[j]; consecutive zcells are at most Jf fine rows and columns apart.
 *     4. With the fine table equal to the table, Z = 1 and Jf = J, ztrack.score_q = track.score_q for any H: the coarse best
 *        track runs through the windows' centres.
 *     5. ztrack.score_q is at most the score of tdoa_process_locate_track with the fine table as the table and max_step = Jf,
 *        and equals it whenever that brute-force track lies inside the windows.
 *   Scope: the rounds (tdoa_process_locate_multi, tdoa_process_locate_track_multi) are not zoomed.
 * Four kernels behind the tracks' launches, in the same step graph: nothing goes through the host, and the windows' centres
 * are data.  The graph's key is the tracks' words plus (Z, H, fine_step, fine_separation, n_cells_f, n_cols_f).
 * The refusals are tdoa_process_locate_track's, and: TDOA_ERR_INVALID: Z outside 1 .. 64, H outside 0 .. 64, fine_step outside
 * 0 .. 16, fine_separation < 1, a NULL ztrack_host.  TDOA_ERR_STATE: no fine table, or one of another n_stations.
 * TDOA_ERR_UNSUPPORTED: with U > 1, a fine table entry with |t| * U >= 2^31.  TDOA_ERR_NOMEM: the window maps
 * [n_stacks_total][(2H+1)^2], the steps E (2 bytes per stack and position) or ztotal do not fit; tdoa_last_error gives the
 * sizes.  All argument checks happen before anything needs a device. */
int tdoa_process_locate_track_zoom(tdoa_ctx *ctx, int windows_per_stack, int max_step, int min_separation, int Z, int H, int fine_step,
                                   int fine_separation,
                                   tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host, int32_t *lags_host,
                                   double *corr_host, int64_t *total_host /* tdoa_process_locate_track's */,
                                   tdoa_cell_track *ztrack_host /* [n_tracks], required; its cells are fine cell indices */,
                                   int32_t *zcells_host   /* [n_tracks][L], may be NULL */,
                                   int64_t *zown_host     /* [n_tracks][L], may be NULL */,
                                   int32_t *zlags_host    /* [n_stacks_total][n_pairs], 1/U sample, may be NULL */,
                                   double  *zcorr_host    /* same shape, may be NULL */,
                                   int64_t *zmap_host     /* [n_stacks_total][(2H+1)^2], may be NULL */,
                                   int64_t *ztotal_host   /* [n_tracks][(2H+1)^2], may be NULL */);

/* tests only: the same kernels on the caller's words, as tdoa_debug_locate_track_from_q, with the context's table, fine table,
 * clocks and settings; outputs as tdoa_process_locate_track_zoom's with n_sets for n_stacks_total and n_sets / track_len
 * tracks.  Refuses what that call and tdoa_debug_locate_track_from_q refuse. */
int tdoa_debug_locate_track_zoom_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int max_step,
                                        int min_separation, int Z, int H, int fine_step, int fine_separation, tdoa_cell_track *track,
                                        int32_t *cells, int64_t *own, int32_t *lags, double *corr, int64_t *total, tdoa_cell_track *ztrack,
                                        int32_t *zcells, int64_t *zown, int32_t *zlags, double *zcorr, int64_t *zmap, int64_t *ztotal);

/* Clocks to fix in one call.  Every capture is [reference | target | reference]: the station clocks are found on the reference
 * blocks, carried over to the target block and the target is located under them.  tdoa_process_sync_fine, a mix of its clock
 * rows, tdoa_locate_set_clock and tdoa_process_locate_zoom do that in two steps with the clocks going through the host; this
 * call does it in one step graph behind one accumulation of the stacks, and the clocks never leave the device.
 *   1. The fine clock search: tdoa_process_sync_fine(windows_per_stack, gate, rounds, U, fine_rounds, ref_delay, centre)
 *      unchanged, on every stack.  The first eight outputs are that call's bytes.
 *   2. A clock row for every stack, from the fine clocks c16 = clock16 of step 1.  Which stacks' clocks make which stack's row
 *      is data: mix[t] = (a, b, wa, wb), one entry per stack, and for station s, in 64 bits,
 *        den = wa + wb,  T = wa c16[a][s] + wb c16[b][s],  row[t][s] = sgn(T) ((2 |T| + den) div (2 den)):
 *      the nearest integer to T / den, halves away from zero.  Two identities:
 *        (t, t, 1, 0) is the stack's own clock, row[t] = c16[t];
 *        (a, b, 1, 1) is the midpoint of two rows, sgn(T) ((|T| + 1) div 2), the rule the target block of
 *        tdoa_processor --sync-fine gets.
 *      Unequal weights give a ramp between two reference stacks.  The sum is rounded, not an increment: a ramp that rounds
 *      its step and adds it (as the coarse clocks' ramp does) differs from this on exact halves of opposite sign, and the two
 *      are not claimed equal.  mix == NULL: every stack takes its own clock.  A stack whose fine record is the zero record
 *      contributes its zero clocks like any other; the records tell.  rows_host receives the rows.
 *   3. The zoom locate: tdoa_process_locate_zoom(windows_per_stack, min_separation, Z, H, fine_separation) unchanged, on every
 *      stack, under those rows: the last eight outputs are that call's bytes after tdoa_locate_set_clock(rows).  It honours the
 *      context's table, fine table, upsample setting and statistics setting as that call does, and tdoa_locate_last_stats
 *      returns what it returns after that call.
 * The context's own clock table (tdoa_locate_set_clock) is neither read nor changed, whatever its shape: the call after
 * this one finds it as it was.
 * One kernel between the two searches' launches; the mix, like ref_delay and centre, is data: a new mix, new delays, centres,
 * table or fine table of the same shape replay the captured graph.  The graph's key is both searches' words, the locate's
 * clock flag on.
 * Scope: the chain for free-running receivers (tdoa_process_sync_drift_fine, the line continued, tdoa_process_locate_track_zoom)
 * needs tdoa_sync_line_clock16's rule on the device, not a mix, and is not this call but tdoa_process_sync_drift_locate, below;
 * the rounds of tdoa_process_locate_multi are in neither.  fine_rounds = 0 gives clock16 = 16 clock, the coarse clock search alone; Z = 1, H = 0 with the
 * fine table set to the table is the form without a zoom.
 * The refusals are those of the two calls, and: TDOA_ERR_INVALID: a mix entry with a or b outside 0 .. n_stacks_total - 1, a
 * negative weight, or wa + wb outside 1 .. 65536.  TDOA_ERR_UNSUPPORTED: with the upsample setting U_loc > 1, a station with
 * 16 (|centre| + gate + 1) U_loc >= 2^31: a row times the factor might not fit 32 bits (the message is the clock table's).
 * The weights form a convex combination, so |row| <= max |c16| <= 16 (|centre| + gate + 1), and no value on the device needs
 * a check.  All checks happen before anything needs a device. */
typedef struct {
    int32_t a, b;         /* the two stacks whose fine clocks are mixed */
    int32_t wa, wb;       /* their weights, >= 0, 1 <= wa + wb <= 65536 */
} tdoa_clock_mix;

int tdoa_process_sync_locate(tdoa_ctx *ctx, int windows_per_stack, int gate /* G */, int rounds /* R */, int U, int fine_rounds /* Rf */,
                             const int32_t *ref_delay /* [n_stations] */, const int32_t *centre /* [n_stations], NULL: all 0 */,
                             const tdoa_clock_mix *mix /* [n_stacks_total], NULL: every stack its own clock */,
                             int min_separation, int Z, int H, int fine_separation,
                             tdoa_sync *sync_host, int32_t *clock_host, int32_t *lags_host, double *corr_host,
                             tdoa_sync *fine_host, int32_t *clock16_host, int32_t *fine_lags_host,
                             double *fine_corr_host /* tdoa_process_sync_fine's eight; sync_host and fine_host required */,
                             int32_t *rows_host /* [n_stacks_total][n_stations], 1/16 sample, may be NULL */,
                             tdoa_location *loc_host, int32_t *loc_lags_host, double *loc_corr_host, int64_t *map_host,
                             tdoa_zoom *zoom_host, int32_t *zlags_host, double *zcorr_host,
                             int64_t *zmap_host /* tdoa_process_locate_zoom's eight; loc_host and zoom_host required */);

/* tests only: the same kernels on the caller's words, as tdoa_debug_sync_fine_from_q and tdoa_debug_locate_zoom_from_q, with
 * the context's table, fine table and settings; mix is [n_sets] and names sets.  Refuses what the call and those two refuse. */
int tdoa_debug_sync_locate_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int n_stations, int n_w, int gate, int rounds, int U,
                                  int fine_rounds, const int32_t *ref_delay, const int32_t *centre, const tdoa_clock_mix *mix,
                                  int min_separation, int Z, int H, int fine_separation, tdoa_sync *sync_host, int32_t *clock_host,
                                  int32_t *lags_host, double *corr_host, tdoa_sync *fine_host, int32_t *clock16_host, int32_t *fine_lags_host,
                                  double *fine_corr_host, int32_t *rows_host, tdoa_location *loc_host, int32_t *loc_lags_host,
                                  double *loc_corr_host, int64_t *map_host, tdoa_zoom *zoom_host, int32_t *zlags_host, double *zcorr_host,
                                  int64_t *zmap_host);

/* Host only: step 2 in plain C.  clock16 [n_stacks][n_stations], mix [n_rows] -> rows [n_rows][n_stations].
 * TDOA_ERR_INVALID: a NULL pointer, a count < 1, or a mix entry the call above refuses (a, b against n_stacks). */
int tdoa_clock_mix_rows(const int32_t *clock16, int n_stacks, int n_stations, const tdoa_clock_mix *mix, int n_rows, int32_t *rows);

/* tests only: the kernel of step 2 alone on the caller's clocks, with U_loc (1, 2, 4, 8 or 16) an argument; the context's
 * setting is not read.  rows [n_rows][n_stations]; cdiff [n_rows][n_pairs] = row[j] - row[i] in tdoa_locate_set_clock's pair
 * order (i < j, i first); cdiff_up = U_loc x cdiff: the two arrays the family's kernels take.  All outputs required.
 * TDOA_ERR_INVALID as tdoa_clock_mix_rows, n_stacks or n_rows above 65535, n_stations outside 2 .. 64, another U_loc. */
int tdoa_debug_clock_mix(tdoa_ctx *ctx, const int32_t *clock16, int n_stacks, int n_stations, const tdoa_clock_mix *mix, int n_rows,
                         int U_loc, int32_t *rows, int64_t *cdiff, int64_t *cdiff_up);

/* Free-running clocks to fix in one call.  Receivers whose clocks run free have no stable offset to carry from the reference
 * blocks to the target block: a line per station is found on a reference block (offset and rate), continued over the target
 * block, and the target is tracked under those rows.  tdoa_process_sync_drift_fine, tdoa_sync_line_clock16 on the host,
 * tdoa_locate_set_clock and tdoa_process_locate_track_zoom do that in two steps that accumulate the same windows twice, with
 * the clocks going through the host; this call does it in one step graph behind one accumulation of the stacks, and the
 * lines never leave the device.
 *   1. The fine clock lines: tdoa_process_sync_drift_fine(windows_per_stack, gate, max_drift, drift_den, rounds, U,
 *      fine_rounds, ref_delay, centre) unchanged, on every block.  The first twelve outputs are that call's bytes.
 *   2. A clock row for every stack, from the lines' c16 = clock16 and eta = fine_rate of step 1.  Which lines, continued to
 *      which positions, make which stack's row is data: mix[t] = (a, xa, b, xb, wa, wb), one entry per stack, and for station
 *      s, in 64-bit integers,
 *        cont(l, x)[s] = c16[l][s] + r(16 eta[l][s] x, U drift_den)
 *        row[t][s] = sgn(T) ((2 |T| + den) div (2 den)),  T = wa cont(a, xa)[s] + wb cont(b, xb)[s],  den = wa + wb.
 *      cont is tdoa_sync_line_clock16's rule: r the nearest integer, halves away from zero.  x is signed: a negative x
 *      continues a line backwards, so the line of the reference block after the target serves as well as the one before.
 *      The mean is tdoa_clock_mix's: the nearest integer to T / den, halves away from zero.  Two identities:
 *        (l, x, l, x, 1, 0) is line l continued to x, tdoa_sync_line_clock16's word;
 *        (0, L + j, 2, j - L, L - j, j + 1) on stack j of the middle one of three blocks of L stacks is the line before
 *        continued forwards and the line after continued backwards, weighted by nearness.
 *      mix == NULL: stack l L + x takes (l, x, l, x, 1, 0), its own line at its own position.  At U = 16 these rows are
 *      fine_rows byte for byte.  At U < 16 they differ from fine_rows by less than 1/U sample: fine_rows rounds the
 *      continuation in units of 1/U sample and scales by 16 / U, this rule rounds it in units of 1/16 sample.
 *      mix_rows_host receives the rows.
 *   3. The zoomed cell tracks: tdoa_process_locate_track_zoom(windows_per_stack, max_step, min_separation, Z, H, fine_step,
 *      fine_separation) unchanged, on every block, under those rows: the last thirteen outputs are that call's bytes after
 *      tdoa_locate_set_clock(rows), the coarse tracks' lags and corr under loc_lags_host and loc_corr_host.  It honours the
 *      context's table, fine table, upsample setting and statistics setting as that call does, and tdoa_locate_last_stats
 *      returns what it returns after that call.
 * Both searches run on every block: a line on the target block and a track on a reference block are returned for what they
 * are worth.  Lines and tracks are the same sets, a block's stacks.
 * The context's own clock table (tdoa_locate_set_clock) is neither read nor changed, whatever its shape: the call after
 * this one finds it as it was.
 * One kernel between the two searches' launches; the mix, like ref_delay and centre, is data: a new mix, new delays, centres,
 * table or fine table of the same shape replay the captured graph.  The graph's key is both searches' words, the tracks'
 * clock flag on.
 * Scope: the rounds of tdoa_process_locate_track_multi are not this call; Z = 1, H = 0 with the fine table set to the table is
 * the form without a zoom.
 * The refusals are those of the two calls, and: TDOA_ERR_INVALID: a mix entry with a or b outside 0 .. n_lines - 1 (n_lines = 3),
 * |xa| or |xb| above 65535, a negative weight, or wa + wb outside 1 .. 65536; with X the larger of L - 1 and the mix's largest
 * |x|, a station with |centre| + gate + 2 + ((max_drift + 1) X) div drift_den >= 2^27: a row in 1/16 sample would not fit int32.
 * TDOA_ERR_UNSUPPORTED: with the upsample setting U_loc > 1, a station with 16 times that sum times U_loc >= 2^31 (the message is
 * the clock table's); TDOA_LAGS_GO.  The bound follows from |clock16| <= 16 (|centre| + gate + 1) and |fine_rate| <=
 * U (max_drift + 1); the mean is a convex combination, so no value on the device needs a check.  All checks happen before
 * anything needs a device. */
typedef struct {
    int32_t a, xa;        /* a line and the position it is continued to, |xa| <= 65535 */
    int32_t b, xb;        /* another (or the same), |xb| <= 65535 */
    int32_t wa, wb;       /* their weights, >= 0, 1 <= wa + wb <= 65536 */
} tdoa_line_mix;

int tdoa_process_sync_drift_locate(tdoa_ctx *ctx, int windows_per_stack, int gate /* G */, int max_drift, int drift_den,
                                   int rounds /* R */, int U, int fine_rounds /* Rf */, const int32_t *ref_delay /* [n_stations] */,
                                   const int32_t *centre /* [n_stations], NULL: all 0 */,
                                   const tdoa_line_mix *mix /* [n_stacks_total], NULL: every stack its own line at its own position */,
                                   int max_step, int min_separation, int Z, int H, int fine_step, int fine_separation,
                                   tdoa_sync_line *line_host, int32_t *clock_host, int32_t *rate_host, int32_t *rows_host,
                                   int32_t *lags_host, double *corr_host, tdoa_sync_line *fine_host, int32_t *clock16_host,
                                   int32_t *fine_rate_host, int32_t *fine_rows_host, int32_t *fine_lags_host,
                                   double *fine_corr_host /* tdoa_process_sync_drift_fine's twelve; line_host and fine_host required */,
                                   int32_t *mix_rows_host /* [n_stacks_total][n_stations], 1/16 sample, may be NULL */,
                                   tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host, int32_t *loc_lags_host,
                                   double *loc_corr_host, int64_t *total_host, tdoa_cell_track *ztrack_host, int32_t *zcells_host,
                                   int64_t *zown_host, int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host,
                                   int64_t *ztotal_host /* tdoa_process_locate_track_zoom's thirteen; track_host and ztrack_host required */);

/* tests only: the same kernels on the caller's words, as tdoa_debug_sync_drift_fine_from_q and
 * tdoa_debug_locate_track_zoom_from_q, with the context's table, fine table and settings: set t track_len + x is position x of
 * line and track t, mix is [n_sets] and names the n_sets / track_len lines.  Refuses what the call and those two refuse. */
int tdoa_debug_sync_drift_locate_from_q(tdoa_ctx *ctx, const int64_t *q, int n_sets, int track_len, int n_stations, int n_w, int gate,
                                        int max_drift, int drift_den, int rounds, int U, int fine_rounds, const int32_t *ref_delay,
                                        const int32_t *centre, const tdoa_line_mix *mix, int max_step, int min_separation, int Z, int H,
                                        int fine_step, int fine_separation, tdoa_sync_line *line_host, int32_t *clock_host,
                                        int32_t *rate_host, int32_t *rows_host, int32_t *lags_host, double *corr_host,
                                        tdoa_sync_line *fine_host, int32_t *clock16_host, int32_t *fine_rate_host, int32_t *fine_rows_host,
                                        int32_t *fine_lags_host, double *fine_corr_host, int32_t *mix_rows_host, tdoa_cell_track *track_host,
                                        int32_t *cells_host, int64_t *own_host, int32_t *loc_lags_host, double *loc_corr_host,
                                        int64_t *total_host, tdoa_cell_track *ztrack_host, int32_t *zcells_host, int64_t *zown_host,
                                        int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host, int64_t *ztotal_host);

/* Host only: step 2 in plain C.  clock16, fine_rate [n_lines][n_stations], mix [n_rows] -> rows [n_rows][n_stations].
 * TDOA_ERR_INVALID: a NULL pointer, a count < 1, U not a factor (2, 4, 8, 16), drift_den < 1, a mix entry the call above
 * refuses (a, b against n_lines), or a continued clock that does not fit int32 (the words are the caller's, so they are
 * looked at one by one). */
int tdoa_line_mix_rows(const int32_t *clock16, const int32_t *fine_rate, int n_lines, int n_stations, int U, int drift_den,
                       const tdoa_line_mix *mix, int n_rows, int32_t *rows);

/* tests only: the kernel of step 2 alone on the caller's words, with U_loc (1, 2, 4, 8 or 16) an argument; the context's
 * setting is not read.  rows [n_rows][n_stations]; cdiff [n_rows][n_pairs] = row[j] - row[i] in tdoa_locate_set_clock's pair
 * order (i < j, i first); cdiff_up = U_loc x cdiff: the two arrays the family's kernels take.  All outputs required.
 * TDOA_ERR_INVALID as tdoa_line_mix_rows, n_lines or n_rows above 65535, n_stations outside 2 .. 64, another U_loc. */
int tdoa_debug_line_mix(tdoa_ctx *ctx, const int32_t *clock16, const int32_t *fine_rate, int n_lines, int n_stations, int U, int drift_den,
                        const tdoa_line_mix *mix, int n_rows, int U_loc, int32_t *rows, int64_t *cdiff, int64_t *cdiff_up);

/* Capture-quality statistics of every (window, station) in one streaming pass over the bytes
 * in HBM: the byte statistics of fastAnalyzeSamples
 * (fast_analyzer.go:117-155) and the block power of validateDataFile (collector.go:219-224).
 * Exact integer sums on the GPU, so every field equals the reference's float64 result. */
typedef struct {
    int64_t n_samples;
    double  i_avg, q_avg, i_std, q_std;   /* fast_analyzer.go:139-142                     */
    double  power_level;                  /* dB, floor -100 (:146-151)                    */
    double  mean_power;                   /* mean of (I-127.5)^2+(Q-127.5)^2 (collector.go:219-224) */
    int32_t i_min, i_max, q_min, q_max;
    int32_t has_clipping, has_overload;   /* :154-155                                     */
} tdoa_window_quality;
/* out_host [n_windows_total][n_stations]; windows of other ranks are zero-filled */
int tdoa_window_quality_all(tdoa_ctx *ctx, int rank, int world, tdoa_window_quality *out_host);
/* the same statistics of one host buffer of raw IQ */
int tdoa_window_quality_u8(tdoa_ctx *ctx, const uint8_t *iq, size_t n_samples, tdoa_window_quality *out);

/* inspection hooks used by the parity tests.  tdoa_fm_preprocess_u8: the normalised discriminator output of one window
 * and its statistics; out_f32 == NULL runs the statistics-only pass of the default (fused) path instead of the one that
 * also writes the codes -- both must give the same statistics */
int tdoa_fm_preprocess_u8(tdoa_ctx *ctx, const uint8_t *iq, size_t n, float *out_f32, tdoa_fm_stats *stats);
int tdoa_fm_xcorr_lags_u8(tdoa_ctx *ctx, const uint8_t *iq1, size_t n1, const uint8_t *iq2, size_t n2,
                          int max_lag, double *lags_out /* [2*max_lag-1] */);

/* tests only: run the selection kernel of tdoa_process_peaks on a caller's raw surface (n_lags values for the lags
 * lag_lo, lag_lo + 1, ...) with scale 1; peak 1 comes from the surface like the others.  A peak key orders lags by
 * 2 |lag| in 31 bits: every lag of the surface must lie in -(2^30 - 1) .. 2^30 - 1, TDOA_ERR_INVALID otherwise */
int tdoa_debug_select_peaks(tdoa_ctx *ctx, const float *surface, int n_lags, int lag_lo, int k, int min_separation,
                            tdoa_peak *peaks, int32_t *count);
/* tests only: run the any-size fallback kernels even where a hot-size kernel exists */
int tdoa_debug_force_generic(tdoa_ctx *ctx, int on);
/* tests / measurements only: pick kernel variants by hand.  flags == 0 is the library's default path; every bit
 * set switches one specialised form OFF.  The same switches can be given once, at tdoa_create time, through the
 * environment (TDOA_NO_SHORT_LAG=1, TDOA_NO_SEGMENT_FORM=1, TDOA_NO_SEGMENT_QUADS=1, TDOA_NO_XCD_ROWS=1,
 * TDOA_NO_DECIMATE=1, TDOA_NO_FUSED_K1=1, TDOA_NO_K1_ONCE=1, TDOA_NO_SEG_PACK3=1, TDOA_NO_DEC_COLS=1, TDOA_POW2_ONLY=1); results are the same to rounding whichever form runs. */
enum {
    TDOA_DEBUG_GENERIC_KERNELS = 1,  /* any-size LDS radix-4 kernels instead of the radix-16 register kernels        */
    TDOA_DEBUG_NO_SHORT_LAG    = 2,  /* general pruned inverse even when the search range is below 4095 lags          */
    TDOA_DEBUG_NO_FUSED_K1     = 4,  /* K1 always writes its 24-bit codes to memory (int32); the forward column kernels
                                        read them instead of evaluating the discriminator on the capture bytes      */
    TDOA_DEBUG_NO_SEGMENT_FORM = 8,  /* no LDS-resident overlap-save correlation for search ranges up to 1024 lags    */
    TDOA_DEBUG_NO_XCD_ROWS     = 16, /* plain 2-D grid of the pair kernel even with more pairs than stations          */
    TDOA_DEBUG_NO_SEGMENT_QUADS = 64, /* segment form one pair-window at a time: no station transforms shared by pairs */
    TDOA_DEBUG_NO_DECIMATE     = 256, /* full inverse transform even where the decimated one applies (4096 x 256 / x 512 plans, search ranges above 4095 lags) */
    TDOA_DEBUG_NO_K1_ONCE      = 512, /* the K1 statistics pre-pass everywhere: no single-look K1 (every capture byte read once,
                                        the mean's residual removed where the lags come out; csrc/k1_single_look.hpp)      */
    TDOA_DEBUG_NO_SEG_PACK3    = 1024, /* the segment form reads int32 code rows instead of the packed 3-byte ones        */
    TDOA_DEBUG_NO_DEC_COLS     = 2048, /* the decimated pair step as 4096-bin tiles in LDS (k_pair_decimate16) instead of the column
                                        walk (csrc/dec_stream.hpp); 4096 x 4096 plans then take the full inverse             */
    TDOA_DEBUG_DEC_COLS_ALWAYS = 4096, /* (switches a form ON) the column walk wherever the decimated inverse
                                        applies, also where the library would pick the tile form (as many pairs as stations)  */
    TDOA_DEBUG_NO_DEC_STAGED   = 16384, /* the column walk one pair-window per wave straight from memory (k_pair_decimate_cols)
                                        instead of one workgroup per window and column block with the stations' rows staged in
                                        LDS (csrc/dec_staged.hpp; environment: TDOA_NO_DEC_STAGED=1)                            */
    TDOA_DEBUG_POW2_ONLY       = 8192, /* transform lengths are powers of two everywhere (the reference's padding rule,
                                        processor.go:563): ten-second windows then run in N = 2^25 instead of 5 x 2^22
                                        (environment: TDOA_POW2_ONLY=1)                                                      */
    TDOA_DEBUG_NO_SMALL_FUSED  = 32768, /* the decimated inverse's small plan as two kernels (row pass -> V' -> column sums + K5)
                                        instead of one workgroup per pair-window that keeps the column sums in registers
                                        (k_small_rows_col_peak; environment: TDOA_NO_SMALL_FUSED=1)                            */
    TDOA_DEBUG_SMALL_FUSED_ALWAYS = 65536 /* (switches a form ON) ... for any number of pair-windows; the library takes it from
                                        1024 pair-windows per launch on (environment: TDOA_SMALL_FUSED_ALWAYS=1).  Never in a
                                        batch that refines: the refinement reads V', which the one kernel does not write      */
};
int tdoa_debug_flags(tdoa_ctx *ctx, unsigned flags);
/* inspection: the K1 statistics of station-window `sw_index` of the last batch (the order of the batch's descriptors:
 * pair calls 0 = first input, 1 = second; tdoa_process: window-major, stations in the order of first use), and whether
 * that batch took the single-look path (every capture byte read once; statistics from the column kernels' tile sums). */
int tdoa_debug_last_k1(tdoa_ctx *ctx, int sw_index, tdoa_fm_stats *stats, int32_t *single_look);
/* tests only: structure of the hipGraph the last tdoa_process captured -- info = {nodes, edges, root nodes, memset nodes};
 * dot_path (may be NULL): also writes the graph in Graphviz form (hipGraphDebugDotPrint).  The library itself refuses a
 * captured step that is not ONE dependency chain of kernel nodes (TDOA_ERR_STATE), see DESIGN.md section 7. */
int tdoa_debug_graph_info(tdoa_ctx *ctx, int32_t info[4], const char *dot_path);
/* tests only: fill the context's float workspaces -- G, V, V', the edge sums, the staged spectra and the segment sums (one
 * buffer), TZ, the refinement's raw neighbours and the single-look edge sums -- over their whole capacity with a quiet NaN
 * (0x7FC00000), then synchronise.  A later call that reads a value it did not write shows NaN instead of an earlier call's
 * bytes.  Buffers of integers, descriptors, peak keys, statistics or phase codes are left alone; unallocated ones are
 * skipped.  TDOA_ERR_INVALID for a NULL context. */
int tdoa_debug_poison_workspace(tdoa_ctx *ctx);
/* tests only (host): the kernel forms of the last batch the library planned (for a replayed step graph: of the batch it
 * captured).  info[TDOA_ROUTE_*] below; TDOA_ERR_STATE before any batch ran. */
enum {
    TDOA_ROUTE_INVERSE = 0,      /* TDOA_INV_*                                                                         */
    TDOA_ROUTE_PAIR_STEP = 1,    /* TDOA_STEP_* (the decimated inverse's pair step; TDOA_STEP_TILES otherwise)          */
    TDOA_ROUTE_COL_PASS = 2,     /* TDOA_COL_*                                                                         */
    TDOA_ROUTE_ROW_PASS = 3,     /* TDOA_ROW_*                                                                         */
    TDOA_ROUTE_FK = 4,           /* short-lag form: column blocks of 256 per side (0: not that form)                   */
    TDOA_ROUTE_SEG_PQ = 5,       /* segment form: search reach in units of 256 lags (0: not that form)                 */
    TDOA_ROUTE_SEG_QUADS = 6,    /* 0/1 below: station quads chosen (only the segment form uses them)                  */
    TDOA_ROUTE_SEG_PACK3 = 7,    /* segment form reads 3-byte codes                                                    */
    TDOA_ROUTE_FUSED_K1 = 8,     /* discriminator inside the forward column kernels                                    */
    TDOA_ROUTE_ONCE = 9,         /* single-look K1                                                                      */
    TDOA_ROUTE_SMALL_FUSED = 10, /* the decimated inverse's small plan in one kernel (k_small_rows_col_peak)             */
    TDOA_ROUTE_PRUNED = 11,      /* pruned inverse column pass                                                          */
    TDOA_ROUTE_XCD_PAIRS = 12,   /* k_inv_row_pair4096 on its XCD-grouped 1-D grid                                      */
    TDOA_ROUTE_DEC_GP = 13,      /* k_pair_decimate16 on its XCD-grouped grid                                           */
    TDOA_ROUTE_STG_FOLDED = 14,  /* staged column walk without a loader wave                                            */
    TDOA_ROUTE_STG_BLOCKED = 15  /* staged column walk, a BIT FIELD (test the bits below, not == 1):                     */
                                 /* TDOA_ROUTE_STG_BLOCKED_BIT | TDOA_ROUTE_STG_MERGED_BIT | TDOA_ROUTE_K1_SPLIT_BIT |  */
                                 /* TDOA_ROUTE_STG_PAIRED_BIT | TDOA_ROUTE_STG_NT_BIT                                   */
};
enum { TDOA_INV_NONE = 0, TDOA_INV_SEGMENTS = 1, TDOA_INV_DECIMATED = 2, TDOA_INV_SHORT_LAG = 3, TDOA_INV_FULL = 4 };
enum { TDOA_STEP_TILES = 0, TDOA_STEP_COLUMNS = 1, TDOA_STEP_STAGED = 2 };
enum {
    TDOA_COL_NONE = 0, TDOA_COL_K1_256 = 1, TDOA_COL_K1_512 = 2, TDOA_COL_K1_TWO_SWEEP = 3, TDOA_COL_C256 = 4,
    TDOA_COL_TWO_SWEEP = 5, TDOA_COL_SHORT16X = 6, TDOA_COL_COLX = 7, TDOA_COL_GENERIC = 8
};
enum {
    TDOA_ROW_NONE = 0, TDOA_ROW_UNPACK_BLOCKS = 1, TDOA_ROW_UNPACK_IN_PLACE = 2, TDOA_ROW_UNPACK_TILES = 3, TDOA_ROW_HOT = 4,
    TDOA_ROW_GENERIC = 5
};
/* info[TDOA_ROUTE_STG_BLOCKED]: */
#define TDOA_ROUTE_STG_BLOCKED_BIT 1 /* the walk reads spectra in blocks of 64 columns                                      */
#define TDOA_ROUTE_STG_MERGED_BIT 2  /* ... and adds the neighbour shares inside a block itself: only the block-edge        */
                                     /* columns' shares go through memory                                                   */
#define TDOA_ROUTE_K1_SPLIT_BIT 4    /* (same slot) the fused column kernel looks angles up in the 96 KB split half-plane     */
                                     /* table -- 160 KB of LDS -- instead of the quadrant table (TDOA_K1_QUAD_TABLE=1)        */
                                     /* (the 4096 x 512 plan's kernel: only under TDOA_K1_SPLIT_512=1)                        */
#define TDOA_ROUTE_STG_PAIRED_BIT 8  /* ... the blocks are paired lines: a row's 64 columns of block cb, then the partner    */
                                     /* row's 64 columns of block 63 - cb -- one KB per LDS-DMA (TDOA_NO_STG_PAIRED=1: off)  */
#define TDOA_ROUTE_STG_NT_BIT 16     /* ... and the loader wave's LDS-DMA is non-temporal: one pair group per window, every  */
                                     /* staged byte read once (TDOA_NO_STG_NT=1: off)                                        */
int tdoa_debug_last_route(const tdoa_ctx *ctx, int32_t info[16]);
/* tests only (host, no GPU): the cover of a window's station pairs by "quads" -- two template stations x two signal
 * stations whose two packed transforms per segment serve up to four pairs in the segment form.
 * pairs[2 i], pairs[2 i + 1] = template, signal station of pair i; quads_out gets 8 ints per quad: stations a, b, c, d
 * (-1 = empty slot) and the pair index of (a,c), (a,d), (b,c), (b,d) (-1 = not wanted).  Returns the number of quads
 * (at most n_pairs), or a negative TDOA_ERR_* value (more than 32 stations: the library then runs the segment form one
 * pair-window at a time and builds no quads). */
int tdoa_debug_segment_quads(int n_stations, const int32_t *pairs, int n_pairs, int32_t *quads_out, int max_quads);

/* tests only (host, no GPU): how the LDS-staged column walk of the decimated pair step (csrc/dec_staged.hpp) deals the
 * n_stations (n_stations - 1) / 2 pairs of a window -- numbered (0,1), (0,2), ..., as tdoa_process lays them out -- to
 * workgroups of at most max_pairs walks (1..15 next to a loader wave; 16: the form without one, full workgroups first): group g
 * takes counts_out[g] pairs, pairs_out[16 g ..] their numbers, and stages the stations of masks_out[g] (bit s = station s).
 * More than eight stations: every group stays within eight.  Returns the number of groups, or a negative TDOA_ERR_* value
 * (stations outside 2..16, max_pairs outside 1..16, more than max_groups). */
int tdoa_debug_staged_groups(int n_stations, int max_pairs, uint32_t *masks_out, int32_t *counts_out, uint8_t *pairs_out, int max_groups);

/* tests only (host, no GPU): where the paired block layout of the staged column walk (csrc/dec_staged.hpp, stg_paired_at) puts
 * element (row, col) of a 4096-column x n2-row spectrum: the element index in [0, 4096 n2), = (cb n2 + k2) 128 + e for line
 * [cb][k2], element e.  n2 = 256 or 512, row in [0, n2), col in [0, 4096); anything else returns -1. */
int64_t tdoa_debug_stg_paired_index(int n2, int row, int col);

/* tests only (host, no GPU): the split half-plane angle table of the fused column kernels as the library builds it --
 * for index i = b_I | (b_Q & 0x7f) << 8 of a sample with b_Q >= 128 and angle code a in (0, 2^23): hi[i] = a >> 8,
 * lo[i] = a & 0xff; 32768 entries each.  Returns TDOA_OK, or TDOA_ERR_INVALID for a NULL pointer. */
int tdoa_debug_k1_split_table(uint16_t *hi, uint8_t *lo);

/* tests only (host, no GPU): what tdoa_process(rank, world) runs for n_stations captures cut into n_windows windows, with
 * launch groups of at most max_per_batch windows before the grid limit.  pw_out gets 6 ints per owned pair-window, in launch
 * order: unit wid * n_pairs + pair, launch group, the template's and the signal's station-window slot (relative to the
 * group) and the stations of those two slots.  quads_out (room for max_pw) gets 9 ints per segment-form quad: launch group,
 * slots a, b, c, d (-1 = empty) and the group-relative pair-window of (a,c), (a,d), (b,c), (b,d) (-1 = not wanted);
 * *n_quads their number.  Returns the number of pair-windows, or a negative TDOA_ERR_* value. */
int tdoa_debug_step_layout(int n_stations, int n_windows, int rank, int world, int max_per_batch, int32_t *pw_out, int max_pw,
                           int32_t *quads_out, int32_t *n_quads);

/* ---- multi-device group ----------------------------------------------------
 * One call that shards tdoa_process over several GPUs (processor.go:816-850 over a node's devices).  A group holds one
 * tdoa_ctx per member; member k is rank k of n_members in the sense of tdoa_process(ctx, rank, world, ...), so the
 * (window, pair) units are dealt exactly as there.  Devices may repeat: several members on one GPU share it.
 *
 * Ownership: the group owns its member contexts; tdoa_group_destroy destroys them.  The library copies what it needs
 * during a call and keeps no host pointer afterwards.
 * Threading: a group is single-caller, like a context.  Inside tdoa_group_capture_upload_files and tdoa_group_process
 * member 0 runs on the caller's thread and every other member on a host thread of its own, started for the call and
 * joined before it returns; each thread calls into its own member only.  No collective library is used: the peak records
 * come back to the host and are merged there. */
typedef struct tdoa_group tdoa_group;

/* one tdoa_ctx per member, member k = rank k of n_members; devices may repeat (several members on one GPU).  p may be NULL
 * (tdoa_default_params); p->device is ignored.  TDOA_ERR_INVALID for n_members < 1, NULL devices / out or a negative
 * ordinal, TDOA_ERR_NO_DEVICE for an ordinal >= tdoa_device_count(), both before any member is created; if a member's
 * tdoa_create fails, the members already made are destroyed and its status returned.  *out is NULL on every failure, and
 * tdoa_group_last_error(NULL) then names the member (the calling thread's last failed tdoa_group_create). */
int         tdoa_group_create(const tdoa_params *p, const int32_t *devices, int n_members, tdoa_group **out);
void        tdoa_group_destroy(tdoa_group *g);   /* NULL: no-op */
const char *tdoa_group_last_error(const tdoa_group *g);  /* "member k (device d): <that ctx's tdoa_last_error>" */
tdoa_ctx   *tdoa_group_member(tdoa_group *g, int k);     /* borrowed; for synth/download/debug calls on one member;
                                                            NULL for k outside 0 .. n_members - 1 */

/* .dat files (raw u8 I,Q, any size): each member preads and uploads only the sample runs its windows need
 * (tdoa_debug_owned_runs; the window grid comes from the shortest file), after dropping its previous captures.  Station s
 * is paths[s]; *n_samples (may be NULL) receives size/2 per file, like tdoa_capture_upload_file. */
int tdoa_group_capture_upload_files(tdoa_group *g, int n_stations, const char *const *paths, size_t *n_samples);

/* every pair on every window, sharded over the members; out_host = [n_windows_total][n_pairs], byte-identical to
 * tdoa_process(single ctx, 0, 1, out_host, NULL) on the same captures.  TDOA_ERR_STATE if the members do not hold the same
 * station count and capture lengths (captures made on single members through tdoa_group_member must agree).  out_host is
 * written only if every member succeeded; otherwise the first failing member's status is returned and
 * tdoa_group_last_error names it.  With one member, its tdoa_process writes out_host directly. */
int tdoa_group_process(tdoa_group *g, tdoa_peak *out_host);

/* tdoa_process_stacked over the members (layouts as there; any output may be NULL, not all): every member sums the windows
 * of its rank, the host adds the members' int64 partial sums, and member 0 finishes the sum with the kernels a single
 * context's call ends with -- the outputs are byte-identical to tdoa_process_stacked(single ctx, 0, 1, ...).  Errors as
 * tdoa_group_process.  With one member, its call writes the outputs directly. */
int tdoa_group_process_stacked(tdoa_group *g, int windows_per_stack, int k, int min_separation, double gate_samples,
                               tdoa_peak *peaks_host, int32_t *count_host, tdoa_fine_peak *fine_host, float *surface_host);

/* tdoa_process_closure over the members: they sum their windows as in tdoa_group_process_stacked, the host adds the
 * partials, and member 0 runs the search on the merged Q -- the records are byte-identical to
 * tdoa_process_closure(single ctx, ...).  Errors as there and as tdoa_group_process.  With one member, its call writes the
 * records directly. */
int tdoa_group_process_closure(tdoa_group *g, int windows_per_stack, int gate, int min_separation,
                               const int32_t *centre, tdoa_closure *closure_host);

/* tdoa_locate_set_table on every member, and tdoa_process_locate over them: they sum their windows as in
 * tdoa_group_process_stacked, the host adds the partials, and member 0 runs the search on the merged Q with its table -- the
 * outputs are byte-identical to tdoa_process_locate(single ctx, ...).  Errors as there and as tdoa_group_process. */
int tdoa_group_locate_set_table(tdoa_group *g, const int32_t *delay, int n_cells, int n_cols, int n_stations);
int tdoa_group_process_locate(tdoa_group *g, int windows_per_stack, int min_separation, tdoa_location *loc_host,
                              int32_t *lags_host, double *corr_host, int64_t *map_host);

/* tdoa_locate_set_clock on every member (tdoa_group_process_locate then searches with member 0's clocks), and
 * tdoa_process_sync over the members: they sum their windows as in tdoa_group_process_stacked, the host adds the partials,
 * and member 0 runs the search on the merged Q -- the outputs are byte-identical to tdoa_process_sync(single ctx, ...).
 * Errors as there and as tdoa_group_process.  With one member, its call writes the outputs directly. */
int tdoa_group_locate_set_clock(tdoa_group *g, const int32_t *clock, int n_stacks, int n_stations);
int tdoa_group_process_sync(tdoa_group *g, int windows_per_stack, int gate, int rounds, const int32_t *ref_delay,
                            const int32_t *centre, tdoa_sync *sync_host, int32_t *clock_host, int32_t *lags_host,
                            double *corr_host);

/* tdoa_process_sync_fine over the members: the merged sum is searched on member 0, coarse stage and refinement, and the group
 * returns a single context's bytes.  Errors as there and as tdoa_group_process_sync. */
int tdoa_group_process_sync_fine(tdoa_group *g, int windows_per_stack, int gate, int rounds, int U, int fine_rounds,
                                 const int32_t *ref_delay, const int32_t *centre, tdoa_sync *sync_host, int32_t *clock_host,
                                 int32_t *lags_host, double *corr_host, tdoa_sync *fine_host, int32_t *clock16_host,
                                 int32_t *fine_lags_host, double *fine_corr_host);

/* tdoa_process_sync_drift over the members: they sum their windows as in tdoa_group_process_stacked, the host adds the
 * partials, and member 0 runs the search on the merged Q.  F is a function of the complete stacked Q only, so the members'
 * partial sums merge as they do for tdoa_group_process_sync.  The group returns a single context's bytes.  Errors as there and
 * as tdoa_group_process.  With one member, its call writes the outputs directly. */
int tdoa_group_process_sync_drift(tdoa_group *g, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds,
                                  const int32_t *ref_delay, const int32_t *centre, tdoa_sync_line *line_host,
                                  int32_t *clock_host, int32_t *rate_host, int32_t *rows_host, int32_t *lags_host,
                                  double *corr_host);

/* tdoa_process_sync_drift_fine over the members: the merged sum is searched on member 0, coarse stage and refinement, and the
 * group returns a single context's bytes.  Errors as there and as tdoa_group_process_sync_drift. */
int tdoa_group_process_sync_drift_fine(tdoa_group *g, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds, int U,
                                       int fine_rounds, const int32_t *ref_delay, const int32_t *centre, tdoa_sync_line *line_host,
                                       int32_t *clock_host, int32_t *rate_host, int32_t *rows_host, int32_t *lags_host,
                                       double *corr_host, tdoa_sync_line *fine_host, int32_t *clock16_host, int32_t *fine_rate_host,
                                       int32_t *fine_rows_host, int32_t *fine_lags_host, double *fine_corr_host);

/* tdoa_process_locate_track over the members (the table and the clocks as set by tdoa_group_locate_set_table and
 * tdoa_group_locate_set_clock): they sum their windows as in tdoa_group_process_stacked, the host adds the partials, and
 * member 0 runs the search and the recurrence on the merged Q -- the outputs are byte-identical to
 * tdoa_process_locate_track(single ctx, ...).  Errors as there and as tdoa_group_process.  With one member, its call writes
 * the outputs directly. */
int tdoa_group_process_locate_track(tdoa_group *g, int windows_per_stack, int max_step, int min_separation,
                                    tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host, int32_t *lags_host,
                                    double *corr_host, int64_t *total_host);

/* tdoa_process_locate_multi over the members (the table and the clocks as set by tdoa_group_locate_set_table and
 * tdoa_group_locate_set_clock): they sum their windows as in tdoa_group_process_stacked, the host adds the partials, and
 * member 0 runs the rounds on the merged Q -- the outputs are byte-identical to tdoa_process_locate_multi(single ctx, ...).
 * Errors as there and as tdoa_group_process.  With one member, its call writes the outputs directly. */
int tdoa_group_process_locate_multi(tdoa_group *g, int windows_per_stack, int n_emitters, int guard, int min_separation,
                                    tdoa_location *loc_host, int32_t *lags_host, double *corr_host, int64_t *map_host);

/* tdoa_process_locate_track_multi over the members (the table and the clocks as set by tdoa_group_locate_set_table and
 * tdoa_group_locate_set_clock): they sum their windows as in tdoa_group_process_stacked, the host adds the partials, and
 * member 0 runs the rounds on the merged Q -- the outputs are byte-identical to tdoa_process_locate_track_multi(single ctx,
 * ...).  Errors as there and as tdoa_group_process.  With one member, its call writes the outputs directly. */
int tdoa_group_process_locate_track_multi(tdoa_group *g, int windows_per_stack, int max_step, int n_emitters, int guard,
                                          int min_separation, tdoa_cell_track *track_host, int32_t *cells_host,
                                          int64_t *own_host, int32_t *pairs_host, int32_t *lags_host, double *corr_host,
                                          int64_t *total_host);

/* tdoa_locate_set_stats on every member (member 0 judges the merged sum), and the last group call's statistics: the bytes a
 * single context returns.  Errors as there. */
int tdoa_group_locate_set_stats(tdoa_group *g, const uint16_t *ranks, int n_ranks, int foot);
int tdoa_group_locate_last_stats(tdoa_group *g, tdoa_map_stats *out, int max_planes, int *n_planes);

/* tdoa_locate_set_upsample on every member.  A group of several upsamples the merged sum on member 0; the outputs are the
 * bytes a single context returns.  Errors as there. */
int tdoa_group_locate_set_upsample(tdoa_group *g, int U);

/* tdoa_locate_set_fine_table on every member, and tdoa_process_locate_zoom over them: the merged sum is searched on member 0,
 * coarse stage and window, and the same bytes go through the merged sum as a single context returns.  Errors as there. */
int tdoa_group_locate_set_fine_table(tdoa_group *g, const int32_t *delay, int n_cells, int n_cols, int n_stations);
int tdoa_group_process_locate_zoom(tdoa_group *g, int windows_per_stack, int min_separation, int Z, int H, int fine_separation,
                                   tdoa_location *loc_host, int32_t *lags_host, double *corr_host, int64_t *map_host, tdoa_zoom *zoom_host,
                                   int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host);

/* tdoa_process_locate_multi_zoom over the members: the merged sum is searched on member 0, rounds and windows, and the same
 * bytes go through the merged sum as a single context returns.  Errors as there. */
int tdoa_group_process_locate_multi_zoom(tdoa_group *g, int windows_per_stack, int n_emitters, int guard, int min_separation, int Z, int H,
                                         int fine_separation, tdoa_location *loc_host, int32_t *lags_host, double *corr_host,
                                         int64_t *map_host, tdoa_zoom *zoom_host, int32_t *zpairs_host, int32_t *zlags_host,
                                         double *zcorr_host, int64_t *zmap_host);

/* tdoa_process_locate_track_zoom over the members: the merged sum is searched on member 0, coarse tracks and windows, and the
 * same bytes go through the merged sum as a single context returns.  Errors as there. */
int tdoa_group_process_locate_track_zoom(tdoa_group *g, int windows_per_stack, int max_step, int min_separation, int Z, int H, int fine_step,
                                         int fine_separation, tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host,
                                         int32_t *lags_host, double *corr_host, int64_t *total_host, tdoa_cell_track *ztrack_host,
                                         int32_t *zcells_host, int64_t *zown_host, int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host,
                                         int64_t *ztotal_host);

/* tdoa_process_sync_locate over the members: the merged sum is searched on member 0 -- its table, fine table and settings,
 * as for the zoom -- and the same bytes go through the merged sum as a single context returns.  Errors as there. */
int tdoa_group_process_sync_locate(tdoa_group *g, int windows_per_stack, int gate, int rounds, int U, int fine_rounds,
                                   const int32_t *ref_delay, const int32_t *centre, const tdoa_clock_mix *mix, int min_separation, int Z, int H,
                                   int fine_separation, tdoa_sync *sync_host, int32_t *clock_host, int32_t *lags_host, double *corr_host,
                                   tdoa_sync *fine_host, int32_t *clock16_host, int32_t *fine_lags_host, double *fine_corr_host,
                                   int32_t *rows_host, tdoa_location *loc_host, int32_t *loc_lags_host, double *loc_corr_host,
                                   int64_t *map_host, tdoa_zoom *zoom_host, int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host);

/* tdoa_process_sync_drift_locate over the members: the merged sum is searched on member 0 -- its table, fine table and
 * settings, as for the zoomed tracks -- and the same bytes go through the merged sum as a single context returns.  Errors as
 * there. */
int tdoa_group_process_sync_drift_locate(tdoa_group *g, int windows_per_stack, int gate, int max_drift, int drift_den, int rounds, int U,
                                         int fine_rounds, const int32_t *ref_delay, const int32_t *centre, const tdoa_line_mix *mix,
                                         int max_step, int min_separation, int Z, int H, int fine_step, int fine_separation,
                                         tdoa_sync_line *line_host, int32_t *clock_host, int32_t *rate_host, int32_t *rows_host,
                                         int32_t *lags_host, double *corr_host, tdoa_sync_line *fine_host, int32_t *clock16_host,
                                         int32_t *fine_rate_host, int32_t *fine_rows_host, int32_t *fine_lags_host, double *fine_corr_host,
                                         int32_t *mix_rows_host, tdoa_cell_track *track_host, int32_t *cells_host, int64_t *own_host,
                                         int32_t *loc_lags_host, double *loc_corr_host, int64_t *total_host, tdoa_cell_track *ztrack_host,
                                         int32_t *zcells_host, int64_t *zown_host, int32_t *zlags_host, double *zcorr_host, int64_t *zmap_host,
                                         int64_t *ztotal_host);

/* the sample runs member `rank` of `world` uploads for a capture of total_samples (window grid from n_min, the shortest
 * capture of the job; block offsets from the capture's own thirds): adjacent owned windows form one run, and with fewer
 * windows than members (the pair-major fallback) the whole capture is one run.  *n_runs receives the number of runs; at
 * most max_runs of them are written to first[] / count[] (max_runs = 0 with NULL arrays asks for the count).
 * host-only, no device needed */
int tdoa_debug_owned_runs(size_t total_samples, size_t n_min, int64_t window_len, int rank, int world,
                          size_t *first, size_t *count, int max_runs, int *n_runs);

/* ---- downstream (processor.go:125-163, 932-1045), host side ---------------- */
void tdoa_latlon_to_ecef(double lat, double lon, double elev, double xyz[3]);
void tdoa_ecef_to_latlon(double x, double y, double z, double lle[3]);
/* reference 3-station solver, bit-compatible call: range_diff[0]=(0,1), [1]=(0,2) */
int  tdoa_solve_3station(const double stations_lle[9], const double *range_diff,
                         double out_lle[3], int *iterations);
/* N-station generalisation: all n(n-1)/2 range differences (pairs i<j), optional weights,
 * X,Y (Z frozen, like the reference) or X,Y,Z unknowns; centroid start, 0.5 damping,
 * 10 iterations, 1 m stop rule as processor.go:950-1010. */
int  tdoa_solve_nstation(const double *stations_lle, int n_stations, const double *range_diff,
                         const double *weights, int solve_z, double out_lle[3], int *iterations);
/* Ground transmitter: the same residuals and weights with the position held on the ellipsoid at height_m (unknowns
 * latitude, longitude; undamped Gauss-Newton from the stations' centroid, at most 20 iterations, 1 m stop rule).  The
 * reference's frozen ECEF Z (processor.go:1004) is a plane that misses a transmitter north or south of the centroid by
 * hundreds of metres to kilometres; this form is what bench.py checks its multi-GPU fix with. */
int  tdoa_solve_surface(const double *stations_lle, int n_stations, const double *range_diff, const double *weights,
                        double height_m, double out_lle[3], int *iterations);

/* ---- measurement ----------------------------------------------------------- */
enum {
    TDOA_K_STATS = 0, TDOA_K_FWD_COL, TDOA_K_FWD_ROW, TDOA_K_INV_ROW, TDOA_K_INV_COL,
    TDOA_K_PEAK,
    TDOA_K_TRACK_STEP, TDOA_K_TRACK_FINISH,      /* tdoa_process_track's two kernels (appended: the scopes above keep their numbers) */
    TDOA_K_COUNT
};
/* on = 1: tdoa_process launches its kernels one by one with HIP events at the boundaries of the selected scopes.
 * on = 2: tdoa_process keeps replaying the whole step as one hipGraph (the default path); the selected scopes are timed by
 *         event-record nodes spliced into the captured graph.  on = 0: off. */
int         tdoa_profile_enable(tdoa_ctx *ctx, int on);
/* which scopes of the profiling path record events: bit k = TDOA_K_* scope k (default: all).  A measurement that needs
 * one kernel's launch durations (bench.py: the dominant kernel's, for the roofline) selects that scope alone, so that the
 * timed steps carry two event records instead of one per kernel boundary. */
int         tdoa_profile_select(tdoa_ctx *ctx, unsigned int scope_mask);
int         tdoa_profile_reset(tdoa_ctx *ctx);
int         tdoa_profile_get(tdoa_ctx *ctx, int kernel, double *total_ms, int64_t *launches,
                             double *algorithmic_bytes);
const char *tdoa_kernel_name(int kernel);
/* plan facts: FFT length N (real), factors N1 x N2 of N/2, passes */
int         tdoa_plan_info(const tdoa_ctx *ctx, int64_t *fft_n, int32_t *n1, int32_t *n2);

#ifdef __cplusplus
}
#endif
#endif
