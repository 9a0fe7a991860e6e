// tdoa_mi355x.hip -- C-ABI implementation (include/tdoa_mi355x.h) for gfx950.
//
// Host side: context, FFT plans, (station, window) x (pair, window) batching,
// HIP stream + event plumbing.  Device side: the kernels in the headers below.
// One translation unit: the .inc files included further down hold one subject each (README.md lists them).
// There is no CPU fallback: without a HIP device every compute entry point
// fails with TDOA_ERR_NO_DEVICE.
#include "../../include/tdoa_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <climits>
#include <cstring>
#include <functional>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "k1_discriminator.hpp"
#include "k1_single_look.hpp"
#include "fft_stockham.hpp"
#include "fft_radix16.hpp"
#include "fft_radix8.hpp"
#include "dec_stream.hpp"
#include "dec_staged.hpp"
#include "exact_reference.hpp"
#include "synth_capture.hpp"
#include "window_quality.hpp"
#include "host_geodesy.hpp"
#include "host_upload.hpp"
#include "segment_quads.hpp"
#include "peak_select.hpp"
#include "stack_surfaces.hpp"
#include "stack_drift.hpp"
#include "stack_track.hpp"
#include "stack_closure.hpp"
#include "stack_locate.hpp"
#include "stack_locate_multi.hpp"
#include "stack_sync.hpp"
#include "stack_sync_drift.hpp"
#include "stack_cell_track.hpp"
#include "stack_locate_track_multi.hpp"
#include "stack_map_stats.hpp"
#include "stack_upsample.hpp"
#include "stack_sync_fine.hpp"
#include "stack_sync_drift_fine.hpp"
#include "stack_locate_zoom.hpp"
#include "stack_locate_track_zoom.hpp"
#include "stack_locate_multi_zoom.hpp"
#include "stack_line_mix.hpp"

using namespace tdoa;

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    template <class T> T *as() const { return static_cast<T *>(p); }
};

struct ProfRec {
    int kernel;
    int e0, e1;          // indices into the context's event pool
    double bytes;
};

}  // namespace

#include "knobs.hpp"

namespace {

// The staged walk's share-out of a window's pairs for every station count 2 .. 16: the groups of all of them back to back
// (what ensure_stg_groups uploads) and, per station count, where its groups start, how many there are, the most stations
// (slots) and the most pairs (max_n) of one group -- tab: next to n_lw loader waves; tab16: the folded form's, up to
// sixteen walks per workgroup
struct StgTable { int off = 0, count = 0, slots = 0, max_n = 0; };
struct StgTables {
    StgTable tab[kStgMaxStations + 1], tab16[kStgMaxStations + 1];
    std::vector<StgGroup> groups;
};

using QuadCache = std::map<std::vector<int>, std::vector<StationQuad>>;    // owned pair ids of a window -> its quad cover

}  // namespace

struct tdoa_ctx {
    tdoa_params prm;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string last_error;

    struct Capture {
        const uint8_t *dev = nullptr;
        size_t n = 0;
        bool owned = false;
        size_t cap_bytes = 0;               // size of an owned allocation (reused by the next upload if it fits)
    };
    std::vector<Capture> caps;

    DevBuf k1_direct;                       // kK1DirectEntries half-plane angle codes of the streaming K1 kernel
    DevBuf k1_quad;                         // kK1QuadrantEntries first-quadrant angle codes (k_fwd_col256_k1)
    DevBuf k1_split;                        // kK1SplitBytes: the half-plane angles as lo | hi, the fused column kernels' default table
    DevBuf sw_desc, pw_desc, partials, stats, codes, codes_lp, k1_power, tz, v, keys, scales, peaks, scratch_a, scratch_b, lagdump;
    DevBuf ex_a, ex_b, ex_c, ex_d, ex_part;

    bool profiling = false;
    unsigned int prof_mask = ~0u;           // scopes that record events (tdoa_profile_select)
    // profiling INSIDE the replayed step graph (tdoa_profile_enable(ctx, 2)): while the step is captured the selected scopes
    // note the capture's last node before their first and after their last kernel; after the capture an event-record NODE
    // goes in at either place (events recorded on a capturing stream are dropped by this ROCm; explicit nodes are timed
    // correctly: scripts/microbench/graph_event_nodes.hip)
    bool graph_prof = false;
    bool capturing = false;
    struct GraphMark { int kernel; double bytes; hipGraphNode_t before, last; hipEvent_t e0, e1; };
    std::vector<GraphMark> graph_marks;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> prof_pool;      // events of the profiling path, reused from call to call
    size_t prof_used = 0;                   // handed out since the last prof_collect
    int prof_last = -1;                     // stop event of the previous scope: the next scope starts there (one event
                                            // between two kernels instead of two)
    double prof_ms[TDOA_K_COUNT] = {0};
    int64_t prof_launches[TDOA_K_COUNT] = {0};
    double prof_bytes[TDOA_K_COUNT] = {0};

    FftPlan plan{};
    int64_t plan_n = 0;

    // whole-step hipGraph of tdoa_process (launch-bound when windows are processed in many groups)
    int n_cu = 256;                         // multiprocessors of this device
    double workspace_limit = 24.0 * 1073741824.0;      // bytes of FFT workspace one launch group may take: a third of the device's memory
    Knobs knobs;
    StgTables stg;                          // the staged walk's share-out of a window's pairs (stg_tables)
    DevBuf stg_groups;                      // ... its groups, uploaded once
    bool stg_ready = false;
    bool k1_split_lds = false;              // the split-table column kernels may ask for kK1SplitLds of dynamic LDS (allow_big_lds)
    int graph_nodes = 0, graph_edges = 0, graph_roots = 0, graph_memsets = 0;      // structure of the captured step (tdoa_debug_graph_info)
    bool once_active = false;               // the last step (run_fm_batch, or the replayed graph) took the single-look path: decode multiplies by slot_gain
    bool graph_once = false;                // ... of the step the cached graph holds (a pair call on another path in between must not change what a replay reports)
    int32_t route[16] = {0};                // the last batch's FmRoute as tdoa_debug_last_route reports it (route_info)
    int32_t graph_route[16] = {0};          // ... of the batch the cached graph captured last
    bool route_set = false;
    DevBuf once_edges, once_tiles, once_fin, slot_gain;
    // decimated inverse (k_pair_decimate16): FIR taps and window correction for (Nc, reach); small plan of the R-point inverse
    DevBuf dec_taps, dec_gain;
    long long dec_nc = 0;
    int dec_reach = -1, dec_T = 0;
    uint64_t alloc_gen = 0;                 // bumped whenever a workspace buffer moves
    std::vector<uint64_t> graph_key;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    DevBuf g_sw_desc, g_pw_desc, g_quad_desc, g_scales, g_keys;
    QuadCache quad_cache;                   // segment-form quad covers (build_step_layout)
    DevBuf qual;                            // QualAcc per (window, station)
    StagedUploader uploader;                // pinned staging buffers + copy streams, created on first use
    DevBuf fine_raw, fine;                  // (f)-4 refinement: 3 raw neighbours and tdoa_fine_peak per slot
    // tdoa_process_lags / _peaks: the K5 kernels' lag arrays [owned pair-window][2 max_lag - 1], the surfaces in the caller's
    // layout [slot][2 max_lag - 1], the selected peaks [slot][k] and their counts [slot]
    DevBuf surf, surf_out, sel_peaks, sel_count;
    // tdoa_process_stacked: the fixed-point sums Q [stack][pair][2 max_lag - 1], the float stack surfaces of the same shape,
    // the stack-pairs' keys, their refined peak 1, and the descriptors (sqrt(n_w) per stack, unit scales, runs, list)
    DevBuf stack_q, stack_surf, stack_keys, stack_fine, stack_desc;
    // tdoa_process_stacked_drift: the shift table [2H+1][stack length], the keys [stack][pair][2H+1] of the slopes' maxima,
    // h* [stack][pair] and the decoded profile [stack][pair][2H+1]
    DevBuf drift_tab, drift_keys, drift_h, drift_prof;
    // tdoa_process_track: where the stack-pairs' windows are (pos [stack][pair][stack length], n_w [stack][pair]), the two
    // halves of T [stack][pair][2 max_lag - 1][2 polarities], the steps D [stack][pair][stack length][2 max_lag - 1][2], and
    // the score, lags and values of every stack-pair's track
    DevBuf track_tab, track_t, track_d, track_score, track_lags, track_values;
    // the closure search: the stations' centres, the tiles' candidates [stack][triple][tile], (u*, v*) and the records
    // [stack][triple]
    DevBuf closure_centre, closure_part, closure_best, closure_out;
    // the delay-table search: the table [station][cell] (state: tdoa_locate_set_table; 0 cells: none), the map [stack][cell],
    // the tiles' candidates [stack][tile], the locations' cells and records [stack], the best cells' lags and correlations
    // [stack][pair]
    DevBuf locate_table, locate_map, locate_part, locate_best, locate_out, locate_lags, locate_corr;
    // ... and the stacks' station clocks as the kernels take them, clock[j] - clock[i] per [stack][pair] (state:
    // tdoa_locate_set_clock; 0 stacks: none)
    DevBuf locate_clock;
    // several emitters per stack (tdoa_process_locate_multi): the buffers above hold one plane per round, and the excluded
    // intervals' centres [stack][pair][round]
    DevBuf locate_centres;
    // cell tracks (tdoa_process_locate_track): the steps D [stack][cell][2], the two halves of T [track][cell], sqrt(N_w) per
    // track, the records [track], the tracks' cells and own scores [stack]
    DevBuf ctrack_d, ctrack_t, ctrack_roots, ctrack_out, ctrack_cells, ctrack_own;
    // several emitters per block (tdoa_process_locate_track_multi): the tracks' buffers above hold one plane per round (T as
    // locate_run.inc lays it out), and pairs_in and reserved [round][stack][2]
    DevBuf ctrack_pairs;
    // map statistics (state: tdoa_locate_set_stats; 0 ranks: off): the ranks (eight words), the bins [plane][rank][2048] and
    // the selection's state [plane] of one group of planes, the statistics [plane], and the last call's on the host
    DevBuf mstat_ranks, mstat_hist, mstat_state, mstat_out;
    int mstat_n_ranks = 0, mstat_foot = 0;
    std::vector<MapStatsOut> mstat_host;
    // the clock search: ref_delay and centre (kSyncMaxStations words each), the start's tiles' candidates [stack][tile], the
    // records [stack], the clocks [stack][station], the lags and correlations [stack][pair]
    DevBuf sync_in, sync_part, sync_out, sync_clock, sync_lags, sync_corr;
    // the fine clock search, behind the clock search's: the fine records [stack], the clocks in 1/16 sample [stack][station],
    // the lags in 1/U sample and the correlations [stack][pair]
    DevBuf sfine_out, sfine_clock, sfine_lags, sfine_corr;
    // the clock-line search: ref_delay and centre, the shift table [rank(h)][position], sqrt(N_w) [line], the stations' clocks
    // [line][station][position], their k and h [line][station], the tiles' candidates [line][tile], `moved` and F after placing
    // [line], the records [line], the clocks and rates [line][station], the rows [stack][station], the lags and correlations
    // [stack][pair]
    DevBuf sline_in, sline_tab, sline_roots, sline_cur, sline_k, sline_h, sline_part, sline_moved, sline_start, sline_out, sline_clock,
        sline_rate, sline_rows, sline_lags, sline_corr;
    // the fine clock lines, behind the clock-line search's: the fine clocks [line][station][position], kappa and eta
    // [line][station], the tiles' candidates [line][tile], `moved` and F_U at the start [line], the fine records [line], the
    // clocks in 1/16 sample and the fine rates [line][station], the rows [stack][station], the lags in 1/U sample and the
    // correlations [stack][pair]
    DevBuf slfine_cur, slfine_kappa, slfine_eta, slfine_part, slfine_moved, slfine_start, slfine_out, slfine_clock, slfine_rate,
        slfine_rows, slfine_lags, slfine_corr;
    // the tdoa_debug_*_from_q entries (debug_search_from_q): the caller's words and sqrt(n_w) per set
    DevBuf debug_q, debug_roots;
    int locate_cells = 0, locate_cols = 0, locate_stations = 0;
    int clock_stacks = 0, clock_stations = 0;
    // sub-sample locate (state: tdoa_locate_set_upsample; 1: off): the factor U, the largest magnitudes of the table's and the
    // clocks' entries (U times either must fit 32 bits), and a run's buffers: the upsampled surfaces [stack][pair][(n - 1) U + 1],
    // U x the table and U x the clock differences.  Also the output of tdoa_debug_upsample_q.
    int locate_up = 1;
    long long locate_table_max = 0, locate_clock_max = 0;
    DevBuf locate_qu, locate_table_up, locate_clock_up;
    // the zoom locate (tdoa_process_locate_zoom), behind the delay-table search: the fine table [station][fine cell] (state:
    // tdoa_locate_set_fine_table; 0 cells: none), U x it, and a run's window maps [stack][(2H+1)^2], tiles' candidates
    // [stack][tile], records [stack], lags and correlations [stack][pair]
    int fine_cells = 0, fine_cols = 0, fine_stations = 0;
    long long locate_fine_max = 0;
    DevBuf locate_fine, locate_fine_up, zoom_map, zoom_part, zoom_out, zoom_lags, zoom_corr;
    // the zoomed cell tracks (tdoa_process_locate_track_zoom), behind the cell tracks: the windows' centres [stack], the steps E
    // [stack][(2H+1)^2][2], the sums F_0 [track][(2H+1)^2], the records [track], the fine cells and own scores [stack]; the
    // window maps, their tiles' candidates and the fine lags and correlations lie in the zoom locate's buffers
    DevBuf tzoom_centre, tzoom_e, tzoom_total, tzoom_out, tzoom_cells, tzoom_own;
    // the zoomed rounds (tdoa_process_locate_multi_zoom), behind the rounds: the counts [round][stack][2]; the K planes of the
    // window maps, their tiles' candidates, the records, the fine lags and correlations lie in the zoom locate's buffers
    DevBuf mzoom_pairs;
    // from reference blocks to fix in one call (tdoa_process_sync_locate, tdoa_process_sync_drift_locate), between the fine clock
    // stage and the locate stage: the mix [stack] as line-mix entries, the stacks' clock rows [stack][station] and their pairs'
    // differences and U x them [stack][pair], which the locate stage of those calls takes where the others take locate_clock and
    // locate_clock_up; tdoa_debug_clock_mix's clocks [stack][station] or tdoa_debug_line_mix's clocks and rates [2][line][station]
    DevBuf mix_in, mix_rows, mix_cdiff, mix_cdiff_up, mix_debug;
    size_t total_mem = 0;                  // of the device, 0: unknown
};

namespace {

static_assert(sizeof(PeakOut) == sizeof(tdoa_peak), "tdoa_peak layout");
static_assert(sizeof(FmStats) == sizeof(tdoa_fm_stats), "tdoa_fm_stats layout");
static_assert(sizeof(ClosureOut) == sizeof(tdoa_closure) && sizeof(tdoa_closure) == 80, "tdoa_closure layout");
static_assert(sizeof(LocateOut) == sizeof(tdoa_location) && sizeof(tdoa_location) == 48, "tdoa_location layout");
static_assert(kLocateDelayUnit == TDOA_DELAY_UNIT, "the table's unit");
static_assert(sizeof(LocateZoomOut) == sizeof(tdoa_zoom) && sizeof(tdoa_zoom) == 64, "tdoa_zoom layout");
static_assert(kLocateMaxEmitters == TDOA_LOCATE_MAX_EMITTERS, "the rounds of tdoa_process_locate_multi");
static_assert(sizeof(SyncOut) == sizeof(tdoa_sync) && sizeof(tdoa_sync) == 32, "tdoa_sync layout");
static_assert(sizeof(CellTrackOut) == sizeof(tdoa_cell_track) && sizeof(tdoa_cell_track) == 48, "tdoa_cell_track layout");
static_assert(offsetof(CellTrackOut, cell) == offsetof(LocateOut, cell) && offsetof(CellTrackOut, score_q) == offsetof(LocateOut, score_q),
              "the statistics' kernels read a track's record as a location's");
static_assert(sizeof(MapStatsOut) == sizeof(tdoa_map_stats) && sizeof(tdoa_map_stats) == 168, "tdoa_map_stats layout");
static_assert(kMapStatsMaxRanks == TDOA_MAP_STATS_MAX_RANKS, "the ranks of tdoa_locate_set_stats");

int fail(tdoa_ctx *ctx, int status, const char *what, hipError_t e = hipSuccess)
{
    if (ctx) {
        char buf[512];
        if (e != hipSuccess)
            snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
        else
            snprintf(buf, sizeof(buf), "%s", what);
        ctx->last_error = buf;
    }
    return status;
}

#define HIPCHK(ctx, call)                                              \
    do {                                                               \
        hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) return fail(ctx, TDOA_ERR_HIP, #call, e_); \
    } while (0)

int ensure(tdoa_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return TDOA_OK;
    if (b.p) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, TDOA_ERR_NOMEM, "hipMalloc", e);
    }
    b.cap = want;
    ctx->alloc_gen++;
    return TDOA_OK;
}

void release(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

int ilog2(long long v)
{
    int l = 0;
    while ((1ll << l) < v) l++;
    return l;
}

long long next_pow2(long long n)   // processor.go:502-512
{
    long long p = 1;
    while (p < n) p <<= 1;
    return p;
}

constexpr size_t kLdsCap = 128 * 1024;

// factor Nc = N1 * N2 for the four-step FFT; rows (N1) live whole in LDS
// zpad: elements of padding after every 256 rows of a two-sweep plan's TZ (tdoa_ctx::zpad; 0 for the small plans)
int make_plan(long long n_real, bool packed, FftPlan *pl, int zpad = 0)
{
    long long nc = packed ? n_real / 2 : n_real;
    // 5 x 2^k (round 5): only the two shapes that have kernels -- 4096 x 2560 (N = 5 x 2^22, the column pass as ten 256-point
    // sub-transforms + k_fwd_col_finish<10>, the pair step as a column walk) and the small plan of its decimated inverse,
    // 4096 x 160
    // 3 x 2^k likewise: 4096 x 3072 (N = 3 x 2^23: twelve sub-transforms + k_fwd_col_finish<12>) and its small plan 4096 x 192
    const int odd = (nc == 4096ll * 2560 || nc == 4096ll * 160) ? 5 : (nc == 4096ll * 3072 || nc == 4096ll * 192) ? 3 : 1;
    if (nc < 32 || nc > (1ll << 24) || (odd == 1 && (nc & (nc - 1)))) return TDOA_ERR_UNSUPPORTED;
    long long n1, n2;
    pl->odd = odd;
    if (nc >= 65536) {
        n1 = 4096;
        n2 = nc / n1;
    } else if (nc >= 256) {
        n2 = 16;
        n1 = nc / n2;
    } else {
        n2 = 2;
        n1 = nc / n2;
    }
    long long c = 32;
    while (c > 1 && (c > n1 || (size_t)(2 * n2 * c * 8) > kLdsCap)) c >>= 1;
    pl->N1 = (int)n1;
    pl->N2 = (int)n2;
    pl->logN1 = ilog2(n1);
    pl->logN2 = ilog2(n2);
    pl->C = (int)c;
    pl->logC = ilog2(c);
    pl->Nc = nc;
    pl->zpad = n1 == 4096 && (n2 == 4096 || n2 == 2048 || n2 == 2560 || n2 == 3072) ? zpad : 0;      // two-sweep column pass (fft_stockham.hpp, FftPlan)
    pl->Zs = nc + (long long)(n2 / 256) * pl->zpad;
    return TDOA_OK;
}

template <typename K>
int set_lds(tdoa_ctx *ctx, K kernel, size_t bytes)
{
    if (bytes > 48 * 1024)
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return TDOA_OK;
}

}  // namespace

#include "profiling.inc"
#include "fm_setup.inc"
#include "fm_route.inc"

namespace {

int check_ctx(tdoa_ctx *ctx)
{
    if (!ctx) return TDOA_ERR_INVALID;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return fail(ctx, TDOA_ERR_HIP, "hipSetDevice", e);
    return TDOA_OK;
}

// Transform length for `need` = window + search range samples.  The reference's rule is the next power of two
// (processor.go:563 -- dead code there, processor.go:638, and a design hint here: any N >= need gives the same linear
// correlation).  Ten-second windows at 2 Msps need 20 020 000 points: 2^25 = 33 554 432 is 40 % zero padding that every pass
// moves; 5 x 2^22 = 20 971 520 (packed 4096 x 2560) holds them with 4.5 %.  That plan exists where the step runs the fused /
// two-sweep column pass and the decimated inverse as a column walk (decimation_applies): everything else -- short search
// ranges, TDOA_LAGS_GO, TDOA_NO_DECIMATE, the any-size kernels -- keeps the power of two, and so does TDOA_POW2_ONLY=1 /
// TDOA_DEBUG_POW2_ONLY (the A/B switch).
long long choose_fft_size(const tdoa_ctx *ctx, long long need, int lag_lo, int lag_hi, int zpad, FftPlan *pl, int *rc)
{
    const long long p = std::max<long long>(next_pow2(need), 64);
    if (!ctx->knobs.pow2_only && p == (1ll << 25)) {
        // 5 x 2^22 = 20 971 520 (4096 x 2560), then 3 x 2^23 = 25 165 824 (4096 x 3072: windows of 10.5 to 12.6 s at 2 Msps)
        for (const long long cand : {5ll << 22, 3ll << 23}) {
            FftPlan q;
            if (need <= cand && make_plan(cand, true, &q, zpad) == TDOA_OK && decimation_applies(ctx->knobs, q, lag_lo, lag_hi)) {
                *pl = q;
                *rc = TDOA_OK;
                return cand;
            }
        }
    }
    *rc = make_plan(p, true, pl, zpad);
    return p;
}

// timeDomainCorrelation's block count for a template of lt samples (processor.go:691: starts 0, cb, 2 cb, ... < lt - cb)
long long go_blocks(long long lt, long long cb) { return lt > cb ? (lt - cb + cb - 1) / cb : 0; }

// IQ bytes of station s's window wid: block wid / wpb of that capture's OWN thirds, window wid % wpb of wlen samples in it
const uint8_t *window_iq(const tdoa_ctx *ctx, int s, int wid, int wpb, long long wlen)
{
    const auto &c = ctx->caps[s];
    return c.dev + 2 * ((long long)(wid / wpb) * (long long)(c.n / 3) + (long long)(wid % wpb) * wlen);
}

// the one statement of the peak selection's k / min_separation rule: nullptr when both are in range, else the message
// (callers that check more arguments with it word their own)
const char *check_k_sep(int k, int min_separation)
{
    return k < 1 || k > kSelMaxK || min_separation < 1 ? "k outside 1..16 or min_separation < 1" : nullptr;
}

// the arguments of the peak selection (k in 1 .. kSelMaxK, min_separation >= 1, an output) and the lag mode it needs
int check_selection(tdoa_ctx *ctx, int k, int min_separation, const void *out)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (check_k_sep(k, min_separation) || !out)
        return fail(ctx, TDOA_ERR_INVALID, "k outside 1..16, min_separation < 1 or output NULL");
    if (ctx->prm.lag_mode == TDOA_LAGS_GO) return fail(ctx, TDOA_ERR_UNSUPPORTED, "peak selection with TDOA_LAGS_GO");
    return TDOA_OK;
}
}  // namespace

#include "fm_pair.inc"
#include "step_graph.inc"
#include "stacked_api.inc"
#include "step_products.inc"

// ===========================================================================
// lifecycle
// ===========================================================================
extern "C" {

void tdoa_default_params(tdoa_params *p)
{
    if (!p) return;
    p->sample_rate = 2000000.0;   // processor.go:440
    p->max_lag = 20000;           // processor.go:633
    p->corr_block = 1000;         // processor.go:682
    p->weak_threshold = 0.001;    // processor.go:476
    p->window_len = 2000000;      // processor.go:772
    p->device = 0;
    p->windows_per_batch = 0;
    p->k1_smooth = 0;
    p->k1_gate = 0;
    p->lag_mode = TDOA_LAGS_SIGNED;
    p->reserved = 0;
}

int tdoa_abi_version(void) { return TDOA_ABI_VERSION; }

int tdoa_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char *tdoa_strerror(int status)
{
    switch (status) {
        case TDOA_OK: return "ok";
        case TDOA_ERR_INVALID: return "invalid argument";
        case TDOA_ERR_NO_DEVICE: return "no HIP device (this library has no CPU fallback)";
        case TDOA_ERR_HIP: return "HIP runtime error";
        case TDOA_ERR_NOMEM: return "out of device memory";
        case TDOA_ERR_UNSUPPORTED: return "unsupported size";
        case TDOA_ERR_STATE: return "invalid call order";
        case TDOA_ERR_SINGULAR: return "singular Jacobian matrix";
        default: return "unknown status";
    }
}

const char *tdoa_last_error(const tdoa_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }

const char *tdoa_kernel_name(int k)
{
    static const char *names[TDOA_K_COUNT] = {"k_fm_demod", "k_fwd_col", "k_fwd_row", "k_inv_row_pair",
                                              "k_inv_col_peak", "k_decode_peaks", "k_track_step", "k_track_finish"};
    return (k >= 0 && k < TDOA_K_COUNT) ? names[k] : "";
}

int tdoa_create(const tdoa_params *p, tdoa_ctx **out)
{
    if (!out) return TDOA_ERR_INVALID;
    *out = nullptr;
    tdoa_params prm;
    if (p)
        prm = *p;
    else
        tdoa_default_params(&prm);
    if (prm.max_lag < 1 || prm.corr_block < 1 || prm.window_len < 2 || !(prm.sample_rate > 0) || prm.k1_smooth < 0 ||
        prm.k1_smooth > 2001 || (prm.lag_mode != TDOA_LAGS_SIGNED && prm.lag_mode != TDOA_LAGS_GO))
        return TDOA_ERR_INVALID;
    int ndev = tdoa_device_count();
    if (ndev <= 0 || prm.device < 0 || prm.device >= ndev) return TDOA_ERR_NO_DEVICE;
    if (hipSetDevice(prm.device) != hipSuccess) return TDOA_ERR_NO_DEVICE;
    tdoa_ctx *ctx = new (std::nothrow) tdoa_ctx();
    if (!ctx) return TDOA_ERR_NOMEM;
    ctx->prm = prm;
    ctx->device = prm.device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, prm.device) == hipSuccess && cus > 0)
            ctx->n_cu = cus;
        size_t total_mem = 0;
        if (hipDeviceTotalMem(&total_mem, prm.device) == hipSuccess && total_mem > 0) ctx->total_mem = total_mem;
        if (total_mem > 0)
            ctx->workspace_limit = std::max(8.0 * 1073741824.0, (double)total_mem / 3.0);
    }
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return TDOA_ERR_HIP;
    }
    if (allow_big_lds(ctx) != TDOA_OK) {
        (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return TDOA_ERR_HIP;
    }
    {   // K1 angle tables, once per context (the first-octant table is the host's source for the two the kernels use)
        std::vector<int32_t> tab, direct, quad;
        std::vector<uint8_t> split;
        k1_build_table_host(tab, direct, quad, &split);
        void *dt = nullptr, *dq = nullptr;
        if (hipMalloc(&dt, kK1DirectBytes) != hipSuccess) {
            (void)hipStreamDestroy(ctx->stream);
            delete ctx;
            return TDOA_ERR_NOMEM;
        }
        ctx->k1_direct.p = dt;
        ctx->k1_direct.cap = kK1DirectBytes;
        if (hipMalloc(&dq, kK1QuadrantBytes) != hipSuccess) {
            tdoa_destroy(ctx);
            return TDOA_ERR_NOMEM;
        }
        ctx->k1_quad.p = dq;
        ctx->k1_quad.cap = kK1QuadrantBytes;
        if (hipMemcpy(dq, quad.data(), kK1QuadrantBytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dt, direct.data(), kK1DirectBytes, hipMemcpyHostToDevice) != hipSuccess) {
            tdoa_destroy(ctx);
            return TDOA_ERR_HIP;
        }
        void *ds = nullptr;
        if (hipMalloc(&ds, kK1SplitBytes) != hipSuccess) {
            tdoa_destroy(ctx);
            return TDOA_ERR_NOMEM;
        }
        ctx->k1_split.p = ds;
        ctx->k1_split.cap = kK1SplitBytes;
        if (hipMemcpy(ds, split.data(), kK1SplitBytes, hipMemcpyHostToDevice) != hipSuccess) {
            tdoa_destroy(ctx);
            return TDOA_ERR_HIP;
        }
    }
    knobs_from_env(ctx->knobs);
    if (!ctx->k1_split_lds) ctx->knobs.k1_split = false;      // the device gives no workgroup 160 KB of LDS: the quadrant route
    ctx->stg = stg_tables(ctx->knobs);
    *out = ctx;
    return TDOA_OK;
}

void tdoa_destroy(tdoa_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    prof_collect(ctx);
    for (hipEvent_t e : ctx->prof_pool) (void)hipEventDestroy(e);
    if (ctx->graph_exec) (void)hipGraphExecDestroy(ctx->graph_exec);
    clear_graph_marks(ctx);
    if (ctx->graph) (void)hipGraphDestroy(ctx->graph);
    tdoa_capture_clear(ctx);
    DevBuf *bufs[] = {&ctx->k1_direct, &ctx->k1_quad, &ctx->k1_split, &ctx->sw_desc, &ctx->pw_desc, &ctx->partials, &ctx->stats, &ctx->codes, &ctx->codes_lp, &ctx->k1_power, &ctx->dec_taps, &ctx->dec_gain, &ctx->stg_groups, &ctx->tz, &ctx->v, &ctx->keys,
                      &ctx->scales, &ctx->peaks, &ctx->scratch_a, &ctx->scratch_b, &ctx->lagdump,
                      &ctx->ex_a, &ctx->ex_b, &ctx->ex_c, &ctx->ex_d, &ctx->ex_part,
                      &ctx->g_sw_desc, &ctx->g_pw_desc, &ctx->g_quad_desc, &ctx->g_scales, &ctx->g_keys, &ctx->fine_raw, &ctx->fine, &ctx->qual,
                      &ctx->once_edges, &ctx->once_tiles, &ctx->once_fin, &ctx->slot_gain, &ctx->surf, &ctx->surf_out,
                      &ctx->sel_peaks, &ctx->sel_count, &ctx->stack_q, &ctx->stack_surf, &ctx->stack_keys, &ctx->stack_fine,
                      &ctx->stack_desc, &ctx->drift_tab, &ctx->drift_keys, &ctx->drift_h, &ctx->drift_prof, &ctx->track_tab,
                      &ctx->track_t, &ctx->track_d, &ctx->track_score, &ctx->track_lags, &ctx->track_values, &ctx->closure_centre,
                      &ctx->closure_part, &ctx->closure_best, &ctx->closure_out, &ctx->locate_table,
                      &ctx->locate_map, &ctx->locate_part, &ctx->locate_best, &ctx->locate_out, &ctx->locate_lags, &ctx->locate_corr,
                      &ctx->locate_clock, &ctx->sync_in, &ctx->sync_part, &ctx->sync_out, &ctx->sync_clock, &ctx->sync_lags,
                      &ctx->sync_corr, &ctx->debug_q, &ctx->debug_roots, &ctx->ctrack_d, &ctx->ctrack_t, &ctx->ctrack_roots,
                      &ctx->ctrack_out, &ctx->ctrack_cells, &ctx->ctrack_own, &ctx->locate_centres, &ctx->ctrack_pairs,
                      &ctx->mstat_ranks, &ctx->mstat_hist, &ctx->mstat_state, &ctx->mstat_out,
                      &ctx->sline_in, &ctx->sline_tab, &ctx->sline_roots, &ctx->sline_cur, &ctx->sline_k, &ctx->sline_h, &ctx->sline_part,
                      &ctx->sline_moved, &ctx->sline_start, &ctx->sline_out, &ctx->sline_clock, &ctx->sline_rate, &ctx->sline_rows,
                      &ctx->sline_lags, &ctx->sline_corr, &ctx->locate_qu, &ctx->locate_table_up, &ctx->locate_clock_up,
                      &ctx->sfine_out, &ctx->sfine_clock, &ctx->sfine_lags, &ctx->sfine_corr,
                      &ctx->slfine_cur, &ctx->slfine_kappa, &ctx->slfine_eta, &ctx->slfine_part, &ctx->slfine_moved, &ctx->slfine_start,
                      &ctx->slfine_out, &ctx->slfine_clock, &ctx->slfine_rate, &ctx->slfine_rows, &ctx->slfine_lags, &ctx->slfine_corr,
                      &ctx->locate_fine, &ctx->locate_fine_up, &ctx->zoom_map, &ctx->zoom_part, &ctx->zoom_out, &ctx->zoom_lags, &ctx->zoom_corr,
                      &ctx->tzoom_centre, &ctx->tzoom_e, &ctx->tzoom_total, &ctx->tzoom_out, &ctx->tzoom_cells, &ctx->tzoom_own, &ctx->mzoom_pairs,
                      &ctx->mix_in, &ctx->mix_rows, &ctx->mix_cdiff, &ctx->mix_cdiff_up, &ctx->mix_debug};
    for (DevBuf *b : bufs) release(*b);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// ===========================================================================
// mode B
// ===========================================================================

// device buffer of `bytes` for a station's capture: the station's previous owned buffer when it is large enough
// (re-uploading captures of the same size keeps the pointers, hence the captured graph), else a new allocation
static int capture_buffer(tdoa_ctx *ctx, int station, size_t bytes, uint8_t **out)
{
    if ((size_t)station >= ctx->caps.size()) ctx->caps.resize(station + 1);
    auto &c = ctx->caps[station];
    if (c.owned && c.dev && c.cap_bytes >= bytes) {
        *out = const_cast<uint8_t *>(c.dev);
        return TDOA_OK;
    }
    if (c.owned && c.dev) (void)hipFree(const_cast<uint8_t *>(c.dev));
    c = tdoa_ctx::Capture{};
    void *d = nullptr;
    const hipError_t e = hipMalloc(&d, bytes + 64);
    if (e != hipSuccess) return fail(ctx, TDOA_ERR_NOMEM, "hipMalloc capture", e);
    c.dev = static_cast<const uint8_t *>(d);
    c.owned = true;
    c.cap_bytes = bytes;
    c.n = 0;
    *out = static_cast<uint8_t *>(d);
    return TDOA_OK;
}

// host memory (src) or file (fd, from byte file_off) -> device, through the context's staged uploader
static int staged_upload(tdoa_ctx *ctx, uint8_t *dst, const uint8_t *src, int fd, size_t bytes, size_t file_off = 0)
{
    if (bytes == 0) return TDOA_OK;
    if (bytes < (1u << 20) && src) {   // small: one plain copy beats waking threads
        HIPCHK(ctx, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return TDOA_OK;
    }
    int n_threads = 4;   // measured: 2-4 copy threads reach ~40 GB/s on the bench node, 12 fall back to 25
    if (const char *e = std::getenv("TDOA_UPLOAD_THREADS")) n_threads = std::atoi(e);
    if (!ctx->uploader.init(ctx->device, n_threads)) {
        (void)hipGetLastError();
        return fail(ctx, TDOA_ERR_HIP, "staging buffers for the uploader");
    }
    const int st = ctx->uploader.run(dst, src, fd, bytes, file_off);
    if (st == 2) return fail(ctx, TDOA_ERR_INVALID, "failed to read data");
    if (st) {
        (void)hipGetLastError();
        return fail(ctx, TDOA_ERR_HIP, "host to device copy failed");
    }
    return TDOA_OK;
}

int tdoa_capture_upload(tdoa_ctx *ctx, int station, const uint8_t *iq, size_t n_samples)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (station < 0 || station > 1023 || (!iq && n_samples)) return fail(ctx, TDOA_ERR_INVALID, "bad station/iq");
    uint8_t *d = nullptr;
    if ((rc = capture_buffer(ctx, station, 2 * n_samples, &d))) return rc;
    ctx->caps[station].n = 0;                                  // not valid until the copy has finished
    if ((rc = staged_upload(ctx, d, iq, -1, 2 * n_samples))) return rc;
    ctx->caps[station].n = n_samples;
    return TDOA_OK;
}

// Sharded ingest: a rank of a multi-GPU job only reads the windows it owns (tdoa_process(rank, world)), so it only
// needs those bytes in its HBM.  The station's buffer has the full capture's size (window offsets stay what they are);
// the samples outside the uploaded ranges are never read by that rank.
int tdoa_capture_upload_range(tdoa_ctx *ctx, int station, size_t total_samples, size_t first_sample, const uint8_t *iq,
                              size_t n_samples)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (station < 0 || station > 1023 || (!iq && n_samples) || first_sample > total_samples ||
        n_samples > total_samples - first_sample)
        return fail(ctx, TDOA_ERR_INVALID, "bad station/iq/range");
    uint8_t *d = nullptr;
    if ((rc = capture_buffer(ctx, station, 2 * total_samples, &d))) return rc;
    const size_t had = ctx->caps[station].n;
    ctx->caps[station].n = 0;                                  // not valid until the copy has finished
    if ((rc = staged_upload(ctx, d + 2 * first_sample, iq, -1, 2 * n_samples))) return rc;
    (void)had;
    ctx->caps[station].n = total_samples;
    return TDOA_OK;
}

// The file form of tdoa_capture_upload_range, for the multi-device group's ingest (group_api.inc): every run
// [first, first + count) of a capture of total_samples is pread from fd at byte 2 first straight into a station buffer of
// the capture's full size, through the same staged uploader.
static int capture_upload_file_runs(tdoa_ctx *ctx, int station, int fd, size_t total_samples,
                                    const std::vector<std::pair<size_t, size_t>> &runs)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (station < 0 || station > 1023 || fd < 0) return fail(ctx, TDOA_ERR_INVALID, "bad station/file");
    for (const auto &r : runs)
        if (r.first > total_samples || r.second > total_samples - r.first) return fail(ctx, TDOA_ERR_INVALID, "run outside capture");
    uint8_t *d = nullptr;
    if ((rc = capture_buffer(ctx, station, 2 * total_samples, &d))) return rc;
    ctx->caps[station].n = 0;                                  // not valid until every copy has finished
    for (const auto &r : runs)
        if ((rc = staged_upload(ctx, d + 2 * r.first, nullptr, fd, 2 * r.second, 2 * r.first))) return rc;
    ctx->caps[station].n = total_samples;
    return TDOA_OK;
}

int tdoa_capture_upload_file(tdoa_ctx *ctx, int station, const char *path, size_t *n_samples)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (station < 0 || station > 1023 || !path) return fail(ctx, TDOA_ERR_INVALID, "bad station/path");
    FILE *f = std::fopen(path, "rb");
    if (!f) return fail(ctx, TDOA_ERR_INVALID, "failed to open file");
    if (std::fseek(f, 0, SEEK_END) != 0) { std::fclose(f); return fail(ctx, TDOA_ERR_INVALID, "failed to get file size"); }
    const long long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (size < 0) { std::fclose(f); return fail(ctx, TDOA_ERR_INVALID, "failed to get file size"); }
    const size_t n = (size_t)size / 2;                       // processor.go:182
    uint8_t *d = nullptr;
    if ((rc = capture_buffer(ctx, station, 2 * n, &d))) { std::fclose(f); return rc; }
    ctx->caps[station].n = 0;
    rc = staged_upload(ctx, d, nullptr, fileno(f), 2 * n);
    std::fclose(f);
    if (rc) return rc;
    ctx->caps[station].n = n;
    if (n_samples) *n_samples = n;
    return TDOA_OK;
}

int tdoa_capture_attach_device(tdoa_ctx *ctx, int station, const void *dev_iq, size_t n_samples)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (station < 0 || station > 1023 || !dev_iq || ((uintptr_t)dev_iq & 1)) return fail(ctx, TDOA_ERR_INVALID, "bad station/pointer");
    if ((size_t)station >= ctx->caps.size()) ctx->caps.resize(station + 1);
    auto &c = ctx->caps[station];
    if (c.owned && c.dev) (void)hipFree(const_cast<uint8_t *>(c.dev));
    c.dev = static_cast<const uint8_t *>(dev_iq);
    c.n = n_samples;
    c.owned = false;
    c.cap_bytes = 0;
    return TDOA_OK;
}

int tdoa_synth_capture(tdoa_ctx *ctx, int station, size_t block_samples, double ref_freq, double tgt_freq,
                       double noise_level, const double station_lle[3], const double tx_lle[3], double tx_power,
                       uint64_t seed)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (station < 0 || station > 1023 || block_samples < 2 || !station_lle || !tx_lle)
        return fail(ctx, TDOA_ERR_INVALID, "bad argument");
    uint8_t *d = nullptr;
    if ((rc = capture_buffer(ctx, station, 6 * block_samples, &d))) return rc;
    ctx->caps[station].n = 0;
    // simulator.go:104-120: distance -> travel time -> carrier phase; amplitude power/d*0.1
    double a[3], b[3];
    geo::latlon_to_ecef(station_lle[0], station_lle[1], station_lle[2], a);
    geo::latlon_to_ecef(tx_lle[0], tx_lle[1], tx_lle[2], b);
    const double dist = geo::range(a, b);
    const double travel = dist / geo::kC;
    const double fs = ctx->prm.sample_rate;
    const double phase = 2 * geo::kPi * tgt_freq * travel;
    const double amp = tx_power / dist * 0.1;
    SynthBlock blk[3] = {
        {2 * geo::kPi * ref_freq / fs, 0.0, 0.01, noise_level, seed, 1},      // simulator.go:126-128
        {2 * geo::kPi * tgt_freq / fs, phase, amp, noise_level, seed, 2},     // simulator.go:131-133
        {2 * geo::kPi * ref_freq / fs, 0.0, 0.01, noise_level, seed, 3},      // simulator.go:136-138
    };
    const long long n = (long long)block_samples;
    for (int k = 0; k < 3; k++)
        hipLaunchKernelGGL(k_synth_tone_block, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                           d + 2 * n * k, n, blk[k]);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->caps[station].n = 3 * block_samples;
    return TDOA_OK;
}

int tdoa_synth_weak_capture(tdoa_ctx *ctx, int station, size_t block_samples, double ref_freq, double tgt_freq,
                            const double station_lle[3], const double tx_lle[3], double ref_power, double tgt_power,
                            uint64_t seed)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (station < 0 || station > 1023 || block_samples < 2 || !station_lle || !tx_lle)
        return fail(ctx, TDOA_ERR_INVALID, "bad argument");
    uint8_t *d = nullptr;
    if ((rc = capture_buffer(ctx, station, 6 * block_samples, &d))) return rc;
    ctx->caps[station].n = 0;
    // weak_signal_simulator.go:155-173: distance -> travel time -> carrier phases; amplitudes power/d*0.1
    double a[3], b[3];
    geo::latlon_to_ecef(station_lle[0], station_lle[1], station_lle[2], a);
    geo::latlon_to_ecef(tx_lle[0], tx_lle[1], tx_lle[2], b);
    const double dist = geo::range(a, b);
    const double travel = dist / geo::kC;
    const double fs = ctx->prm.sample_rate;
    const double ref_amp = ref_power / dist * 0.1, tgt_amp = tgt_power / dist * 0.1;
    // weak profile, weak_signal_simulator.go:180-186; the strong block adds 0.001 sigma of noise only (:141-143)
    SynthWeakBlock weak = {2 * geo::kPi * ref_freq / fs, 2 * geo::kPi * ref_freq * travel, ref_amp, ref_amp * 0.8, 0.001,
                           ref_amp * 5.0, 0.05 / fs, ref_amp * 0.1, seed, 1, 1};
    SynthWeakBlock strong = {2 * geo::kPi * tgt_freq / fs, 2 * geo::kPi * tgt_freq * travel, tgt_amp, 0.001, 0.0, 0.0, 0.0,
                             0.0, seed, 2, 0};
    const long long n = (long long)block_samples;
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    hipLaunchKernelGGL(k_synth_weak_block, grid, blk, 0, ctx->stream, d, n, weak);                    // block 1: weak reference
    hipLaunchKernelGGL(k_synth_weak_block, grid, blk, 0, ctx->stream, d + 2 * n, n, strong);          // block 2: strong target
    weak.block_id = 3;
    hipLaunchKernelGGL(k_synth_weak_block, grid, blk, 0, ctx->stream, d + 4 * n, n, weak);            // block 3: weak reference
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->caps[station].n = 3 * block_samples;
    return TDOA_OK;
}

int tdoa_capture_download(tdoa_ctx *ctx, int station, size_t first_sample, size_t n_samples, uint8_t *out)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (station < 0 || (size_t)station >= ctx->caps.size() || !ctx->caps[station].dev || !out)
        return fail(ctx, TDOA_ERR_INVALID, "no such capture");
    const auto &c = ctx->caps[station];
    if (first_sample > c.n || n_samples > c.n - first_sample) return fail(ctx, TDOA_ERR_INVALID, "range outside capture");
    HIPCHK(ctx, hipMemcpy(out, c.dev + 2 * first_sample, 2 * n_samples, hipMemcpyDeviceToHost));
    return TDOA_OK;
}

int tdoa_capture_clear(tdoa_ctx *ctx)
{
    if (!ctx) return TDOA_ERR_INVALID;
    (void)hipSetDevice(ctx->device);         // the caller's thread may last have used another context's device
    for (auto &c : ctx->caps)
        if (c.owned && c.dev) (void)hipFree(const_cast<uint8_t *>(c.dev));
    ctx->caps.clear();
    return TDOA_OK;
}

static int window_geometry(const tdoa_ctx *ctx, long long *block, long long *wlen, int *wpb)
{
    if (ctx->caps.size() < 2) return TDOA_ERR_STATE;
    size_t nmin = (size_t)-1;
    for (auto &c : ctx->caps) {
        if (!c.dev) return TDOA_ERR_STATE;
        nmin = std::min(nmin, c.n);
    }
    // every capture is cut into its OWN thirds (processor.go:214 takes len(signal)/3 per file); the window grid
    // comes from the shortest one, so captures of unequal length still pair block k window w with block k window w
    long long b = (long long)(nmin / 3);
    if (b < 2) return TDOA_ERR_UNSUPPORTED;
    long long l = std::min<long long>(ctx->prm.window_len, b);
    *block = b;
    *wlen = l;
    *wpb = (int)std::max<long long>(1, b / l);
    return TDOA_OK;
}

int tdoa_num_windows(const tdoa_ctx *ctx, int *windows_per_block, int *n_windows_total)
{
    if (!ctx) return TDOA_ERR_INVALID;
    long long b, l;
    int wpb;
    int rc = window_geometry(ctx, &b, &l, &wpb);
    if (rc) return rc;
    if (windows_per_block) *windows_per_block = wpb;
    if (n_windows_total) *n_windows_total = 3 * wpb;
    return TDOA_OK;
}

int tdoa_num_pairs(const tdoa_ctx *ctx)
{
    if (!ctx) return 0;
    int s = (int)ctx->caps.size();
    return s * (s - 1) / 2;
}

int tdoa_plan_info(const tdoa_ctx *ctx, int64_t *fft_n, int32_t *n1, int32_t *n2)
{
    if (!ctx || !ctx->plan_n) return TDOA_ERR_STATE;
    if (fft_n) *fft_n = ctx->plan_n;
    if (n1) *n1 = ctx->plan.N1;
    if (n2) *n2 = ctx->plan.N2;
    return TDOA_OK;
}

static int process_impl(tdoa_ctx *ctx, int rank, int world, tdoa_peak *out_host, void *out_dev,
                        tdoa_fine_peak *fine_host, double gate, StepProduct *prod = nullptr)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (world < 1 || rank < 0 || rank >= world) return fail(ctx, TDOA_ERR_INVALID, "bad rank/world");
    long long block, wlen;
    int wpb;
    if ((rc = window_geometry(ctx, &block, &wlen, &wpb))) return fail(ctx, rc, "captures missing or too small");
    const int S = (int)ctx->caps.size();
    const int P = S * (S - 1) / 2;
    const int W = 3 * wpb;
    // TDOA_LAGS_GO: every window has the same length, so timeDomainCorrelation evaluates lag 0 only (processor.go:668-678)
    const bool go = ctx->prm.lag_mode == TDOA_LAGS_GO;
    const int lag_lo = go ? 0 : -(ctx->prm.max_lag - 1), lag_hi = go ? 0 : ctx->prm.max_lag - 1;
    FftPlan pl;
    const long long n = choose_fft_size(ctx, wlen + ctx->prm.max_lag, lag_lo, lag_hi, ctx->knobs.zpad, &pl, &rc);
    if (rc) return fail(ctx, rc, "FFT size unsupported");
    ctx->plan = pl;
    ctx->plan_n = n;
    // (TDOA_LAGS_GO) ... over the first B corr_block samples; with the template cut there the signal's samples beyond do not enter
    // lag 0 either, so every station-window is cut for the transforms (K1 and its statistics see the whole window)
    if (go && fine_host) return fail(ctx, TDOA_ERR_UNSUPPORTED, "sub-sample refinement with TDOA_LAGS_GO");
    const long long corr_len = go ? go_blocks(wlen, ctx->prm.corr_block) * ctx->prm.corr_block : wlen;

    // a launch group of n_sw station-windows and n_pw pair-windows as run_fm_batch sees it
    const bool pair_major = W < world;       // (build_step_layout's sharding rule)
    auto shape_of = [&](int n_sw, int n_pw, int n_quads) {
        FmBatchShape b = batch_shape(ctx);
        b.n_sw = n_sw;
        b.n_pw = n_pw;
        b.maxlen = (int)wlen;
        b.pairs_per_window = pair_major ? 0 : P;
        b.stations_per_window = pair_major ? 0 : S;
        b.n_quads = n_quads;
        b.allow_fused_k1 = corr_len >= 2;
        b.separate_stats = go;
        b.equal_len = !go;                   // every window has wlen samples
        b.fine = fine_host != nullptr;
        return b;
    };
    StepLayout lay;
    if (build_step_layout(S, W, rank, world, batch_bound(ctx, pl, lag_lo, lag_hi, shape_of(S, P, 0)), ctx->quad_cache, &lay))
        return fail(ctx, TDOA_ERR_UNSUPPORTED, "too many station pairs for one launch group");
    const int per_batch = lay.per_batch;
    const size_t n_mine = lay.mine.size();

    // all descriptors, uploaded once.  TDOA_LAGS_GO: a second copy of the station-window descriptors with the full window
    // length follows the first
    const size_t n_sw_all = lay.sw_station.size();
    std::vector<SWDesc> sw;
    for (size_t wi = 0; wi < n_mine; wi++)
        for (size_t k = lay.sw_off[wi]; k < lay.sw_off[wi + 1]; k++)
            sw.push_back(SWDesc{window_iq(ctx, lay.sw_station[k], lay.mine[wi], wpb, wlen), (int32_t)corr_len, 0});
    for (size_t k = 0; go && k < n_sw_all; k++) sw.push_back(SWDesc{sw[k].base, (int32_t)wlen, 0});
    for (PWDesc &d : lay.pw) d.len_a = (int32_t)corr_len;
    const size_t slots = (size_t)W * P;
    if (go && corr_len == 0) {                                 // windows of at most one block: (0, 0.0) everywhere (:708-717)
        if (out_host) std::memset(out_host, 0, sizeof(tdoa_peak) * slots);
        if (out_dev) HIPCHK(ctx, hipMemset(out_dev, 0, sizeof(PeakOut) * slots));
        return TDOA_OK;
    }
    hipStream_t st = ctx->stream;
    const int n_first = (int)std::min<size_t>(per_batch, n_mine);
    if ((rc = ensure(ctx, ctx->peaks, sizeof(PeakOut) * slots))) return rc;
    if ((rc = ensure(ctx, ctx->g_keys, sizeof(unsigned long long) * slots))) return rc;
    if ((rc = ensure(ctx, ctx->g_scales, sizeof(double) * slots))) return rc;
    if ((rc = ensure(ctx, ctx->slot_gain, sizeof(double) * slots))) return rc;
    if ((rc = ensure(ctx, ctx->g_sw_desc, sizeof(SWDesc) * std::max<size_t>(2 * n_sw_all, 1)))) return rc;
    if ((rc = ensure(ctx, ctx->g_pw_desc, sizeof(PWDesc) * std::max<size_t>(lay.pw.size(), 1)))) return rc;
    if ((rc = ensure(ctx, ctx->g_quad_desc, sizeof(QuadDesc) * std::max<size_t>(lay.quads.size(), 1)))) return rc;
    if (fine_host) {
        if ((rc = ensure(ctx, ctx->fine_raw, 3 * sizeof(float) * slots))) return rc;
        if ((rc = ensure(ctx, ctx->fine, sizeof(FineOut) * slots))) return rc;
    }
    if (n_first && (rc = reserve_fm_batch(ctx, plan_fm_batch(ctx->knobs, ctx->stg, ctx->n_cu, pl, lag_lo, lag_hi, shape_of(n_first * S, n_first * P, 0)))))
        return rc;
    auto *d_sw = ctx->g_sw_desc.as<SWDesc>();
    auto *d_pw = ctx->g_pw_desc.as<PWDesc>();
    auto *d_quads = ctx->g_quad_desc.as<QuadDesc>();
    auto *d_keys = ctx->g_keys.as<unsigned long long>();
    auto *d_scales = ctx->g_scales.as<double>();
    // the product's buffers: allocated after the grouping is fixed (batch_bound counts these buffers as held, so a later
    // call groups as this one did)
    const int n_lags = lag_hi - lag_lo + 1;
    const StepView view{ctx, &lay, slots, n_lags, lag_lo, P, wpb, d_pw, d_keys, d_scales, nullptr};
    if (prod && (rc = prod->reserve(view))) return rc;

    std::vector<uint64_t> key = step_graph_key(ctx, rank, world, per_batch, wlen, block, go, fine_host != nullptr, gate);
    if (prod)
        prod->key(&key);
    else
        key.insert(key.end(), {StepProduct::None, 0, 0, 0});
    if (!step_graph_replays(ctx, key)) {
        if (prod && (rc = prod->upload(view))) return rc;
        std::vector<double> scales(slots, 1.0 / (4.0 * (double)n * std::sqrt((double)corr_len)));
        HIPCHK(ctx, hipMemcpyAsync(d_scales, scales.data(), sizeof(double) * slots, hipMemcpyHostToDevice, st));
        if (!sw.empty()) {
            HIPCHK(ctx, hipMemcpyAsync(d_sw, sw.data(), sizeof(SWDesc) * sw.size(), hipMemcpyHostToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(d_pw, lay.pw.data(), sizeof(PWDesc) * lay.pw.size(), hipMemcpyHostToDevice, st));
        }
        if (!lay.quads.empty())
            HIPCHK(ctx, hipMemcpyAsync(d_quads, lay.quads.data(), sizeof(QuadDesc) * lay.quads.size(), hipMemcpyHostToDevice, st));

        HIPCHK(ctx, hipStreamSynchronize(st));   // host vectors go out of scope below
    }
    if (prod && (rc = prod->refresh(view))) return rc;      // every call, replayed or not, before the step is launched

    auto enqueue = [&]() -> int {
        ctx->prof_last = -1;
        if (ctx->knobs.memset_nodes)         // probe only (TDOA_DEBUG_MEMSET_NODES=1)
            (void)hipMemsetAsync(d_keys, 0, sizeof(unsigned long long) * slots, st);
        else
            hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, d_keys, slots);
        float *fine_raw = fine_host ? ctx->fine_raw.as<float>() : nullptr;
        for (size_t w0 = 0; w0 < n_mine; w0 += per_batch) {
            const int nw = (int)std::min<size_t>(per_batch, n_mine - w0);
            const int n_sw = (int)(lay.sw_off[w0 + nw] - lay.sw_off[w0]), n_pw = (int)(lay.pw_off[w0 + nw] - lay.pw_off[w0]);
            FmBufs bf{d_sw + lay.sw_off[w0], go ? d_sw + n_sw_all + lay.sw_off[w0] : nullptr, d_pw + lay.pw_off[w0],
                      d_quads + lay.q_off[w0], d_keys, nullptr, 1.0f, (double)wlen * n_sw, fine_raw};
            if (prod) {                                // the K5 kernels' lag arrays, pair-window i of the batch at i * n_lags
                bf.lag_dump = ctx->surf.as<float>() + lay.pw_off[w0] * (size_t)n_lags;
                bf.dump_stride = (size_t)n_lags;
            }
            const int r = run_fm_batch(ctx, shape_of(n_sw, n_pw, (int)(lay.q_off[w0 + nw] - lay.q_off[w0])), pl, lag_lo, lag_hi, bf);
            if (r) return r;
        }
        // (every batch of a step takes the same path: same plan, same lag range, same lengths)
        launch_decode(ctx, d_keys, d_scales, slots, fine_raw, gate);
        StepView v = view;
        v.slot_gain = ctx->once_active ? ctx->slot_gain.as<const double>() : nullptr;
        if (prod) {
            ctx->prof_last = -1;             // unscoped launches
            prod->enqueue(v);
        }
        return TDOA_OK;
    };
    if ((rc = run_step_graph(ctx, key, enqueue))) return rc;

    if (out_dev)
        HIPCHK(ctx, hipMemcpyAsync(out_dev, ctx->peaks.p, sizeof(PeakOut) * slots, hipMemcpyDeviceToDevice, st));
    if (out_host)
        HIPCHK(ctx, hipMemcpyAsync(out_host, ctx->peaks.p, sizeof(PeakOut) * slots, hipMemcpyDeviceToHost, st));
    if (fine_host)
        HIPCHK(ctx, hipMemcpyAsync(fine_host, ctx->fine.p, sizeof(FineOut) * slots, hipMemcpyDeviceToHost, st));
    if (prod && (rc = prod->download(view))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(st));
    prof_collect(ctx);
    collect_step_graph_marks(ctx);
    return TDOA_OK;
}

int tdoa_process(tdoa_ctx *ctx, int rank, int world, tdoa_peak *out_host, void *out_dev)
{
    return process_impl(ctx, rank, world, out_host, out_dev, nullptr, 0.0);
}

int tdoa_process_fine(tdoa_ctx *ctx, int rank, int world, double gate_samples, tdoa_peak *out_host,
                      tdoa_fine_peak *fine_host)
{
    if (!fine_host || !(gate_samples >= 0.0)) return fail(ctx, TDOA_ERR_INVALID, "fine_host is NULL or gate < 0");
    return process_impl(ctx, rank, world, out_host, nullptr, fine_host, gate_samples);
}

int tdoa_process_lags(tdoa_ctx *ctx, int rank, int world, float *lags_host, void *lags_dev)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (!lags_host && !lags_dev) return fail(ctx, TDOA_ERR_INVALID, "lags_host and lags_dev are NULL");
    if (ctx->prm.lag_mode == TDOA_LAGS_GO) return fail(ctx, TDOA_ERR_UNSUPPORTED, "correlation surfaces with TDOA_LAGS_GO");
    LagsProduct prod;
    prod.lags_host = lags_host;
    prod.lags_dev = lags_dev;
    return process_impl(ctx, rank, world, nullptr, nullptr, nullptr, 0.0, &prod);
}

int tdoa_process_peaks(tdoa_ctx *ctx, int rank, int world, int k, int min_separation, tdoa_peak *peaks_host,
                       int32_t *count_host)
{
    int rc;
    if ((rc = check_selection(ctx, k, min_separation, peaks_host))) return rc;
    PeaksProduct prod;
    prod.k = k;
    prod.min_sep = min_separation;
    prod.peaks_host = peaks_host;
    prod.count_host = count_host;
    return process_impl(ctx, rank, world, nullptr, nullptr, nullptr, 0.0, &prod);
}

// What every entry on stacks refuses before it builds its product, in this order: a null context, a negative
// windows_per_stack, the entry's own arguments (bad_args: its check's message, which needs no context), TDOA_LAGS_GO under
// the entry's own name, and for the searches the captures.
static int refuse_stacked(tdoa_ctx *ctx, int windows_per_stack, const char *bad_args, const char *go_what, bool need_captures = false)
{
    if (!ctx) return TDOA_ERR_INVALID;
    if (windows_per_stack < 0) return fail(ctx, TDOA_ERR_INVALID, "windows_per_stack < 0");
    if (bad_args) return fail(ctx, TDOA_ERR_INVALID, bad_args);
    if (ctx->prm.lag_mode == TDOA_LAGS_GO) return fail(ctx, TDOA_ERR_UNSUPPORTED, go_what);
    if (need_captures && ctx->caps.empty()) return fail(ctx, TDOA_ERR_STATE, "captures missing");
    return TDOA_OK;
}

// the stack of a product: its length, its selection and its outputs (the searches on Q ask for none: k = min_separation = 1)
static void fill_stack(StackProduct *sp, int windows_per_stack, int k = 1, int min_separation = 1, double gate = 0.0,
                       tdoa_peak *peaks_host = nullptr, int32_t *count_host = nullptr, tdoa_fine_peak *fine_host = nullptr,
                       float *surface_host = nullptr, int64_t *partial_host = nullptr)
{
    sp->m = windows_per_stack;
    sp->k = k;
    sp->min_sep = min_separation;
    sp->gate = gate;
    sp->peaks_host = peaks_host;
    sp->count_host = count_host;
    sp->fine_host = fine_host;
    sp->surface_host = surface_host;
    sp->partial_host = partial_host;
}

int tdoa_process_stacked(tdoa_ctx *ctx, int rank, int world, int windows_per_stack, int k, int min_separation,
                         double gate_samples, tdoa_peak *peaks_host, int32_t *count_host, tdoa_fine_peak *fine_host,
                         float *surface_host, int64_t *partial_host)
{
    const char *bad = check_stacked_args(windows_per_stack, k, min_separation, gate_samples,
                                         peaks_host || count_host || fine_host || surface_host || partial_host);
    if (int rc = refuse_stacked(ctx, windows_per_stack, bad, "stacked correlation with TDOA_LAGS_GO")) return rc;
    StackProduct prod;
    fill_stack(&prod, windows_per_stack, k, min_separation, gate_samples, peaks_host, count_host, fine_host, surface_host, partial_host);
    // (the gate stays a word of the step graph's key through the step's own gate argument)
    return process_impl(ctx, rank, world, nullptr, nullptr, nullptr, gate_samples, &prod);
}

int tdoa_process_stacked_drift(tdoa_ctx *ctx, int windows_per_stack, int k, int min_separation, double gate_samples,
                               int max_drift, int drift_den, tdoa_peak *peaks_host, int32_t *count_host, tdoa_fine_peak *fine_host,
                               float *surface_host, int64_t *partial_host, int32_t *drift_host, tdoa_peak *profile_host)
{
    const char *bad = check_stacked_args(windows_per_stack, k, min_separation, gate_samples,
                                         peaks_host || count_host || fine_host || surface_host || partial_host || drift_host ||
                                             profile_host);
    if (!bad && drift_den < 1) bad = "drift_den < 1";
    if (!bad && (max_drift < 0 || max_drift > 512)) bad = "max_drift outside 0 .. 512";
    if (int rc = refuse_stacked(ctx, windows_per_stack, bad, "stacked correlation with TDOA_LAGS_GO")) return rc;
    int wpb = 0;
    if (int rc = tdoa_num_windows(ctx, &wpb, nullptr)) return fail(ctx, rc, "captures missing or too small");
    if (drift_shift(max_drift, stack_geom(wpb, windows_per_stack).mm - 1, drift_den) > ctx->prm.max_lag - 1)
        return fail(ctx, TDOA_ERR_INVALID, "the search's largest shift exceeds max_lag - 1");
    StackDriftProduct prod;
    fill_stack(&prod, windows_per_stack, k, min_separation, gate_samples, peaks_host, count_host, fine_host, surface_host, partial_host);
    prod.H = max_drift;
    prod.D = drift_den;
    prod.drift_host = drift_host;
    prod.profile_host = profile_host;
    return process_impl(ctx, 0, 1, nullptr, nullptr, nullptr, gate_samples, &prod);
}

int tdoa_process_track(tdoa_ctx *ctx, int windows_per_stack, int max_step, tdoa_peak *score_host, int32_t *lags_host,
                       double *values_host, float *surface_host, int64_t *total_host)
{
    const char *bad = nullptr;
    if (max_step < 0 || max_step > kTrackMaxStep)
        bad = "max_step outside 0 .. 64";
    else if (!score_host && !lags_host && !values_host && !surface_host && !total_host)
        bad = "every output is NULL";
    if (int rc = refuse_stacked(ctx, windows_per_stack, bad, "delay tracks with TDOA_LAGS_GO")) return rc;
    int wpb = 0;
    if (int rc = tdoa_num_windows(ctx, &wpb, nullptr)) return fail(ctx, rc, "captures missing or too small");
    if (stack_geom(wpb, windows_per_stack).mm > 4096) return fail(ctx, TDOA_ERR_INVALID, "a stack of more than 4096 windows");
    StackTrackProduct prod;
    prod.m = windows_per_stack;
    prod.J = max_step;
    prod.score_host = score_host;
    prod.lags_host = lags_host;
    prod.values_host = values_host;
    prod.surface_host = surface_host;
    prod.total_host = total_host;
    return process_impl(ctx, 0, 1, nullptr, nullptr, nullptr, 0.0, &prod);
}

// fast_analyzer.go:139-155 and collector.go:224 from the exact integer sums, in the reference's expression order
static void finalize_quality(const QualAcc &q, long long n_samples, tdoa_window_quality *out)
{
    std::memset(out, 0, sizeof(*out));
    out->n_samples = n_samples;
    if (n_samples <= 0) return;
    const double n = (double)n_samples;
    const double isum = (double)q.si, qsum = (double)q.sq, isq = (double)q.sii, qsq = (double)q.sqq;   // exact (< 2^53)
    out->i_avg = isum / n;
    out->q_avg = qsum / n;
    out->i_std = std::sqrt((isq / n) - (out->i_avg * out->i_avg));
    out->q_std = std::sqrt((qsq / n) - (out->q_avg * out->q_avg));
    const double pm = std::sqrt(out->i_std * out->i_std + out->q_std * out->q_std);
    out->power_level = pm <= 1e-10 ? -100.0 : 20 * std::log10(pm);
    // sum of (b-127.5)^2 over both components: every term is a multiple of 1/4, so the f64 running sum is exact
    const double sumsq = (isq + qsq) - 255.0 * (isum + qsum) + 2.0 * n * 16256.25;
    out->mean_power = sumsq / n;
    out->i_min = (int32_t)q.imin; out->i_max = (int32_t)q.imax; out->q_min = (int32_t)q.qmin; out->q_max = (int32_t)q.qmax;
    out->has_clipping = (q.imin == 0 || q.imax == 255 || q.qmin == 0 || q.qmax == 255) ? 1 : 0;
    out->has_overload = (out->i_std < 2 || out->q_std < 2) ? 1 : 0;
}

static int run_quality(tdoa_ctx *ctx, const SWDesc *d_sw, int n_sw, long long max_len, std::vector<QualAcc> *host)
{
    int rc;
    if ((rc = ensure(ctx, ctx->qual, sizeof(QualAcc) * (size_t)std::max(n_sw, 1)))) return rc;
    auto *acc = ctx->qual.as<QualAcc>();
    host->resize(n_sw);
    if (n_sw == 0) return TDOA_OK;
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_quality_init, dim3((n_sw + 255) / 256), dim3(256), 0, st, acc, n_sw);
    const unsigned chunks = (unsigned)std::max<long long>(1, (max_len + kQualChunk - 1) / kQualChunk);
    hipLaunchKernelGGL(k_window_quality, dim3(chunks, n_sw), dim3(256), 0, st, d_sw, acc);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(host->data(), acc, sizeof(QualAcc) * (size_t)n_sw, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return TDOA_OK;
}

int tdoa_window_quality_all(tdoa_ctx *ctx, int rank, int world, tdoa_window_quality *out_host)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (world < 1 || rank < 0 || rank >= world || !out_host) return fail(ctx, TDOA_ERR_INVALID, "bad rank/world/out");
    long long block, wlen;
    int wpb;
    if ((rc = window_geometry(ctx, &block, &wlen, &wpb))) return fail(ctx, rc, "captures missing or too small");
    const int S = (int)ctx->caps.size();
    const int W = 3 * wpb;
    std::vector<int> mine;
    for (int w = rank; w < W; w += world) mine.push_back(w);
    std::vector<SWDesc> sw(mine.size() * (size_t)S);
    for (size_t wi = 0; wi < mine.size(); wi++) {
        const int wid = mine[wi];
        for (int s = 0; s < S; s++) {
            sw[wi * S + s] = SWDesc{window_iq(ctx, s, wid, wpb, wlen), (int32_t)wlen, 0};
        }
    }
    if ((rc = ensure(ctx, ctx->g_sw_desc, sizeof(SWDesc) * std::max<size_t>(sw.size(), 1)))) return rc;
    ctx->graph_key.clear();     // the descriptor buffer of a captured tdoa_process graph is being rewritten
    if (!sw.empty())
        HIPCHK(ctx, hipMemcpyAsync(ctx->g_sw_desc.p, sw.data(), sizeof(SWDesc) * sw.size(), hipMemcpyHostToDevice, ctx->stream));
    std::vector<QualAcc> acc;
    if ((rc = run_quality(ctx, ctx->g_sw_desc.as<const SWDesc>(), (int)sw.size(), wlen, &acc))) return rc;
    std::memset(out_host, 0, sizeof(tdoa_window_quality) * (size_t)W * S);
    for (size_t wi = 0; wi < mine.size(); wi++)
        for (int s = 0; s < S; s++) finalize_quality(acc[wi * S + s], wlen, &out_host[(size_t)mine[wi] * S + s]);
    return TDOA_OK;
}

int tdoa_window_quality_u8(tdoa_ctx *ctx, const uint8_t *iq, size_t n_samples, tdoa_window_quality *out)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!out || (!iq && n_samples) || n_samples > 0x7fffffff) return fail(ctx, TDOA_ERR_INVALID, "bad argument");
    if (n_samples == 0) { finalize_quality(QualAcc{}, 0, out); return TDOA_OK; }
    if ((rc = ensure(ctx, ctx->scratch_a, 2 * n_samples + 16))) return rc;
    if ((rc = ensure(ctx, ctx->sw_desc, sizeof(SWDesc)))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->scratch_a.p, iq, 2 * n_samples, hipMemcpyHostToDevice, ctx->stream));
    const SWDesc d{ctx->scratch_a.as<const uint8_t>(), (int32_t)n_samples, 0};
    HIPCHK(ctx, hipMemcpyAsync(ctx->sw_desc.p, &d, sizeof(d), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // d is a stack object
    std::vector<QualAcc> acc;
    if ((rc = run_quality(ctx, ctx->sw_desc.as<const SWDesc>(), 1, (long long)n_samples, &acc))) return rc;
    finalize_quality(acc[0], (long long)n_samples, out);
    return TDOA_OK;
}

int tdoa_process_u8(tdoa_ctx *ctx, const uint8_t *const *station_iq, const size_t *n_samples, int n_stations,
                    tdoa_peak *out)
{
    if (!ctx || !station_iq || !n_samples || n_stations < 2 || !out) return fail(ctx, TDOA_ERR_INVALID, "bad argument");
    int rc = TDOA_OK;
    if ((int)ctx->caps.size() != n_stations) rc = tdoa_capture_clear(ctx);   // else the uploads reuse the buffers
    for (int s = 0; s < n_stations && !rc; s++) rc = tdoa_capture_upload(ctx, s, station_iq[s], n_samples[s]);
    if (rc) return rc;
    return tdoa_process(ctx, 0, 1, out, nullptr);
}

int tdoa_fm_preprocess_u8(tdoa_ctx *ctx, const uint8_t *iq, size_t n, float *out_f32, tdoa_fm_stats *stats)
{
    int rc;
    if ((rc = check_ctx(ctx))) return rc;
    if (!iq || n == 0 || n > 0x3fffffff) return fail(ctx, TDOA_ERR_INVALID, "bad argument");
    if ((rc = ensure(ctx, ctx->scratch_a, 2 * n + 16))) return rc;
    if ((rc = ensure(ctx, ctx->scratch_b, sizeof(float) * n))) return rc;
    if ((rc = ensure(ctx, ctx->sw_desc, sizeof(SWDesc)))) return rc;
    const int pieces = (int)((n + kDemodPiece - 1) / kDemodPiece);
    const long long code_stride = ((long long)n + 15) / 8 * 8;
    if ((rc = ensure(ctx, ctx->partials, sizeof(StatsPartial)))) return rc;
    if ((rc = ensure(ctx, ctx->stats, sizeof(FmStats)))) return rc;
    if ((rc = ensure(ctx, ctx->codes, sizeof(int) * (size_t)code_stride))) return rc;
    hipStream_t st = ctx->stream;
    SWDesc sw = {ctx->scratch_a.as<uint8_t>(), (int32_t)n, 0};
    HIPCHK(ctx, hipMemcpyAsync(ctx->scratch_a.p, iq, 2 * n, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->sw_desc.p, &sw, sizeof(sw), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    auto *d_sw = ctx->sw_desc.as<SWDesc>();
    if (ctx->prm.k1_smooth > 1 && (rc = ensure(ctx, ctx->codes_lp, sizeof(int) * (size_t)code_stride))) return rc;
    if (ctx->prm.k1_gate && (rc = ensure(ctx, ctx->k1_power, sizeof(unsigned long long)))) return rc;
    // no output array wanted and no option that needs the codes: the reduce-only pass of the fused path
    const bool stats_only = !out_f32 && ctx->prm.k1_smooth <= 1 && !ctx->prm.k1_gate;
    int *codes_used = launch_k1(ctx, st, d_sw, 1, (int)n, pieces, code_stride, !stats_only);
    if (codes_used)
        hipLaunchKernelGGL(k_fm_dump, dim3((unsigned)((n + 255) / 256), 1), dim3(256), 0, st, d_sw,
                           codes_used, ctx->stats.as<FmStats>(),
                           ctx->scratch_b.as<float>());
    HIPCHK(ctx, hipGetLastError());
    if (out_f32) HIPCHK(ctx, hipMemcpyAsync(out_f32, ctx->scratch_b.p, sizeof(float) * n, hipMemcpyDeviceToHost, st));
    if (stats) HIPCHK(ctx, hipMemcpyAsync(stats, ctx->stats.p, sizeof(FmStats), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return TDOA_OK;
}

// ===========================================================================
// downstream geodesy / solver (host)
// ===========================================================================
void tdoa_latlon_to_ecef(double lat, double lon, double elev, double xyz[3]) { geo::latlon_to_ecef(lat, lon, elev, xyz); }
void tdoa_ecef_to_latlon(double x, double y, double z, double lle[3]) { geo::ecef_to_latlon(x, y, z, lle); }
int tdoa_solve_3station(const double stations_lle[9], const double *range_diff, double out_lle[3], int *iterations)
{
    if (!stations_lle || !range_diff || !out_lle) return TDOA_ERR_INVALID;
    return geo::solve_3station(stations_lle, range_diff, out_lle, iterations) ? TDOA_ERR_SINGULAR : TDOA_OK;
}

int tdoa_solve_nstation(const double *stations_lle, int n_stations, const double *range_diff, const double *weights,
                        int solve_z, double out_lle[3], int *iterations)
{
    if (!stations_lle || !range_diff || !out_lle) return TDOA_ERR_INVALID;
    const int rc = geo::solve_nstation(stations_lle, n_stations, range_diff, weights, solve_z, 10, 0.5, 1.0, out_lle,
                                       iterations);
    return rc == 0 ? TDOA_OK : (rc == -2 ? TDOA_ERR_UNSUPPORTED : rc == -3 ? TDOA_ERR_INVALID : TDOA_ERR_SINGULAR);
}

int tdoa_solve_surface(const double *stations_lle, int n_stations, const double *range_diff, const double *weights,
                       double height_m, double out_lle[3], int *iterations)
{
    if (!stations_lle || !range_diff || !out_lle || !std::isfinite(height_m)) return TDOA_ERR_INVALID;
    const int rc = geo::solve_surface(stations_lle, n_stations, range_diff, weights, height_m, 20, 1.0, out_lle, iterations);
    return rc == 0 ? TDOA_OK : (rc == -2 ? TDOA_ERR_UNSUPPORTED : rc == -3 ? TDOA_ERR_INVALID : TDOA_ERR_SINGULAR);
}

}  // extern "C"

#include "debug_api.inc"
#include "exact_reference_api.inc"
#include "group_api.inc"
// The searches on the stacks' sums.  stack_search.inc's drivers call process_impl above and the group's helpers, which is why
// it and the searches' files come last; a search's file needs nothing of another's but what its header names.  The last one
// chains two of the others (a fine clock stage, k_line_mix, a locate stage) for the two calls that go from reference blocks to fix.
#include "stack_search.inc"
#include "closure_api.inc"
#include "map_stats_api.inc"
#include "locate_api.inc"
#include "locate_run.inc"
#include "locate_zoom_api.inc"
#include "locate_multi_zoom_api.inc"
#include "locate_track_zoom_api.inc"
#include "sync_api.inc"
#include "sync_fine_api.inc"
#include "sync_drift_api.inc"
#include "sync_drift_fine_api.inc"
#include "sync_locate_api.inc"
