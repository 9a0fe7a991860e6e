// fm_route.inc -- mode B: the forms a batch takes (plan_fm_batch), then its launches (run_fm_batch, launch_decode).
// Included by tdoa_mi355x.hip after fm_setup.inc.

namespace {

// f(std::integral_constant<int, V>{}) for the V of Vs equal to v -- the last one when none is: a launcher's template ladder
// (every V listed is instantiated)
template <int V, int... More, typename F>
void with_int(int v, F &&f)
{
    if constexpr (sizeof...(More) == 0) f(std::integral_constant<int, V>{});
    else if (v == V) f(std::integral_constant<int, V>{});
    else with_int<More...>(v, f);
}
// f(std::integral_constant<int, V>{}) for every V of Vs
template <int... Vs, typename F>
void for_ints(F &&f) { (f(std::integral_constant<int, Vs>{}), ...); }
template <typename F>
void with_bool(bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// zero n_sw window accumulators (a kernel node: the captured step holds kernel nodes only, DESIGN.md section 7)
void zero_partials(hipStream_t st, StatsPartial *partials, int n_sw, bool memset_node = false)
{
    static_assert(sizeof(StatsPartial) == 32, "four 64-bit words per station-window");
    const size_t words = 4 * (size_t)n_sw;
    if (memset_node) {                       // probe only (TDOA_DEBUG_MEMSET_NODES=1)
        (void)hipMemsetAsync(partials, 0, 8 * words, st);
        return;
    }
    hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<unsigned long long *>(partials), words);
}

// K1 for n_sw station-windows: capture bytes -> exact window statistics, and -- when `materialise` -- the 24-bit codes
// (int32) for the consumers that read them from memory; every buffer must have been reserved (no allocation here: the
// caller may be capturing a graph).  Returns the code array downstream reads (nullptr: fused path, the forward column
// kernels evaluate the discriminator themselves).
// Optional steps (tdoa_params): k1_gate -- the prebuilt binary's power gate (windows of mean power <= 0.01 get envelope
// codes instead of phase codes); k1_smooth -- its moving average on the discriminator output.  Both need the codes.
// pack3: the codes go to memory at 3 bytes each (k1_store8_packed; only the segment kernels read that layout, so it is
// never combined with k1_gate / k1_smooth, whose kernels work on int32 rows).
int *launch_k1(tdoa_ctx *ctx, hipStream_t st, const SWDesc *d_sw, int n_sw, int maxlen, int pieces, long long code_stride,
               bool materialise, bool pack3 = false)
{
    auto *partials = ctx->partials.as<StatsPartial>();
    auto *stats = ctx->stats.as<FmStats>();
    auto *codes = ctx->codes.as<int>();
    const auto *table = ctx->k1_direct.as<const int>();
    const dim3 per_chunk((unsigned)((maxlen + 2047) / 2048), n_sw);
    unsigned long long *power = nullptr;
    if (ctx->prm.k1_gate) {
        power = ctx->k1_power.as<unsigned long long>();
        hipLaunchKernelGGL(k_zero_u64, dim3((unsigned)(((size_t)n_sw + 255) / 256)), dim3(256), 0, st, power, (size_t)n_sw);
        hipLaunchKernelGGL(k_k1_power, per_chunk, dim3(256), 0, st, d_sw, power);
    }
    zero_partials(st, partials, n_sw, ctx->knobs.memset_nodes);
    const long long items = (long long)((pieces + kDemodItem - 1) / kDemodItem) * n_sw;      // workgroup items
    const int blocks = (int)std::max<long long>(1, std::min<long long>(items, ctx->n_cu));        // one workgroup per CU (128 KB table)
    if (materialise && pack3)
        hipLaunchKernelGGL((k_fm_demod<true, true>), dim3(blocks), dim3(kDemodThreads), kK1DirectBytes, st, d_sw, n_sw, pieces, table,
                           codes, code_stride, partials, power);
    else if (materialise)
        hipLaunchKernelGGL(k_fm_demod<true>, dim3(blocks), dim3(kDemodThreads), kK1DirectBytes, st, d_sw, n_sw, pieces, table,
                           codes, code_stride, partials, power);
    else
        hipLaunchKernelGGL(k_fm_demod<false>, dim3(blocks), dim3(kDemodThreads), kK1DirectBytes, st, d_sw, n_sw, pieces, table,
                           static_cast<int *>(nullptr), code_stride, partials, power);
    if (power) hipLaunchKernelGGL(k_k1_envelope, per_chunk, dim3(256), 0, st, d_sw, power, codes, code_stride, partials);
    if (ctx->prm.k1_smooth > 1) {
        // statistics of the smoothed codes replace those of the raw ones
        auto *lp = ctx->codes_lp.as<int>();
        zero_partials(st, partials, n_sw);
        hipLaunchKernelGGL(k_k1_smooth, per_chunk, dim3(256), 0, st, d_sw, codes, lp, code_stride, ctx->prm.k1_smooth / 2,
                           partials, power);
        codes = lp;
    }
    hipLaunchKernelGGL(k_fm_stats_final, dim3((n_sw + 63) / 64), dim3(64), 0, st, d_sw, partials, stats, n_sw);
    return materialise ? codes : nullptr;
}

// ---- mode B: the forms a batch takes (plan_fm_batch), then the launches (run_fm_batch) --------------------------------
// What the caller knows of a batch of station-windows (sw) and pair-windows (pw).
struct FmBatchShape {
    int n_sw = 0, n_pw = 0, maxlen = 0;      // maxlen: longest window
    int pairs_per_window = 0;        // > 0: every window of the batch carries this many pair-windows (window-major sharding)
    int stations_per_window = 0;     // > 0: ... and they are all the S (S - 1) / 2 pairs of its S stations, station-windows laid
                                     // out window by window, pairs in the order (0,1), (0,2), ..., (S-2,S-1) -- process_impl's
                                     // window-major layout, which the staged walk's groups are built for; 0 otherwise
    int n_quads = 0;                 // segment form: quads of the batch (two station transforms serve up to four pair-windows)
    bool allow_fused_k1 = true;      // false: a window may be shorter than two samples
    bool separate_stats = false;     // K1 and its statistics run over other windows than the transforms (TDOA_LAGS_GO)
    bool equal_len = false;          // every station-window of the batch has `maxlen` samples
    bool fine = false;               // sub-sample refinement: the peaks' neighbours are read back
    int k1_smooth = 0;               // tdoa_params' optional K1 steps (both work on codes in memory)
    bool k1_gate = false;
};
// ... with the context's optional K1 steps filled in
FmBatchShape batch_shape(const tdoa_ctx *ctx)
{
    FmBatchShape b;
    b.k1_smooth = ctx->prm.k1_smooth;
    b.k1_gate = ctx->prm.k1_gate != 0;
    return b;
}

enum class ColPass { None, K1_256, K1_512, K1_TwoSweep, C256, TwoSweep, Short16x, Colx, Generic };
enum class RowPass { None, UnpackBlocks, UnpackInPlace, UnpackTiles, Hot, Generic };
enum class Inverse { None, Segments, Decimated, ShortLag, Full };
enum class PairStep { Tiles, Columns, Staged };        // the decimated inverse's pair step

// the LDS-staged column walk's launch (dec_staged.hpp)
struct StagedGeometry {
    bool folded = false, blocked = false;
    bool paired = false;             // blocked, as the paired lines of stg_paired_at: one contiguous KB per LDS-DMA
    bool nt = false;                 // the loader wave's LDS-DMA non-temporal (one pair group: a staged byte has one reader)
    bool merged = false;             // the walks of a 64-column block add the neighbour shares among themselves; X: block edges only
    int n_lw = 0, n_cw = 0, slots = 0, groups = 0, off = 0, rows = 0, nb = 0, n_items = 0;
    unsigned int blocks = 0;
    size_t lds = 0;
};

// Bytes of every workspace buffer a batch uses (0: not used)
struct FmBytes { size_t partials, stats, codes, codes_lp, k1_power, once_edges, once_tiles, once_fin, tz, v; };

// Every choice of a batch's kernels, made once by plan_fm_batch
struct FmRoute {
    int status = TDOA_OK;            // != TDOA_OK: the batch cannot run, `error` says why
    const char *error = nullptr;
    FftPlan pl{}, ps2{};             // the plan; the small plan of the decimated inverse
    int lag_lo = 0, lag_hi = 0;
    FmBatchShape b;
    long long code_stride = 0;
    bool row16 = false;              // hot-size kernels (fft_radix16.hpp), else the any-size ones of fft_stockham.hpp
    ColPass col = ColPass::None;
    int col_f = 0;                   // Short16x: N2 / 16, Colx: N2 / 256 (template argument)
    RowPass row = RowPass::None;
    Inverse inv = Inverse::None;
    PairStep step = PairStep::Tiles;
    bool fused_k1 = false, once = false, pruned = false, seg_quads = false, seg_pack3 = false, small_fused = false;
    bool k1_split = false;           // the fused column kernel looks angles up in the split half-plane table (160 KB of LDS)
    bool dec_tables = false;         // the decimated inverse applies: its filter and the staged tables are set up
    int fk = 0, np = 0, nn = 0, np2 = 0, nn2 = 0, seg_pq = 0, seg_chunks = 0;
    int shares = kSharesTiles;       // where the small plan's row pass finds the neighbours' shares (kShares*, fft_radix8.hpp)
    int xcd_pairs = 0, dec_gp = 0;   // pair-windows of a window on one XCD: k_inv_row_pair4096's 1-D grid, k_pair_decimate16's (0: plain)
    unsigned int xcd_grid = 0;
    dim3 dec_grid;
    StagedGeometry stg;
    FmBytes bytes{};
};

FmRoute plan_fm_batch(const Knobs &k, const StgTables &t, int n_cu, const FftPlan &pl, int lag_lo, int lag_hi, const FmBatchShape &b)
{
    FmRoute r;
    r.pl = pl;
    r.lag_lo = lag_lo;
    r.lag_hi = lag_hi;
    r.b = b;
    const int n_sw = b.n_sw, n_pw = b.n_pw, ppw = b.pairs_per_window, reach = lag_reach(lag_lo, lag_hi);
    r.code_stride = ((long long)b.maxlen + 15) / 8 * 8;      // rows stay 16-byte aligned
    r.row16 = pl.N1 == 4096 && !k.force_generic;
    pruned_outputs(pl, lag_lo, lag_hi, &r.np, &r.nn);
    // short-lag form: the inverse row kernel emits its shares of the few column sums that can hold a lag and V is
    // never written (needs lag_lo - 1 .. lag_hi + 1 inside [-512 fk, 512 fk - 1] for the refinement neighbours)
    if (r.row16 && k.short_lag) r.fk = reach <= 511 ? 1 : reach <= 1023 ? 2 : reach <= 2047 ? 4 : reach <= 4095 ? 8 : 0;
    r.pruned = !k.force_generic && pl.N1 >= 128 && pl.N2 <= 4096 && r.np + r.nn <= kPruneMax && r.np + r.nn <= pl.N2 &&
               lag_hi < pl.Nc && lag_lo > -pl.Nc;
    r.dec_tables = n_pw > 0 && decimation_applies(k, pl, lag_lo, lag_hi);
    // segment form (search ranges up to 1024 lags): overlap-save over 4096-point frames entirely in LDS; neither the
    // column pass nor TZ nor V rows are touched.  Lags lag_lo - 1 .. lag_hi + 1 must lie in [-P, P], P = 256 seg_pq.  Its
    // chunk sums and lag array live where the short-lag form keeps its shares (inside this pair-window's V row), which
    // bounds the chunk count by N2 / 2.
    {
        const int pq = reach <= 256 ? 1 : reach <= 512 ? 2 : reach <= 1024 ? 4 : 0;
        r.seg_pq = pq && r.row16 && k.short_lag && k.segment_form && n_pw > 0 && pl.N2 >= 8 ? pq : 0;
    }
    // quads (two station transforms per segment serve up to four pair-windows) when that is fewer transforms than one
    // per pair-window
    r.seg_quads = k.segment_quads && b.n_quads > 0 && 2 * b.n_quads < n_pw;
    if (r.seg_pq) {
        const int hop = 4096 - 512 * r.seg_pq;
        const int frames = (b.maxlen + hop - 1) / hop;
        const int trips = r.seg_quads ? frames : (frames + 1) / 2;        // the pair kernel takes two frames per trip
        const int units = r.seg_quads ? b.n_quads : n_pw;
        // chunks per unit: the grid runs in rounds of 2 workgroups per CU (64 KB LDS, 128 VGPRs x 512 threads); cost
        // model = rounds x (trips of the longest chunk + 1 for the prologue and the final inverse transform).  The model
        // is flat over a wide range (measured: 10 ... 36 chunks within 2 % on cfg2); among the near-ties take the most
        // chunks -- more, shorter workgroups balance better than one round of long ones (5 chunks: 4 % slower).
        const int c_max = std::max(1, std::min({trips / 8, pl.N2 / 2 - 1, (8192 + units - 1) / units}));
        const long long slots = 2ll * n_cu;
        auto cost = [&](int c) { return (double)(((long long)c * units + slots - 1) / slots) * ((trips + c - 1) / c + 1); };
        double best = cost(1);
        for (int c = 2; c <= c_max; c++) best = std::min(best, cost(c));
        for (int c = 1; c <= c_max; c++)
            if (cost(c) <= 1.03 * best) r.seg_chunks = c;
        if (k.seg_chunks_override > 0) r.seg_chunks = std::max(1, std::min({k.seg_chunks_override, trips, pl.N2 / 2 - 1}));
    }
    // its code rows at 3 bytes per code (round 4; the gate and the smoother work on int32 rows)
    r.seg_pack3 = r.seg_chunks > 0 && k.seg_pack3 && !b.k1_gate && b.k1_smooth <= 1;
    // K1 evaluated inside the forward column kernels (no code array): the plans with a k_fwd_col*_k1 kernel, unless a
    // consumer needs the codes in memory (segment form, k1_smooth, k1_gate) or a window may be shorter than two samples
    r.fused_k1 = b.allow_fused_k1 && k.fused_k1 && !k.force_generic && b.k1_smooth <= 1 && !b.k1_gate && pl.N1 == 4096 &&
                 (pl.N2 == 256 || pl.N2 == 512 || pl.N2 == 2048 || pl.N2 == 2560 || pl.N2 == 3072 || pl.N2 == 4096) && r.seg_pq == 0;
    // single-look K1 (k1_single_look.hpp): no statistics pre-pass.  Needs windows of one length, the peak picked by
    // k_small_col_peak or a pruned column kernel, and head / tail runs of K samples that do not meet.
    r.once = k.k1_once && r.fused_k1 && b.equal_len && !b.separate_stats && n_pw > 0 && !r.seg_chunks && r.fk == 0 && r.pruned &&
             reach < b.maxlen / 2 && reach + 1 <= kOncePiece * kOnceMaxPieces;
    // forward column pass (two sweeps -- 256-point sub-transforms + a G-point finish -- on the 4096 x 2048 and larger plans)
    const bool two_sweep = pl.N2 == 4096 || pl.N2 == 2048 || pl.N2 == 2560 || pl.N2 == 3072;
    if (r.seg_chunks) r.col = ColPass::None;
    else if (r.fused_k1) r.col = pl.N2 == 256 ? ColPass::K1_256 : pl.N2 == 512 ? ColPass::K1_512 : ColPass::K1_TwoSweep;
    else if (!r.row16) r.col = ColPass::Generic;
    else if (pl.N2 == 256) r.col = ColPass::C256;
    else if (two_sweep) r.col = ColPass::TwoSweep;
    else if (pl.N2 >= 16 && pl.N2 <= 128) { r.col = ColPass::Short16x; r.col_f = pl.N2 / 16; }      // k_fwd_col16x_c16<F>
    else if (pl.N2 == 512 || pl.N2 == 1024) { r.col = ColPass::Colx; r.col_f = pl.N2 / 256; }     // last radix of k_fwd_colx_c16
    else r.col = ColPass::Generic;
    // (the 4096 x 512 plan's kernel keeps the quadrant table unless asked: measured slower with the split one, knobs.hpp)
    r.k1_split = k.k1_split && (r.col == ColPass::K1_256 || r.col == ColPass::K1_TwoSweep || (r.col == ColPass::K1_512 && k.k1_split_512));
    // XCD-aware 1-D grid of the pair kernel when every window of the group carries the same `pairs_per_window` > S pairs
    // (window-major sharding with more pairs than stations): see k_inv_row_pair4096
    // ... or when a window's spectra are too large to wait in the Infinity Cache for their second reader (cfg3: 3 x 134 MB per
    // window, and the plain grid runs ALL rows of one pair-window before the next: 62 ms against 73-75 for its pair-row pass;
    // one workgroup running a group's pair-windows one after the other measured 67)
    const bool uniform = ppw > 0 && n_pw % ppw == 0 && n_sw > 0;
    if (r.row16 && k.xcd_rows && uniform && pl.N2 > 2) {
        const int stations = n_sw / (n_pw / ppw);
        if (ppw > stations || (ppw > 1 && (size_t)stations * (size_t)pl.Nc * sizeof(float2) > ((size_t)64 << 20))) {
            const long long groups = (long long)(n_pw / ppw) * (pl.N2 / 2 - 1);
            const long long blocks = (groups + 7) / 8 * 8 * ppw;
            if (blocks < (1ll << 31)) { r.xcd_pairs = ppw; r.xcd_grid = (unsigned int)blocks; }
        }
    }
    if (n_pw == 0) r.inv = Inverse::None;
    else if (r.seg_chunks) r.inv = Inverse::Segments;
    else if (r.pruned && r.fk == 0 && r.dec_tables) r.inv = Inverse::Decimated;
    else r.inv = r.fk ? Inverse::ShortLag : Inverse::Full;
    if (r.inv == Inverse::Decimated) {
        // Which form the pair step takes.  The column walk (dec_stream.hpp, dec_staged.hpp) is the only one on the 4096 x 2048
        // and larger plans.  On the others: with the stations' rows staged in LDS it is ahead from three stations on (cfg2, 3
        // pairs: 0.57 ms against 0.60 for the tile form; cfg4: 3.0 against 5.05; cfg5: 72 against 118); one pair-window per
        // wave from memory (batches the staged walk does not take) where windows carry more pairs than stations; the tile form
        // otherwise -- it asks for a tile's 32 KB at once and a lone pair waits for nothing else.
        const int S = b.stations_per_window;
        const int staged_s = uniform && S >= 2 && S <= kStgMaxStations && S * (S - 1) / 2 == ppw && n_sw == (n_pw / ppw) * S ? S : 0;
        bool walks = false;
        if (k.dec_cols && TDOA_HAVE_DEC_COLS)      // (TDOA_DEC_STEPS other than 8 / 12: the walk is not built)
            walks = cols_only_plan(pl) || k.dec_cols_always || (uniform && ((k.dec_staged && staged_s >= 3) || ppw > n_sw / (n_pw / ppw)));
        r.step = !walks ? PairStep::Tiles : k.dec_staged && staged_s ? PairStep::Staged : PairStep::Columns;
        if (r.step == PairStep::Staged) {
            // One loader wave, the other waves of at most sixteen walk one pair each; the share-out of the window's pairs comes
            // from build_stg_groups.  What the geometry is chosen for is the BARRIER: one per phase stops all sixteen waves, and
            // the pair step of BASELINE config 4 took 4.33 / 3.57 / 3.38 ms with 2 / 4 / 8 rows per phase (the ring's depth
            // made no difference: 3, 6 or 8 phases of two rows all 4.3 ms) -- so the most rows per phase of which TWO phases
            // fit the workgroup's share of the LDS: 8 rows up to eight station slots; small workgroups (three pairs: four
            // waves) leave room for their neighbours on the CU.
            StagedGeometry &g = r.stg;
            // spectra in blocks of 64 columns (out of place, where the tile form keeps its tiles: the plans that have that room;
            // the 4096 x 2048 and larger plans keep their rows in place).  A loader's piece of a row is then followed in memory
            // by its piece of the next row -- 4 KB runs per station and phase instead of 512-byte pieces 32 KB apart.
            g.blocked = k.stg_blocks && !cols_only_plan(pl);
            // ... as paired lines [cb][k2][fwd 64 | partner 64] (stg_paired_at): what the ring holds for a station and row is then
            // ONE KB of memory, a station's rows one ascending stream -- three 8 KB runs per phase of cfg2 instead of six of 4 KB
            g.paired = g.blocked && k.stg_paired && (pl.N2 == 256 || pl.N2 == 512);
            // the FOLDED form (dec_staged.hpp: no loader wave, up to sixteen walks, the last waves bring one station each): blocked
            // spectra, a two-phase ring -- where sixteen walks per workgroup make FEWER workgroups (16 stations: eight groups
            // instead of nine, cfg5 pair step 73.5 -> 70.2 ms; 8 stations: 16 + 12 walks measured 3.21 ms against 3.12 for
            // 14 + 14 next to a loader wave, and keep the loader).  Every group's stations need a wave to bring them: no more
            // station slots than walks (TDOA_DEC_STAGED_CW=2..6 on eight stations, or two stations, would break that).
            const StgTable &t16 = t.tab16[staged_s];
            g.folded = g.blocked && k.stg_folded && !k.stg_loaders && k.stg_bufs <= 2 && t16.slots <= 8 && t16.slots <= t16.max_n &&
                       (t16.count < t.tab[staged_s].count || k.stg_folded_always);
            const StgTable &tab = g.folded ? t16 : t.tab[staged_s];
            g.groups = tab.count;
            g.off = tab.off;
            g.n_cw = tab.max_n;
            g.slots = tab.slots;
            // One pair group per (window, column block): every staged byte is read once in the launch, and the loader wave asks
            // for it non-temporally.  Several groups keep the default policy -- the later ones find the rows in their XCD's L2,
            // which is what holds cfg4's traffic at its compulsory bytes.
            g.nt = g.paired && k.stg_nt && !g.folded && g.groups == 1;
            g.n_lw = g.folded ? 0 : std::max(1, std::min(k.stg_loaders ? k.stg_loaders : 1, std::min(4, g.slots)));
            // neighbour shares merged inside the walk (dec_staged.hpp, "merged shares"): the blocked plans.  The merging kernel
            // needs 177 - 191 VGPRs: two waves per SIMD, kStgMergeWaves = 8 per CU.  Merged only where TWO workgroups still share
            // the CU as they do unmerged -- at most four waves each: three walks and a loader, cfg2's three stations (measured:
            // DESIGN.md section 9).  A seven-wave workgroup (four stations) would fall from two per CU to one, twelve walks in
            // flight to six, on a kernel that waits for memory: not measured, not merged; larger groups do not fit at all.
            g.merged = k.stg_merge && g.blocked && (pl.N2 == 256 || pl.N2 == 512) && 2 * (g.n_cw + g.n_lw) <= kStgMergeWaves;
            // (few-station batches wait for memory rather than for the barrier: eight rows per phase there as well, and on the
            //  blocked plans a third phase in the ring where two workgroups still share a CU's LDS -- cfg2: 0.594 -> 0.571 ms;
            //  a fourth, or a third on the in-place plans, lost: cfg2 0.63, cfg3 17.8 against 16.3)
            const int wgs_by_waves = std::max(1, (g.merged ? kStgMergeWaves : kStgMaxWaves) / (g.n_cw + g.n_lw));      // workgroups a CU's wave slots hold
            const int budget = wgs_by_waves >= 2 ? 80 * 1024 : kStgLdsBytes;
            const int phase = g.slots * 1024;      // bytes of one row of every station
            g.rows = k.stg_rows ? k.stg_rows : 2 * 8 * phase <= kStgLdsBytes ? 8 : 2 * 4 * phase <= kStgLdsBytes ? 4 : 2;
            const int per_phase = g.n_lw ? g.rows * ((g.slots + g.n_lw - 1) / g.n_lw) : g.rows;
            if (g.rows * phase * 2 > kStgLdsBytes) {
                r.status = TDOA_ERR_INVALID;
                r.error = "TDOA_DEC_STAGED_ROWS: two phases do not fit the LDS ring";
            }
            g.nb = g.folded ? 2 : k.stg_bufs ? k.stg_bufs : g.blocked ? std::max(2, std::min(3, budget / (g.rows * phase))) : 2;
            g.nb = std::min(g.nb, kStgLdsBytes / (g.rows * phase));
            g.nb = std::max(2, std::min(g.nb, 2 + kStgMaxInFlight / per_phase));
            g.n_items = (n_pw / ppw) * 32;
            g.blocks = (unsigned int)((g.n_items + 7) / 8 * 8) * (unsigned int)g.groups;
            g.lds = (size_t)g.nb * g.rows * phase;
        }
        r.shares = r.step == PairStep::Tiles ? kSharesTiles : r.stg.merged ? kSharesBlockEdges : kSharesColumns;
        // pair-windows of a window that share station tiles on one XCD (k_pair_decimate16): when the batch is uniform and
        // a window's spectra are too many to come from on-die memory for their other readers (ctx->xcd_pair_mb: cfg5, 16
        // stations x 16.8 MB: its step 258 -> 237 ms in round 3; cfg4, 8 x 8.4 MB: -1.3 % since round 4; cfg2: plain grid)
        r.dec_grid = dim3(pl.N2 / 2, n_pw);
        if (k.xcd_rows && ppw > 1 && uniform &&
            (size_t)(n_sw / (n_pw / ppw)) * (size_t)pl.Nc * sizeof(float2) > ((size_t)k.xcd_pair_mb << 20)) {
            const long long groups = (long long)(n_pw / ppw) * (pl.N2 / 2);
            const long long blocks = (groups + 7) / 8 * 8 * ppw;
            if (blocks < (1ll << 31)) { r.dec_gp = ppw; r.dec_grid = dim3((unsigned int)blocks); }
        }
        // the R = Nc/16-point inverse on the small plan (rows, pruned column pass with the window divided out, K5)
        if (int rc = make_plan(2 * (pl.Nc / kDecD), true, &r.ps2)) {
            r.status = rc;
            r.error = "decimated plan";
        } else {
            pruned_outputs(r.ps2, lag_lo, lag_hi, &r.np2, &r.nn2);
        }
        // rows, column sums and K5 in one pass, V' never written (the reference's 20 000 lags on the 4096 x 16 / x 32 small
        // plans).  One workgroup per pair-window and CU at a time: for batches of a thousand pair-windows and more -- cfg5
        // (4500 per launch, 32 rows each) 25.2 -> 21.7 ms per step, cfg4 (2772, 16 rows) 1.26 -> 1.24; cfg2's 297 pair-windows
        // are one round and a tail of such workgroups (0.165 -> 0.253 ms) and keep the two kernels.
        // Not for a batch that refines: the refinement reads the peak's neighbours out of V' (launch_refine), which this
        // kernel never writes -- such a batch runs the two kernels, whose integer peaks carry the same bits.
        r.small_fused = k.small_fused && !b.fine && r.np2 == 3 && r.nn2 == 3 && r.ps2.odd == 1 && r.ps2.N1 == 4096 && r.ps2.N2 >= 8 &&
                        (n_pw >= 1024 || k.small_fused_always);
    }
    if (r.seg_chunks) r.row = RowPass::None;
    else if (!r.row16) r.row = RowPass::Generic;
    else if (r.inv != Inverse::Decimated) r.row = RowPass::Hot;
    else if (r.step == PairStep::Staged && r.stg.blocked) r.row = RowPass::UnpackBlocks;     // unpacked spectra in blocks of 64 columns
    else if (r.step != PairStep::Tiles) r.row = RowPass::UnpackInPlace;     // unpacked spectra back into their rows (the walk reads columns)
    else r.row = RowPass::UnpackTiles;     // unpacked spectra in COLS-column tiles behind G and V' in the V workspace
    FmBytes &by = r.bytes;
    by.partials = sizeof(StatsPartial) * (size_t)n_sw;
    by.stats = sizeof(FmStats) * (size_t)n_sw;
    if (!r.fused_k1) {
        by.codes = sizeof(int) * (size_t)r.code_stride * n_sw;
        if (b.k1_smooth > 1) by.codes_lp = by.codes;
    }
    if (b.k1_gate) by.k1_power = sizeof(unsigned long long) * (size_t)n_sw;
    if (r.once) {
        by.once_edges = sizeof(float) * 2 * (size_t)once_k1(lag_lo, lag_hi) * n_sw;
        by.once_tiles = sizeof(OnceTile) * (size_t)once_tiles_per_sw(pl) * n_sw;
        by.once_fin = sizeof(OnceFin) * (size_t)n_sw;
    }
    by.tz = sizeof(float2) * (size_t)pl.Zs * n_sw;
    if (n_pw) {
        size_t v_elems = (size_t)pl.Nc * n_pw;
        if (r.dec_tables)      // G + V' of the pairs, then the tiled spectra of the stations
            v_elems = std::max(v_elems, dec_spectra_offset(pl, n_pw) + (cols_only_plan(pl) ? 0 : (size_t)pl.Nc * n_sw));
        by.v = sizeof(float2) * v_elems;
    }
    return r;
}

// make every workspace buffer of a batch large enough (no allocation may happen while a stream capture is open)
int reserve_fm_batch(tdoa_ctx *ctx, const FmRoute &r)
{
    const FmBytes &by = r.bytes;
    const std::pair<DevBuf *, size_t> bufs[] = {{&ctx->partials, by.partials}, {&ctx->stats, by.stats}, {&ctx->codes, by.codes},
                                                {&ctx->codes_lp, by.codes_lp}, {&ctx->k1_power, by.k1_power},
                                                {&ctx->once_edges, by.once_edges}, {&ctx->once_tiles, by.once_tiles},
                                                {&ctx->once_fin, by.once_fin}, {&ctx->tz, by.tz}};
    int rc;
    for (const auto &x : bufs)
        if ((rc = ensure(ctx, *x.first, x.second))) return rc;
    if (r.dec_tables && (rc = ensure_decimation(ctx, r.pl, r.lag_lo, r.lag_hi))) return rc;
    if (r.dec_tables && (rc = ensure_stg_groups(ctx))) return rc;
    return ensure(ctx, ctx->v, by.v);
}

// second sweep of the two-sweep column pass: the G = N2 / 256 rows kb + 256 a of every column, in place
void launch_col_finish(hipStream_t st, float2 *tz, const FftPlan &pl, int n_sw)
{
    with_int<16, 10, 12, 8>(pl.N2 / 256, [&](auto g) {
        hipLaunchKernelGGL(k_fwd_col_finish<decltype(g)::value>, dim3(pl.N1 / 512, 256, n_sw), dim3(256), 0, st, tz, pl);
    });
}

// what the launchers of a batch read and write: the caller's descriptors and outputs, then (run_fm_batch) the workspace
struct FmBufs {
    const SWDesc *sw = nullptr;
    const SWDesc *sw_stats = nullptr;        // FmBatchShape::separate_stats: the windows K1 and its statistics run over
    const PWDesc *pw = nullptr;
    const QuadDesc *quads = nullptr;
    unsigned long long *keys = nullptr;
    float *lag_dump = nullptr;
    float dump_scale = 1.0f;
    double sum_len = 0.0;                    // samples of all station-windows (the profiling scopes' bytes)
    float *fine_raw = nullptr;               // FmBatchShape::fine: 3 raw neighbours per slot
    size_t dump_stride = 0;                  // lag_dump: floats between the lag arrays of consecutive pair-windows of the batch
    hipStream_t st = nullptr;
    FmStats *stats = nullptr;
    float2 *tz = nullptr, *v = nullptr;
    const int *codes = nullptr;              // K1's codes in memory (nullptr: fused into the column pass)
    OnceCorr oc{};                           // single-look path: what a K5 kernel needs to correct its candidates
};

// K1 -- capture bytes -> exact window statistics (fused: nothing else; the column pass evaluates the discriminator itself)
// and, materialised, the 24-bit phase codes -- or the single-look path's estimates and edge sums.  Returns the codes in
// memory (nullptr: none).
const int *launch_stats(tdoa_ctx *ctx, const FmRoute &r, const FmBufs &bf)
{
    const int n_sw = r.b.n_sw;
    if (r.once) {
        // 4096 samples per window -> the estimates (m0, s0) the column kernels normalise with; then the running sums of the
        // first and the last K samples of every window (streamed like k_fm_demod, 2 x (K + 1) samples per window)
        const int k_max = lag_reach(r.lag_lo, r.lag_hi), pieces = (k_max + 1 + kOncePiece - 1) / kOncePiece;
        const auto *table = ctx->k1_direct.as<const int>();
        ProfScope ps(ctx, TDOA_K_STATS, (2.0 * (2.0 * (k_max + 1) + (double)kOnceRuns * (kOnceRun + 1)) + 8.0 * (k_max + 1)) * n_sw);
        hipLaunchKernelGGL(k_once_estimate, dim3(n_sw), dim3(kOnceRuns), 0, bf.st, bf.sw, table, bf.stats);
        hipLaunchKernelGGL(k_once_edges, dim3(std::max(1, std::min(2 * n_sw, ctx->n_cu))), dim3(kDemodThreads), kK1DirectBytes, bf.st, bf.sw,
                           n_sw, table, bf.stats, ctx->once_edges.as<float>(), k_max, bf.oc.k1, pieces);
        return nullptr;
    }
    const int pieces = std::max(1, (r.b.maxlen + kDemodPiece - 1) / kDemodPiece);
    ProfScope ps(ctx, TDOA_K_STATS, (r.fused_k1 ? 2.0 : r.seg_pack3 ? 5.0 : 6.0) * bf.sum_len);
    return launch_k1(ctx, bf.st, bf.sw_stats ? bf.sw_stats : bf.sw, n_sw, r.b.maxlen, pieces, r.code_stride, !r.fused_k1, r.seg_pack3);
}

// forward column pass; on the single-look path then the tiles' exact sums -> the window statistics
void launch_fwd_cols(tdoa_ctx *ctx, const FmRoute &r, const FmBufs &bf)
{
    if (r.col == ColPass::None) return;
    const FftPlan &pl = r.pl;
    const int n_sw = r.b.n_sw;
    auto *tiles = r.once ? ctx->once_tiles.as<OnceTile>() : nullptr;
    const auto *qtable = r.k1_split ? ctx->k1_split.as<const int>() : ctx->k1_quad.as<const int>();
    const bool two_sweep = r.col == ColPass::K1_TwoSweep || r.col == ColPass::TwoSweep;
    const size_t lds16 = sizeof(float2) * 256 * 32;
    {
        // two-sweep column pass (N2 = 2048, 4096): 8 Nc written, read and written again -- SURVEY's third pass
        ProfScope ps(ctx, TDOA_K_FWD_COL, (r.fused_k1 ? 2.0 : 4.0) * bf.sum_len + (two_sweep ? 3.0 : 1.0) * (8.0 * (double)pl.Nc) * n_sw);
        switch (r.col) {
        case ColPass::K1_256:
        case ColPass::K1_TwoSweep:
            with_bool(two_sweep, [&](auto sub) { with_bool(r.once, [&](auto once) { with_bool(r.k1_split, [&](auto split) {
                hipLaunchKernelGGL((k_fwd_col256_k1<decltype(sub)::value, decltype(once)::value, decltype(split)::value>), dim3(ctx->n_cu),
                                   dim3(1024), decltype(split)::value ? kK1SplitLds : kColK1Lds, bf.st, bf.sw, qtable, bf.stats, bf.tz, pl,
                                   n_sw, tiles);
            }); }); });
            break;
        case ColPass::K1_512:
            with_bool(r.once, [&](auto once) { with_bool(r.k1_split, [&](auto split) {
                hipLaunchKernelGGL((k_fwd_col512_k1<decltype(once)::value, decltype(split)::value>), dim3(ctx->n_cu), dim3(1024),
                                   decltype(split)::value ? kK1SplitLds : kCol512Lds, bf.st, bf.sw, qtable, bf.stats, bf.tz, pl, n_sw, tiles);
            }); });
            break;
        case ColPass::C256:
            hipLaunchKernelGGL(k_fwd_col256_c16<false>, dim3(pl.N1 / 32, n_sw), dim3(512), lds16, bf.st, bf.sw, bf.codes, r.code_stride,
                               bf.stats, bf.tz, pl);
            break;
        case ColPass::TwoSweep:
            hipLaunchKernelGGL(k_fwd_col256_c16<true>, dim3(pl.N1 / 32, n_sw, pl.N2 / 256), dim3(512), lds16, bf.st, bf.sw, bf.codes,
                               r.code_stride, bf.stats, bf.tz, pl);
            break;
        case ColPass::Short16x:
            with_int<1, 2, 4, 8>(r.col_f, [&](auto f) {
                hipLaunchKernelGGL(k_fwd_col16x_c16<decltype(f)::value>, dim3(pl.N1 * decltype(f)::value / 256, n_sw), dim3(256), 0, bf.st,
                                   bf.sw, bf.codes, r.code_stride, bf.stats, bf.tz, pl);
            });
            break;
        case ColPass::Colx:
            with_int<2, 4>(r.col_f, [&](auto x) {
                hipLaunchKernelGGL(k_fwd_colx_c16<decltype(x)::value>, dim3(pl.N1 * decltype(x)::value / 32, n_sw), dim3(512), lds16, bf.st,
                                   bf.sw, bf.codes, r.code_stride, bf.stats, bf.tz, pl);
            });
            break;
        default:
            hipLaunchKernelGGL(k_fwd_col_c16, dim3(pl.N1 / pl.C, n_sw), dim3(256), sizeof(float2) * 2 * (size_t)pl.N2 * pl.C, bf.st,
                               bf.sw, bf.codes, r.code_stride, bf.stats, bf.tz, pl);
        }
        if (two_sweep) launch_col_finish(bf.st, bf.tz, pl, n_sw);
    }
    if (r.once) {
        ProfScope ps(ctx, TDOA_K_STATS, sizeof(OnceTile) * (double)once_tiles_per_sw(pl) * n_sw);
        hipLaunchKernelGGL(k_once_final, dim3(n_sw), dim3(256), 0, bf.st, bf.sw, tiles, once_tiles_per_sw(pl), bf.stats,
                           ctx->once_fin.as<OnceFin>(), n_sw);
    }
}

// forward row pass: the spectra in TZ, or unpacked where the decimated pair step reads them
void launch_fwd_rows(tdoa_ctx *ctx, const FmRoute &r, const FmBufs &bf)
{
    if (r.row == RowPass::None) return;
    const FftPlan &pl = r.pl;
    const int n_sw = r.b.n_sw;
    float2 *spectra = bf.v + dec_spectra_offset(pl, r.b.n_pw);
    const bool k1_cols = r.col == ColPass::K1_256 || r.col == ColPass::K1_512;
    const dim3 half(pl.N2 / 2, n_sw);
    const size_t lds = sizeof(float2) * 2 * kRowLds;
    ProfScope ps(ctx, TDOA_K_FWD_ROW, 2.0 * (8.0 * (double)pl.Nc) * n_sw);
    if (r.row == RowPass::UnpackBlocks)
        hipLaunchKernelGGL(k_fwd_row4096_unpack<false>, half, dim3(512), lds, bf.st, bf.tz, pl, spectra, k1_cols, kStgBlockCols, r.stg.paired);
    else if (r.row == RowPass::UnpackInPlace)
        hipLaunchKernelGGL(k_fwd_row4096_unpack<true>, half, dim3(512), lds, bf.st, bf.tz, pl, bf.tz, k1_cols, 0, false);
    else if (r.row == RowPass::UnpackTiles)
        hipLaunchKernelGGL(k_fwd_row4096_unpack<false>, half, dim3(512), lds, bf.st, bf.tz, pl, spectra, k1_cols, 0, false);
    else if (r.row == RowPass::Hot)
        hipLaunchKernelGGL(k_fwd_row4096, dim3(pl.N2, n_sw), dim3(256), 0, bf.st, bf.tz, pl, k1_cols);
    else
        hipLaunchKernelGGL(k_fwd_row, dim3(pl.N2, n_sw), dim3(256), sizeof(float2) * 2 * (size_t)pl.N1, bf.st, bf.tz, pl);
}

// segment form: the pair (or quad) kernel, the chunk reduction with the peak pick, the refinement's neighbours
void launch_segments(tdoa_ctx *ctx, const FmRoute &r, const FmBufs &bf)
{
    const FftPlan &pl = r.pl;
    const int n_pw = r.b.n_pw, n_quads = r.b.n_quads, chunks = r.seg_chunks, hop = 4096 - 512 * r.seg_pq;
    const double frames = (double)((r.b.maxlen + hop - 1) / hop), code_bytes = r.seg_pack3 ? 3.0 : 4.0;
    const float mul = (float)(4.0 * 2.0 * (double)pl.Nc / 4096.0);          // 4 N / M
    const size_t lds = sizeof(float2) * 2 * kRow8Lds;
    with_int<1, 2, 4>(r.seg_pq, [&](auto pq) {
        constexpr int PQ = decltype(pq)::value;
        with_bool(r.seg_pack3, [&](auto pack) {
            constexpr bool PACK = decltype(pack)::value;
            if (r.seg_quads) {
                ProfScope ps(ctx, TDOA_K_INV_ROW, 4.0 * code_bytes * 4096.0 * frames * n_quads);      // four frames of codes
                hipLaunchKernelGGL((k_xcorr_segments_quad<PQ, PACK>), dim3(chunks, n_quads), dim3(512), lds, bf.st, bf.sw, bf.quads,
                                   bf.codes, r.code_stride, bf.stats, bf.v, pl, chunks);
            } else {
                ProfScope ps(ctx, TDOA_K_INV_ROW, 2.0 * code_bytes * 4096.0 * frames * n_pw);         // two frames of codes
                hipLaunchKernelGGL((k_xcorr_segments<PQ, PACK>), dim3(chunks, n_pw), dim3(512), lds, bf.st, bf.sw, bf.pw, bf.codes,
                                   r.code_stride, bf.stats, bf.v, pl, chunks);
            }
        });
        {
            ProfScope ps(ctx, TDOA_K_INV_COL, 4.0 * 512.0 * PQ * (chunks + 1) * n_pw);
            hipLaunchKernelGGL(k_segments_reduce<PQ>, dim3(2 * PQ + 1, n_pw), dim3(256), 0, bf.st, bf.v, bf.keys, bf.pw,
                               bf.sw_stats ? bf.sw_stats : bf.sw, bf.stats, pl,
                               chunks, mul, r.lag_lo, r.lag_hi, bf.lag_dump, bf.dump_scale, bf.dump_stride);
        }
        if (r.b.fine) {
            ctx->prof_last = -1;          // unscoped launch: the next scope records its own start
            hipLaunchKernelGGL(k_refine_segments<PQ>, dim3((n_pw + 63) / 64), dim3(64), 0, bf.st, bf.v, bf.keys, bf.pw, pl, n_pw, bf.fine_raw);
        }
    });
}

// the neighbour shares between the pair step and the small plan, one way: E [N2][2 C] per pair-window (tiles), X [2 C][4096]
// (column walks), or X's slots of the two edge columns of every 64-column block (merged staged walk: 2 C - 1 values per edge)
double dec_share_bytes(const FmRoute &r)
{
    const double per_pw = r.shares == kSharesTiles ? (double)r.pl.N2 * (2 * kDecEdge) : r.shares == kSharesColumns ? 4096.0 * (2 * kDecEdge)
                                                                                       : (4096.0 / kStgBlockCols) * (2 * kDecEdge - 1);
    return 8.0 * per_pw * r.b.n_pw;
}

// decimated inverse, pair step: K3 + FIR decimation of the pair's spectrum (one read of the two station spectra) into G
void launch_pair_step(tdoa_ctx *ctx, const FmRoute &r, const FmBufs &bf)
{
    const FftPlan &pl = r.pl;
    const int n_pw = r.b.n_pw;
    float2 *g = bf.v, *edges = bf.v + dec_edge_offset(pl, n_pw), *spectra = bf.v + dec_spectra_offset(pl, n_pw);
    const auto *taps = ctx->dec_taps.as<const float>();
    ProfScope ps(ctx, TDOA_K_INV_ROW, 2.0 * (8.0 * (double)pl.Nc) * n_pw + 8.0 * (double)(pl.Nc / kDecD) * n_pw + dec_share_bytes(r));      // two spectra read, G and the shares written
#if TDOA_HAVE_DEC_COLS
    if (r.step == PairStep::Staged) {
        const StagedGeometry &sg = r.stg;
        const StgGroup *gt = ctx->stg_groups.as<const StgGroup>() + sg.off;
        with_int<256, 512, 2048, 2560, 3072, 4096>(pl.N2, [&](auto n2) { with_int<8, 4, 2>(sg.rows, [&](auto rows) {
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(sg.blocks), dim3(64 * (sg.n_cw + sg.n_lw)), sg.lds, bf.st, bf.pw, sg.blocked ? spectra : bf.tz, g,
                                   edges, pl, taps, gt, sg.n_items, r.b.pairs_per_window, sg.slots, sg.n_cw, sg.groups, sg.nb,
                                   sg.blocked ? (long long)pl.Nc : (long long)pl.Zs,
                                   (sg.blocked ? kStgLayoutBlocked : 0) | (sg.paired ? kStgLayoutPaired : 0) | (sg.nt ? kStgLayoutNt : 0));
            };
            constexpr int N2 = decltype(n2)::value, R = decltype(rows)::value;
            if constexpr (N2 == 256 || N2 == 512) {
                if (sg.merged) return launch(k_pair_decimate_staged<N2, R, true>);
            }
            launch(k_pair_decimate_staged<N2, R>);
        }); });
        return;
    }
    if (r.step == PairStep::Columns) {
        const dim3 grid(32, (unsigned int)((n_pw + kDecWavesPerWg - 1) / kDecWavesPerWg)), block(64 * kDecWavesPerWg);
        with_int<256, 512, 2048, 2560, 3072, 4096>(pl.N2, [&](auto n2) {
            hipLaunchKernelGGL(k_pair_decimate_cols<decltype(n2)::value>, grid, block, 0, bf.st, bf.pw, bf.tz, g, edges, pl, taps, n_pw);
        });
        return;
    }
#endif
    // W_N^DK, DK = N2 / 8 bins between a thread's consecutive elements of a tile (N = 2 Nc)
    const double ang = -2.0 * M_PI * (double)(pl.N2 / 8) / (2.0 * (double)pl.Nc);
    const float2 rot = make_float2((float)std::cos(ang), (float)std::sin(ang));
    with_int<8, 9>(pl.N2 == 256 ? 8 : 9, [&](auto lg) {
        hipLaunchKernelGGL(k_pair_decimate16<decltype(lg)::value>, r.dec_grid, dim3(512), sizeof(float2) * 2 * 16 * kDecPitch, bf.st, bf.pw,
                           spectra, g, edges, pl, taps, r.ps2.N2, r.dec_gp, n_pw, rot);
    });
}

// decimated inverse, small plan: the R = Nc/16-point inverse of G (rows, pruned column pass with the window divided out, K5)
void launch_small_plan(tdoa_ctx *ctx, const FmRoute &r, const FmBufs &bf)
{
    const FftPlan &pl = r.pl, &ps2 = r.ps2;
    const int n_pw = r.b.n_pw, by_col = r.shares;
    const size_t rc_pts = (size_t)(pl.Nc / kDecD);
    float2 *g = bf.v, *vs = bf.v + rc_pts * (size_t)n_pw, *edges = bf.v + dec_edge_offset(pl, n_pw);      // G, V': [n_pw][R] each
    const auto *gain = ctx->dec_gain.as<const float>();
    const size_t lds = sizeof(float2) * 2 * kRow8Lds;
    ProfScope ps(ctx, TDOA_K_INV_COL, 3.0 * 8.0 * (double)rc_pts * n_pw + dec_share_bytes(r));
    if (r.small_fused) {
        hipLaunchKernelGGL(k_small_rows_col_peak, dim3(n_pw), dim3(512), lds, bf.st, g, edges, bf.keys, bf.pw, ps2, pl.N2, by_col, r.lag_lo,
                           r.lag_hi, bf.lag_dump, bf.dump_scale, bf.dump_stride, gain, bf.oc);
        return;
    }
    hipLaunchKernelGGL(k_inv_rows_plain_r8, dim3(ps2.N2 / 2, n_pw), dim3(512), lds, bf.st, g, edges, vs, ps2, pl.N2, by_col);
    with_int<3, 0>(r.np2 == 3 && r.nn2 == 3 ? 3 : 0, [&](auto n) {      // 3: the reference's 20 000 lags on either small plan
        hipLaunchKernelGGL((k_small_col_peak<decltype(n)::value, decltype(n)::value>), dim3(ps2.N1 / 256, n_pw), dim3(256), 0, bf.st, vs,
                           bf.keys, bf.pw, ps2, r.lag_lo, r.lag_hi, r.np2, r.nn2, bf.lag_dump, bf.dump_scale, bf.dump_stride, gain, bf.oc);
    });
}

// full or short-lag inverse: pair rows (K3 + inverse rows), then the column pass with the peak pick
void launch_inverse(tdoa_ctx *ctx, const FmRoute &r, const FmBufs &bf)
{
    const FftPlan &pl = r.pl;
    const int n_pw = r.b.n_pw;
    const double nc8 = 8.0 * (double)pl.Nc;
    {
        ProfScope ps(ctx, TDOA_K_INV_ROW, 3.0 * nc8 * n_pw);     // SURVEY's model: two spectra read, V written, per pair
        if (r.row16) {
            const size_t lds = sizeof(float2) * 2 * kRowLds;
            with_int<0, 1, 2, 4, 8>(r.fk, [&](auto fk) {
                constexpr int FK = decltype(fk)::value;
                if (pl.N2 > 2)
                    hipLaunchKernelGGL((k_inv_row_pair4096<false, FK>), r.xcd_pairs ? dim3(r.xcd_grid) : dim3(pl.N2 / 2 - 1, n_pw), dim3(256),
                                       lds, bf.st, bf.pw, bf.tz, bf.v, pl, r.xcd_pairs, n_pw);
                hipLaunchKernelGGL((k_inv_row_pair4096<true, FK>), dim3(1, n_pw), dim3(256), lds, bf.st, bf.pw, bf.tz, bf.v, pl, 0, n_pw);
            });
        } else {
            hipLaunchKernelGGL(k_inv_row_pair, dim3(pl.N2 / 2, n_pw), dim3(256), sizeof(float2) * 4 * (size_t)pl.N1, bf.st, bf.pw, bf.tz, bf.v, pl);
        }
    }
    ProfScope ps(ctx, TDOA_K_INV_COL, r.fk ? 8.0 * 256 * r.fk * pl.N2 * n_pw : nc8 * n_pw);
    const dim3 grid(pl.N1 / 128, n_pw);
    const size_t lds_wtab = sizeof(float2) * (size_t)pl.N2;
    const bool fixed = (pl.N2 & 31) == 0;     // the compile-time forms of the pruned kernel read 32 rows per trip unguarded
    if (r.fk)
        with_int<1, 2, 4, 8>(r.fk, [&](auto fk) {
            hipLaunchKernelGGL(k_fused_reduce<decltype(fk)::value>, dim3(2 * decltype(fk)::value, n_pw), dim3(256), 0, bf.st, bf.v, bf.keys,
                               bf.pw, pl, r.lag_lo, r.lag_hi, bf.lag_dump, bf.dump_scale, bf.dump_stride);
        });
    else if (r.pruned && fixed && r.np == r.nn && r.np >= 1 && r.np <= 4)
        with_int<3, 1, 2, 4>(r.np, [&](auto n) {
            hipLaunchKernelGGL((k_inv_col_pruned<decltype(n)::value, decltype(n)::value>), grid, dim3(256), lds_wtab, bf.st, bf.v, bf.keys,
                               bf.pw, pl, r.lag_lo, r.lag_hi, bf.lag_dump, bf.dump_scale, bf.dump_stride, bf.oc);
        });
    else if (r.pruned)
        hipLaunchKernelGGL(k_inv_col_pruned_any, grid, dim3(256), lds_wtab, bf.st, bf.v, bf.keys, bf.pw, pl, r.lag_lo, r.lag_hi, r.np, r.nn,
                           bf.lag_dump, bf.dump_scale, bf.dump_stride, bf.oc);
    else
        hipLaunchKernelGGL(k_inv_col_peak, dim3(pl.N1 / pl.C, n_pw), dim3(256), sizeof(float2) * 2 * (size_t)pl.N2 * pl.C, bf.st, bf.v,
                           bf.keys, bf.pw, pl, r.lag_lo, r.lag_hi, bf.lag_dump, bf.dump_scale, bf.dump_stride);
}

// refinement: V (the short-lag array; the small plan's row-pass output behind G) of this batch is still in place -- the
// peak's neighbours for the parabola (the segment form's: launch_segments)
void launch_refine(tdoa_ctx *ctx, const FmRoute &r, const FmBufs &bf)
{
    const int n_pw = r.b.n_pw;
    ctx->prof_last = -1;      // unscoped launches: the next scope records its own start
    if (r.inv == Inverse::ShortLag)
        with_int<1, 2, 4, 8>(r.fk, [&](auto fk) {
            hipLaunchKernelGGL(k_refine_fused<decltype(fk)::value>, dim3((n_pw + 63) / 64), dim3(64), 0, bf.st, bf.v, bf.keys, bf.pw, r.pl,
                               n_pw, bf.fine_raw);
        });
    else if (r.inv == Inverse::Decimated)      // window divided out per lag
        hipLaunchKernelGGL(k_refine_peaks, dim3(n_pw), dim3(64), 0, bf.st, bf.v + (size_t)(r.pl.Nc / kDecD) * (size_t)n_pw, bf.keys, bf.pw,
                           r.ps2, bf.fine_raw, ctx->dec_gain.as<const float>(), bf.oc);
    else if (r.inv == Inverse::Full)
        hipLaunchKernelGGL(k_refine_peaks, dim3(n_pw), dim3(64), 0, bf.st, bf.v, bf.keys, bf.pw, r.pl, bf.fine_raw,
                           static_cast<const float *>(nullptr), bf.oc);
}

// a route as tdoa_debug_last_route reports it (include/tdoa_mi355x.h TDOA_ROUTE_*, numbered as the enums here)
static_assert((int)Inverse::Full == TDOA_INV_FULL && (int)Inverse::Decimated == TDOA_INV_DECIMATED, "TDOA_INV_*");
static_assert((int)PairStep::Staged == TDOA_STEP_STAGED && (int)ColPass::Generic == TDOA_COL_GENERIC &&
              (int)RowPass::Generic == TDOA_ROW_GENERIC && (int)RowPass::UnpackTiles == TDOA_ROW_UNPACK_TILES, "TDOA_STEP/COL/ROW_*");
void route_info(const FmRoute &r, int32_t out[16])
{
    const int32_t v[16] = {(int32_t)r.inv, (int32_t)r.step, (int32_t)r.col, (int32_t)r.row, r.fk, r.seg_pq, r.seg_quads, r.seg_pack3,
                           r.fused_k1, r.once, r.small_fused, r.pruned, r.xcd_pairs > 0, r.dec_gp > 0, r.stg.folded,
                           (r.stg.blocked ? TDOA_ROUTE_STG_BLOCKED_BIT : 0) | (r.stg.merged ? TDOA_ROUTE_STG_MERGED_BIT : 0) |
                               (r.k1_split ? TDOA_ROUTE_K1_SPLIT_BIT : 0) | (r.stg.paired ? TDOA_ROUTE_STG_PAIRED_BIT : 0) |
                               (r.stg.nt ? TDOA_ROUTE_STG_NT_BIT : 0)};
    std::memcpy(out, v, sizeof(v));
}

// ---- mode B core: K1 + forward transforms + inverse + peak pick over descriptors already in device memory
int run_fm_batch(tdoa_ctx *ctx, const FmBatchShape &shape, const FftPlan &pl, int lag_lo, int lag_hi, FmBufs bf)
{
    const FmRoute r = plan_fm_batch(ctx->knobs, ctx->stg, ctx->n_cu, pl, lag_lo, lag_hi, shape);
    if (r.error) return fail(ctx, r.status, r.error);
    int rc;
    if ((rc = reserve_fm_batch(ctx, r))) return rc;
    ctx->once_active = r.once;
    route_info(r, ctx->route);
    ctx->route_set = true;
    bf.st = ctx->stream;
    bf.stats = ctx->stats.as<FmStats>();
    bf.tz = ctx->tz.as<float2>();
    bf.v = ctx->v.as<float2>();
    if (r.once)
        bf.oc = OnceCorr{ctx->once_edges.as<const float>(), ctx->once_fin.as<const OnceFin>(),
                         ctx->slot_gain.as<double>(), once_k1(lag_lo, lag_hi), lag_reach(lag_lo, lag_hi),
                         (float)(8.0 * (double)pl.Nc)};          // raw = 4 N sum w w, N = 2 Nc
    bf.codes = launch_stats(ctx, r, bf);
    launch_fwd_cols(ctx, r, bf);
    launch_fwd_rows(ctx, r, bf);
    if (r.inv == Inverse::Segments) {
        launch_segments(ctx, r, bf);
    } else if (r.inv == Inverse::Decimated) {
        launch_pair_step(ctx, r, bf);
        launch_small_plan(ctx, r, bf);
    } else if (r.inv != Inverse::None) {
        launch_inverse(ctx, r, bf);
    }
    if (r.inv != Inverse::None && r.b.fine) launch_refine(ctx, r, bf);
    HIPCHK(ctx, hipGetLastError());
    return TDOA_OK;
}

// The decode epilogue of a step and of a pair call: the n_slots keys the batches left -> peak records in ctx->peaks and,
// with fine_raw (the refinement's neighbours), tdoa_fine_peak records in ctx->fine.  On the single-look path
// (ctx->once_active, set by run_fm_batch or the replayed graph) both multiply by the pair-window's slot_gain.
void launch_decode(tdoa_ctx *ctx, const unsigned long long *keys, const double *scales, size_t n_slots, const float *fine_raw, double gate)
{
    const double *slot_gain = ctx->once_active ? ctx->slot_gain.as<const double>() : nullptr;
    const dim3 grid((unsigned)((n_slots + 255) / 256));
    if (fine_raw) {
        ctx->prof_last = -1;             // unscoped launch: the next scope records its own start
        hipLaunchKernelGGL(k_decode_fine, grid, dim3(256), 0, ctx->stream, keys, scales, fine_raw, ctx->fine.as<FineOut>(), gate,
                           (int)n_slots, slot_gain);
    }
    ProfScope ps(ctx, TDOA_K_PEAK, 32.0 * (double)n_slots);
    hipLaunchKernelGGL(k_decode_peaks, grid, dim3(256), 0, ctx->stream, keys, scales, ctx->peaks.as<PeakOut>(), (int)n_slots, slot_gain);
}
// raise the dynamic-LDS limit of every kernel that needs more than the default once per context
int allow_big_lds(tdoa_ctx *ctx)
{
    int rc;
    const size_t all = 136 * 1024;   // largest dynamic request: 128 KiB (kLdsCap tiles, generic row pair); static LDS comes on top
    if ((rc = set_lds(ctx, k_once_edges, all))) return rc;
    if ((rc = set_lds(ctx, k_fm_demod<true>, all))) return rc;
    if ((rc = set_lds(ctx, k_fm_demod<false>, all))) return rc;
    if ((rc = set_lds(ctx, k_fwd_col512_k1<false>, all))) return rc;
    if ((rc = set_lds(ctx, k_fwd_col512_k1<true>, all))) return rc;
    if ((rc = set_lds(ctx, k_fwd_row4096_unpack<false>, all))) return rc;
    if ((rc = set_lds(ctx, k_fwd_row4096_unpack<true>, all))) return rc;
    if ((rc = set_lds(ctx, (k_fwd_col256_k1<false, false>), all))) return rc;
    if ((rc = set_lds(ctx, (k_fwd_col256_k1<true, false>), all))) return rc;
    if ((rc = set_lds(ctx, (k_fwd_col256_k1<false, true>), all))) return rc;
    if ((rc = set_lds(ctx, (k_fwd_col256_k1<true, true>), all))) return rc;
    if ((rc = set_lds(ctx, k_fwd_col_c16, all))) return rc;
    {   // the split-table forms of the fused column kernels take the CU's whole LDS.  A device that refuses the size runs the
        // quadrant forms above instead (tdoa_create clears Knobs::k1_split): not an error.
        hipError_t e = hipSuccess;
        auto ask = [&](auto kernel) {
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kK1SplitLds);
        };
        for_ints<0, 1>([&](auto once) {
            ask(k_fwd_col512_k1<(bool)decltype(once)::value, true>);
            ask(k_fwd_col256_k1<false, (bool)decltype(once)::value, true>);
            ask(k_fwd_col256_k1<true, (bool)decltype(once)::value, true>);
        });
        if (e != hipSuccess) (void)hipGetLastError();
        ctx->k1_split_lds = e == hipSuccess;
    }
    if ((rc = set_lds(ctx, k_fwd_row, all))) return rc;
    if ((rc = set_lds(ctx, k_inv_row_pair, all))) return rc;
    if ((rc = set_lds(ctx, k_inv_col_peak, all))) return rc;
    if ((rc = set_lds(ctx, k_fwd_col256_c16<false>, all))) return rc;
    if ((rc = set_lds(ctx, k_fwd_col256_c16<true>, all))) return rc;
    if ((rc = set_lds(ctx, k_fwd_colx_c16<2>, all))) return rc;
    if ((rc = set_lds(ctx, k_fwd_colx_c16<4>, all))) return rc;
    if ((rc = set_lds(ctx, (k_fm_demod<true, true>), all))) return rc;
    if ((rc = set_lds(ctx, k_pair_decimate16<8>, all))) return rc;
    if ((rc = set_lds(ctx, k_pair_decimate16<9>, all))) return rc;
    if ((rc = set_lds(ctx, k_inv_rows_plain_r8, all))) return rc;
    if ((rc = set_lds(ctx, k_small_rows_col_peak, all))) return rc;
    for_ints<0, 1, 2, 4, 8>([&](auto fk) {
        if (!rc) rc = set_lds(ctx, k_inv_row_pair4096<false, decltype(fk)::value>, all);
        if (!rc) rc = set_lds(ctx, k_inv_row_pair4096<true, decltype(fk)::value>, all);
    });
    for_ints<1, 2, 4>([&](auto pq) {
        for_ints<0, 1>([&](auto pack) {
            if (!rc) rc = set_lds(ctx, k_xcorr_segments<decltype(pq)::value, (bool)decltype(pack)::value>, all);
            if (!rc) rc = set_lds(ctx, k_xcorr_segments_quad<decltype(pq)::value, (bool)decltype(pack)::value>, all);
        });
    });
#if TDOA_HAVE_DEC_COLS
    for_ints<256, 512, 2048, 2560, 3072, 4096>([&](auto n2) {
        for_ints<2, 4, 8>([&](auto rv) {
            if (!rc) rc = set_lds(ctx, k_pair_decimate_staged<decltype(n2)::value, decltype(rv)::value>, all);
            if constexpr (decltype(n2)::value == 256 || decltype(n2)::value == 512)
                if (!rc) rc = set_lds(ctx, (k_pair_decimate_staged<decltype(n2)::value, decltype(rv)::value, true>), all);
        });
    });
#endif
    return rc;
}

}  // namespace
