// fm_setup.inc -- what the host prepares for a mode-B batch's kernels: the K1 angle tables, the decimated inverse's filter,
// the single-look path's sizes and the staged walk's share-out of a window's pairs.
// Included by tdoa_mi355x.hip after tdoa_ctx and ensure().

namespace {

// The K1 angle table (k1_discriminator.hpp): first-octant directions (mn, mx), index mx (mx + 1) / 2 + mn over the
// indices of the odd magnitudes 2 idx + 1; entry = llround(atan2(mn', mx') 2^23 / pi) of the gcd-reduced pair, float64.
// (oracle/tdoa_oracle.c: ob_octant_code states the same expression; tests compare the device's codes with it bit for bit)
// `split` (optional): the direct table in three bytes per angle, as the fused column kernels keep it in LDS -- lo[i] =
// direct[i] & 0xff (32768 uint8), then hi[i] = direct[i] >> 8 (32768 uint16, < 2^15), same index: kK1SplitBytes
void k1_build_table_host(std::vector<int32_t> &tab, std::vector<int32_t> &direct, std::vector<int32_t> &quad,
                         std::vector<uint8_t> *split = nullptr)
{
    tab.resize(kK1TableEntries);
    for (int mx = 0; mx < 128; mx++)
        for (int mn = 0; mn <= mx; mn++) {
            int a = 2 * mx + 1, b = 2 * mn + 1;
            int g = a, h = b;
            while (h) { const int t = g % h; g = h; h = t; }
            a /= g;
            b /= g;
            tab[(size_t)mx * (mx + 1) / 2 + mn] = (int32_t)std::llround(std::atan2((double)b, (double)a) * (8388608.0 / M_PI));
        }
    // the direct half-plane table of the streaming kernel: D[b_I | (b_Q & 0x7f) << 8] = a(I, Q) for b_Q >= 128 (Q > 0),
    // placed from the first-octant codes by the integer rules of k1_discriminator.hpp
    direct.resize(kK1DirectEntries);
    for (int bq = 128; bq < 256; bq++)
        for (int bi = 0; bi < 256; bi++) {
            const int ia = bi >= 128 ? bi - 128 : 127 - bi, iq = bq - 128;
            const int mx = std::max(ia, iq), mn = std::min(ia, iq);
            int c = tab[(size_t)mx * (mx + 1) / 2 + mn];
            if (iq > ia) c = (kK1Half >> 1) - c;
            if (bi < 128) c = kK1Half - c;
            direct[(size_t)bi | ((size_t)(bq & 0x7f) << 8)] = c;
        }
    // the first-quadrant table Q[iq][ia] = a(2 ia + 1, 2 iq + 1): the |Q| > |I| reflection done here instead of per sample
    quad.resize(kK1QuadrantEntries);
    for (int iq = 0; iq < 128; iq++)
        for (int ia = 0; ia < 128; ia++) {
            const int mx = std::max(ia, iq), mn = std::min(ia, iq);
            const int c = tab[(size_t)mx * (mx + 1) / 2 + mn];
            quad[(size_t)iq * 128 + ia] = (iq > ia ? (kK1Half >> 1) - c : c) * 256;      // scaled: a full turn = 2^32
        }
    if (split) {
        split->resize(kK1SplitBytes);
        uint8_t *lo = split->data();
        uint16_t *hi = reinterpret_cast<uint16_t *>(split->data() + kK1DirectEntries);
        for (int i = 0; i < kK1DirectEntries; i++) {
            lo[i] = (uint8_t)(direct[i] & 0xff);
            hi[i] = (uint16_t)(direct[i] >> 8);
        }
    }
}

// ---- decimated inverse (fft_radix8.hpp, k_pair_decimate16) ----------------------------------------------------------
// applies to the general form on 4096 x 256 plans when the packed search range M = reach/2 + 2 leaves a transition band:
// R = Nc/16 = 65536, pass band |m| <= M, stop band |m| >= R - M
// Filter design: Kaiser-windowed sinc with T taps a side, T = what 140 dB needs on the transition band, at most kDecTmax
// (fft_radix8.hpp: 95 with 12 steps per phase); the attenuation is then what T buys there, A = 8 + 2.285 dw 2T, and the
// form applies from 120 dB on (cfg2 / cfg4: 126 dB, T = 95; cfg5: 140 dB, T = 87).  Alias leakage measured in float64 on
// noise-level simulator.go peaks: ~4 x 10^(-A/20) of the peak (7e-7 at 126 dB; scripts/dec_filter_sweep.py).
constexpr double kDecAttenuationDb = 140.0, kDecMinAttenuationDb = 120.0;
struct DecDesign { bool ok; int T; double att; };
DecDesign decimation_design(const FftPlan &pl, int reach)
{
    const long long M = reach / 2 + 2, R = pl.Nc / kDecD;
    if (R - 2 * M <= 0) return {false, 0, 0.0};
    const double dw = 2.0 * M_PI * (double)(R - 2 * M) / (double)pl.Nc;
    int T = (int)std::ceil((kDecAttenuationDb - 8.0) / (2.285 * dw) / 2.0);
    double att = kDecAttenuationDb;
    if (T > kDecTmax) {
        T = kDecTmax;
        att = 8.0 + 2.285 * dw * 2.0 * T;
    }
    return {att >= kDecMinAttenuationDb, T, att};
}

// two-sweep plans with a decimated inverse: a 4096-bin tile of their spectrum is (less than) one column, so only the column
// walk (dec_stream.hpp) serves them, and the row pass leaves the unpacked spectra in TZ
// (N2 = 2048 -- windows of 4 to 8 s at 2 Msps, N = 2^24 -- joined in round 5: until then that plan ran the full inverse)
bool cols_only_plan(const FftPlan &pl) { return pl.N1 == 4096 && (pl.N2 == 4096 || pl.N2 == 3072 || pl.N2 == 2560 || pl.N2 == 2048); }

// largest |lag| an inverse looks at: the searched lags and their refinement neighbours
int lag_reach(int lag_lo, int lag_hi) { return std::max(lag_hi + 1, -(lag_lo - 1)); }

// column outputs of a pruned inverse that can hold a searched lag: np at the start of the column, nn at its end
void pruned_outputs(const FftPlan &pl, int lag_lo, int lag_hi, int *np, int *nn)
{
    const long long n_real = 2 * pl.Nc;
    *np = lag_hi >= 0 ? (int)((lag_hi / 2) / pl.N1) + 1 : 0;
    *nn = lag_lo < 0 ? pl.N2 - (int)(((n_real + lag_lo) / 2) / pl.N1) : 0;
}

bool decimation_applies(const Knobs &k, const FftPlan &pl, int lag_lo, int lag_hi)
{
    if (!k.decimate || k.force_generic || pl.N1 != 4096 || (pl.N2 != 256 && pl.N2 != 512 && !cols_only_plan(pl))) return false;
    if (cols_only_plan(pl) && !(k.dec_cols && TDOA_HAVE_DEC_COLS)) return false;
    {   // the small plan's K5 kernel evaluates the column outputs that can hold a searched lag as direct sums: at most kPruneMax
        // of them (FmRoute::pruned; 4096 packed lags per output: search ranges up to ~32 000 lags).  choose_fft_size
        // relies on this function alone -- a 5 x 2^k plan has no other inverse to fall back to.
        int np, nn;
        pruned_outputs(pl, lag_lo, lag_hi, &np, &nn);
        if (np + nn > kPruneMax || lag_hi >= pl.Nc || lag_lo <= -pl.Nc) return false;
    }
    const int reach = lag_reach(lag_lo, lag_hi);
    if (reach <= 4095) return false;                       // the short-lag forms take those
    return decimation_design(pl, reach).ok;
}

// modified Bessel function I0 (Kaiser window)
double bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 200; k++) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// layout of the decimated inverse inside the V workspace (float2 elements): G [n_pw][R], V' [n_pw][R], the tiles' edge
// shares E [n_pw][N2][2 kDecEdge], then the stations' spectra in tiles [n_sw][Nc]
size_t dec_edge_offset(const FftPlan &pl, int n_pw) { return 2 * (size_t)(pl.Nc / kDecD) * (size_t)n_pw; }
// (E: [n_pw][N2][12] for the tile kernel, X: [n_pw][12][4096] for the column walk -- room for the larger)
size_t dec_spectra_offset(const FftPlan &pl, int n_pw)
{
    return dec_edge_offset(pl, n_pw) + (size_t)n_pw * (size_t)std::max(pl.N2, 4096) * (2 * kDecEdge);
}

// taps h[t] = sinc(t/16) * kaiser(t), |t| <= T, rounded to f32; gain[m] = 1 / w[m], w[m] = sum_t h[t] cos(2 pi t m / Nc) / 16
// evaluated from the ROUNDED taps, so the correction is exact for the filter that runs.  No-op when already built.
int ensure_decimation(tdoa_ctx *ctx, const FftPlan &pl, int lag_lo, int lag_hi)
{
    const int reach = lag_reach(lag_lo, lag_hi);
    if (ctx->dec_nc == pl.Nc && ctx->dec_reach == reach) return TDOA_OK;
    const long long M = reach / 2 + 2;
    const DecDesign dd = decimation_design(pl, reach);
    const int T = dd.T;
    const double beta = 0.1102 * (dd.att - 8.7), i0b = bessel_i0(beta);
    std::vector<float> taps(2 * T + 1);
    for (int t = -T; t <= T; t++) {
        const double x = (double)t / kDecD, r = (double)t / T;
        const double sinc = t == 0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        taps[t + T] = (float)(sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b);
    }
    std::vector<float> gain(M + 4);
    for (long long m = 0; m < M + 4; m++) {
        double w = 0.0;
        for (int t = -T; t <= T; t++) w += (double)taps[t + T] * std::cos(2.0 * M_PI * (double)t * (double)m / (double)pl.Nc);
        gain[m] = (float)((double)kDecD / w);
    }
    // the kernel's layout: phase p x step s, the tap t = 16 (s - kDecCentre) + p (zero where |t| > T)
    // (then W_N^p, p = 0..15, N = 2 Nc, as float2: the row rotations of k_pair_decimate_cols)
    // (then, at 288: phase 0 with its steps reversed -- the upward walks' row of phase 0)
    std::vector<float> tab(256 + 32 + 16, 0.0f);
    for (int t = -T; t <= T; t++) {
        const int p = ((t % 16) + 16) % 16, sidx = (t - p) / 16 + kDecCentre;
        tab[16 * p + sidx] = taps[t + T];
    }
    for (int s = 0; s < kDecSteps; s++) tab[288 + s] = tab[kDecSteps - 1 - s];
    for (int p = 0; p < 16; p++) {
        const double ang = -M_PI * (double)p / (double)pl.Nc;
        tab[256 + 2 * p] = (float)std::cos(ang);
        tab[256 + 2 * p + 1] = (float)std::sin(ang);
    }
    int rc;
    if ((rc = ensure(ctx, ctx->dec_taps, sizeof(float) * tab.size()))) return rc;
    if ((rc = ensure(ctx, ctx->dec_gain, sizeof(float) * gain.size()))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->dec_taps.p, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dec_gain.p, gain.data(), sizeof(float) * gain.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // host vectors go out of scope
    ctx->dec_nc = pl.Nc;
    ctx->dec_reach = reach;
    ctx->dec_T = T;
    return TDOA_OK;
}

// single-look K1 (k1_single_look.hpp): entries per edge array (the largest |lag| K = lag_reach, + 1, rounded up), tile
// records per station-window of the fused column kernels
int once_k1(int lag_lo, int lag_hi) { return (lag_reach(lag_lo, lag_hi) + 1 + 3) & ~3; }
int once_tiles_per_sw(const FftPlan &pl)      // records per station-window: one per wave and tile (k1_single_look.hpp)
{
    return kOnceWavesPerTile * (pl.N2 == 512 ? pl.N1 / 32 : (pl.N1 / 64) * std::max(1, pl.N2 / 256));
}

// The staged column walk (dec_staged.hpp) gives a workgroup up to `cap` of a window's pairs and stages the rows of every
// station those pairs touch.  Pairs are numbered as process_impl lays them out: (0,1), (0,2), ..., (S-2,S-1).
//  * Up to eight stations: consecutive runs of equal length (28 pairs: 14 + 14) -- every group touches every station anyway.
//  * More: what the loader can bring in is the bound there (the CU's memory pipeline takes ~1 KB of LDS-DMA per 50 - 65 cycles),
//    and sixteen stations per group leave room for four rows per phase only.  Groups are grown greedily around the first pair
//    not yet placed -- the station that adds the most unplaced pairs joins until `cap` pairs or eight stations are reached
//    (the first groups are the 15 pairs of six stations) --, then small leftovers are merged: 16 stations become 9 groups that
//    stage 62 station-rows per row of the window instead of 8 x 16 = 128, each within eight stations: eight rows per phase.
std::vector<StgGroup> build_stg_groups(int S, int cap, bool fill = false)
{
    const int P = S * (S - 1) / 2, M = 8;
    std::vector<std::pair<int, int>> pairs;
    for (int i = 0; i < S; i++)
        for (int j = i + 1; j < S; j++) pairs.emplace_back(i, j);
    auto pidx = [&](int a, int b) { if (a > b) std::swap(a, b); return a * S - a * (a + 1) / 2 + (b - a - 1); };
    std::vector<StgGroup> out;
    if (S <= M) {
        // (fill: full groups first -- sixteen walks are four per SIMD, the remainder of 28 pairs three -- instead of equal runs)
        const int groups = (P + cap - 1) / cap, n = fill ? cap : (P + groups - 1) / groups;
        for (int g = 0; g < groups; g++) {
            StgGroup sg{};
            for (int p = g * n; p < std::min(P, (g + 1) * n); p++) {
                sg.pair[sg.n++] = (uint8_t)p;
                sg.mask |= (1u << pairs[p].first) | (1u << pairs[p].second);
            }
            out.push_back(sg);
        }
        return out;
    }
    std::vector<char> open(P, 1);
    int left = P;
    while (left) {
        int seed = 0;
        while (!open[seed]) seed++;
        std::vector<int> T = {pairs[seed].first, pairs[seed].second};
        auto inside = [&] {
            int c = 0;
            for (size_t x = 0; x < T.size(); x++)
                for (size_t y = x + 1; y < T.size(); y++) c += open[pidx(T[x], T[y])];
            return c;
        };
        while ((int)T.size() < M && inside() < cap) {
            int best = -1, gain = 0;
            for (int v = 0; v < S; v++) {
                if (std::find(T.begin(), T.end(), v) != T.end()) continue;
                int g = 0;
                for (int t : T) g += open[pidx(t, v)];
                if (g > gain) { gain = g; best = v; }
            }
            if (best < 0) break;
            T.push_back(best);
        }
        std::sort(T.begin(), T.end());
        StgGroup sg{};
        for (size_t x = 0; x < T.size(); x++)
            for (size_t y = x + 1; y < T.size(); y++) {
                const int p = pidx(T[x], T[y]);
                if (!open[p] || sg.n >= cap) continue;
                open[p] = 0;
                left--;
                sg.pair[sg.n++] = (uint8_t)p;
                sg.mask |= (1u << T[x]) | (1u << T[y]);
            }
        out.push_back(sg);
    }
    for (bool merged = true; merged;) {          // leftovers: two groups that fit one workgroup and eight stations together
        merged = false;
        for (size_t a = 0; a < out.size() && !merged; a++)
            for (size_t b = a + 1; b < out.size() && !merged; b++)
                if (out[a].n + out[b].n <= cap && __builtin_popcount(out[a].mask | out[b].mask) <= M) {
                    for (int q = 0; q < out[b].n; q++) out[a].pair[out[a].n++] = out[b].pair[q];
                    out[a].mask |= out[b].mask;
                    out.erase(out.begin() + (long)b);
                    merged = true;
                }
    }
    return out;
}

// the staged walk's tables (StgTables) for the knobs that shape them -- ctx->stg, built once by tdoa_create
StgTables stg_tables(const Knobs &k)
{
    StgTables t;
    const int n_lw = std::max(1, std::min(k.stg_loaders ? k.stg_loaders : 1, 4));
    const int cap = k.stg_cw > 0 ? std::min(k.stg_cw, kStgMaxWaves - n_lw) : kStgMaxWaves - n_lw;
    for (int pass = 0; pass < 2; pass++)
    for (int S = 2; S <= kStgMaxStations; S++) {
        const std::vector<StgGroup> g = pass ? build_stg_groups(S, k.stg_cw > 0 ? std::min(k.stg_cw + 1, kStgMaxWaves) : kStgMaxWaves, true)
                                             : build_stg_groups(S, cap);
        StgTable &e = pass ? t.tab16[S] : t.tab[S];
        e.off = (int)t.groups.size();
        e.count = (int)g.size();
        for (const StgGroup &x : g) {
            e.slots = std::max(e.slots, __builtin_popcount(x.mask));
            e.max_n = std::max(e.max_n, (int)x.n);
        }
        t.groups.insert(t.groups.end(), g.begin(), g.end());
    }
    return t;
}

int ensure_stg_groups(tdoa_ctx *ctx)
{
    if (ctx->stg_ready) return TDOA_OK;
    const std::vector<StgGroup> &all = ctx->stg.groups;
    int rc;
    if ((rc = ensure(ctx, ctx->stg_groups, sizeof(StgGroup) * all.size()))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->stg_groups.p, all.data(), sizeof(StgGroup) * all.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stg_ready = true;
    return TDOA_OK;
}

}  // namespace
