"""Mode A (csrc/exact_reference.hpp, csrc/exact_reference_api.inc) against the CPU oracle at the sizes where its kernels
change tile, path or launch shape: the 256-lag tile and the 64-lag switch of the two correlation kernels, the block count,
exact ties in the first-max reduction, non-default corr_block / sample_rate / weak_threshold / max_lag, the geometry
bound, the moving average's path switch and tile + halo sizes, signed zeros, more than 256 power chunks, the two-job and
single-job DC launches, simpleCorrelate's template and lag tiles, and short fastDFT sizes.

Tolerances are those of tests/test_gpu_reference.py: equal bits wherever the reference's evaluation order is reproduced
(preprocess, correlations over >= 64 lags, simpleCorrelate, fastSNR) and wherever the inputs are integers (every sum is
exact in any order); corr within 1e-12 relative where fewer than 64 lags are searched (the wave-per-(lag, block) kernel
sums an f64 block as a tree).  Where the block size is not the oracle's 1000 the reference is tests/reference_model.py,
itself held to the oracle by tests/test_reference_model_cpu.py."""
import math

import numpy as np
import pytest

from reference_model import tdc_model, tie_cases

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def ctxs():
    """one context per parameter set, made on first use and kept for the module: ctxs() is the default one"""
    import tdoa_amd
    made = {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in made:
            made[key] = tdoa_amd.Context(**kw)
        return made[key]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def ctx(ctxs):
    return ctxs()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.complex64).view(np.uint32)


def _rand(n, seed, dc=0j, scale=1.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return (scale * (x + dc)).astype(np.complex64)


def _same_corr(got, want, n_lags):
    """the existing file's rule: delay identical; corr equal bits from 64 searched lags on, else within 1e-12"""
    (d, c), (od, oc) = got, want
    assert d == od, (got, want)
    if n_lags >= 64:
        assert c == oc, (got, want, n_lags)
    else:
        assert abs(c - oc) <= 1e-12 * abs(oc), (got, want, n_lags)


# ---- a. lag-count edges: the 64-lag switch between the two kernels, the 256-lag tile ---------------------------------
LAG_EDGES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 513]


def _shifts(L):
    return sorted({0, max(L - 1, 0)} | {k for k in (255, 256) if k < L})


@pytest.mark.parametrize("L", LAG_EDGES)
def test_lag_count_edges_by_signal_length(ctx, oracle, L):
    s = _rand(2001 + L, 1000 + L)
    for shift in _shifts(L):                              # the peak on lag 0, on the last lag, on both sides of a tile edge
        t = s[shift:shift + 2001].copy()
        got = ctx.time_domain_correlation(t, s, 20000)
        want = oracle.time_domain_correlation(t, s, 20000)
        assert want[0] == shift
        _same_corr(got, want, max(L, 1))
        assert ctx.time_domain_correlation(s, t, 20000) == got            # the shorter input is the template


@pytest.mark.parametrize("L", LAG_EDGES)
def test_lag_count_edges_by_max_lag(ctx, oracle, L):
    s = _rand(2001 + 600, 2000 + L)
    for shift in _shifts(L):
        t = s[shift:shift + 2001].copy()
        got = ctx.time_domain_correlation(t, s, L)
        want = oracle.time_domain_correlation(t, s, L)
        assert want[0] == shift
        _same_corr(got, want, max(L, 1))
        assert ctx.time_domain_correlation(s, t, L) == got
    t = s[L + 3:L + 3 + 2001].copy()                      # the true peak three lags past the searched range
    _same_corr(ctx.time_domain_correlation(t, s, L), oracle.time_domain_correlation(t, s, L), max(L, 1))


# ---- b. block-count edges: block starts below tl - 1000 ---------------------------------------------------------------
@pytest.mark.parametrize("tl,nb", [(1000, 0), (1001, 1), (1999, 1), (2000, 1), (2001, 2), (3001, 3)])
@pytest.mark.parametrize("extra", [300, 3])
def test_block_count_edges(ctx, oracle, tl, nb, extra):
    s = _rand(tl + extra, 7 * tl + extra)
    shift = extra - 2
    t = s[shift:shift + tl].copy()
    t[nb * 1000:] *= np.complex64(1e3)                    # one block too many, or one too few, cannot agree with the oracle
    got = ctx.time_domain_correlation(t, s, 20000)
    want = oracle.time_domain_correlation(t, s, 20000)
    if nb == 0:
        assert got == want == (0, 0.0)
    else:
        assert want[0] == shift
        _same_corr(got, want, extra)
    assert ctx.time_domain_correlation(s, t, 20000) == got


# ---- c. exact ties in k_ex_first_max ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tie_cases(), ids=lambda c: c[0])
def test_exact_ties_resolve_to_the_lowest_lag(ctx, oracle, case):
    name, t, s, (lo, hi), sign = case
    want = oracle.time_domain_correlation(t, s, 20000)
    got = ctx.time_domain_correlation(t, s, 20000)
    assert want[0] == lo and (want[1] < 0) == (sign < 0)
    assert got == want                                    # integer samples: every sum exact, so ==
    assert ctx.time_domain_correlation(s, t, 20000) == want
    # the range ending on the second copy, and one lag short of it: then the first copy stands alone
    assert ctx.time_domain_correlation(t, s, hi + 1) == want
    assert ctx.time_domain_correlation(t, s, hi) == oracle.time_domain_correlation(t, s, hi)


# ---- d. corr_block off its default, against the model ----------------------------------------------------------------
@pytest.mark.parametrize("block", [1, 7, 999, 3622])
@pytest.mark.parametrize("lags", [257, 64, 3])
def test_corr_block_against_the_model(ctxs, block, lags):
    c = ctxs(corr_block=block)
    tl = 3 * block + 1                                    # three blocks and one sample: nb = 3
    s = _rand(tl + lags, 31 * block + lags)
    for shift in (0, lags - 1):
        t = s[shift:shift + tl].copy()
        t[3 * block:] *= np.complex64(1e3)                # the sample past the last block must stay unread
        want = tdc_model(t, s, 20000, block)
        if block >= 999:
            assert want[0] == shift
        _same_corr(c.time_domain_correlation(t, s, 20000), want[:2], lags)
        assert c.time_domain_correlation(s, t, 20000) == c.time_domain_correlation(t, s, 20000)


def test_corr_block_1000_is_the_default(ctxs, ctx):
    s = _rand(3301, 12)
    t = s[123:123 + 3001].copy()
    assert ctxs(corr_block=1000).time_domain_correlation(t, s, 20000) == ctx.time_domain_correlation(t, s, 20000)


# ---- e. the geometry bound: 2 * block * 8 + 256 * 8 bytes of LDS against 60000 ----------------------------------------
def test_geometry_bound_is_an_error_status_and_the_context_lives(ctxs, oracle):
    import tdoa_amd
    c = ctxs(corr_block=3623)
    s = _rand(2 * 3623 + 1 + 100, 13)
    t = s[40:40 + 2 * 3623 + 1].copy()
    for lags_sig in (s, s[:t.size + 3]):                  # both kernels' launches are refused alike
        with pytest.raises(tdoa_amd.TdoaError) as e:
            c.time_domain_correlation(t, lags_sig, 20000)
        assert e.value.status == ERR_UNSUPPORTED
    # the same context afterwards: no block fits a 3623-sample template; the other mode A calls answer as ever
    assert c.time_domain_correlation(t[:3623], s, 20000) == (0, 0.0)
    got, weak = c.preprocess(s)
    want, oweak = oracle.preprocess(s)
    assert weak == oweak and np.array_equal(_bits(got), _bits(want))
    assert c.simple_correlate(t[:700], s[:1500]) == oracle.simple_correlate(t[:700], s[:1500])
    with pytest.raises(tdoa_amd.TdoaError) as e:
        c.time_domain_correlation(t, s, 20000)
    assert e.value.status == ERR_UNSUPPORTED


# ---- f. many blocks: 70 000 rows of grid.y ---------------------------------------------------------------------------
def test_seventy_thousand_blocks(ctxs):
    """corr_block 1, template 70 001, 64 lags: k_ex_tdc_blocks is launched with one grid row per block.  Either the
    model's (delay, bits) or TDOA_ERR_UNSUPPORTED with the context usable afterwards; never a raw HIP launch error."""
    import tdoa_amd
    c = ctxs(corr_block=1)
    s = _rand(70065, 14)
    t = s[63:63 + 70001].copy()
    want = tdc_model(t, s, 20000, 1)
    assert want[0] == 63
    try:
        got = c.time_domain_correlation(t, s, 20000)
    except tdoa_amd.TdoaError as e:
        assert e.status == ERR_UNSUPPORTED, e
        got = None
    if got is not None:
        assert got == want[:2]
    small = tdc_model(t[:41], s[:120], 20000, 1)
    assert c.time_domain_correlation(t[:41], s[:120], 20000) == small[:2]


# ---- g. preprocess off the default rate: the moving average's path switch, tiles and halos ----------------------------
RATES = [6.4e5, 5.6e5, 4e5, 1e5, 48000.0, 8000.0]
CUTOFFS = [57.5, 62.5, 117.5, 122.5, 975000.0, 100.0, 40000.0, 500.0, 50000.0]


def _largest_half(oracle, fs):
    return max([oracle.cutoff_window(f, fs) for f in CUTOFFS] + [50, 100]) // 2


def test_filter_windows_are_the_ones_these_rates_were_chosen_for(oracle):
    """read on the CPU: the windows of the 40 kHz, 50 kHz and 500 Hz edges at each rate (halves 4 and 3 are the two sides
    of the moving average's fast-path switch, 2 * half >= 7)"""
    got = {fs: tuple(oracle.cutoff_window(f, fs) for f in (40000.0, 50000.0, 500.0)) for fs in RATES}
    assert got == {6.4e5: (8, 6, 640), 5.6e5: (7, 5, 560), 4e5: (5, 4, 400), 1e5: (3, 3, 100), 48000.0: (3, 3, 48),
                   8000.0: (3, 3, 8)}
    assert [oracle.cutoff_window(f, 1e5) for f in (57.5, 62.5, 117.5, 122.5, 100.0)] == [869, 800, 425, 408, 500]
    assert [oracle.cutoff_window(f, 48000.0) for f in (57.5, 62.5, 117.5, 122.5, 100.0)] == [417, 384, 204, 195, 240]
    assert [oracle.cutoff_window(f, 8000.0) for f in (57.5, 62.5, 117.5, 122.5, 100.0)] == [69, 64, 34, 32, 40]


@pytest.mark.parametrize("fs", RATES)
def test_preprocess_at_other_sample_rates(ctxs, oracle, fs):
    c = ctxs(sample_rate=fs)
    h = _largest_half(oracle, fs)
    for n in [1, 2, 3, 2047, 2048, 2049, 4097, 2048 + h - 1, 2048 + h, 2048 + h + 1]:
        strong = _rand(n, int(fs) + n, dc=0.3 - 0.2j)
        for sig, is_weak in ((strong, False), ((strong * np.complex64(1e-3)).astype(np.complex64), True)):
            want, oweak = oracle.preprocess(sig, fs)
            got, weak = c.preprocess(sig)
            assert weak == oweak == is_weak, (fs, n)
            assert np.array_equal(_bits(got), _bits(want)), (fs, n, is_weak)


# ---- h, i. signed zeros, constants, and weak_threshold: either chain for any input -----------------------------------
def _standard_chain(o, sig, fs=2e6):
    return o.normalize(o.lowpass(o.bandpass(o.remove_dc(sig)[0], 500, 50000, fs), 100))


def _zero_inputs():
    n = 3000
    holes = _rand(n, 15, dc=0.1 + 0.05j)
    holes[750:2250] = 0
    mixed = np.zeros(n, dtype=np.complex64)
    mixed.real[::2] = -0.0
    mixed.imag[1::3] = -0.0
    return {"plus_zero": np.zeros(n, dtype=np.complex64),
            "minus_zero": np.full(n, complex(-0.0, -0.0), dtype=np.complex64),
            "mixed_zero": mixed,
            "constant": np.full(n, 0.3 - 0.2j, dtype=np.complex64),
            "zero_stretch": holes}


@pytest.mark.parametrize("name", ["plus_zero", "minus_zero", "mixed_zero", "constant", "zero_stretch"])
def test_signed_zeros_and_constants_through_both_chains(ctxs, oracle, name):
    sig = _zero_inputs()[name]
    if name == "minus_zero":
        assert np.signbit(sig.real).all() and np.signbit(sig.imag).all()
    want, oweak = oracle.preprocess(sig)
    got, weak = ctxs().preprocess(sig)
    assert weak == oweak == (name not in ("constant", "zero_stretch"))
    assert np.array_equal(_bits(got), _bits(want))        # bits: the sign of a zero counts
    assert not np.isnan(got.view(np.float32)).any()
    std, std_weak = ctxs(weak_threshold=0.0).preprocess(sig)
    assert not std_weak and np.array_equal(_bits(std), _bits(_standard_chain(oracle, sig)))
    wk, wk_weak = ctxs(weak_threshold=1e9).preprocess(sig)
    assert wk_weak and np.array_equal(_bits(wk), _bits(oracle.enhance_weak(sig)))
    assert not np.isnan(std.view(np.float32)).any() and not np.isnan(wk.view(np.float32)).any()


@pytest.mark.parametrize("n", [9, 2049, 6000])
def test_weak_threshold_selects_the_chain(ctxs, oracle, n):
    strong = _rand(n, 16 + n, dc=0.3 - 0.2j)
    weak_sig = (strong * np.complex64(1e-3)).astype(np.complex64)
    assert oracle.preprocess(strong)[1] is False and oracle.preprocess(weak_sig)[1] is True
    got, weak = ctxs(weak_threshold=0.0).preprocess(weak_sig)             # a weak signal down the standard chain
    assert not weak and np.array_equal(_bits(got), _bits(_standard_chain(oracle, weak_sig)))
    got, weak = ctxs(weak_threshold=1e9).preprocess(strong)               # a strong one down the weak chain
    assert weak and np.array_equal(_bits(got), _bits(oracle.enhance_weak(strong)))


# ---- j. more than 256 power chunks: k_ex_power_final's second trip ---------------------------------------------------
@pytest.mark.parametrize("n", [8191, 8192, 8193, 256 * 8192 + 1])
def test_power_chunk_edges(ctxs, oracle, n):
    """sample_rate 8000 keeps every window below 70 taps, so the oracle's chain stays under a second at 2 097 153 samples.
    The output's scale is 1 / sqrt(power): a chunk's partial sum dropped changes every sample.  The last sample -- alone
    in chunk 256 -- is some 15 times the largest of the others, so that its loss moves the f32 scale by many ulps."""
    c = ctxs(sample_rate=8000.0)
    rng = np.random.default_rng(n)
    sig = np.empty(n, dtype=np.complex64)
    sig.real = rng.uniform(-1, 1, n).astype(np.float32)
    sig.imag = rng.uniform(-1, 1, n).astype(np.float32)
    sig *= np.complex64(2e-3)
    sig[-1] = np.complex64(0.03 - 0.02j)
    want, oweak = oracle.preprocess(sig, 8000.0)
    got, weak = c.preprocess(sig)
    assert weak and oweak
    assert np.array_equal(_bits(got), _bits(want))


# ---- k. the two-job DC launch through cross_correlate ----------------------------------------------------------------
def _pair(n1, n2, seed):
    """two strong signals with DIFFERENT means (a swapped DC job shows), the shorter a noisy cut of the longer"""
    long_ = _rand(max(n1, n2), seed, dc=-0.1 + 0.4j)
    rng = np.random.default_rng(seed + 1)
    m = min(n1, n2)
    shift = (max(n1, n2) - m) // 3
    short = long_[shift:shift + m] + np.complex64(0.4 + 0.6j)
    short = (short + 0.1 * (rng.standard_normal(m) + 1j * rng.standard_normal(m))).astype(np.complex64)
    return (short, long_) if n1 <= n2 else (long_, short)


@pytest.mark.parametrize("n1,n2", [(1025, 5000), (2049, 2049), (1024 + 1001, 3 * 1024), (5000, 1025)])
def test_cross_correlate_dc_chain_edges(ctx, oracle, n1, n2):
    a, b = _pair(n1, n2, n1 + n2)
    _same_corr(ctx.cross_correlate(a, b), oracle.cross_correlate(a, b), max(abs(n2 - n1), 1))


def test_cross_correlate_takes_max_lag_from_the_context(ctxs, oracle):
    a, b = _pair(1025, 5000, 17)                          # the cut sits at lag 1325: outside 300 lags
    want = oracle.time_domain_correlation(oracle.preprocess(a)[0], oracle.preprocess(b)[0], 300)
    assert want != oracle.cross_correlate(a, b)
    _same_corr(ctxs(max_lag=300).cross_correlate(a, b), want, 300)
    want = oracle.time_domain_correlation(oracle.preprocess(a)[0], oracle.preprocess(b)[0], 63)
    _same_corr(ctxs(max_lag=63).cross_correlate(a, b), want, 63)


# ---- l. batch: equal pairs, >= 64 lags, odd counts (the single-job DC launch) ----------------------------------------
@pytest.fixture(scope="module")
def batch_signals():
    base = _rand(4600, 18, dc=0.2 - 0.1j)
    out = []
    for k, n in enumerate([3001, 3001, 3070, 4500, 2500]):
        rng = np.random.default_rng(19 + k)
        x = base[5 * k:5 * k + n] + np.complex64(0.1 * k) + 0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        out.append(x.astype(np.complex64))
    return out


@pytest.mark.parametrize("count", [2, 3, 5])
def test_batch_of_non_empty_signals(ctx, oracle, batch_signals, count):
    sigs = batch_signals[:count]
    got = ctx.cross_correlate_batch(sigs)
    assert len(got) == count * (count - 1) // 2
    p = 0
    for i in range(count):
        for j in range(i + 1, count):
            assert got[p] == ctx.cross_correlate(sigs[i], sigs[j]), (i, j)
            _same_corr(got[p], oracle.cross_correlate(sigs[i], sigs[j]), max(abs(sigs[i].size - sigs[j].size), 1))
            p += 1


def test_batch_of_sixty_five_signals_is_invalid(ctx, batch_signals):
    import tdoa_amd
    with pytest.raises(tdoa_amd.TdoaError) as e:
        ctx.cross_correlate_batch([batch_signals[0][:16]] * 65)
    assert e.value.status == ERR_INVALID
    assert len(ctx.cross_correlate_batch([batch_signals[0][:1100]] * 64)) == 64 * 63 // 2
    assert ctx.cross_correlate_batch(batch_signals[:2])[0] == ctx.cross_correlate(*batch_signals[:2])


# ---- m. simpleCorrelate: 512-sample template tiles, 256-lag tiles, per-lag signal power --------------------------------
@pytest.mark.parametrize("tl", [511, 512, 513, 1025])
def test_simple_correlate_tile_edges(ctx, oracle, tl):
    for extra in (0, 1, 255, 256, 257, 999, 1000, 2000):
        s = _rand(tl + extra, 20 * tl + extra)
        last = max(min(extra, 1000) - 1, 0)               # the last searched lag
        for shift in sorted({0, last}):
            t = s[shift:shift + tl].copy()
            want = oracle.simple_correlate(t, s)
            got = ctx.simple_correlate(t, s)
            assert want[0] == shift and want[1] > 0.99
            assert got == want, (tl, extra, shift)
            assert ctx.simple_correlate(s, t) == want
            neg = (-t).astype(np.complex64)
            want = oracle.simple_correlate(neg, s)
            assert want[0] == shift and want[1] < -0.99
            assert ctx.simple_correlate(neg, s) == want, (tl, extra, shift)


def test_simple_correlate_skips_lags_without_signal_power(ctx, oracle):
    s = _rand(512 + 700, 21)
    s[:600] = 0                                           # lags 0..88 see 512 exact zeros: power 0, skipped
    t = s[650:650 + 512].copy()
    want = oracle.simple_correlate(t, s)
    assert want[0] == 650 and ctx.simple_correlate(t, s) == want
    t = s[:512].copy()                                    # an all-zero template: no lag qualifies
    assert oracle.simple_correlate(t, s) == (0, 0.0) and ctx.simple_correlate(t, s) == (0, 0.0)
    s[100] = np.complex64(1e-30)                          # lags 0..100 have a power that underflows to 0
    t = s[650:650 + 512].copy()
    assert ctx.simple_correlate(t, s) == oracle.simple_correlate(t, s)


# ---- n. fastSNR at short DFT sizes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [2, 3, 255, 256, 257, 8191, 8192, 8193])
def test_fast_snr_sizes(ctx, oracle, total):
    rng = np.random.default_rng(total)
    k = np.arange(total)
    tone = 127.5 + 60 * np.stack([np.cos(0.7 * k), np.sin(0.7 * k)], axis=1) + rng.normal(0, 6, (total, 2))
    for raw in (np.clip(np.rint(tone), 0, 255).astype(np.uint8).ravel(), rng.integers(0, 256, 2 * total, dtype=np.uint8)):
        got, want = ctx.fast_snr(raw, total), oracle.fast_snr(raw, total)
        assert got == want or (math.isnan(got) and math.isnan(want)), (got, want)
