"""CPU: what the narrowband inputs of tests/spectral_inputs.py can detect, before any kernel sees them.

On broadband input every one of the Nc spectral bins carries about 1 / Nc of a correlation surface, so an error confined to
one bin stays below every bound the suite asserts relative to the peak; on a tone the centre bin carries half of it.  Held
here, in float64: the inputs put their energy on the bins they name; losing such a bin moves a searched lag by 5 % of the peak
or more; losing a bin of a broadband pair moves it by less than the suite's tightest bound; the two oracles agree on such input;
the float64 statement of the 16:1 spectrum decimation leaves on tones what it leaves on noise-level peaks."""
import numpy as np
import pytest

import spectral_inputs as si
from oracle import float_pipeline as fp

ML = 20000
CPU_PLANS = ("2^21", "2^22", "2^17")                                  # the ten-second comb has a GPU case alone
ALL_INPUTS = [(p, name, bins) for p in CPU_PLANS for name, bins in si.inputs(si.PLANS[p]["N2"])]
IDS = ["%s-%s" % (p, name) for p, name, _ in ALL_INPUTS]


def test_tables_cover_every_class():
    """every class on every plan, the bins re-addressed for the plan's N2; tones of one comb at least 1000 bins apart; the
    ten-second comb holds k = 1, a row-0 bin, a row-N2/2 bin and Nc - 1"""
    for p in CPU_PLANS:
        N, N2 = si.PLANS[p]["N"], si.PLANS[p]["N2"]
        assert N == 2 * si.N1 * N2
        table = si.inputs(N2)
        held = sorted(k for _, bins in table for k in bins)
        want = sorted(si._k(a, N2) for _, a in si.bin_classes(N2))
        assert held == want and len(set(held)) == len(held)
        for _, bins in table:
            assert 1 <= len(bins) <= 4 and all(abs(a - b) >= 1000 for a in bins for b in bins if a != b)
        classes = {c for c, _ in si.bin_classes(N2)}
        assert classes == {"end", "self-mirror", "row 0", "row N2/2", "column end", "block edge", "no neighbour"}
        for k in (1, 2, N // 2 - 1, N // 2, N // 4, N // 4 + 1, N // 4 - 1):
            assert k in held
        for k2, k1 in [(0, 1), (0, 63), (0, 64), (0, 4095), (N2 // 2, 0), (N2 // 2, 2047), (N2 // 2, 4095), (1, 30), (N2 - 1, 30),
                       (1, 63), (N2 - 1, 63), (1, 64), (N2 - 1, 64), (N2 - 1, 0), (1, 4095)]:
            assert si.bin_of(k2, k1, N2) in held
    held = {k for _, bins in si.inputs(256) for k in bins}
    for k2 in (1, 15, 16, 95, 96, 160, 240, 255):
        assert si.bin_of(k2, 30, 256) in held
    held = {k for _, bins in si.inputs(512) for k in bins}
    for k2 in (1, 15, 16, 95, 96, 416, 496, 511):
        assert si.bin_of(k2, 30, 512) in held
    name, bins = si.ten_second_comb()
    nc = si.PLANS["5x2^22"]["N"] // 2
    assert bins[0] == 1 and bins[1] % 2560 == 0 and bins[2] % 2560 == 1280 and bins[3] == nc - 1


def test_tone_iq_is_the_wanted_discriminator_output():
    """float64 atan2 discriminator of the bytes against the cosines: 8-bit rounding at 100 LSB leaves well under 0.02 rad; the
    bytes stay inside 27 .. 228; a delay is a shift by whole samples; too much amplitude is refused"""
    N, n = 1 << 17, 70_000
    for bins, delay in (((1,), 0), ((N // 2,), 5), ((1008, 40000, 65535), 37)):
        iq = si.tone_iq(bins, n, N, delay)
        assert iq.dtype == np.uint8 and iq.size == 2 * n and 27 <= iq.min() and iq.max() <= 228
        i = np.arange(n) - delay
        a = 1.0 if len(bins) == 1 else 2.0 / len(bins)
        want = sum(a * np.cos(2 * np.pi * k * i / N) for k in bins)
        assert np.abs(fp.discriminate(iq)[1:] - want[1:]).max() < 0.02
        assert np.array_equal(si.tone_iq(bins, n, N, delay), iq)
    with pytest.raises(AssertionError):
        si.tone_iq((100, 5000, 9000), n, N, 0, amps=(1.0, 1.0, 1.0))


@pytest.mark.parametrize("plan,name,bins", ALL_INPUTS, ids=IDS)
def test_inputs_sit_on_their_bins_and_losing_one_shows(plan, name, bins):
    """>= 0.9 of the normalised codes' energy within +-3 bins of the tones (the rest is the window's leakage: L < N); setting
    the centre bin of any tone to zero in one station's spectrum changes a searched lag by >= 5 % of the peak"""
    P = si.PLANS[plan]
    a = si.tone_iq(bins, P["L"], P["N"], si.DELAYS[0])
    b = si.tone_iq(bins, P["L"], P["N"], si.DELAYS[1])
    share = si.concentration(a, P["N"], bins)
    effect = si.zero_bin_effect(a, b, P["N"], ML, list(bins))
    print("%s %s: share %.3f, zero-bin effect %s" % (plan, name, share, " ".join("%.3f" % e for e in effect)))
    assert share >= 0.9, share
    assert min(effect) >= 0.05, effect


def test_broadband_input_cannot_show_a_lost_bin(oracle):
    """the gap: on a delayed-FM pair, the suite's usual input, a lost bin changes no searched lag by more than 1e-5 of the
    peak -- the bound the kernels are held to (measured: about 1e-6); and the one-bin term zero_bin_effect evaluates is the
    difference of two full inverses"""
    L, N = 1_100_000, 1 << 21
    a, b = oracle.simulate_delayed_fm(L, 0, 4242, 1), oracle.simulate_delayed_fm(L, 37, 4242, 2)
    ks = [1, 256, 65536, 524288, 1048575]
    effect = si.zero_bin_effect(a, b, N, ML, ks)
    print("broadband FM: zero-bin effect %s" % " ".join("%.2e" % e for e in effect))
    assert max(effect) <= 1e-5, effect
    A, B = np.fft.rfft(si.codes(a), N), np.fft.rfft(si.codes(b), N)
    d = np.arange(-(ML - 1), ML)
    full = np.fft.irfft(np.conj(A) * B, N)[d % N]
    A[ks[2]] = 0.0
    plain = np.abs(np.fft.irfft(np.conj(A) * B, N)[d % N] - full).max() / np.abs(full).max()
    assert abs(plain - effect[2]) <= 1e-6 * effect[2] + 1e-15


def _three(plan):
    t = si.inputs(si.PLANS[plan]["N2"])
    return [t[0], t[len(t) // 2], t[-1]]


@pytest.mark.parametrize("plan", ["2^21", "2^17"])
def test_the_two_oracles_agree_on_tones(oracle, plan):
    """the integer-code oracle against the float64 atan2 pipeline at every lag, three inputs per plan: 1e-6 of the peak
    (measured: 1.9e-8)"""
    P = si.PLANS[plan]
    for name, bins in _three(plan):
        a = si.tone_iq(bins, P["L"], P["N"], si.DELAYS[0])
        b = si.tone_iq(bins, P["L"], P["N"], si.DELAYS[1])
        _, _, oc = oracle.b_xcorr_peak_fft(oracle.b_preprocess(a)[0], oracle.b_preprocess(b)[0], ML)
        _, fcorr, fc = fp.xcorr_peak_u8(a, b, ML)
        dev = np.abs(oc - fc).max() / abs(fcorr)
        print("%s %s: oracle vs float pipeline %.2e of the peak" % (plan, name, dev))
        assert dev <= 1e-6, (name, dev)


def test_decimation_model_on_tones(oracle):
    """the float64 statement of the 16:1 spectrum decimation (test_mode_b_anchors.py) on three inputs of the 4096 x 256 plan:
    below that test's own 1.5e-6 of the peak (measured: at most 6.5e-7, the level it leaves on noise-level peaks), so the
    decimated routes are expected inside the project's 1e-5"""
    P = si.PLANS["2^21"]
    t, h = si.decimation_taps(P["N"], ML)
    assert t.size == 191 and h[95] == 1.0 and np.array_equal(h, h[::-1])
    for name, bins in _three("2^21"):
        ta = oracle.b_preprocess(si.tone_iq(bins, P["L"], P["N"], si.DELAYS[0]))[0].astype(np.float64)
        tb = oracle.b_preprocess(si.tone_iq(bins, P["L"], P["N"], si.DELAYS[1]))[0].astype(np.float64)
        err = si.decimation_model_error(ta, tb, P["N"], ML)
        print("%s: decimation model leaves %.2e of the peak" % (name, err))
        assert err < 1.5e-6, (name, err)
