"""Narrowband inputs for mode B: u8 IQ whose discriminator output is a sum of cosines on chosen bins of the N-point real
transform, the tables of bins that single out the kernels' special cases, and the float64 experiment that shows what such an
input can detect (tests/test_spectral_inputs_cpu.py, tests/test_gpu_spectral_bins.py).

A bin is addressed as (k2, k1) of the packed spectrum [k2][k1] of a plan N = 2 N1 N2 (N1 = 4096): k = k2 + N2 k1 < Nc = N / 2;
NYQUIST stands for k = Nc, the alternating codes.  On broadband input every bin carries 1 / Nc of a surface; on a tone the
centre bin carries about half of it."""
import functools

import numpy as np

from oracle import float_pipeline as fp

N1 = 4096
NYQUIST = "nyquist"
MIN_GAP = 1000                                    # tones of one comb lie at least this many bins apart
MAX_TONES = 4

# the plans the GPU file runs: N, N2, window length, and the delays of up to four stations (pair calls use the first two)
PLANS = {
    "2^21": dict(N=1 << 21, N2=256, L=1_100_000),
    "2^22": dict(N=1 << 22, N2=512, L=2_200_001),
    "2^17": dict(N=1 << 17, N2=16, L=70_000),
    "5x2^22": dict(N=5 << 22, N2=2560, L=20_000_000),
}
DELAYS = (0, 37, -113, 204)


def bin_of(k2, k1, N2):
    return k2 + N2 * k1


def tone_iq(bins, n, N, delay, amps=None):
    """u8 IQ of n samples whose discriminator output is y_i = sum_j A_j cos(2 pi k_j (i - delay) / N): the phase is the
    running sum of y, the bytes rint(127.5 + 100 (cos, sin)) -- deterministic, no noise, inside 27 .. 228.  sum A_j <= 2.5 keeps
    every step inside +-pi; A_j = 1 for one tone, 2 / J for J tones"""
    bins = [int(k) for k in np.atleast_1d(bins)]
    assert 1 <= len(bins) <= MAX_TONES and all(0 <= k <= N // 2 for k in bins)
    if amps is None:
        amps = [1.0] if len(bins) == 1 else [2.0 / len(bins)] * len(bins)
    assert len(amps) == len(bins) and sum(abs(a) for a in amps) <= 2.5
    i = np.arange(n, dtype=np.int64) - int(delay)
    y = np.zeros(n)
    for k, a in zip(bins, amps):
        y += a * np.cos((2.0 * np.pi / N) * ((k * i) % N))             # the argument reduced on integers: exact at any n
    phi = np.cumsum(y)
    iq = np.empty(2 * n, dtype=np.uint8)
    iq[0::2] = np.rint(127.5 + 100.0 * np.cos(phi)).astype(np.uint8)
    iq[1::2] = np.rint(127.5 + 100.0 * np.sin(phi)).astype(np.uint8)
    return iq


def bin_classes(N2):
    """[(class, (k2, k1) or NYQUIST)]: every bin class of the issue on a plan 4096 x N2, classes that need N2 >= 256 left out on
    shorter columns"""
    h, top = N2 // 2, N2 - 1
    out = [("end", (1, 0)), ("end", (2, 0)), ("end", (top, N1 - 1)), ("end", NYQUIST),
           ("self-mirror", (0, N1 // 2)), ("self-mirror", (1, N1 // 2)), ("self-mirror", (top, N1 // 2 - 1)),
           ("row 0", (0, 1)), ("row 0", (0, 63)), ("row 0", (0, 64)), ("row 0", (0, N1 - 1)),
           ("row N2/2", (h, 0)), ("row N2/2", (h, N1 // 2 - 1)), ("row N2/2", (h, N1 - 1))]
    col_ends = sorted({k2 for k2 in (1, 15, 16, 95, 96) if k2 < h} | {N2 - k2 for k2 in (96, 16, 1) if k2 < h})
    out += [("column end", (k2, 30)) for k2 in col_ends]
    out += [("block edge", (k2, k1)) for k1 in (63, 64) for k2 in (1, top)]
    out += [("no neighbour", (top, 0)), ("no neighbour", (1, N1 - 1))]  # (1, 0) and (top, 4095) are the ends above
    return out


def _k(addr, N2):
    return N1 * N2 if addr == NYQUIST else bin_of(addr[0], addr[1], N2)


@functools.lru_cache(maxsize=None)
def inputs(N2):
    """the case table of a plan: ((name, (bin, ...)), ...) -- the classes packed first-fit, in the order of bin_classes, into
    combs of at most four tones at least MIN_GAP bins apart (on short columns most bins lie closer than that: single tones)"""
    combs = []
    for cls, addr in bin_classes(N2):
        k = _k(addr, N2)
        for comb in combs:
            if len(comb) < MAX_TONES and all(abs(k - kk) >= MIN_GAP for _, _, kk in comb):
                comb.append((cls, addr, k))
                break
        else:
            combs.append([(cls, addr, k)])
    name = lambda a: "nyq" if a == NYQUIST else "%d.%d" % a
    return tuple(("+".join(name(a) for _, a, _ in comb), tuple(k for _, _, k in comb)) for comb in combs)


def classes_of(N2, bins):
    """the class names of an input's tones, in the order of the tones"""
    by_k = {_k(a, N2): c for c, a in bin_classes(N2)}
    return tuple(by_k[k] for k in bins)


def ten_second_comb():
    """the one comb of the 4096 x 2560 plan: k = 1, a row-0 bin, a row-N2/2 bin, Nc - 1"""
    N2 = PLANS["5x2^22"]["N2"]
    return "1.0+0.64+%d.2047+%d.4095" % (N2 // 2, N2 - 1), (1, bin_of(0, 64, N2), bin_of(N2 // 2, 2047, N2), N1 * N2 - 1)


def codes(iq):
    """the normalised discriminator output in float64 (oracle/float_pipeline.py)"""
    return fp.preprocess(iq)


def concentration(iq, N, bins, half_width=3):
    """the share of |rfft(normalised codes, N)|^2 within +-half_width bins of the tones, summed over the tones"""
    p = np.abs(np.fft.rfft(codes(iq), N)) ** 2
    near = np.zeros(p.size, dtype=bool)
    for k in bins:
        near[max(k - half_width, 0):k + half_width + 1] = True
    return float(p[near].sum() / p.sum())


def zero_bin_effect(a, b, N, ml, k):
    """float64: the largest change of a searched lag (|d| < ml), relative to the peak, when bin k of the first input's spectrum
    is set to zero.  k may be a sequence: one value per bin.  The change is one bin's term of the inverse transform, w / N
    Re(conj(A_k) B_k e^(2 pi i k d / N)) with w = 2 (1 at k = 0 and N / 2), evaluated at the searched lags alone (the CPU file
    holds it to the difference of two full inverses)"""
    A, B = np.fft.rfft(codes(a), N), np.fft.rfft(codes(b), N)
    d = np.arange(-(ml - 1), ml)
    peak = np.abs(np.fft.irfft(np.conj(A) * B, N)[d % N]).max()
    out = []
    for kk in np.atleast_1d(k):
        kk = int(kk)
        w = 1.0 if kk in (0, N // 2) else 2.0
        term = (w / N) * (np.conj(A[kk]) * B[kk] * np.exp(2j * np.pi * ((kk * d) % N) / N)).real
        out.append(float(np.abs(term).max() / peak))
    return out if np.ndim(k) else out[0]


# ---- the float64 statement of the 16:1 spectrum decimation (tests/test_mode_b_anchors.py, restated: the library's design) ----
def decimation_taps(N, ml, D=16, max_half=95):
    """(t, h): sinc(t / 16) x Kaiser, the attenuation the 191 taps buy on this plan, rounded to float32"""
    nc, r, mp = N // 2, N // 2 // D, ml // 2 + 2
    dw = 2 * np.pi * (r - 2 * mp) / nc
    th = min(int(np.ceil((140.0 - 8.0) / (2.285 * dw) / 2.0)), max_half)
    att = 8.0 + 2.285 * dw * 2 * th
    beta = 0.1102 * (att - 8.7)
    t = np.arange(-th, th + 1)
    h = (np.sinc(t / D) * np.i0(beta * np.sqrt(1.0 - (t / th) ** 2)) / np.i0(beta)).astype(np.float32).astype(np.float64)
    return t, h


def decimation_model_error(ta, tb, N, ml, D=16):
    """the largest error, relative to the peak, of the packed lags |m| <= ml / 2 + 2 when the Nc-point spectrum of the packed
    lags is filtered and decimated 16:1, inverted on Nc / 16 points and divided by the pass-band response -- all in float64"""
    nc, r, mp = N // 2, N // 2 // D, ml // 2 + 2
    t, h = decimation_taps(N, ml, D)
    m = np.arange(-mp, mp + 1)
    w = (h[None, :] * np.cos(2 * np.pi * t[None, :] * m[:, None] / nc)).sum(axis=1) / D
    c = np.fft.irfft(np.conj(np.fft.rfft(ta, N)) * np.fft.rfft(tb, N), N)
    q = c[0::2] + 1j * c[1::2]
    Q = np.fft.fft(q)
    idx = np.arange(r) * D
    G = np.zeros(r, dtype=complex)
    for tt, ht in zip(t, h):
        G += ht * Q[(idx + tt) % nc]
    est = (np.fft.ifft(G) * r)[m % r] / w
    ref = (q * nc)[m % nc]
    return float(np.abs(est - ref).max() / np.abs(ref).max())
