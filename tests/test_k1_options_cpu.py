"""CPU: the oracle of tdoa_params' optional K1 steps at their edges.

- ob_smooth_codes (k1_smooth = W) against float_pipeline.lowpass, the float64 statement of processor.go:270-296's centred,
  edge-truncated moving average: half-window W // 2 (even and odd W share it), round half up, for the widths and the short
  lengths tests/test_gpu_k1_options.py runs on the device -- windows shorter than the half-window included.
- ob_envelope_class (k1_gate) exactly at its threshold 100 M == 65025 n, and one step (M + 8) above it, on captures built
  for that (threshold_capture)."""
import numpy as np
import pytest

from oracle import float_pipeline as fp

WIDTHS = (2, 3, 4, 11, 64, 2001)


def edge_lengths(window):
    """the window lengths that hit k_k1_smooth's edges for width `window`: a sample or two, the half-window h = W // 2 and its
    neighbours, the kernel's 2048-sample chunk boundary, a few chunks"""
    h = window // 2
    return sorted({n for n in (1, 2, 7, h - 1, h, h + 1, 2047, 2048, 2049, 16383, 16385) if n >= 1})


# every sample's m = (2I - 255)^2 + (2Q - 255)^2 is 2 (mod 8), so 100 M == 65025 n needs n to be a multiple of 32.  A block of
# 32 samples at the threshold: 30 x 650 + 26 + 1282 = 20808 = 65025 * 32 / 100.  One step above: 26 -> 34 (M + 8).
_THRESHOLD_BLOCK = [(25, 5)] * 30 + [(5, 1), (29, 21)]      # (2I - 255, 2Q - 255): m = 650, 26, 1282
_ABOVE = (5, 3)                                               # m = 34


def threshold_capture(n, above=False, seed=0):
    """u8 IQ of n samples (n % 32 == 0) whose power sum M is exactly 65025 n / 100 (mean power 0.01: the envelope class,
    ob_envelope_class's equality), or exactly 8 more (above: one sample of the first block moved from m = 26 to 34 -- the
    discriminator class).  Each 32-sample block holds the same multiset of m in a seeded order, each sample with random
    signs and I/Q order, so the phase and the envelope both move."""
    assert n % 32 == 0
    rng = np.random.default_rng(seed)
    ab = np.array(_THRESHOLD_BLOCK * (n // 32), dtype=np.int64).reshape(n // 32, 32, 2)
    if above:
        ab[0, 30] = _ABOVE
    ab = np.take_along_axis(ab, rng.permuted(np.tile(np.arange(32), (n // 32, 1)), axis=1)[:, :, None], axis=1).reshape(n, 2)
    swap = rng.integers(0, 2, size=n).astype(bool)
    ab[swap] = ab[swap][:, ::-1]
    ab *= np.where(rng.integers(0, 2, size=(n, 2)) == 1, 1, -1)
    return ((ab + 255) // 2).astype(np.uint8).reshape(-1)


@pytest.mark.parametrize("window", WIDTHS)
def test_smooth_codes_vs_the_float_moving_average(oracle, window):
    """ob_smooth_codes == floor(lowpass + 1/2) (round half up, so within 0.5 of processor.go's average) on phase codes of a
    delayed-FM capture and of random bytes (codes over the whole 24-bit range, sums of either sign)"""
    n_max = 16385
    fm = oracle.simulate_delayed_fm(n_max, 0, 9, 1)
    noise = np.random.default_rng(window).integers(0, 256, size=2 * n_max, dtype=np.uint8)
    for raw in (fm, noise):
        for n in edge_lengths(window):
            code = oracle.b_discriminate(raw[:2 * n])
            lp = oracle.b_smooth_codes(code, window).astype(np.float64)
            want = fp.lowpass(code.astype(np.float64), window)
            assert np.abs(lp - want).max() <= 0.5, (window, n)
            assert np.array_equal(lp, np.floor(want + 0.5)), (window, n)
            # the half-window is W // 2: an even width and the odd width above it are the same filter
            if window % 2 == 0:
                assert np.array_equal(oracle.b_smooth_codes(code, window + 1), lp.astype(np.int32)), (window, n)


def test_smooth_codes_half_window_by_hand(oracle):
    """W = 4 and W = 5 both average code[i-2 .. i+2]; W = 3 averages code[i-1 .. i+1]: on a ramp with one spike"""
    code = np.arange(10, dtype=np.int32) * 8
    code[5] = 1000
    for w, h in ((3, 1), (4, 2), (5, 2)):
        want = [int(np.floor(code[max(i - h, 0):i + h + 1].sum() / len(code[max(i - h, 0):i + h + 1]) + 0.5)) for i in range(10)]
        assert oracle.b_smooth_codes(code, w).tolist() == want, w


@pytest.mark.parametrize("n", [32, 2048, 16416, 2_000_000])
def test_envelope_class_at_its_threshold(oracle, n):
    """100 M == 65025 n is the envelope class (mean power <= 0.01), M + 8 is not; float_pipeline.mean_power sits on 0.01
    within rounding there (its float64 `<= 0.01` may go either way at equality, which is why the gate is integer)"""
    at, above = threshold_capture(n, seed=n), threshold_capture(n, above=True, seed=n)
    m_at, m_above = oracle.b_power_sum(at), oracle.b_power_sum(above)
    assert 100 * m_at == 65025 * n and m_above == m_at + 8
    assert oracle.b_envelope_class(m_at, n) == 1 and oracle.b_envelope_class(m_above, n) == 0
    assert oracle.b_envelope_class(m_at - 8, n) == 1
    assert oracle.b_preprocess_gate(at)[2] == 1 and oracle.b_preprocess_gate(above)[2] == 0
    assert abs(fp.mean_power(at) - 0.01) < 1e-12
