"""tests/reference_model.py against the CPU oracle, before tests/test_gpu_reference_edges.py lets it judge the GPU:
tdc_model at the oracle's own block size (1000) must give the oracle's bits at every lag, and the constructed tie
inputs must have the property their GPU test relies on in the REFERENCE alone -- so a GPU failure there cannot be blamed
on the model or on the input."""
import numpy as np
import pytest

from reference_model import tdc_model, tie_cases


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("tl,lags", [
    (2001, 0),                     # equal lengths: the one lag 0
    (2001, 63), (2001, 64), (2001, 257),
    (1001, 70), (2000, 70), (2001, 70),                    # 1, 1 and 2 blocks
    (1000, 5),                     # no block fits
    (2500, 2500),                  # a shape with the peak inside
])
def test_model_equals_oracle_at_block_1000(oracle, tl, lags):
    s = _rand(tl + lags, 100 * tl + lags)
    shift = lags // 2
    t = s[shift:shift + tl].copy()
    for max_lag in (20000, max(lags - 1, 1)):
        d, c, al = tdc_model(t, s, max_lag, 1000)
        want = oracle.time_domain_all_lags(t, s, max_lag)
        assert al.size == want.size == max(1, min(max_lag, lags))
        assert np.array_equal(_bits64(al), _bits64(want))
        assert (d, c) == oracle.time_domain_correlation(t, s, max_lag)
        assert tdc_model(s, t, max_lag, 1000)[:2] == (d, c)               # the shorter input is the template
    if tl > 1000 and lags > 1:
        assert d == shift


def test_model_follows_the_block_argument(oracle):
    """the block size reaches every term: a template of 2 * block + 1 samples at block 500 is two blocks of the first
    1000 samples, which the oracle sees as ONE block of 1000 when handed 1001 samples -- equal sums up to the f64
    rounding of the two block quotients, and the gain sqrt(nb * block) equal"""
    s = _rand(1001 + 80, 9)
    t = s[11:11 + 1001].copy()
    d, c, al = tdc_model(t, s, 20000, 500)
    od, oc = oracle.time_domain_correlation(t, s, 20000)
    assert d == od == 11 and abs(c - oc) <= 1e-13 * abs(oc)
    assert np.allclose(al, oracle.time_domain_all_lags(t, s, 20000), rtol=0, atol=1e-12 * abs(oc))
    # block 1: every product its own block
    d1, c1, _ = tdc_model(t[:5], s[:40], 20000, 1)
    tr, sr = t[:4], s[:40]
    want = [sum(float(np.float32(np.float32(a.real * np.float32(b.real)) + np.float32(a.imag * np.float32(b.imag))))
                for a, b in zip(tr, sr[k:k + 4])) / 4 * 2.0 for k in range(35)]
    k = int(np.argmax(np.abs(want)))
    assert d1 == k and abs(c1 - want[k]) <= 1e-15 * abs(want[k])


@pytest.mark.parametrize("case", tie_cases(), ids=lambda c: c[0])
def test_tie_inputs_tie_exactly_in_the_oracle(oracle, case):
    name, t, s, (lo, hi), sign = case
    al = oracle.time_domain_all_lags(t, s, 20000)
    assert al.size == 2560
    a = np.abs(al)
    assert sorted(np.flatnonzero(a == a.max()).tolist()) == [lo, hi]      # exactly these two lags are maximal
    assert _bits64(a[lo]) == _bits64(a[hi])
    assert al[lo] == sign * a.max() and al[hi] == a.max()
    d, c = oracle.time_domain_correlation(t, s, 20000)
    assert d == lo and c == al[lo] and (c < 0) == (sign < 0)              # the first strictly greater |corr| wins
    assert np.array_equal(_bits64(tdc_model(t, s, 20000, 1000)[2]), _bits64(al))
    assert tdc_model(t, s, 20000, 1000)[:2] == (d, c)
