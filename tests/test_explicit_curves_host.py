"""-m "not gpu": the host twin of the EXPLICIT bid curves (adc_explicit_curve_host) - the law k_explicit_curves evaluates on the
device - against threshold_sigmoid, a numpy restatement of the median cost, and the reference's estimator in distribution;
and experiment_metrics.get_explicit_kw_bid_cpc_impressions against the reference's definition."""
import numpy as np
import pytest
from scipy import stats

from adcraft_amd import _ffi, experiment_metrics as em
from adcraft_amd.engine import explicit_curve_host

GRIDS = [np.arange(0.01, 3.00, 0.01), np.arange(0.05, 2.0, 0.05), np.arange(0.002, 0.6, 0.002)]


def _ulps(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.abs(x - y) / np.spacing(np.maximum(np.abs(x), np.abs(y)))


def _median_cost(z_lo, z_hi, bids):
    """np.median of the clamped costs of the two middle normals (src/lib.rs:54-67), float64"""
    sq = np.sqrt(bids)
    mu, sigma = sq / 4.0 + 2.2, 1e-10 + sq / 6.0
    c_lo, c_hi = np.clip(mu + sigma * np.float64(z_lo), 0.0, 4.4), np.clip(mu + sigma * np.float64(z_hi), 0.0, 4.4)
    return (c_lo + c_hi) * 0.5


def test_impression_rate_is_threshold_sigmoid():
    lib = _ffi.lib()
    rng = np.random.default_rng(11)
    for grid in GRIDS:
        for _ in range(20):
            a, b = np.float32(rng.random() * 1.5), np.float32(rng.beta(5, 5) * 25)
            ir, _, _ = explicit_curve_host(int(rng.integers(2**63)), 3, 7, 64, a, b, grid)
            want = np.array([lib.adc_threshold_sigmoid(float(x), float(np.float32(0.05)), float(a), float(b)) for x in grid])
            assert (_ulps(ir, want) <= 2).all()
            assert ((ir >= 0.0) & (ir <= 1.0)).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 101, 2048, 5000])
def test_cpc_is_the_median_of_the_two_middle_costs_bit_for_bit(n):
    rng = np.random.default_rng(n)
    for grid in GRIDS:
        for _ in range(5):
            _, cpc, (z_lo, z_hi) = explicit_curve_host(int(rng.integers(2**63)), int(rng.integers(100)), int(rng.integers(4096)), n,
                                                       0.5, 8.0, grid)
            assert z_lo <= z_hi and (n % 2 == 0 or z_lo == z_hi)
            assert np.array_equal(cpc, _median_cost(z_lo, z_hi, grid))
            assert ((cpc >= 0.0) & (cpc <= 4.4)).all()


def _ks_p(x, y):
    return stats.ks_2samp(x, y).pvalue


@pytest.mark.parametrize("n", [2048, 101])
def test_cpc_has_the_reference_estimators_distribution(n):
    """the median of n costs, src/lib.rs:54-67 with numpy's own normals, vs the twin's cpc over 20 000 keys (two-sample KS)"""
    bids = np.array([0.05, 0.5, 2.0])
    keys = 20000
    rng = np.random.default_rng(1000 + n)
    twin = np.empty((keys, bids.size))
    for i, key in enumerate(rng.integers(1, 2**63, keys)):
        twin[i] = explicit_curve_host(int(key), 0, int(i % 256), n, 0.5, 8.0, bids)[1]
    sq = np.sqrt(bids)
    ref = np.empty((keys, bids.size))
    for s in range(0, keys, 1000):
        z = rng.standard_normal((1000, n))
        for j, b in enumerate(bids):
            ref[s:s + 1000, j] = np.median(np.clip(sq[j] / 4.0 + 2.2 + z * (1e-10 + sq[j] / 6.0), 0.0, 4.4), axis=1)
    for j in range(bids.size):
        assert _ks_p(twin[:, j], ref[:, j]) > 1e-3, (n, bids[j])


class _StubKeyword:
    """an ExplicitKeyword's two samplers: a sigmoid impression rate and n costs per call"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.calls = []

    def impression_rate(self, b):
        return float(1.0 / (1.0 + np.exp(-7.0 * (b - 0.8))))

    def cost_per_buyside_click(self, b, n):
        self.calls.append((b, n))
        return np.clip(np.sqrt(b) / 4 + 2.2 + self.rng.standard_normal(n) * (1e-10 + np.sqrt(b) / 6), 0, 4.4)


def test_get_explicit_kw_bid_cpc_impressions_is_the_reference_definition():
    bids = np.arange(0.01, 3.00, 0.25)
    ir, cpc = em.get_explicit_kw_bid_cpc_impressions(_StubKeyword(4), bids, n_samples=64)
    ref_kw = _StubKeyword(4)
    want_ir = np.array([ref_kw.impression_rate(b) for b in bids])
    want_cpc = np.array([np.median(ref_kw.cost_per_buyside_click(b, 64)) for b in bids])
    assert np.array_equal(ir, want_ir) and np.array_equal(cpc, want_cpc)
    kw = _StubKeyword(5)
    em.get_explicit_kw_bid_cpc_impressions(kw, bids)
    assert kw.calls == [(b, 2048) for b in bids]                      # n_samples defaults to the reference's 2048


def test_twin_rejects_bad_arguments():
    lib = _ffi.lib()
    g = np.array([1.0])
    out = np.zeros(1)
    for n in (0, -1, (1 << 20) + 1):
        assert lib.adc_explicit_curve_host(1, 0, 0, n, 0.05, 0.5, 8.0, g.ctypes.data, 1, out.ctypes.data, out.ctypes.data, None) != 0
    assert lib.adc_explicit_curve_host(1, 0, -1, 8, 0.05, 0.5, 8.0, g.ctypes.data, 1, out.ctypes.data, out.ctypes.data, None) != 0
