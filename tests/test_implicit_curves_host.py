"""-m "not gpu": the references the IMPLICIT curve tests (test_gpu_implicit_curves.py) stand on - the oracle's batch METRIC sampler,
the exact estimator (helpers.exact_implicit_curve) - and the argument checks adc_bid_curves_from_samples makes before any HIP call."""
import numpy as np
import pytest

from oracle import capi as orc, ref_numpy as rn
from tests import helpers as H

NOTEBOOK = np.arange(0.01, 3.00, 0.01)


@pytest.mark.parametrize("key,tick,k,loc,scale", [(0x0123456789ABCDEF, 0, 0, 0.55, 0.08), (0xFEDCBA9876543210, 17, 5, 12.0, 2.0),
                                                  (1, 4000000000, 1023, 0.0, 2.0e7)])
@pytest.mark.parametrize("n", [1, 6, 257])
def test_batch_metric_sampler_is_the_per_sample_route(key, tick, k, loc, scale, n):
    got = orc.metric_competitor_cents(key, tick, k, n, loc, scale)
    L = orc.lib()
    want = []
    for q in range((n + 3) // 4):
        w = orc.philox([q, 6, k, tick], [key & 0xFFFFFFFF, key >> 32])          # ST_METRIC = 6
        want += [L.orc_competitor_cents_from_v(int(x) >> 8, loc, scale) for x in w]
    assert got.tolist() == want[:n]


def _check_against_numpy(cents, grid):
    ir, cpc = H.exact_implicit_curve(cents, grid)
    rir, rcpc = rn.implicit_bid_cpc_impressions(np.asarray(cents, np.float64).reshape(1, -1) / 100.0, grid)
    assert np.array_equal(ir, rir)
    np.testing.assert_allclose(cpc, rcpc, rtol=1e-12)
    return ir, cpc


def test_exact_estimator_on_the_reference_samples(golden):
    g = golden("g5_metrics.json")
    grid = np.array(g["bid_array"], dtype=np.float64)
    for c in g["bid_curves"]:
        ir, cpc = _check_against_numpy(np.array(c["samples_cents"], dtype=np.int64), grid)
        assert ir.tolist() == c["impression_rates"]
        np.testing.assert_allclose(cpc, c["cpc"], rtol=1e-12)


@pytest.mark.parametrize("n", [1, 2, 5, 64, 2049])
def test_exact_estimator_on_synthetic_samples(n):
    rng = np.random.default_rng(n)
    grids = [NOTEBOOK, np.round(NOTEBOOK, 2), np.arange(0.002, 2.5, 0.002), rng.permutation(NOTEBOOK),
             np.array([0.0, -0.01, -0.05, 0.1, 20.46])]
    for cents in (orc.metric_competitor_cents(99, 3, 7, n, 0.55, 0.1), rng.integers(0, 400, n), np.full(n, 100),
                  rng.integers(0, 2046, n), orc.metric_competitor_cents(5, 0, 1, n, 0.0, 2.0e7)):
        for grid in grids:
            _check_against_numpy(cents, grid)
    # the float-dollar comparison: the notebooks' "0.10" (0.09999999999999999) does not take a 10-cent sample
    ir, cpc = H.exact_implicit_curve([10, 30], NOTEBOOK[:10])
    assert ir[9] == 0.0 and cpc[9] == 0.1 and ir[8] == 0.0
    assert H.exact_implicit_curve([10, 30], [0.1])[0][0] == 0.5


def _from_samples(cents, grid):
    from adcraft_amd import _ffi
    s = np.ascontiguousarray(cents, dtype=np.int32)
    g = np.ascontiguousarray(grid, dtype=np.float64)
    ir, cpc = np.zeros(max(g.size, 1)), np.zeros(max(g.size, 1))
    rc = _ffi.lib().adc_bid_curves_from_samples(0, s.ctypes.data, s.size, g.ctypes.data, g.size, ir.ctypes.data, cpc.ctypes.data)
    return rc, (_ffi.lib().adc_last_error() or b"").decode()


@pytest.mark.parametrize("case", ["negative_sample", "nan_bid", "inf_bid", "minus_inf_bid", "bid_above_ceiling", "bid_30",
                                  "too_many_samples"])
def test_bid_curves_from_samples_refuses_before_any_hip_call(case):
    """(no GPU here: an argument that got as far as a HIP call would come back as ADC_EHIP, not ADC_EINVAL)"""
    from adcraft_amd import _ffi
    cents, grid = np.arange(1, 200, dtype=np.int32), NOTEBOOK.copy()
    want = "bid grid"
    if case == "negative_sample":
        cents[50], want = -3, "negative"
    elif case == "nan_bid":
        grid[7] = np.nan
    elif case == "inf_bid":
        grid[7] = np.inf
    elif case == "minus_inf_bid":
        grid[7] = -np.inf
    elif case == "bid_above_ceiling":
        grid[-1] = 20.47
    elif case == "bid_30":
        grid[-1] = 30.0
    elif case == "too_many_samples":
        cents, want = np.zeros((1 << 20) + 1, dtype=np.int32), "2^20"
    rc, msg = _from_samples(cents, grid)
    assert rc == _ffi.ADC_EINVAL and want in msg, (rc, msg)
