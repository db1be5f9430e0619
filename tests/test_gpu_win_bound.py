"""-m gpu: the engine against the CPU oracle, bit for bit, on the shapes where a keyword's win intervals come from
adc::lower_bound_v on the device (its own exp2 / rcp in the window's estimate, ballots around the rare stages).  The oracle
resolves every auction from the sampled competitor bid and knows nothing of intervals, so a bound that is off by one v shows
up as a win or a click that moved.  Four steps per shape; each case runs in about a second."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _four_steps(amd, N, K, planes, budget, bid_lo=0.3, bid_hi=1.0):
    e = amd.StepEngine(N, K, model=0, seed=7, drift_enabled=False, max_days=60, loss_threshold=1e4, auto_reset=False)
    e.set_all_params(planes)
    e.reset()
    o = H.mirror_oracle(e, planes, drift_on=False, max_days=60, loss_threshold=1e4, auto_reset=False)
    rerun = 0
    for _ in range(4):
        bids = o.sample_bids(bid_lo, bid_hi)
        got = e.step(bids, budget)
        ref = o.step(bids, budget)
        H.assert_step_equal(got, ref, implicit=True)
        rerun += int((ref["cost_cents"].sum(axis=1) >= np.rint(np.float64(np.float32(budget)) * 100)).sum())
    e.close()
    return rerun


def test_full_dense_tile(amd):
    _four_steps(amd, 3, 256, H.implicit_params(3, 256, seed=501, mean_volume=40), 1.0e9)


def test_narrow_partial_tile(amd):
    _four_steps(amd, 5, 70, H.implicit_params(5, 70, seed=502, mean_volume=60), 1.0e9)


def test_binding_budget_row_and_rest_of_day_kernels(amd):
    n = _four_steps(amd, 3, 256, H.implicit_params(3, 256, seed=503, mean_volume=40), 12.0, bid_lo=0.5, bid_hi=1.2)
    assert n > 0          # the budget did bind: the row / rest-of-day kernels set up their keywords' intervals


def test_edge_laws(amd):
    """|scale| 0, denormal, 1e-6 and huge, a negative scale, NaN and +-inf in loc or scale, a negative and a huge loc - keywords
    whose window is worthless, next to ordinary ones in the same waves (the rare stages run with some lanes idle)"""
    planes = H.implicit_params(2, 64, seed=504, mean_volume=40)
    loc, scale = planes[2], planes[3]
    scale[0, 0:3] = 0.0
    scale[0, 3:6] = np.float32(1e-40)
    scale[0, 6:9] = np.float32(1e-6)
    scale[0, 9:12] = np.float32(1e30)
    scale[0, 12:15] = np.inf
    scale[0, 15:18] = np.nan
    scale[0, 18:21] = -0.08
    scale[0, 21:24] = 50.0
    loc[1, 0:3] = np.nan
    loc[1, 3:6] = np.inf
    loc[1, 6:9] = -np.inf
    loc[1, 9:12] = -0.4
    loc[1, 12:15] = np.float32(1e7)
    loc[1, 15:18] = 0.0
    scale[1, 15:18] = 0.0
    loc[1, 18:21] = np.nan
    scale[1, 18:21] = np.nan
    _four_steps(amd, 2, 64, planes, 1.0e9, bid_lo=0.01, bid_hi=1.5)
