"""-m gpu: the kernels that take their win-interval offsets from adc::offset_reaching (the float32 candidate verified on its
exact residual, adc_law.h) against the CPU oracle, which resolves every auction the long way: bit for bit, on the smallest
shapes that reach every path of the routine - a partial tile, a full tile, two tiles, the end cases and the float64 routine
behind the ballot (click rates of 0 and 1 make a multiplier of 0; 2^-30 and the largest float below 1 saturate it), and a
binding budget, under which the row kernel finds its clicked-win intervals with the same routine."""
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


def _run_vs_oracle(amd, N, K, planes, steps, budget, bid_lo=0.3, bid_hi=1.0):
    e = amd.StepEngine(N, K, seed=7)
    e.set_all_params(planes)
    e.reset()
    o = H.mirror_oracle(e, planes)
    bound = 0
    for _ in range(steps):
        bids = o.sample_bids(bid_lo, bid_hi)
        got, ref = e.step(bids, budget), o.step(bids, budget)
        H.assert_step_equal(got, ref, implicit=True)
        bound += int((ref["cost_cents"].sum(axis=1) >= np.rint(np.float64(np.float32(budget)) * 100)).sum())
    e.close()
    return bound


@pytest.mark.parametrize("N,K", [(3, 70), (2, 256), (2, 300)])
def test_dense_tiles_match_oracle(amd, N, K):
    """one partial tile, one full tile, two tiles: the benchmark's law at the benchmark's volume (every tile dense)"""
    _run_vs_oracle(amd, N, K, H.implicit_params(N, K, seed=900 + K), steps=3, budget=1.0e9)


def test_end_cases_and_the_float64_routine(amd):
    """one env x 64 keywords, click rates forced to 0, 1, the largest float below 1 and 2^-30 in turn: multipliers of 0 (the float64
    routine, with the whole wave) and saturated ones, thresholds of 0, 4, 2^32 - 256 and 2^32; bids wide enough for bounds of 0 and 2^24"""
    planes = H.implicit_params(1, 64, seed=964)
    rates = np.array([0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 2.0**-30], np.float32)
    planes[4, 0, :] = rates[np.arange(64) % 4]
    planes[4, 0, 40:48] = H.implicit_params(1, 64, seed=965)[4, 0, 40:48]          # (and ordinary lanes in the same wave)
    _run_vs_oracle(amd, 1, 64, planes, steps=3, budget=1.0e9, bid_lo=0.01, bid_hi=2.0)


def test_binding_budget_matches_oracle(amd):
    """3 envs x 70 keywords with a budget that binds: k_step_exact_rows (clicked_win_interval) and the rest-of-day kernels after it"""
    planes = H.implicit_params(3, 70, seed=970)
    assert _run_vs_oracle(amd, 3, 70, planes, steps=4, budget=25.0, bid_lo=0.5, bid_hi=1.2) > 0
