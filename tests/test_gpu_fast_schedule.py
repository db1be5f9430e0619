"""-m gpu: the engine against the CPU oracle, bit for bit, on the shapes where phase 2 of k_step_implicit_fast deals its auctions
differently: per-wave round counts for the full work items, the keywords' tails as whole Philox calls over a second prefix, and
the partial calls last (csrc/adc_fast_schedule.h; tests/test_fast_schedule_host.py checks the schedule itself on the host).  Volumes
are exact (vol_std = 0), so each case is the tile it says.  The oracle resolves auction by auction and knows no schedule: an auction
dealt twice, skipped or run past V_k moves an impression count.  Four steps per shape; each case runs in about a second."""
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


def _planes(N, K, seed, volumes):
    planes = H.implicit_params(N, K, seed=seed, mean_volume=40)
    planes[0] = np.broadcast_to(np.asarray(volumes, dtype=np.float32), (N, K))
    planes[1] = 0.0
    return planes


def _four_steps(amd, N, K, planes, budget, bid_lo=0.3, bid_hi=1.0):
    e = amd.StepEngine(N, K, model=0, seed=11, drift_enabled=False, max_days=60, loss_threshold=1e4, auto_reset=False)
    e.set_all_params(planes)
    e.reset()
    o = H.mirror_oracle(e, planes, drift_on=False, max_days=60, loss_threshold=1e4, auto_reset=False)
    bound = 0
    for _ in range(4):
        bids = o.sample_bids(bid_lo, bid_hi)
        got = e.step(bids, budget)
        ref = o.step(bids, budget)
        H.assert_step_equal(got, ref, implicit=True)
        bound += int((ref["cost_cents"].sum(axis=1) >= np.rint(np.float64(np.float32(budget)) * 100)).sum())
    e.close()
    return bound


def test_volumes_multiples_of_16(amd):
    """no tails at all: passes 1 and 2 are skipped"""
    vol = 16 * (1 + np.arange(3 * 256).reshape(3, 256) % 5)
    _four_steps(amd, 3, 256, _planes(3, 256, 601, vol), 1.0e9)


def test_volumes_17_to_31_mixed(amd):
    """every tail length 1 .. 15: tail calls 0 .. 3 and partial calls of 0 .. 3 auctions, side by side in every wave"""
    vol = 17 + (np.arange(3 * 256) * 7 % 15).reshape(3, 256)
    assert vol.min() == 17 and vol.max() == 31
    _four_steps(amd, 3, 256, _planes(3, 256, 602, vol), 1.0e9)


def test_100_live_keywords_at_30(amd):
    """3 000 auctions in the tile: items of four, still resolved by intervals (30 per live keyword); no tail calls, partials of 2"""
    vol = np.zeros((3, 256), np.int64)
    vol[0, :100] = 30
    vol[1, 156:] = 30
    vol[2, ::3][:100] = 30
    assert (vol > 0).sum(axis=1).max() <= 100
    _four_steps(amd, 3, 256, _planes(3, 256, 603, vol), 1.0e9)


def test_one_keyword_at_5000(amd):
    """312 full items of one keyword spread over every lane of the wave-rounds they fill, 8 auctions of tail in two calls"""
    vol = np.zeros((2, 256), np.int64)
    vol[0, 0] = 5000
    vol[1, 201] = 5000
    _four_steps(amd, 2, 256, _planes(2, 256, 604, vol), 1.0e9)


def test_narrow_tiles(amd):
    vol = 20 + (np.arange(5 * 70) * 11 % 90).reshape(5, 70)
    _four_steps(amd, 5, 70, _planes(5, 70, 605, vol), 1.0e9)


def test_two_tiles_the_second_partial(amd):
    vol = 5 + (np.arange(2 * 300) * 13 % 120).reshape(2, 300)
    _four_steps(amd, 2, 300, _planes(2, 300, 606, vol), 1.0e9)


def test_binding_budget_listing_variant(amd):
    """the budget binds on day 1, so the listing variant of the kernel runs from day 2 on"""
    vol = 25 + (np.arange(3 * 256) * 7 % 31).reshape(3, 256)
    n = _four_steps(amd, 3, 256, _planes(3, 256, 607, vol), 12.0, bid_lo=0.5, bid_hi=1.2)
    assert n > 0          # the budget did bind
