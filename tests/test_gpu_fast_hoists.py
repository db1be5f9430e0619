"""-m gpu: the engine against the CPU oracle, bit for bit, on the shapes that reach what the dense pass of k_step_implicit_fast
hoists out of its stages: the Philox call from the folded tick ^ key_hi word (stages A and B), the call index carried from call
to call (full items, tail calls, the partial call, up to a keyword's 2^18 calls), the clicked win's price without its clamp, and
the law records found by the accumulators' offset added to itself.  The oracle draws every auction with the plain adc draw and
prices it with the clamp; impressions, clicks, conversions, cost, revenue and the env totals (reward, cumulative profit) must
agree on each of three days, auto-reset off.  tests/test_law_hoists_host.py checks the routines themselves on the host."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

VOLUME_MAX = 1 << 20            # adc::kVolumeMax


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _three_days(amd, N, K, planes, budget=1.0e9, bids=None, bid_lo=0.3, bid_hi=1.0):
    """returns (env-days on which the budget bound, clicks seen)"""
    e = amd.StepEngine(N, K, model=0, seed=23, drift_enabled=False, max_days=60, loss_threshold=1e6, auto_reset=False)
    e.set_all_params(planes)
    e.reset()
    o = H.mirror_oracle(e, planes, drift_on=False, max_days=60, loss_threshold=1e6, auto_reset=False)
    bound = clicks = 0
    for _ in range(3):
        b = o.sample_bids(bid_lo, bid_hi)
        if bids is not None:
            b = np.full_like(b, bids)
        got = e.step(b, budget)
        ref = o.step(b, budget)
        H.assert_step_equal(got, ref, implicit=True)
        bound += int((ref["cost_cents"].sum(axis=1) >= np.rint(np.float64(np.float32(budget)) * 100)).sum())
        clicks += int(ref["clicks"].sum())
    e.close()
    return bound, clicks


def test_cfg2_law_three_envs(amd):
    _, clicks = _three_days(amd, 3, 256, H.implicit_params(3, 256, seed=701))
    assert clicks > 64 * 3 * 4          # (every wave drained full batches of clicked wins)


def test_narrow_tiles(amd):
    _three_days(amd, 2, 70, H.implicit_params(2, 70, seed=702))


def test_two_tiles_the_last_ragged(amd):
    _three_days(amd, 2, 300, H.implicit_params(2, 300, seed=703))


def test_one_keyword_at_the_volume_cap(amd):
    """2^20 auctions of one keyword: call indices up to 2^18 - 1 in the full items, and the tail paths of the others"""
    planes = H.implicit_params(2, 256, seed=704)
    planes[0][0, 17] = planes[0][1, 255] = float(VOLUME_MAX)
    planes[1][0, 17] = 0.0              # exactly the cap in env 0; in env 1 the draw is clipped to it or falls below
    _three_days(amd, 2, 256, planes)


def test_bids_of_ten_million_dollars(amd):
    """the bid is the 1e9-cent cap: everything is won, at every price the law gives"""
    _, clicks = _three_days(amd, 2, 256, H.implicit_params(2, 256, seed=705), bids=1.0e7)
    assert clicks > 0


def test_bids_of_zero(amd):
    """a bid of 0 counts as one cent: only a competitor at 0 cents loses to it"""
    _three_days(amd, 2, 256, H.implicit_params(2, 256, seed=706), bids=0.0)


def test_mean_volume_3_is_the_direct_form(amd):
    """too few auctions per keyword for intervals: the tile is resolved auction by auction (DIRECT), clamp and all"""
    _, clicks = _three_days(amd, 2, 256, H.implicit_params(2, 256, seed=707, mean_volume=3))
    assert clicks > 0


def test_binding_budget_listing_variant(amd):
    """the budget binds from day 1, so the listing variant of the kernel runs from day 2 on"""
    bound, _ = _three_days(amd, 4, 256, H.implicit_params(4, 256, seed=708), budget=12.0, bid_lo=0.5, bid_hi=1.2)
    assert bound > 0                    # the budget did bind
