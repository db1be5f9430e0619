"""-m gpu: the engine against the CPU oracle, bit for bit, where k_step_implicit_fast deals no work to a keyword that cannot win
(adc_law.h fast_keyword_is_dead: phase 1 leaves it out of the items, tail calls and partial calls) and where its clicked-win queue
is at an end of its range: every word a push, no push ever, a drain after every word.  Volumes are exact (vol_std = 0) and the
competitor's law is the same for every keyword - loc 0.60, scale 0.02: its price stays within 27 .. 93 cents - so a bid of 5 cents (or
0: "no bid") is dead, a bid of 60 cents wins about every other auction and a bid of 5 dollars wins them all.  The oracle resolves
auction by auction and knows neither intervals nor a schedule.  Four steps per case; 3 envs x 256 keywords (tiles of 16 keywords: a
handful of envs is spread over the chip) unless the case says otherwise; each case runs in about a second."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

DEAD, LIVE, TOP = 0.05, 0.60, 5.00


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _planes(N, K, seed, volumes, bctr=None):
    planes = H.implicit_params(N, K, seed=seed, mean_volume=40)
    planes[0] = np.broadcast_to(np.asarray(volumes, dtype=np.float32), (N, K))
    planes[1] = 0.0
    planes[2] = 0.60
    planes[3] = 0.02
    if bctr is not None:
        planes[4] = bctr
    return planes


def _four_steps(amd, N, K, planes, bids, budget=1.0e9):
    """bids: [N, K] dollars, or a function of the step; returns the oracle's four days"""
    e = amd.StepEngine(N, K, model=0, seed=11, drift_enabled=False, max_days=60, loss_threshold=1e4, auto_reset=False)
    e.set_all_params(planes)
    e.reset()
    o = H.mirror_oracle(e, planes, drift_on=False, max_days=60, loss_threshold=1e4, auto_reset=False)
    days = []
    for step in range(4):
        b = np.ascontiguousarray(bids(step) if callable(bids) else bids, dtype=np.float32)
        got = e.step(b, budget)
        ref = o.step(b, budget)
        H.assert_step_equal(got, ref, implicit=True)
        days.append({k: np.array(v) for k, v in ref.items() if k in ("impressions", "clicks", "conversions", "cost_cents")})
    e.close()
    return days


def _mixed_volumes(N, K):
    return np.array([0, 5, 17, 31, 128])[(np.arange(N * K) % 5).reshape(N, K)]


def test_every_keyword_dead(amd):
    """phase 2 has no item at all, and every output is zero"""
    vol = 25 + (np.arange(3 * 256) * 7 % 31).reshape(3, 256)
    for day in _four_steps(amd, 3, 256, _planes(3, 256, 701, vol), np.full((3, 256), DEAD)):
        assert not day["impressions"].any() and not day["clicks"].any() and not day["cost_cents"].any()


def test_no_bid_is_dead(amd):
    """the bid 0 (1 cent to the engine) in every keyword"""
    vol = 25 + (np.arange(3 * 256) * 7 % 31).reshape(3, 256)
    for day in _four_steps(amd, 3, 256, _planes(3, 256, 702, vol), np.zeros((3, 256))):
        assert not day["impressions"].any()


def test_one_live_keyword_at_5000(amd):
    vol = np.full((3, 256), 40)
    bids = np.full((3, 256), DEAD)
    for env, kw in enumerate((0, 201, 255)):
        vol[env, kw] = 5000
        bids[env, kw] = LIVE
    days = _four_steps(amd, 3, 256, _planes(3, 256, 703, vol), bids)
    assert all((d["impressions"] > 0).sum() == 3 for d in days)


def test_dead_and_live_alternating(amd):
    """volumes 0 / 5 / 17 / 31 / 128 against dead / live: every combination, tails and partial calls of dead keywords included; the
    roles swap from day to day"""
    vol = _mixed_volumes(3, 256)
    live_even = np.where(np.arange(256) % 2 == 0, LIVE, DEAD)[None, :].repeat(3, axis=0)
    live_odd = np.where(np.arange(256) % 2 == 1, LIVE, DEAD)[None, :].repeat(3, axis=0)
    days = _four_steps(amd, 3, 256, _planes(3, 256, 704, vol), lambda step: live_even if step % 2 == 0 else live_odd)
    assert all(d["impressions"].any() for d in days)


def test_full_tiles_dead_and_live(amd):
    """256 envs: tiles of 256 keywords, the kernel of the throughput configuration; a third of the keywords dead, an env all dead,
    an env with one live keyword"""
    N, K = 256, 256
    vol = 20 + (np.arange(N * K) * 11 % 50).reshape(N, K)
    rng = np.random.default_rng(705)
    bids = np.where(rng.random((N, K)) < 1.0 / 3.0, DEAD, np.rint(rng.uniform(30, 100, (N, K))) / 100.0)
    bids[7] = DEAD
    bids[8] = DEAD
    bids[8, 77] = LIVE
    days = _four_steps(amd, N, K, _planes(N, K, 705, vol), bids)
    assert not days[0]["impressions"][7].any() and (days[0]["impressions"][8] > 0).sum() == 1


def test_direct_tile_with_zero_bids(amd):
    """3 auctions per keyword: resolved auction by auction from the sampled competitor bid; no bid in every fourth column"""
    bids = np.full((3, 256), LIVE)
    bids[:, ::4] = 0.0
    days = _four_steps(amd, 3, 256, _planes(3, 256, 706, np.full((3, 256), 3)), bids)
    assert all(not d["impressions"][:, ::4].any() and d["impressions"].any() for d in days)


def test_every_word_a_clicked_win(amd):
    """click rate 1 and a bid far above the competitor, 64 auctions per keyword: every word is pushed, the queue drains after
    every word, and the day's impressions are all clicked wins"""
    for day in _four_steps(amd, 3, 256, _planes(3, 256, 707, np.full((3, 256), 64), bctr=1.0), np.full((3, 256), TOP)):
        assert (day["impressions"] == 64).all() and (day["clicks"] == 64).all()


def test_every_word_an_unclicked_win(amd):
    """click rate 0: no push ever, and the day's impressions are all unclicked wins"""
    for day in _four_steps(amd, 3, 256, _planes(3, 256, 708, np.full((3, 256), 64), bctr=0.0), np.full((3, 256), TOP)):
        assert (day["impressions"] == 64).all() and not day["clicks"].any()


@pytest.mark.parametrize("bctr", [0.0, 0.01])
def test_rare_clicks(amd, bctr):
    """click rate 0 and 0.01 at bids that win about every other auction, dead keywords in between"""
    vol = _mixed_volumes(3, 256) + 40
    bids = np.where(np.arange(256) % 3 == 0, DEAD, LIVE)[None, :].repeat(3, axis=0)
    days = _four_steps(amd, 3, 256, _planes(3, 256, 709, vol, bctr=bctr), bids)
    assert all(d["impressions"].any() for d in days)


@pytest.mark.parametrize("K", [100, 40])
def test_narrow_tiles(amd, K):
    vol = 20 + (np.arange(5 * K) * 11 % 90).reshape(5, K)
    bids = np.where(np.arange(5 * K).reshape(5, K) % 3 == 1, DEAD, LIVE)
    _four_steps(amd, 5, K, _planes(5, K, 710, vol), bids)


def test_two_tiles_the_second_partial(amd):
    vol = 5 + (np.arange(2 * 300) * 13 % 120).reshape(2, 300)
    bids = np.where(np.arange(2 * 300).reshape(2, 300) % 4 == 2, DEAD, LIVE)
    bids[1, 256:] = DEAD            # (the partial tile of env 1: all dead)
    _four_steps(amd, 2, 300, _planes(2, 300, 711, vol), bids)


def test_binding_budget_listing_variant(amd):
    """the budget binds on day 1, so the listing variant of the kernel runs from day 2 on (built as tests/test_gpu_fast_schedule.py
    builds it: the benchmark's competitor laws, bids of 0.5 .. 1.2), here with every fifth keyword left unbid"""
    N, K = 3, 256
    vol = 25 + (np.arange(N * K) * 7 % 31).reshape(N, K)
    planes = H.implicit_params(N, K, seed=607, mean_volume=40)
    planes[0] = vol.astype(np.float32)
    planes[1] = 0.0
    planes[2, :, ::5] = 0.60
    planes[3, :, ::5] = 0.02
    rng = np.random.default_rng(712)

    def bids(step):
        b = np.rint(rng.uniform(50, 120, (N, K))) / 100.0
        b[:, ::5] = 0.0
        return b
    days = _four_steps(amd, N, K, planes, bids, budget=12.0)
    bound = sum(int((d["cost_cents"].sum(axis=1) >= 1200).sum()) for d in days)
    assert bound > 0          # the budget did bind
    assert all(not d["impressions"][:, ::5].any() for d in days)
