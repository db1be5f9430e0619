"""-m gpu: the engine against the CPU oracle, bit for bit on every output, where k_step_implicit_fast adds a clicked win's price and
revenue with one atomic (a tile whose keyword-days all keep cost and revenue below 2^32 cents: adc_law.h fast_money_packs) and where
it may not: a keyword bid at $50 000 with 5 000 auctions, revenue laws of 1e7 and 1e6 dollars (a day's revenue then really passes
2^32 cents), a NaN law, and a pair of laws on either side of the bound, found with the host predicate.  The oracle keeps cost and
revenue apart in 64 bits and knows no tiles.  Four steps per case.  A handful of envs is spread over the chip in tiles of 16 keywords
(k_step_implicit_fast<true>); the cases that say tile_kw = 256 ask for the throughput configuration's tiles of 256 keywords
(<false>) through ADCRAFT_FAST_TILE_KW, and each case checks the name of the kernel that ran."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

P_VOL, P_VOL_STD, P_LOC, P_SCALE, P_BCTR, P_SCTR, P_MU, P_SD = range(8)


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(scope="module")
def packs():
    """the host predicate: packs(V, bid, mu, sd) -> bool"""
    from oracle import build as obuild
    lib = C.CDLL(obuild.build_shims_host())
    vp = C.c_void_p
    lib.adc_fast_money_packs_host.argtypes = [C.c_int64, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    lib.adc_fast_money_packs_host.restype = C.c_int

    def f(V, bid, mu, sd):
        V, bid, mu, sd = np.array([V], np.int32), np.array([bid], np.float32), np.array([mu], np.float32), np.array([sd], np.float32)
        out, bid_c, r_max = np.zeros(1, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int64)
        assert lib.adc_fast_money_packs_host(1, V.ctypes.data, bid.ctypes.data, mu.ctypes.data, sd.ctypes.data, None, 0, out.ctypes.data,
                                             bid_c.ctypes.data, r_max.ctypes.data, None, None) == 0
        return bool(out[0])
    return f


def _bids(N, K, seed, lo=0.3, hi=1.0):
    return (np.rint(np.random.default_rng(seed).uniform(lo, hi, (N, K)) * 100.0) / 100.0).astype(np.float32)


def _four_steps(amd, monkeypatch, N, K, planes, bids, budget=1.0e9, tile_kw=None, variant=None, kernel="k_step_implicit_fast<true>"):
    if tile_kw is not None:
        monkeypatch.setenv("ADCRAFT_FAST_TILE_KW", str(tile_kw))
    if variant is not None:
        monkeypatch.setenv("ADCRAFT_FAST_VARIANT", str(variant))
    e = amd.StepEngine(N, K, model=0, seed=11, drift_enabled=False, max_days=60, loss_threshold=1e12, auto_reset=False)
    e.set_all_params(planes)
    e.reset()
    o = H.mirror_oracle(e, planes, drift_on=False, max_days=60, loss_threshold=1e12, auto_reset=False)
    days, kernels = [], []
    for step in range(4):
        b = np.ascontiguousarray(bids(step) if callable(bids) else bids, dtype=np.float32)
        got = e.step(b, budget)
        ref = o.step(b, budget)
        kernels.append(e.step_kernel_name())
        H.assert_step_equal(got, ref, implicit=True)
        days.append({k: np.array(v) for k, v in ref.items() if k in ("impressions", "clicks", "conversions", "cost_cents", "revenue_cents")})
    e.close()
    assert kernels[0] == kernel, kernels
    assert all(k.startswith(kernel[:-1]) for k in kernels), kernels
    return days, kernels


def _ordinary(N, K, seed, mean_volume=40):
    return H.implicit_params(N, K, seed=seed, mean_volume=mean_volume)


def _with_big_bidder(planes, bids, env, kw):
    """one keyword bid at $50 000 with about 5 000 auctions: V (bid_c - 1) is 2.5e10 cents, its tile cannot pack"""
    planes[P_VOL, env, kw] = 5000.0
    planes[P_VOL_STD, env, kw] = 100.0
    bids[env, kw] = 50000.0


TILINGS = [pytest.param(None, "k_step_implicit_fast<true>", id="tiles16"), pytest.param(256, "k_step_implicit_fast<false>", id="tiles256")]


@pytest.mark.parametrize("tile_kw,kernel", TILINGS)
def test_ordinary_law_packs(amd, monkeypatch, tile_kw, kernel):
    days, _ = _four_steps(amd, monkeypatch, 4, 256, _ordinary(4, 256, 801), _bids(4, 256, 801), tile_kw=tile_kw, kernel=kernel)
    assert all(d["conversions"].any() and d["revenue_cents"].any() for d in days)


@pytest.mark.parametrize("tile_kw,kernel", TILINGS)
def test_one_keyword_at_50000_dollars(amd, monkeypatch, tile_kw, kernel):
    """env 1's tile does not pack, its neighbours' do"""
    planes, bids = _ordinary(4, 256, 802), _bids(4, 256, 802)
    _with_big_bidder(planes, bids, 1, 100)
    days, _ = _four_steps(amd, monkeypatch, 4, 256, planes, bids, tile_kw=tile_kw, kernel=kernel)
    assert all(d["clicks"][1, 100] > 500 for d in days)


@pytest.mark.parametrize("tile_kw,kernel", TILINGS)
def test_cost_really_passes_2_32(amd, monkeypatch, tile_kw, kernel):
    """the competitor around $40 000 against a bid of $50 000 at 5 000 auctions: a clicked win costs about 4e6 cents, the keyword's day
    about 1e10 - a tile that packed it all the same would carry into the revenue half and lose the cost's high bits"""
    planes, bids = _ordinary(4, 256, 813), _bids(4, 256, 813)
    _with_big_bidder(planes, bids, 2, 60)
    planes[P_LOC, 2, 60] = 40000.0
    planes[P_SCALE, 2, 60] = 1000.0
    planes[P_BCTR, 2, 60] = 0.8
    days, _ = _four_steps(amd, monkeypatch, 4, 256, planes, bids, tile_kw=tile_kw, kernel=kernel)
    assert all(d["cost_cents"][2, 60] >= 2**32 and d["conversions"][2, 60] > 0 for d in days)


@pytest.mark.parametrize("tile_kw,kernel", TILINGS)
def test_huge_revenue_laws(amd, monkeypatch, tile_kw, kernel):
    """mu = 1e7 dollars (every conversion is worth the cap of 1e9 cents: five of them pass 2^32) and sd = 1e6 dollars"""
    planes, bids = _ordinary(4, 256, 803), _bids(4, 256, 803, lo=0.8, hi=1.2)
    planes[P_MU, 0, 7] = 1.0e7
    planes[P_SD, 2, 250] = 1.0e6
    for env, kw in ((0, 7), (2, 250)):
        planes[P_VOL, env, kw] = 1000.0
        planes[P_BCTR, env, kw] = 0.8
    days, _ = _four_steps(amd, monkeypatch, 4, 256, planes, bids, tile_kw=tile_kw, kernel=kernel)
    assert all(d["revenue_cents"][0, 7] >= 2**32 for d in days)
    assert max(int(d["revenue_cents"][2, 250]) for d in days) >= 2**32


@pytest.mark.parametrize("tile_kw,kernel", TILINGS)
def test_laws_straddling_the_bound(amd, monkeypatch, packs, tile_kw, kernel):
    """64 auctions exactly: the largest bid and the largest mu (in whole dollars) that still pack in env 0, one dollar more in env 1"""
    planes, bids = _ordinary(4, 256, 804), _bids(4, 256, 804)
    V = 64

    def last_that_packs(f):
        lo, hi = 1, 10**7          # f(lo) packs, f(hi) does not
        assert f(lo) and not f(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if f(mid) else (lo, mid)
        return lo
    bid_edge = last_that_packs(lambda d: packs(V, float(d), 1.0, 0.1))
    mu_edge = last_that_packs(lambda d: packs(V, 0.9, float(d), 0.1))
    assert 5.0e5 < bid_edge < 7.0e5 and 5.0e5 < mu_edge < 7.0e5          # 64 x 6.25e7 cents = 4.0e9
    for env, extra in ((0, 0.0), (1, 1.0)):
        for kw in (40, 41):
            planes[P_VOL, env, kw] = float(V)
            planes[P_VOL_STD, env, kw] = 0.0
            planes[P_BCTR, env, kw] = 0.9
            planes[P_SD, env, kw] = 0.1
        planes[P_MU, env, 40] = 1.0
        bids[env, 40] = bid_edge + extra
        planes[P_MU, env, 41] = mu_edge + extra
        bids[env, 41] = 0.9
    days, _ = _four_steps(amd, monkeypatch, 4, 256, planes, bids, tile_kw=tile_kw, kernel=kernel)
    assert all(d["clicks"][0, 40] > 30 and d["clicks"][1, 40] > 30 for d in days)
    assert sum(int(d["conversions"][0, 41]) + int(d["conversions"][1, 41]) for d in days) > 0


def test_one_unpackable_tile_among_eight(amd, monkeypatch):
    """2 envs x 1024 keywords in tiles of 256: only tile 2 of env 0 keeps three accumulators; the env's totals mix both kinds"""
    planes, bids = _ordinary(2, 1024, 805), _bids(2, 1024, 805)
    _with_big_bidder(planes, bids, 0, 2 * 256 + 77)
    _four_steps(amd, monkeypatch, 2, 1024, planes, bids, tile_kw=256, kernel="k_step_implicit_fast<false>")


def test_one_unpackable_tile_among_narrow_ones(amd, monkeypatch):
    """the same in the tiling such a shape gets by itself (tiles of 16 keywords)"""
    planes, bids = _ordinary(2, 1024, 806), _bids(2, 1024, 806)
    _with_big_bidder(planes, bids, 0, 2 * 256 + 77)
    _four_steps(amd, monkeypatch, 2, 1024, planes, bids)


@pytest.mark.parametrize("N,K", [(3, 16), (1, 100)])
def test_narrow_tiles(amd, monkeypatch, N, K):
    planes, bids = _ordinary(N, K, 807), _bids(N, K, 807)
    days, _ = _four_steps(amd, monkeypatch, N, K, planes, bids)
    assert all(d["conversions"].any() for d in days)
    _with_big_bidder(planes, bids, 0, K - 3)
    _four_steps(amd, monkeypatch, N, K, planes, bids)


def test_direct_tiles_packed(amd, monkeypatch):
    """256 x 256 at mean volume 8: every tile is resolved auction by auction (the queue entry carries the price), and packs.  (Such a
    keyword set goes to k_step_implicit_sparse by the engine's volume hint; ADCRAFT_FAST_VARIANT=1 keeps it on this kernel.)"""
    N, K = 256, 256
    planes, bids = _ordinary(N, K, 808, mean_volume=8), _bids(N, K, 808, lo=0.5, hi=1.2)
    days, _ = _four_steps(amd, monkeypatch, N, K, planes, bids, variant=1, kernel="k_step_implicit_fast<false>")
    assert all(d["conversions"].any() for d in days)


def test_direct_tiles_one_unpackable(amd, monkeypatch):
    """DIRECT tiles, one of which does not pack: mean volume 8 with a revenue law of 1e7 dollars in env 5"""
    N, K = 256, 256
    planes, bids = _ordinary(N, K, 809, mean_volume=8), _bids(N, K, 809, lo=0.5, hi=1.2)
    planes[P_MU, 5, 9] = 1.0e7
    planes[P_BCTR, 5, 9] = 0.9
    bids[5, 9] = 3.0
    days, _ = _four_steps(amd, monkeypatch, N, K, planes, bids, variant=1, kernel="k_step_implicit_fast<false>")
    assert sum(int(d["conversions"][5, 9]) for d in days) > 0


def test_full_tiles_interval_form(amd, monkeypatch):
    """256 x 256 at 20 .. 69 auctions per keyword: the throughput configuration's kernel and tiling with nothing asked for; a
    $50 000 keyword in three envs, a revenue law of 1e7 dollars in a fourth"""
    N, K = 256, 256
    planes, bids = _ordinary(N, K, 810), _bids(N, K, 810)
    planes[P_VOL] = 20 + (np.arange(N * K) * 11 % 50).reshape(N, K)
    planes[P_VOL_STD] = 0.0
    for env in (0, 100, 255):
        _with_big_bidder(planes, bids, env, (env * 7) % K)
    planes[P_MU, 17, 3] = 1.0e7
    days, _ = _four_steps(amd, monkeypatch, N, K, planes, bids, kernel="k_step_implicit_fast<false>")
    assert all(d["clicks"][100, (100 * 7) % K] > 500 for d in days)


@pytest.mark.parametrize("big", [False, True], ids=["packed", "unpacked"])
@pytest.mark.parametrize("tile_kw,kernel", TILINGS)
def test_binding_budget_listing_variants(amd, monkeypatch, big, tile_kw, kernel):
    """a budget of $20 a day binds on day 1, so the listing variant runs from day 2 on: the prices it lists for k_step_click_walk are
    the true prices (the oracle walks the day's clicks in order and stops at the budget), packed or not"""
    N, K = 4, 256
    planes = _ordinary(N, K, 811)
    rng = np.random.default_rng(811)

    def bids(step):
        b = (np.rint(rng.uniform(50, 120, (N, K))) / 100.0).astype(np.float32)
        if big:
            b[2, 31] = 50000.0
        return b
    if big:
        planes[P_VOL, 2, 31] = 5000.0
        planes[P_VOL_STD, 2, 31] = 100.0
    days, kernels = _four_steps(amd, monkeypatch, N, K, planes, bids, budget=20.0, tile_kw=tile_kw, kernel=kernel)
    listed = [k for k in kernels if "lists" in k]
    assert len(listed) >= 2, kernels          # the listing variant did run
    assert sum(int((d["cost_cents"].sum(axis=1) >= 2000).sum()) for d in days) > 0          # the budget did bind


@pytest.mark.parametrize("cvr", [0.0, 1.0])
@pytest.mark.parametrize("tile_kw,kernel", TILINGS)
def test_no_conversion_and_every_click_converts(amd, monkeypatch, cvr, tile_kw, kernel):
    """the rev_cents = 0 path alone, and a revenue with every click; one NaN mu (its revenue is the floor of 1 cent; its tile keeps
    three accumulators)"""
    planes, bids = _ordinary(4, 256, 812), _bids(4, 256, 812, lo=0.6, hi=1.2)
    planes[P_SCTR] = cvr
    planes[P_MU, 3, 200] = np.nan
    planes[P_BCTR, 3, 200] = 0.9
    days, _ = _four_steps(amd, monkeypatch, 4, 256, planes, bids, tile_kw=tile_kw, kernel=kernel)
    for d in days:
        assert np.array_equal(d["conversions"], d["clicks"] if cvr == 1.0 else np.zeros_like(d["clicks"]))
        assert d["clicks"][3, 200] > 0
        if cvr == 1.0:
            assert d["revenue_cents"][3, 200] == d["clicks"][3, 200]          # 1 cent each
