"""-m gpu: the engine against the CPU oracle, bit for bit on every output, where a drain of k_step_implicit_fast's clicked-win queue
moves the queue down FIRST and resolves its batch from registers after that (parts/kernel_fast.inc, drain; the protocol alone is
tests/test_fast_queue_order_host.py).  The laws differ from env to env so that a wave's drains meet every state of its queue:
  env % 5 == 0   click rate 1 and a bid of $50, above every competitor price: every auction word pushes 64 entries, a full queue at
                 every drain
  env % 5 == 1   click rate 0.04 at ordinary bids: about one clicked win per auction word, so drains fall in the middle of an item
                 with anything from 0 to 63 entries behind the batch
  env % 5 == 2   click rate 0: no clicked win at all, no drain, nothing left at the end
  env % 5 == 3   one keyword with one auction, which it wins and which is clicked, next to keywords that never click: the last,
                 partial batch of that wave is exactly one entry
  env % 5 == 4   the ordinary laws as they are (only the 64-env shape has such envs)
Four steps per case; every case runs 4 x 256 as the engine tiles it (tiles of 16 keywords, <true>), 4 x 256 in tiles of 256
(ADCRAFT_FAST_TILE_KW, <false>) and 64 x 256 (tiles of 64, <true>), and checks the name of the kernel that ran.  The oracle knows
neither tiles nor queues."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

P_VOL, P_VOL_STD, P_LOC, P_SCALE, P_BCTR, P_SCTR, P_MU, P_SD = range(8)
TOP = 50.0          # dollars: above every price the competitor's law can give (loc <= 1, scale <= 0.3, |deviate| < 17)
ONE, QUIET_A, QUIET_B = 200, 10, 201          # env % 5 == 3: the keyword with one auction; two that win 100 auctions and never click


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _laws(N, K, seed, mean_volume=40, lo=0.3, hi=1.0):
    """-> planes [8][N][K], bids [N][K]"""
    planes = H.implicit_params(N, K, seed=seed, mean_volume=mean_volume)
    bids = (np.rint(np.random.default_rng(seed).uniform(lo, hi, (N, K)) * 100.0) / 100.0).astype(np.float32)
    for e in range(N):
        kind = e % 5
        if kind == 0:
            planes[P_BCTR, e] = 1.0
            bids[e] = TOP
        elif kind == 1:
            planes[P_BCTR, e] = 0.04
        elif kind == 2:
            planes[P_BCTR, e] = 0.0
        elif kind == 3:
            planes[P_VOL, e] = 0.0
            planes[P_VOL_STD, e] = 0.0
            planes[P_BCTR, e] = 0.0
            planes[P_VOL, e, [QUIET_A, QUIET_B]] = 100.0
            planes[P_VOL, e, ONE] = 1.0
            planes[P_BCTR, e, ONE] = 1.0
            bids[e] = TOP
    return planes, bids


def _four_steps(amd, monkeypatch, N, K, planes, bids, kernel, budget=1.0e9, tile_kw=None, variant=None):
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


def _check_queue_states(days, N, direct=False):
    """the laws did what they are there for (on the oracle's days, which the engine's equal)"""
    for d in days:
        imp, clk = d["impressions"], d["clicks"]
        for e in range(N):
            kind = e % 5
            if kind == 0:          # every auction a clicked win
                assert imp[e].sum() > 0 and np.array_equal(imp[e], clk[e])
            elif kind == 1:        # about one clicked win per word of 64 auctions (the wins are a third to a half of the auctions)
                assert 0 < clk[e].sum() * 8 < imp[e].sum()
            elif kind == 2:
                assert imp[e].sum() > 0 and not clk[e].any()
            elif kind == 3:
                assert clk[e, ONE] == 1 and clk[e].sum() == 1 and imp[e, QUIET_A] == 100 and imp[e, QUIET_B] == 100 and imp[e].sum() == 201
            else:
                assert 0 < clk[e].sum() < imp[e].sum()


# N, K, ADCRAFT_FAST_TILE_KW, the kernel that runs
SHAPES = [pytest.param(4, 256, None, "k_step_implicit_fast<true>", id="4x256-tiles16"),
          pytest.param(4, 256, 256, "k_step_implicit_fast<false>", id="4x256-tiles256"),
          pytest.param(64, 256, None, "k_step_implicit_fast<true>", id="64x256")]


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_ordinary_laws(amd, monkeypatch, N, K, tile_kw, kernel):
    planes, bids = _laws(N, K, 911)
    days, _ = _four_steps(amd, monkeypatch, N, K, planes, bids, kernel, tile_kw=tile_kw)
    _check_queue_states(days, N)
    assert all(d["conversions"].any() and d["revenue_cents"].any() for d in days)


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_a_tile_that_does_not_pack(amd, monkeypatch, N, K, tile_kw, kernel):
    """a keyword bid at $50 000 with about 5 000 auctions, in the env whose queue is always full and in the one whose drains fall
    mid-item, and a revenue law of 1e7 dollars (1e9 cents a conversion) in both: those tiles keep three accumulators, and the batch
    that is resolved after the move-down adds to all three"""
    planes, bids = _laws(N, K, 912)
    for e in (0, 1):
        planes[P_VOL, e, 100] = 5000.0
        planes[P_VOL_STD, e, 100] = 100.0
        bids[e, 100] = 50000.0
        planes[P_MU, e, 7] = 1.0e7
        planes[P_SD, e, 7] = 0.0
        planes[P_VOL, e, 7] = 1000.0
        planes[P_BCTR, e, 7] = 0.8 if e == 1 else 1.0
        bids[e, 7] = TOP
    days, _ = _four_steps(amd, monkeypatch, N, K, planes, bids, kernel, tile_kw=tile_kw)
    for d in days:
        assert d["clicks"][0, 100] > 4000 and d["clicks"][1, 100] > 50
        for e in (0, 1):
            assert d["conversions"][e, 7] > 0 and int(d["revenue_cents"][e, 7]) == 10**9 * int(d["conversions"][e, 7])
        assert d["clicks"][3, ONE] == 1 and d["clicks"][3].sum() == 1 and not d["clicks"][2].any()


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_a_keyword_that_always_converts(amd, monkeypatch, N, K, tile_kw, kernel):
    """sctr == 1 on one keyword of the full-queue env, of the mid-item env and on the keyword with the single auction: its
    conversions are its clicks, and its tile takes the conversion's second compare"""
    planes, bids = _laws(N, K, 913)
    for e, k in ((0, 100), (1, 100), (3, ONE)):
        planes[P_SCTR, e, k] = 1.0
    planes[P_BCTR, 1, 100] = 0.9
    bids[1, 100] = TOP
    days, _ = _four_steps(amd, monkeypatch, N, K, planes, bids, kernel, tile_kw=tile_kw)
    for d in days:
        for e, k in ((0, 100), (1, 100), (3, ONE)):
            assert d["clicks"][e, k] > 0 and d["conversions"][e, k] == d["clicks"][e, k]
        assert (d["conversions"][0] < d["clicks"][0]).any() and d["clicks"][3].sum() == 1


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_direct_tiles(amd, monkeypatch, N, K, tile_kw, kernel):
    """mean volume 8: the tiles are resolved auction by auction (DIRECT: the entry carries the price), through the same queue and
    the same drain; ADCRAFT_FAST_VARIANT=1 keeps such a keyword set on this kernel.  (The env of the single auction stays in the
    interval form: its two quiet keywords make its tiles dense.)"""
    planes, bids = _laws(N, K, 914, mean_volume=8, lo=0.5, hi=1.2)
    planes[P_SCTR, 0, 255] = 1.0
    days, _ = _four_steps(amd, monkeypatch, N, K, planes, bids, kernel, tile_kw=tile_kw, variant=1)
    _check_queue_states(days, N)
    assert all(d["conversions"][0, 255] == d["clicks"][0, 255] for d in days) and sum(int(d["clicks"][0, 255]) for d in days) > 0


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_binding_budget_runs_the_listing_variant(amd, monkeypatch, N, K, tile_kw, kernel):
    """a budget of $20 a day binds on day 1 in the envs that click, so the listing variant runs from day 2 on: it lists the
    clicked wins of the batch it resolves after the move-down (the oracle walks the day's clicks in order)"""
    planes, _ = _laws(N, K, 915)
    planes[P_SCTR, 1, 255] = 1.0
    rng = np.random.default_rng(915)
    top = np.array([e % 5 in (0, 3) for e in range(N)])[:, None]

    def bids(step):
        return np.where(top, TOP, np.rint(rng.uniform(50, 120, (N, K))) / 100.0).astype(np.float32)
    days, kernels = _four_steps(amd, monkeypatch, N, K, planes, bids, kernel, budget=20.0, tile_kw=tile_kw)
    assert "lists" in kernels[1], kernels          # the listing variant ran on the second day
    assert sum(int((d["cost_cents"].sum(axis=1) >= 2000).sum()) for d in days) > 0          # the budget did bind
