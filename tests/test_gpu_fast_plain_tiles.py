"""-m gpu: the engine against the CPU oracle, bit for bit on every output, where stage B of k_step_implicit_fast resolves a clicked
win of a PLAIN tile (every live keyword packs and converts below a threshold of 2^32: adc_law.h fast_keyword_plain) without the
revenue's upper clamp and with one compare for the conversion, and where it may not: a conversion rate of 1 (threshold 2^32), a tile
that does not pack, a NaN law.  The queue tags are auction << 11 | keyword << 3 on every path (interval form, DIRECT, listing).
Four steps per case; every case runs 4 x 256 as the engine tiles it (tiles of 16 keywords, <true>), 4 x 256 in tiles of 256
(ADCRAFT_FAST_TILE_KW, <false>) and 256 x 256, and checks the name of the kernel that ran.  The oracle knows neither tiles nor
plain laws."""
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
def plain():
    """the host predicate: plain(V, bid, mu, sd, sctr) -> bool"""
    from oracle import build as obuild
    lib = C.CDLL(obuild.build_shims_host())
    vp = C.c_void_p
    lib.adc_fast_plain_tiles_host.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    lib.adc_fast_plain_tiles_host.restype = C.c_int

    def f(V, bid, mu, sd, sctr):
        V = np.array([V], np.int32)
        bid, mu, sd, sctr = (np.array([x], np.float32) for x in (bid, mu, sd, sctr))
        out, t32, T, rmax2, bad = np.zeros(1, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint64), np.zeros(2, np.int32), np.zeros(1, np.int32)
        assert lib.adc_fast_plain_tiles_host(1, V.ctypes.data, bid.ctypes.data, mu.ctypes.data, sd.ctypes.data, sctr.ctypes.data, None, 0, 0, 0,
                                             out.ctypes.data, t32.ctypes.data, T.ctypes.data, None, None, rmax2.ctypes.data, bad.ctypes.data) == 0
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


# N, K, ADCRAFT_FAST_TILE_KW, the kernel that runs
SHAPES = [pytest.param(4, 256, None, "k_step_implicit_fast<true>", id="4x256-tiles16"),
          pytest.param(4, 256, 256, "k_step_implicit_fast<false>", id="4x256-tiles256"),
          pytest.param(256, 256, None, "k_step_implicit_fast<false>", id="256x256")]


def _run(amd, monkeypatch, shape, planes, bids):
    N, K, tile_kw, kernel = shape
    return _four_steps(amd, monkeypatch, N, K, planes, bids, tile_kw=tile_kw, kernel=kernel)[0]


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_ordinary_laws_are_plain(amd, monkeypatch, plain, N, K, tile_kw, kernel):
    planes, bids = H.implicit_params(N, K, seed=901, mean_volume=40), _bids(N, K, 901)
    assert plain(40, 1.0, 1.5, 0.45, 0.8)
    days = _run(amd, monkeypatch, (N, K, tile_kw, kernel), planes, bids)
    assert all(d["conversions"].any() and d["revenue_cents"].any() for d in days)


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_one_keyword_always_converts(amd, monkeypatch, plain, N, K, tile_kw, kernel):
    """sctr == 1 on keyword 100 of env 1: its conversions are its clicks; its tile is not plain, its neighbours' are"""
    planes, bids = H.implicit_params(N, K, seed=902, mean_volume=40), _bids(N, K, 902, lo=0.6, hi=1.2)
    planes[P_SCTR, 1, 100] = 1.0
    planes[P_BCTR, 1, 100] = 0.9
    assert not plain(40, 1.0, 1.0, 0.1, 1.0) and plain(40, 1.0, 1.0, 0.1, 0.8)
    days = _run(amd, monkeypatch, (N, K, tile_kw, kernel), planes, bids)
    assert all(d["conversions"][1, 100] == d["clicks"][1, 100] for d in days) and sum(int(d["clicks"][1, 100]) for d in days) > 0
    assert all((d["conversions"][0] < d["clicks"][0]).any() for d in days)


@pytest.mark.parametrize("cvr", [0.0, 1.0])
@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_no_conversion_and_every_click_converts(amd, monkeypatch, cvr, N, K, tile_kw, kernel):
    planes, bids = H.implicit_params(N, K, seed=903, mean_volume=40), _bids(N, K, 903, lo=0.6, hi=1.2)
    planes[P_SCTR] = cvr
    days = _run(amd, monkeypatch, (N, K, tile_kw, kernel), planes, bids)
    for d in days:
        assert d["clicks"].any()
        assert np.array_equal(d["conversions"], d["clicks"] if cvr == 1.0 else np.zeros_like(d["clicks"]))


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_plain_tile_next_to_one_that_does_not_pack(amd, monkeypatch, N, K, tile_kw, kernel):
    """a keyword bid at $50 000 with about 5 000 auctions in env 1 and a revenue law of 1e7 dollars in env 2 (its revenue is the
    clamp's 1e9 cents a conversion): those tiles keep three accumulators and the clamp, every other tile is plain"""
    planes, bids = H.implicit_params(N, K, seed=904, mean_volume=40), _bids(N, K, 904, lo=0.8, hi=1.2)
    planes[P_VOL, 1, 100] = 5000.0
    planes[P_VOL_STD, 1, 100] = 100.0
    bids[1, 100] = 50000.0
    planes[P_MU, 2, 7] = 1.0e7
    planes[P_SD, 2, 7] = 0.0
    planes[P_VOL, 2, 7] = 1000.0
    planes[P_BCTR, 2, 7] = 0.8
    days = _run(amd, monkeypatch, (N, K, tile_kw, kernel), planes, bids)
    assert all(d["clicks"][1, 100] > 500 for d in days)
    assert all(d["conversions"][2, 7] > 0 and int(d["revenue_cents"][2, 7]) == 10**9 * int(d["conversions"][2, 7]) for d in days)


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_revenue_just_under_the_bound_still_packs(amd, monkeypatch, plain, N, K, tile_kw, kernel):
    """mu = 9.9e6 dollars at three auctions a day: plain (3 x 9.9e8 cents < 4.0e9), with revenues a percent below the clamp that is
    no longer applied"""
    planes, bids = H.implicit_params(N, K, seed=905, mean_volume=40), _bids(N, K, 905, lo=0.8, hi=1.2)
    kws = [(e, k) for e in (0, 3) for k in (5, 77, 130, 255)]
    for e, k in kws:
        planes[P_VOL, e, k] = 3.0
        planes[P_VOL_STD, e, k] = 0.0
        planes[P_BCTR, e, k] = 0.9
        planes[P_SCTR, e, k] = 0.9
        planes[P_MU, e, k] = 9.9e6
        planes[P_SD, e, k] = 1.0e3
        bids[e, k] = 3.0
    assert plain(3, 3.0, 9.9e6, 1.0e3, 0.9) and not plain(5, 3.0, 9.9e6, 1.0e3, 0.9)
    days = _run(amd, monkeypatch, (N, K, tile_kw, kernel), planes, bids)
    conv = sum(int(d["conversions"][e, k]) for d in days for e, k in kws)
    assert conv > 0
    for d in days:
        for e, k in kws:
            c = int(d["conversions"][e, k])
            assert 980_000_000 * c <= int(d["revenue_cents"][e, k]) <= 1_000_000_000 * c - c


@pytest.mark.parametrize("N,K,tile_kw,kernel", SHAPES)
def test_nan_law(amd, monkeypatch, plain, N, K, tile_kw, kernel):
    """a NaN revenue mean: its revenue is the floor of 1 cent a conversion, and its tile is not plain"""
    planes, bids = H.implicit_params(N, K, seed=906, mean_volume=40), _bids(N, K, 906, lo=0.6, hi=1.2)
    planes[P_MU, 3, 200] = np.nan
    planes[P_BCTR, 3, 200] = 0.9
    assert not plain(40, 1.0, np.nan, 0.1, 0.8)
    days = _run(amd, monkeypatch, (N, K, tile_kw, kernel), planes, bids)
    assert all(d["clicks"][3, 200] > 0 and d["revenue_cents"][3, 200] == d["conversions"][3, 200] for d in days)
    assert sum(int(d["conversions"][3, 200]) for d in days) > 0


def test_direct_tiles(amd, monkeypatch):
    """256 x 256 at mean volume 8: every tile is resolved auction by auction (DIRECT: today's stage B, with the new tags), one
    keyword with sctr == 1.  (Such a keyword set goes to k_step_implicit_sparse by the engine's volume hint;
    ADCRAFT_FAST_VARIANT=1 keeps it on this kernel.)"""
    N, K = 256, 256
    planes, bids = H.implicit_params(N, K, seed=907, mean_volume=8), _bids(N, K, 907, lo=0.5, hi=1.2)
    planes[P_SCTR, 9, 255] = 1.0
    planes[P_BCTR, 9, 255] = 0.9
    bids[9, 255] = 3.0
    days, _ = _four_steps(amd, monkeypatch, N, K, planes, bids, variant=1, kernel="k_step_implicit_fast<false>")
    assert all(d["conversions"].any() for d in days)
    assert all(d["conversions"][9, 255] == d["clicks"][9, 255] for d in days) and sum(int(d["clicks"][9, 255]) for d in days) > 0


@pytest.mark.parametrize("tile_kw,kernel", [pytest.param(None, "k_step_implicit_fast<true>", id="tiles16"),
                                            pytest.param(256, "k_step_implicit_fast<false>", id="tiles256")])
def test_binding_budget_runs_the_listing_variant(amd, monkeypatch, tile_kw, kernel):
    """a budget of $20 a day binds on day 1, so the listing variant runs from day 2 on: jcut and the records it writes for
    k_step_click_walk read the keyword and the auction from the new tags (the oracle walks the day's clicks in order)"""
    N, K = 4, 256
    planes = H.implicit_params(N, K, seed=908, mean_volume=40)
    planes[P_SCTR, 2, 255] = 1.0
    rng = np.random.default_rng(908)

    def bids(step):
        return (np.rint(rng.uniform(50, 120, (N, K))) / 100.0).astype(np.float32)
    days, kernels = _four_steps(amd, monkeypatch, N, K, planes, bids, budget=20.0, tile_kw=tile_kw, kernel=kernel)
    assert "lists" in kernels[1], kernels          # the listing variant ran on the second day
    assert sum(int((d["cost_cents"].sum(axis=1) >= 2000).sum()) for d in days) > 0          # the budget did bind
