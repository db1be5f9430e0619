"""The interpolation agent's per-keyword act and cache key on the host (adc_interp_act_host, adc_interp_key_host: the code
the device kernel runs, adc_interp.h) against the numpy restatement in tests/interp_ref.py."""
import numpy as np
import pytest

from tests import interp_ref as R


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _twin(lib, cache, grid, threshold, bid_step, u):
    return R.twin_act(lib, cache, grid, threshold, bid_step, u)[:4]


def _random_cache(rng, n_points, cpc_share, max_cent=300):
    c = R.KeywordCache()
    cents = np.sort(rng.choice(np.arange(1, max_cent + 1), size=n_points, replace=False)) if n_points else []
    for cent in cents:
        c.clicks[int(cent)] = [np.float32(rng.integers(0, 40) * rng.random()), int(rng.integers(1, 9))]
        if rng.random() < cpc_share:
            c.cpc[int(cent)] = [float(np.float32(rng.random() * 3)) / float(np.float32(rng.integers(1, 30))), int(rng.integers(1, 9))]
    c.n_rpc = int(rng.integers(0, 5)) if rng.random() < 0.6 else 0
    c.n_sctr = int(rng.integers(0, 9)) if rng.random() < 0.8 else 0
    c.ave_rpc = np.float32(rng.random() * 4)
    c.ave_sctr = np.float32(rng.random())
    keys = [x / 100 for x in cents] + [0.03]
    c.max_observed = max(keys + ([rng.choice([-0.5, 0.0, 3.5, 12.0])] if rng.random() < 0.2 else []))
    return c


def test_host_twin_equals_the_restatement_on_random_caches(lib):
    rng = np.random.default_rng(13)
    grids = [np.linspace(0.01, 3.00, 300), np.arange(0.01, 0.31, 0.01), np.array([0.05]),
             rng.permutation(np.concatenate([np.arange(0.005, 1.5, 0.01), [3.2, 4.0]])), rng.random(700) * 3.5,
             np.arange(0.01, 3.01, 0.01)[::7].copy()]
    checked = draws = 0
    for t in range(1500):
        n_points = int(rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 12, 40, 120]))
        cache = _random_cache(rng, n_points, rng.choice([0.0, 0.5, 1.0]))
        grid = grids[t % len(grids)]
        threshold = float(rng.choice([-0.2, -0.1, -1.0, 0.3]))
        bid_step = float(rng.choice([0.03, 0.05, 1.0, -0.2]))
        u = float(rng.random())
        margin, cost, idx, bid = _twin(lib, cache, grid, threshold, bid_step, u)
        want_m, want_c = cache.curves(grid)
        assert np.array_equal(margin, np.broadcast_to(want_m, grid.shape)), t
        assert np.array_equal(cost, np.broadcast_to(want_c, grid.shape)), t
        a, mass = cache.acquisition(np.array(want_m, dtype=np.float64), threshold, bid_step)
        if mass > 0:
            want = R.choice_index(a / mass, u)
            assert (idx, bid) == (want, grid[want]), t
            draws += 1
        else:
            assert (idx, bid) == (-1, 0.01), t
        checked += 1
    assert draws > 300


def test_pairwise_mass_matches_numpy_sum_for_every_length(lib):
    """the streaming pairwise sum inside adc::interp_pick against np.sum, lengths 1..2048 (blocks, splits, tails): the mass
    itself, bit for bit, and the draw it leads to"""
    rng = np.random.default_rng(5)
    for L in list(range(1, 300)) + [383, 511, 512, 513, 1000, 1023, 1024, 1031, 2047, 2048]:
        c = _random_cache(rng, 30, 1.0)
        c.max_observed = 100.0                        # end_index = L: the whole grid
        grid = rng.random(L) * 3.0
        margin, _, idx, _, got_mass = R.twin_act(lib, c, grid, -0.2, 0.03, 0.5)
        a, mass = c.acquisition(margin.copy(), -0.2, 0.03)
        assert got_mass == np.sum(a[:L]) == mass, L
        assert np.float64(got_mass).tobytes() == np.sum(a).tobytes(), L      # bit for bit, not merely equal
        if mass > 0:
            assert idx == R.choice_index(a / mass, 0.5), L
        else:
            assert idx == -1


def test_key_function_is_round_of_the_float32_bid(lib):
    key = lib.adc_interp_key_host
    vals = []
    for h in range(-200, 5001):                       # every half cent in [-1, 25], +-4 ulp of its float32
        x = np.float32(h / 200.0)
        v = x
        for _ in range(4):
            v = np.nextafter(v, np.float32(-np.inf))
        for _ in range(9):
            vals.append(v)
            v = np.nextafter(v, np.float32(np.inf))
    for v in vals:
        assert key(float(v)) == round(float(v), 2), v
    rng = np.random.default_rng(3)
    other = np.concatenate([(rng.random(500000) * 50 - 10), rng.standard_normal(300000) * 1e3,
                            np.float32(2.0) ** rng.integers(-30, 60, 200000) * rng.random(200000)]).astype(np.float32)
    got = np.array([key(float(v)) for v in other])
    want = np.array([round(float(v), 2) for v in other])
    assert np.array_equal(got, want)
    assert key(0.125) == 0.12 and key(0.375) == 0.38 and key(np.float32(0.015)) == 0.01


def test_arange_points_hit_exactly(lib):
    """a grid equal to the interpolation x values returns the smoothed points themselves (np.interp's exact hits)"""
    c = R.KeywordCache()
    for cent in (3, 10, 11, 57, 200, 300):
        c.clicks[cent] = [np.float32(cent % 7), 2]
        c.cpc[cent] = [cent / 97.0, 1]
    grid = np.linspace(0.01, 3.00, 300)
    assert np.array_equal(grid, R.ARANGE)
    m, cost, _, _ = _twin(lib, c, grid, -0.2, 0.03, 0.3)
    wm, wc = c.curves(grid)
    assert np.array_equal(m, wm) and np.array_equal(cost, wc)
