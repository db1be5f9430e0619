"""GPU: the ideal profit, bid curves and oracle bidder of EXPLICIT keywords (get_explicit_kw_bid_cpc_impressions,
experiment_metrics.py:10-17): k_explicit_curves against its host twin (adc_explicit_curve_host), the per-step ideal against
the numpy restatement, contender lists against the whole grid, the oracle and the closed loop against host recomputations."""
import numpy as np
import pytest

from oracle import ref_numpy as rn
from tests import helpers as H

pytestmark = pytest.mark.gpu

NOTEBOOK = np.arange(0.01, 3.00, 0.01)
GRIDS = {"notebook": NOTEBOOK, "coarse": np.arange(0.05, 2.0, 0.05), "fine": np.arange(0.002, 0.6, 0.002),
         "long": np.arange(0.005, 3.0, 0.005)}             # 299, 39, 299 (<= 304: contender lists) and 599 points (the whole grid)
THRESH = float(np.float32(0.05))


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _engine(amd, N, K, seed, planes=None, **kw):
    """default-constructor keywords (generated on the device) with 12x their revenue: the constructor's own revenue (1.5 Beta(2, 5))
    never covers a cost of 2.2 or more, so every ideal would be 0"""
    e = amd.StepEngine(N, K, model=amd.MODEL_EXPLICIT, seed=seed, **kw)
    e.reset(seeds=np.arange(N, dtype=np.uint64) + np.uint64(seed))
    if planes is None:
        e.generate_explicit_keywords()
        planes = e.get_all_params()
        planes[6:8] *= np.float32(12.0)
    e.set_all_params(planes)
    return e


def _ir_close(got, want):
    """within 4 ulp of ir + th: the device's exp is ocml's, the host's libm's (each within an ulp), and (1 + 2 th) r - th carries
    the difference of r at the scale of r (measured: at most 3 ulp of ir)"""
    got, want = np.asarray(got), np.asarray(want)
    return np.abs(got - want) <= 4 * np.spacing(np.abs(want) + THRESH)


def _twin(amd, keys, ticks, planes, n, grid, env, k):
    ir, cpc, _ = amd.explicit_curve_host(int(keys[env]), int(ticks[env]), k, n, planes[2, env, k], planes[3, env, k], grid, THRESH)
    return ir, cpc


@pytest.mark.parametrize("grid_name", list(GRIDS))
@pytest.mark.parametrize("n", [1, 2, 3, 101, 2048, 5000, 65536])
def test_device_curves_are_the_host_twins(amd, n, grid_name):
    grid = GRIDS[grid_name]
    N, K = 2, 8
    e = _engine(amd, N, K, seed=31 + n)
    e.bid_curves_build(n, grid)
    ir, cpc = e.bid_curves_fetch()
    keys, ticks = e.get_rng_state()
    planes = e.get_all_params()
    e.close()
    for env in range(N):
        for k in range(K):
            tir, tcpc = _twin(amd, keys, ticks, planes, n, grid, env, k)
            assert np.array_equal(cpc[env, k], tcpc), (env, k)
            assert _ir_close(ir[env, k], tir).all(), (env, k, np.max(np.abs(ir[env, k] - tir)))


def _numpy_ideal(planes, ir, cpc):
    N, K = ir.shape[:2]
    val, arg = np.zeros((N, K)), np.zeros((N, K), np.int64)
    for n in range(N):
        for k in range(K):
            kwp = [[float(planes[0][n, k]), 0.0], 0.0, 0.0, float(planes[4][n, k]), float(planes[5][n, k]), float(planes[6][n, k]), 0.0]
            mx, _, am = rn.max_expected_bid_profits(kwp, cpc[n, k], ir[n, k])
            val[n, k], arg[n, k] = mx, am
    return val, arg


@pytest.mark.parametrize("n", [2048, 101])
def test_ideal_profit_equals_the_first_ideal_step_and_numpy(amd, n):
    N, K = 4, 33
    e = _engine(amd, N, K, seed=7)
    first = e.ideal_profit(n)
    e.bid_curves_build(n)
    ideal, best = e.ideal_step()
    ir, cpc = e.bid_curves_fetch()
    planes = e.get_all_params()
    e.close()
    assert np.array_equal(first, ideal)
    val, arg = _numpy_ideal(planes, ir, cpc)
    assert np.array_equal(ideal, val)
    assert np.array_equal(best[val > 0], arg[val > 0]) and (best[val == 0] == 0).all()
    assert (val > 0).mean() > 0.5


def test_ideal_step_under_drift_is_the_reference_formula(amd):
    N, K = 4, 40
    e = _engine(amd, N, K, seed=23, drift_enabled=True, drift=(0.2, 0.2, 0.2), max_days=50)
    e.bid_curves_build(2048)
    ir, cpc = e.bid_curves_fetch()
    planes0 = e.get_all_params()
    e.sample_actions(0.3, 1.0, 1e9)
    for _ in range(4):
        e.step_device()
        ideal, best = e.ideal_step()
        p = e.get_all_params()
        val, arg = _numpy_ideal(p, ir, cpc)
        assert np.array_equal(ideal, val)
        assert np.array_equal(best[val > 0], arg[val > 0])
    assert not np.array_equal(p[0], planes0[0])
    e.close()


@pytest.mark.parametrize("case", ["notebook", "few_samples", "coarse_grid", "fine_grid", "long_grid", "extremes", "descending_grid",
                                  "shuffled_grid"])
def test_contender_lists_give_the_full_scans_ideal_bit_for_bit(amd, monkeypatch, case):
    N, K, days = 24, 160, 12
    n_samples, grid = 2048, None
    planes = H.explicit_params(N, K, seed=96)
    planes[6:8] *= np.float32(12.0)                        # (see _engine)
    if case == "few_samples":
        n_samples = 3
    elif case == "coarse_grid":
        grid = GRIDS["coarse"]
    elif case == "fine_grid":
        grid = GRIDS["fine"]
    elif case == "long_grid":
        grid = GRIDS["long"]                               # more points than the lists take: the whole grid, still identical
    elif case == "descending_grid":
        grid = NOTEBOOK[::-1].copy()                       # the impression rate falls along the grid: the whole grid
    elif case == "shuffled_grid":
        grid = np.random.default_rng(3).permutation(NOTEBOOK)
    elif case == "extremes":
        planes[5, 0] = 0.0                                 # no conversions
        planes[5, 1] = 1.0
        planes[6, 2] = 2.0e6                               # margin beyond kMarginMax
        planes[6, 3] = 1e-6
        planes[4, 4] = 0.0                                 # no clicks
        planes[0, 5] = 0.0                                 # no volume
        planes[6, 6] = np.nan
        planes[3, 7] = -5.0                                # a falling impression rate: the whole grid
        planes[3, 8] = 1e-3                                # nearly flat
        planes[3, 9] = 2000.0                              # a step
    runs = []
    for full in ("1", "0"):
        monkeypatch.setenv("ADCRAFT_IDEAL_FULL_SCAN", full)
        e = _engine(amd, N, K, seed=37, planes=planes, drift_enabled=True, drift=(0.3, 0.3, 0.5), max_days=1 << 20, loss_threshold=1e12)
        e.bid_curves_build(n_samples, grid)
        e.sample_actions(0.3, 1.0, 1e9)
        out = []
        for _ in range(days):
            ideal, best = e.ideal_step()
            out.append((ideal.copy(), best.copy()))
            e.step_device()
        if full == "0":
            count = e.bid_curves_contenders()[0]
        runs.append(out)
        e.close()
    for (i_full, b_full), (i_fast, b_fast) in zip(*runs):
        assert np.array_equal(i_full, i_fast, equal_nan=True)
        assert np.array_equal(b_full, b_fast)
    if case == "long_grid":
        assert (count == 65535).all()
    elif case in ("descending_grid", "shuffled_grid"):
        assert (count == 65535).mean() > 0.9
    elif case == "extremes":
        assert (count[7] == 65535).all()
    else:
        assert (count != 65535).mean() > 0.9
    assert len({tuple(b.ravel()) for _, b in runs[0]}) > 1 or case == "extremes"


@pytest.mark.parametrize("n_samples,grid", [(2048, None), (3, None), (512, GRIDS["fine"])])
def test_contender_lists_hold_the_argmax_at_every_margin(amd, n_samples, grid):
    N, K = 6, 96
    e = _engine(amd, N, K, seed=5)
    e.bid_curves_build(n_samples, grid)
    ir, cpc = e.bid_curves_fetch()
    count, idx, iv = e.bid_curves_contenders()
    e.close()
    assert (count != 65535).mean() > 0.9 and count[count != 65535].max() > 2
    margins = np.concatenate([np.linspace(0.0, 6.0, 701), np.exp(np.linspace(np.log(1e-4), np.log(50.0), 300))])
    checked = 0
    for n in range(N):
        for k in range(K):
            c = int(count[n, k])
            if c == 65535:
                continue
            ids, lo, hi = idx[n, k, :c], iv[n, k, :c, 0].astype(np.float64), iv[n, k, :c, 1].astype(np.float64)
            assert (np.diff(ids) > 0).all()
            assert (lo[1:] >= lo[:-1]).all() and (hi[1:] >= hi[:-1]).all()
            profit = ir[n, k][None, :] * (margins[:, None] - cpc[n, k][None, :])
            profit = np.where(profit > 0.0, profit, 0.0)
            best = profit.argmax(axis=1)
            pos = profit.max(axis=1) > 0.0
            for m, b in zip(margins[pos], best[pos]):
                j = np.searchsorted(ids, b)
                assert j < c and ids[j] == b, (n, k, m, b)
                assert lo[j] <= m <= hi[j], (n, k, m, b, lo[j], hi[j])
                checked += 1
    assert checked > 10000


def test_policy_oracle_bids_the_argmax(amd):
    N, K = 3, 50
    e = _engine(amd, N, K, seed=11)
    e.bid_curves_build(2048)
    _, best = e.ideal_step()
    e.policy_oracle(123.0)
    bids, budget = e.get_actions()
    e.close()
    want = np.maximum(np.rint(NOTEBOOK[best] * 100.0), 1.0) / 100.0
    assert np.array_equal(bids, want.astype(np.float32)) and (budget == 123.0).all()


def _host_akncp_ncp(profit, ideal, ideal_pos, days):
    with np.errstate(divide="ignore", invalid="ignore"):
        akncp = np.median((profit / days) / (ideal_pos / days), axis=1)
    den = ideal.sum(axis=1)
    return akncp, profit.sum(axis=1) / np.where(den <= 0.0, 1.0, den)


def test_run_days_oracle_and_baseline_episodes(amd):
    from adcraft_amd.closed_loop import run_baseline_episode
    N, K, days = 5, 40, 8
    kw = dict(drift_enabled=True, drift=(0.05, 0.05, 0.05), max_days=1 << 20, loss_threshold=1e12)
    # run_days("oracle") vs the same days driven from the host: ideal_step + policy_oracle + step per day
    res = []
    for host_loop in (False, True):
        e = _engine(amd, N, K, seed=19, **kw)
        e.bid_curves_build(2048)
        e.metrics_enable(True)
        e.metrics_reset()
        if host_loop:
            for _ in range(days):
                e.ideal_step(fetch=False)
                e.policy_oracle(500.0)
                e.step_device()
        else:
            e.run_days("oracle", days, budget=500.0, graph=False)
        profit, ideal, ideal_pos = e.metrics_read_nk()
        akncp, ncp = e.metrics_akncp_ncp(float(days))
        ha, hn = _host_akncp_ncp(profit, ideal, ideal_pos, float(days))
        assert np.array_equal(akncp, ha)
        np.testing.assert_allclose(ncp, hn, rtol=1e-12)    # (the device sums whole cents and a tree of ideals: other roundings)
        assert (ideal > 0).mean() > 0.5 and np.abs(profit).sum() > 0
        res.append((profit, ideal, ideal_pos, akncp, ncp))
        e.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    for policy in ("oracle", "zero_margin"):
        e = _engine(amd, N, K, seed=21, **kw)
        r = run_baseline_episode(e, policy, steps=days, agent_seeds=np.arange(N, dtype=np.uint64))
        akncp, ncp = e.metrics_akncp_ncp(float(days))
        ha, hn = _host_akncp_ncp(r["kw_profit_sum"], r["ideal_sum"], r["ideal_pos_sum"], float(days))
        assert np.array_equal(r["AKNCP"], ha) and np.array_equal(r["NCP"], hn)
        assert np.array_equal(akncp, ha)
        np.testing.assert_allclose(ncp, hn, rtol=1e-12)
        e.close()


def test_grouped_chain_equals_one_group(amd):
    N, K, days = 2048, 32, 5
    out = []
    for groups in (None, 1):
        e = _engine(amd, N, K, seed=41, drift_enabled=True, max_days=1 << 20, loss_threshold=1e12)
        if groups:
            e.set_env_groups(groups)
        e.bid_curves_build(2048)
        e.metrics_enable(True)
        e.run_days("oracle", days, budget=200.0, graph=False)
        if groups is None:
            assert e.env_groups() > 1
        else:
            assert e.env_groups() == 1
        out.append((e.metrics_read_nk(), e.ideal_step(), e.get_actions(), e.get_all_params()))
        e.close()
    (ma, ia, aa, pa), (mb, ib, ab, pb) = out
    for x, y in zip(ma + ia + aa, mb + ib + ab):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(pa, pb)


def test_full_size_oracle_days(amd):
    """4096 x 256 default-constructor keywords: curve build, six chained oracle days; a 16-env slice (four per env group) against
    the host twin and the numpy ideal"""
    N, K, days = 4096, 256, 6
    e = _engine(amd, N, K, seed=1729, max_days=1 << 20, loss_threshold=1e12)
    keys, ticks = e.get_rng_state()
    planes = e.get_all_params()
    first = e.ideal_profit(2048)
    e.bid_curves_build(2048)
    ideal, best = e.ideal_step()
    assert np.array_equal(first, ideal)
    G = max(e.env_groups(), 1)
    envs = sorted({int(g * N / G + j) for g in range(min(G, 4)) for j in range(16 // min(G, 4))})[:16]
    for env in envs:
        for k in range(0, K, 37):
            tir, tcpc = _twin(amd, keys, ticks, planes, 2048, NOTEBOOK, env, k)
            kwp = [[float(planes[0][env, k]), 0.0], 0.0, 0.0, float(planes[4][env, k]), float(planes[5][env, k]),
                   float(planes[6][env, k]), 0.0]
            mx, _, _ = rn.max_expected_bid_profits(kwp, tcpc, tir)
            assert abs(ideal[env, k] - mx) <= 1e-12 * max(1.0, mx), (env, k)
    e.metrics_enable(True)
    e.run_days("oracle", days, budget=1000.0)
    akncp, ncp = e.metrics_akncp_ncp(float(days))
    profit, s_ideal, s_pos = e.metrics_read_nk()
    ha, hn = _host_akncp_ncp(profit, s_ideal, s_pos, float(days))
    assert np.array_equal(akncp, ha)
    np.testing.assert_allclose(ncp, hn, rtol=1e-12)
    assert np.isfinite(akncp).all() and (s_ideal > 0).mean() > 0.5
    count = e.bid_curves_contenders()[0]
    assert (count != 65535).mean() > 0.95
    e.close()


def test_implicit_general_refuses(amd):
    e = amd.StepEngine(2, 8, model=2, seed=1)
    e.set_all_params(H.implicit_params(2, 8, seed=1, mean_volume=6, cvr=0.5))
    e.reset()
    with pytest.raises(ValueError, match="IMPLICIT_GENERAL"):            # (ADC_EINVAL)
        e.ideal_profit(2048)
    with pytest.raises(ValueError, match="IMPLICIT_GENERAL"):
        e.bid_curves_build(2048)
    e.close()


def test_facade_keywords_run_the_reference_estimator(amd):
    from adcraft_amd import experiment_metrics as em
    from adcraft_amd.gymnasium_kw_env import BiddingSimulation
    env = BiddingSimulation(num_keywords=8)
    env.reset(seed=5)
    eng = env._engine
    eng.bid_curves_build(2048)
    ir_dev, _ = eng.bid_curves_fetch()
    for k in range(8):
        ir, cpc = em.get_explicit_kw_bid_cpc_impressions(env.keywords[k], NOTEBOOK)
        assert ir.shape == cpc.shape == NOTEBOOK.shape and ((cpc >= 0) & (cpc <= 4.4)).all()
        np.testing.assert_allclose(ir, ir_dev[0, k], rtol=1e-6, atol=1e-7)
    env.close()
