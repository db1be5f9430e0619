"""GPU parity of the device-resident NaiveInterpolationStrategy (parts/kernel_interp_agent.inc) with the numpy restatement
(tests/interp_ref.py): through the C ABI on host observations and replayed uniforms, in the closed loop on the agent's own
Philox stream, at full size, in env groups and under the day graph; plus its capacity and input checks."""
import numpy as np
import pytest

from oracle import capi as orc
from tests import helpers as H
from tests import interp_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _uniform53(a, b):
    return float(((int(a) >> 5) << 26) | (int(b) >> 6)) * 2.0 ** -53


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def _own_uniforms(seeds, K, tick):
    """the uniforms the agent draws at `tick`: Philox call (0, stage 13, keyword, tick) under splitmix64(seed ^ const)"""
    keys = [_splitmix64(int(s) ^ 0x3C6EF372FE94F82B) for s in seeds]
    u = np.zeros((len(seeds), K))
    for n, key in enumerate(keys):
        for k in range(K):
            w = orc.philox([0, 13, k, tick], [key & 0xFFFFFFFF, key >> 32])
            u[n, k] = _uniform53(w[0], w[1])
    return u


def _grid_bids(st, grid):
    idx = st["bid_index"]
    return np.where(idx >= 0, np.asarray(grid)[np.maximum(idx, 0)], 0.01)


def _assert_caches(e, ref, st=None, envs=None):
    st = e.interp_state() if st is None else st
    ent = e.interp_entries()
    for r, n in enumerate(range(ref.N) if envs is None else envs):
        for k in range(ref.K):
            c = ref.caches[r][k]
            assert st["ave_rpc"][n, k] == c.ave_rpc and st["num_rpc_obs"][n, k] == c.n_rpc
            assert st["num_sctr_obs"][n, k] == c.n_sctr and st["max_observed"][n, k] == c.max_observed
            assert c.n_sctr == 0 or st["ave_sctr"][n, k] == c.ave_sctr
            kc, m = sorted(c.clicks), ent["n_clicks"][n, k]
            assert list(ent["clicks_cent"][n, k, :m]) == kc
            assert list(ent["ave_clicks"][n, k, :m]) == [c.clicks[x][0] for x in kc]
            assert list(ent["clicks_count"][n, k, :m]) == [c.clicks[x][1] for x in kc]
            pc, m = sorted(c.cpc), ent["n_cpc"][n, k]
            assert list(ent["cpc_cent"][n, k, :m]) == pc
            assert list(ent["ave_cpc"][n, k, :m]) == [c.cpc[x][0] for x in pc]
            assert list(ent["cpc_count"][n, k, :m]) == [c.cpc[x][1] for x in pc]


def test_c_abi_on_host_observations_and_replayed_uniforms(amd):
    """host updates (the agent's own bids; caller bids at half cents, 0, negative and above $3.00), the default, a growing
    and a shuffled grid, replayed uniforms: bids, action buffer, float64 budget and beliefs and the caches bit for bit"""
    rng = np.random.default_rng(41)
    N, K, T = 2, 9, 40
    for case in range(3):
        e = amd.StepEngine(N, K, seed=3, max_days=T)
        if case == 0:
            grid, thr, step = np.linspace(0.01, 3.00, 300), -0.2, 0.03
        elif case == 1:
            grid, thr, step = np.arange(0.01, 0.11, 0.01), -0.1, 0.03
        else:
            grid = rng.permutation(np.concatenate([np.arange(0.005, 2.0, 0.01), [3.1, 3.5, 4.25]]))
            thr, step = -0.3, 0.05
        e.interp_init(thr, step, grid, 0)
        ref = R.InterpAgentRef(N, K, thr, step)
        prev = np.full((N, K), 0.01)
        max_bid = 0.10
        for t in range(T):
            clicks = rng.integers(0, 6, (N, K)) * (rng.random((N, K)) < 0.7)
            cost = (clicks * rng.random((N, K)) * 0.9).astype(np.float32)
            conv = np.minimum(clicks, rng.integers(0, 3, (N, K)))
            rev = (conv * rng.random((N, K)) * 4).astype(np.float32)
            if case == 2 and t % 3 == 1:
                prev = np.where(rng.random((N, K)) < 0.5, prev,
                                rng.choice([0.0, -0.4, 3.7, 0.125, 0.015, 1.005, 2.995, 12.0], (N, K)))
            e.interp_update(prev, clicks, cost, conv, rev)
            ref.update(prev, clicks, cost, conv, rev)
            if case == 1:
                grid = np.arange(0.01, max_bid + 0.01, 0.01)
                e.interp_set_allowed_bids(grid)
                max_bid = min(max_bid + 0.03, 3.0)
            u = rng.random((N, K))
            e.interp_act(0.0, u)
            bids_ref, drew = ref.act(grid, u)
            st = e.interp_state()
            bids, budget = e.get_actions()
            assert np.array_equal(_grid_bids(st, grid), bids_ref), (case, t)
            assert np.array_equal(st["bid_index"] >= 0, drew), (case, t)
            assert np.array_equal(bids, (np.maximum(np.rint(bids_ref * 100.0), 1.0) / 100.0).astype(np.float32)), (case, t)
            assert np.array_equal(st["budget"], ref.budget), (case, t)
            assert np.array_equal(st["profit_beliefs"], ref.profit_beliefs), (case, t)
            assert np.array_equal(st["cost_beliefs"], ref.cost_beliefs), (case, t)
            assert np.array_equal(budget, (np.rint(ref.budget * 100.0) / 100.0).astype(np.float32)), (case, t)
            _assert_caches(e, ref, st)
            prev = bids_ref
        e.close()


@pytest.mark.parametrize("model", ["implicit", "explicit"])
def test_closed_loop_on_the_agents_own_stream(amd, model):
    """interp_step + step_device on device-resident observations vs the restatement fed the fetched observations and the
    uniforms of the agent's Philox stream"""
    N, K, T = 3, 70, 12
    if model == "implicit":
        e = amd.StepEngine(N, K, seed=17, max_days=T)
        e.set_all_params(H.implicit_params(N, K, seed=91, mean_volume=64, cvr=0.5))
    else:
        e = amd.StepEngine(N, K, model=1, seed=18, max_days=T)
        e.set_all_params(H.explicit_params(N, K, seed=92))
    e.reset()
    seeds = np.array([5, 6, 7], np.uint64)
    e.interp_init(-0.2, 0.03, None, 0, seeds)
    grid = np.linspace(0.01, 3.00, 300)
    ref = R.InterpAgentRef(N, K)
    prev = np.full((N, K), 0.01)
    z = np.zeros((N, K))
    obs = dict(buyside_clicks=z, cost=z, sellside_conversions=z, revenue=z)
    for t in range(T):
        e.interp_step(100000.0)
        ref.update(prev, obs["buyside_clicks"], obs["cost"], obs["sellside_conversions"], obs["revenue"])
        bids_ref, _ = ref.act(grid, _own_uniforms(seeds, K, t))
        st = e.interp_state()
        assert np.array_equal(_grid_bids(st, grid), bids_ref), t
        assert np.array_equal(st["budget"], ref.budget) and np.array_equal(st["cost_beliefs"], ref.cost_beliefs), t
        _, budget = e.get_actions()
        assert np.all(budget == 100000.0)
        e.step_device()
        obs = e.fetch()
        prev = bids_ref
    _assert_caches(e, ref)
    assert sum(len(c.cpc) for row in ref.caches for c in row) > 20        # the loop did reach the interpolation
    e.close()


def _episode(amd, N, K, days, groups, graph, seed=23):
    e = amd.StepEngine(N, K, seed=seed, max_days=days)
    e.set_all_params(H.implicit_params(N, K, seed=seed + 1, mean_volume=8, cvr=0.5))
    e.reset()
    e.set_env_groups(groups)
    e.interp_init(-0.2, 0.03, None, 0, np.arange(N, dtype=np.uint64) + 100)
    e.run_days("interpolation", days, 100000.0, graph=graph)
    out = e.interp_state(), e.interp_entries(), e.fetch()
    e.close()
    return out


def test_run_days_is_the_same_in_groups_as_one_group_and_under_the_graph(amd):
    N, K, days = 2048, 48, 10
    base = _episode(amd, N, K, days, 1, False)
    for groups, graph in ((4, False), (2, False), (1, True)):
        got = _episode(amd, N, K, days, groups, graph)
        for a, b in zip(base[:2], got[:2]):
            for key in a:
                assert np.array_equal(a[key], b[key]), (groups, graph, key)
        for key in ("buyside_clicks", "cost", "revenue"):
            assert np.array_equal(base[2][key], got[2][key]), (groups, graph, key)


def test_full_size_episode_slice_matches_the_restatement(amd):
    """4096 x 256, 60 days of run_days("interpolation") on the default grid with the per-step ideal; the same days stepped
    one by one give the same state, and 4 envs of them (one per group, the last included) match the restatement"""
    N, K, days = 4096, 256, 60
    planes = H.implicit_params(N, K, seed=77, mean_volume=8, cvr=0.5)
    seeds = np.arange(N, dtype=np.uint64) + 1000
    a = amd.StepEngine(N, K, seed=31, max_days=days)
    a.set_all_params(planes)
    a.reset()
    a.bid_curves_build(256)
    a.interp_init(-0.2, 0.03, None, 0, seeds)
    a.run_days("interpolation", days, 100000.0)
    sa = a.interp_state()
    a.close()
    envs = [0, 1024 + 3, 2048 + 77, N - 1]
    b = amd.StepEngine(N, K, seed=31, max_days=days)
    b.set_all_params(planes)
    b.reset()
    b.interp_init(-0.2, 0.03, None, 0, seeds)
    grid = np.linspace(0.01, 3.00, 300)
    ref = R.InterpAgentRef(len(envs), K)
    prev = np.full((len(envs), K), 0.01)
    z = np.zeros((len(envs), K))
    obs = dict(buyside_clicks=z, cost=z, sellside_conversions=z, revenue=z)
    for t in range(days):
        b.interp_step(100000.0)
        ref.update(prev, obs["buyside_clicks"], obs["cost"], obs["sellside_conversions"], obs["revenue"])
        prev, _ = ref.act(grid, _own_uniforms(seeds[envs], K, t))
        b.step_device()
        f = b.fetch()
        obs = {k: f[k][envs] for k in ("buyside_clicks", "cost", "sellside_conversions", "revenue")}
    sb = b.interp_state()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert np.array_equal(sb["budget"][envs], ref.budget) and np.array_equal(sb["profit_beliefs"][envs], ref.profit_beliefs)
    _assert_caches(b, ref, sb, envs)
    b.close()


def test_capacity_refuses_the_update_that_could_overflow(amd):
    N, K = 2, 5
    e = amd.StepEngine(N, K, seed=1, max_days=60)
    e.set_all_params(H.implicit_params(N, K, seed=2))
    e.reset()
    e.interp_init(-0.2, 0.03, None, 5)
    z = np.zeros((N, K))
    for t in range(5):
        e.interp_update(np.full((N, K), 0.01 * (t + 1)), z + 1, z + 0.5, z, z)
    before = e.interp_entries(), e.interp_state()
    with pytest.raises(ValueError):
        e.interp_update(np.full((N, K), 0.5), z + 1, z + 0.5, z, z)
    with pytest.raises(ValueError):
        e.interp_step(0.0)
    with pytest.raises(ValueError):
        e.run_days("interpolation", 1, 1000.0)
    after = e.interp_entries(), e.interp_state()
    for a, b in zip(before, after):
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    assert before[0]["capacity"] == 5 and np.all(before[0]["n_clicks"] == 5)
    e.close()
    e = amd.StepEngine(N, K, seed=1, max_days=10)
    e.interp_init(-0.2, 0.03, None, 300)
    for t in range(320):
        e.interp_update(np.full((N, K), 0.01 * (t % 300 + 1)), z + 1, z + 0.5, z, z)
    assert np.all(e.interp_entries()["n_clicks"] == 300)
    e.close()


def test_bad_input_is_refused(amd):
    e = amd.StepEngine(1, 4, seed=1)
    g = np.linspace(0.01, 3.00, 300)
    for bad in (np.array([0.1, np.nan]), np.array([np.inf]), np.zeros(2049) + 0.5, np.zeros(0)):
        with pytest.raises(ValueError):
            e.interp_init(-0.2, 0.03, bad, 0)
    for thr, step in ((np.nan, 0.03), (-0.2, np.inf), (-np.inf, 0.03)):
        with pytest.raises(ValueError):
            e.interp_init(thr, step, g, 0)
    with pytest.raises(ValueError):
        e.interp_init(-0.2, 0.03, g, 301)
    e.interp_init(-0.2, 0.03, g, 0)
    with pytest.raises(ValueError):
        e.interp_set_allowed_bids(np.array([0.2, np.nan]))
    with pytest.raises(ValueError):
        e.interp_set_allowed_bids(np.zeros(4096) + 0.2)
    z = np.zeros((1, 4))
    with pytest.raises(ValueError):
        e.interp_update(np.array([[0.1, np.nan, 0.2, 0.3]]), z, z, z, z)
    assert np.all(e.interp_entries()["n_clicks"] == 0)
    e.close()


def test_run_baseline_episode_matches_a_step_by_step_run(amd):
    from adcraft_amd.closed_loop import run_baseline_episode
    N, K, days = 4, 32, 15
    planes = H.implicit_params(N, K, seed=5, mean_volume=8, cvr=0.5)
    seeds = np.arange(N, dtype=np.uint64) + 7

    def fresh():
        e = amd.StepEngine(N, K, seed=11, max_days=days)
        e.set_all_params(planes)
        e.reset()
        return e
    e = fresh()
    got = run_baseline_episode(e, policy="interpolation", agent_seeds=seeds, n_samples=256, per_keyword_sums=False)
    e.close()
    e = fresh()
    e.bid_curves_build(256)
    e.metrics_enable(True)
    e.metrics_reset()
    e.interp_init(-0.2, 0.03, None, 0, seeds)
    for _ in range(days):
        e.interp_step(100000.0)
        e.ideal_step(fetch=False)
        e.step_device()
    akncp, ncp = e.metrics_akncp_ncp(float(days))
    e.close()
    assert np.array_equal(got["AKNCP"], akncp) and np.array_equal(got["NCP"], ncp)
