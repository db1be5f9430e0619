"""GPU parity of the device-resident MLP policy (parts/kernel_mlp_policy.inc) with the numpy restatement (tests/mlp_ref.py):
acts on the observation the last step left, the closed loop of run_days("mlp") against a day-by-day loop of restatement act +
the engine's host step, the rollout record, the metrics of run_baseline_episode, env groups, weight re-upload, refusals."""
import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _planes(model, N, K, seed, mean_volume=24):
    return H.explicit_params(N, K, seed) if model == 1 else H.implicit_params(N, K, seed, mean_volume=mean_volume, cvr=0.5)


def _engine(amd, N, K, model=0, seed=3, mean_volume=24, **kw):
    e = amd.StepEngine(N, K, model=model, seed=seed, **kw)
    e.set_all_params(_planes(model, N, K, seed + 1, mean_volume))
    e.reset()
    return e


def _assert_last(e, ref, envs=None, what=None):
    st = e.mlp_last()
    bids, budget = e.get_actions()
    st["bids"], st["budget"] = bids, budget
    for k in ("mean", "log_std", "action", "logp", "value", "bids", "budget"):
        got = st[k] if envs is None else st[k][envs]
        assert _same(got, ref[k]), (what, k, got, ref[k])


HIDDEN = [(32, 32), (64,), (256, 128, 64)]
# the host test's shapes, K x hidden, at a few envs; and a single env at every K
SHAPES = [(3 + i % 3, K, h) for i, K in enumerate((1, 7, 100, 256)) for h in HIDDEN] + [(1, K, (32, 32)) for K in (1, 7, 100, 256)]


@pytest.mark.parametrize("N,K,hidden", SHAPES)
def test_act_equals_the_restatement_on_the_last_observation(amd, N, K, hidden):
    """first day (zeros), then the observation a step left: replayed normals, the agent's own stream, deterministic"""
    rng = np.random.default_rng(7 * N + K)
    A = K + 1
    for case, (activation, two_heads) in enumerate((("tanh", False), ("relu", True), ("tanh", True))):
        value = normalize = case != 1
        pol = R.random_policy(rng, K, hidden, activation, two_heads, value, normalize, scale=1.0 if normalize else 0.05,
                              log_std_clamp=(-4.0, 1.0) if case == 2 else None, bid_clip=2.0 if case == 0 else None)
        if normalize:
            pol.shift, pol.scale = R.realistic_norm(K)
        e = _engine(amd, N, K, seed=11 + case)
        seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
        keys = [R.agent_key(s) for s in seeds]
        e.mlp_init(pol, seeds)
        zero = np.zeros((N, 5 * K + 2), F)
        z = rng.standard_normal((N, A)).astype(F)
        e.mlp_act(0.0, z)                                           # tick 0 -> 1
        _assert_last(e, R.act(pol, zero, z), what=(case, "first day"))
        e.step_device()
        obs = R.flat_obs(e.fetch())
        assert obs[:, 2 * K + 1].min() == 1.0
        z = rng.standard_normal((N, A)).astype(F)
        e.mlp_act(0.0, z)                                           # tick 1 -> 2
        _assert_last(e, R.act(pol, obs, z), what=(case, "replay"))
        e.mlp_act(77.25)                                            # tick 2 -> 3, drawn at tick 2
        _assert_last(e, R.act(pol, obs, R.normals(keys, [2] * N, A), budget_override=77.25), what=(case, "own stream"))
        e.mlp_set_deterministic(True)
        e.mlp_act()
        ref = R.act(pol, obs, None, deterministic=True)
        _assert_last(e, ref, what=(case, "deterministic"))
        assert _same(ref["action"], ref["mean"])
        if value:
            assert _same(e.mlp_bootstrap_value(), ref["value"])
        e.close()


def test_first_day_input_is_zeros_after_an_auto_reset(amd):
    N, K = 6, 12
    rng = np.random.default_rng(3)
    pol = R.random_policy(rng, K, (32, 32), "tanh", value=True, scale=0.3)
    e = _engine(amd, N, K, seed=5, max_days=3, auto_reset=True)
    e.mlp_init(pol, deterministic=True)
    for day in range(3):
        e.mlp_step()
    out = e.fetch()
    assert out["terminated"].all() and np.abs(R.flat_obs(out)).sum() > 0        # the terminal observation is still in the arrays
    e.mlp_act()
    _assert_last(e, R.act(pol, np.zeros((N, 5 * K + 2), F), None, deterministic=True), what="after auto-reset")
    e.close()


def test_full_size_engine_on_a_seeded_slice(amd):
    N, K = 4096, 256
    rng = np.random.default_rng(99)
    pol = R.random_policy(rng, K, (32, 32), "tanh", value=True, normalize=True, scale=1.0)
    pol.shift, pol.scale = R.realistic_norm(K)
    e = _engine(amd, N, K, seed=21, mean_volume=8)
    seeds = np.arange(N, dtype=np.uint64) + 500
    e.mlp_init(pol, seeds)
    e.mlp_step()
    e.mlp_step()
    obs = R.flat_obs(e.fetch())
    envs = np.sort(rng.choice(N, 8, replace=False))
    envs[0], envs[-1] = 0, N - 1
    e.mlp_act()
    keys = [R.agent_key(s) for s in seeds[envs]]
    _assert_last(e, R.act(pol, obs[envs], R.normals(keys, [2] * len(envs), K + 1)), envs=envs, what="slice")
    e.close()


def test_many_small_envs(amd):
    """4096 envs of 4 keywords: the first envs, a seeded few and the last against the restatement"""
    N, K = 4096, 4
    rng = np.random.default_rng(17)
    pol = R.random_policy(rng, K, (32, 32), "tanh", two_heads=True, value=True, scale=0.3)
    e = _engine(amd, N, K, seed=23)
    seeds = np.arange(N, dtype=np.uint64) + 3
    e.mlp_init(pol, seeds)
    e.mlp_step()
    obs = R.flat_obs(e.fetch())
    envs = np.unique(np.concatenate([np.arange(9), rng.choice(N, 6, replace=False), [N - 2, N - 1]]))
    e.mlp_act()
    keys = [R.agent_key(s) for s in seeds[envs]]
    _assert_last(e, R.act(pol, obs[envs], R.normals(keys, [1] * len(envs), K + 1)), envs=envs, what="small envs")
    e.close()


def _loop(amd, model, N, K, T, pol, seeds, budget, deterministic, engine_kw):
    """the day-by-day loop: restatement act on the fetched observation + the engine's host step"""
    e = _engine(amd, N, K, model=model, **engine_kw)
    keys = [R.agent_key(s) for s in seeds]
    obs = np.zeros((N, 5 * K + 2), F)
    rec = {k: [] for k in ("action", "logp", "value", "reward", "terminated", "truncated", "obs", "bids", "out")}
    for t in range(T):
        z = None if deterministic else R.normals(keys, [t] * N, K + 1)
        a = R.act(pol, obs, z, deterministic=deterministic, budget_override=budget)
        out = e.step(a["bids"], a["budget"])
        done = out["terminated"].astype(bool) | out["truncated"].astype(bool)
        obs = R.flat_obs(out)
        obs[done] = 0.0                                            # auto-reset: the next episode's first observation
        for k in ("action", "logp", "value", "bids"):
            rec[k].append(a[k])
        rec["obs"].append(a["x"])
        rec["reward"].append(out["reward"].astype(F))
        rec["terminated"].append(out["terminated"].astype(bool))
        rec["truncated"].append(out["truncated"].astype(bool))
        rec["out"].append(out)
    boot = R.act(pol, obs, None, deterministic=True)["value"]
    state = e.get_rng_state()
    e.close()
    return {k: (np.stack(v) if k != "out" else v) for k, v in rec.items()}, boot, state


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("deterministic", [False, True])
def test_run_days_equals_the_day_by_day_loop_and_the_record_holds_it(amd, model, deterministic):
    """drift on, a binding budget, T crossing an auto-reset.  Three runs from the same rng state: run_days with the record, the
    same days one mlp_step at a time with every day's outputs and action buffers fetched, and the loop of restatement act + host
    step.  Every day: integer counts, float32 cost / revenue, float64 reward and cumulative profit, day, terminated / truncated,
    the cent bids and budgets the env got; the record's fields and the bootstrap value; bit for bit.  The deterministic runs have
    no normalisation, so their recorded observations are the raw outputs.  Then the record's refusal at T+1 and its reset"""
    N, K, T = 5, 24, 7
    rng = np.random.default_rng(40 + model)
    normalize = not deterministic
    pol = R.random_policy(rng, K, (32, 32), "tanh", two_heads=model == 1, value=True, normalize=normalize, scale=1.0 if normalize else 0.05)
    if normalize:
        pol.shift, pol.scale = R.realistic_norm(K)
    pol.layers[-1][1][1:K + 1] += F(0.8)                           # bids around 80 cents: auctions are won
    seeds = np.arange(N, dtype=np.uint64) + 9
    kw = dict(seed=60 + model, max_days=4, auto_reset=True, drift_enabled=True)
    # a budget that binds: half of what the least-spending env spends on the first day under an ample one (the first day's input
    # is zeros, so its actions do not depend on the budget)
    free, _, _ = _loop(amd, model, N, K, 1, pol, seeds, 1.0e9, deterministic, kw)
    free_spent = free["out"][0]["cost"].sum(axis=1, dtype=np.float64)
    budget = float(np.floor(50.0 * free_spent.min()) / 100.0)
    assert budget >= 0.5, free_spent
    e = _engine(amd, N, K, model=model, **kw)
    e.mlp_init(pol, seeds, deterministic)
    e.rollout_enable(T, obs=True)
    e.run_days("mlp", T, budget)
    got = e.rollout_fetch(bootstrap=True)
    last = e.fetch()
    state = e.get_rng_state()
    want, boot, want_state = _loop(amd, model, N, K, T, pol, seeds, budget, deterministic, kw)
    for k in ("obs", "action", "logp", "value", "reward", "terminated", "truncated"):
        assert _same(got[k], want[k]), (k, got[k], want[k])
    assert _same(R.cent_bids(got["action"][:, :, 1:], pol.bid_clip), want["bids"])
    if not normalize:                                              # the recorded input of day t + 1 is day t's raw observation
        for t in range(T - 1):
            raw = R.flat_obs(want["out"][t])
            raw[want["terminated"][t] | want["truncated"][t]] = 0.0
            assert _same(got["obs"][t + 1], raw), t
    assert want["terminated"][3].all() and not want["terminated"][2].any()
    bids, bud = e.get_actions()
    assert _same(bids, want["bids"][-1]) and np.all(bud == F(budget))
    outputs = ("impressions", "buyside_clicks", "sellside_conversions", "cost", "revenue", "reward", "cumulative_profit", "days_passed",
               "terminated", "truncated")
    for k in outputs:
        assert _same(np.asarray(last[k]), np.asarray(want["out"][-1][k])), k
    # the same days one device step at a time: every day's raw outputs and the actions the env was given
    d = _engine(amd, N, K, model=model, **kw)
    d.mlp_init(pol, seeds, deterministic)
    for t in range(T):
        d.mlp_step(budget)
        day, (bids_t, bud_t) = d.fetch(), d.get_actions()
        for k in outputs:
            assert _same(np.asarray(day[k]), np.asarray(want["out"][t][k])), (t, k)
        assert day["reward"].dtype == np.float64
        assert _same(bids_t, want["bids"][t]) and np.all(bud_t == F(budget)), t
    d.close()
    assert _same(free["bids"][0], want["bids"][0])
    spent = want["out"][0]["cost"].sum(axis=1, dtype=np.float64)
    print("model", model, "first day: spent", spent, "of", budget, "- with an ample budget", free_spent)
    assert (spent < free_spent).all() and (model != 0 or (spent <= budget + 1e-3).all())          # the budget did bind
    assert want["out"][-1]["buyside_clicks"].sum() > 0
    assert _same(got["bootstrap_value"], boot)
    assert all(np.array_equal(a, b) for a, b in zip(state, want_state))
    # day T+1 is refused, by either entry point, and changes nothing; a reset starts over
    with pytest.raises(ValueError, match="rollout"):
        e.run_days("mlp", 1, budget)
    with pytest.raises(ValueError, match="rollout"):
        e.mlp_step(budget)
    assert all(np.array_equal(a, b) for a, b in zip(state, e.get_rng_state()))
    assert _same(e.rollout_fetch()["action"], want["action"])
    e.rollout_reset()
    assert e.rollout_fetch()["action"].shape == (0, N, K + 1)
    e.mlp_step(budget)
    again = e.rollout_fetch()
    assert again["action"].shape == (1, N, K + 1) and _same(again["action"][0], e.mlp_last()["action"])
    e.close()


def _grouped(amd, groups, N, K, T, pol, seeds):
    e = _engine(amd, N, K, seed=70, mean_volume=8, max_days=4, auto_reset=True)
    e.set_env_groups(groups)
    e.mlp_init(pol, seeds)
    e.rollout_enable(T)
    e.run_days("mlp", T, 50.0)
    rec, last, g = e.rollout_fetch(bootstrap=True), e.fetch(), e.env_groups()
    e.close()
    return rec, last, g


def test_run_days_in_env_groups_equals_one_group(amd):
    N, K, T = 2048, 16, 6
    rng = np.random.default_rng(8)
    pol = R.random_policy(rng, K, (32, 32), "tanh", value=True, scale=0.3)
    pol.layers[-1][1][1:] += F(0.7)
    seeds = np.arange(N, dtype=np.uint64) + 1
    base, base_last, g1 = _grouped(amd, 1, N, K, T, pol, seeds)
    assert g1 == 1 and base["reward"].any()
    for groups in (2, 4, 0):
        rec, last, g = _grouped(amd, groups, N, K, T, pol, seeds)
        assert groups == 0 or g == groups
        for k in base:
            assert _same(rec[k], base[k]), (groups, k)
        for k in ("buyside_clicks", "cost", "revenue", "reward"):
            assert _same(np.asarray(last[k]), np.asarray(base_last[k])), (groups, k)


def test_run_baseline_episode_gives_the_host_formula_on_the_loop_trajectories(amd):
    from adcraft_amd.closed_loop import run_baseline_episode
    N, K, days = 4, 20, 9
    rng = np.random.default_rng(12)
    pol = R.random_policy(rng, K, (32, 32), "relu", scale=0.2)
    pol.layers[-1][1][1:] += F(0.6)
    pol.layers[-1][1][0] = F(500.0)                                # the policy's own budget (budget=0.0 below: no override)
    kw = dict(seed=33, max_days=days)
    e = _engine(amd, N, K, **kw)
    got = run_baseline_episode(e, policy="mlp", mlp=pol, deterministic=True, n_samples=256, budget=0.0)
    e.close()
    # the same days by the restatement and the host step, the ideal sums from the engine
    e = _engine(amd, N, K, **kw)
    e.bid_curves_build(256)
    e.metrics_enable(True)
    e.metrics_reset()
    obs = np.zeros((N, 5 * K + 2), F)
    cents = np.zeros((N, K), np.int64)
    for t in range(days):
        a = R.act(pol, obs, None, deterministic=True)
        e.ideal_step(fetch=False)
        out = e.step(a["bids"], a["budget"])
        obs = R.flat_obs(out)
        cents += np.rint(out["revenue"].astype(np.float64) * 100).astype(np.int64) - np.rint(out["cost"].astype(np.float64) * 100).astype(np.int64)
    _, ideal, ideal_pos = e.metrics_read_nk()
    e.close()
    profit, n = cents / 100.0, float(days)
    akncp = np.median((profit / n) / (ideal_pos / n), axis=1)
    den = ideal.sum(axis=1)
    ncp = profit.sum(axis=1) / np.where(den <= 0.0, 1.0, den)
    assert np.array_equal(got["kw_profit_sum"], profit) and np.abs(profit).sum() > 0
    assert np.array_equal(got["AKNCP"], akncp) and np.array_equal(got["NCP"], ncp)


def test_weight_reupload_changes_the_next_actions_and_nothing_else(amd):
    N, K = 4, 10
    rng = np.random.default_rng(2)
    pol1 = R.random_policy(rng, K, (32, 32), "tanh", value=True, scale=0.3)
    pol2 = R.random_policy(rng, K, (32, 32), "tanh", value=True, scale=0.3)
    seeds = np.arange(N, dtype=np.uint64) + 77
    keys = [R.agent_key(s) for s in seeds]
    engines = [_engine(amd, N, K, seed=13) for _ in range(2)]
    for e in engines:
        e.mlp_init(pol1, seeds)
        e.mlp_step()
        e.mlp_step()
    obs = R.flat_obs(engines[0].fetch())
    assert _same(obs, R.flat_obs(engines[1].fetch()))
    engines[0].mlp_set_weights(pol2)
    for e in engines:
        e.mlp_act()
    z = R.normals(keys, [2] * N, K + 1)                            # the third act's draws, with or without the upload
    _assert_last(engines[0], R.act(pol2, obs, z), what="new weights")
    _assert_last(engines[1], R.act(pol1, obs, z), what="old weights")
    assert not _same(engines[0].mlp_last()["action"], engines[1].mlp_last()["action"])
    for a, b in zip(engines[0].get_rng_state(), engines[1].get_rng_state()):
        assert np.array_equal(a, b)
    engines[0].mlp_set_weights(pol1)
    for e in engines:
        e.mlp_act()
    assert _same(engines[0].mlp_last()["action"], engines[1].mlp_last()["action"])      # tick 3 on both: the agents' streams moved alike
    for e in engines:
        e.close()


def test_default_agent_keys_in_a_stochastic_act(amd):
    """without per-env seeds the agents' keys come from the engine's seed and the global env id"""
    N, K, base = 5, 9, 4096
    rng = np.random.default_rng(31)
    pol = R.random_policy(rng, K, (32, 32), "tanh", value=True, scale=0.3)
    e = amd.StepEngine(N, K, seed=123456789, env_id_base=base)
    e.set_all_params(_planes(0, N, K, 5))
    e.reset()
    e.mlp_init(pol)
    keys = [R.default_agent_key(123456789, base + n) for n in range(N)]
    zero = np.zeros((N, 5 * K + 2), F)
    for tick in range(2):
        e.mlp_act()
        _assert_last(e, R.act(pol, zero, R.normals(keys, [tick] * N, K + 1)), what=("default keys", tick))
    e.close()


def test_act_at_the_most_keywords_the_engine_takes(amd):
    """4096 keywords, means and log-stds from the network: 114 KB of dynamic LDS per workgroup, the most a policy can ask for and
    more than the 64 KB a launch gets without asking; first day and after a step"""
    N, K = 2, 4096
    rng = np.random.default_rng(55)
    pol = R.random_policy(rng, K, (32,), "tanh", two_heads=True, value=True, normalize=True, scale=1.0)
    pol.shift, pol.scale = R.realistic_norm(K)
    e = _engine(amd, N, K, seed=41, mean_volume=8)
    seeds = np.array([7, 8], np.uint64)
    keys = [R.agent_key(s) for s in seeds]
    e.mlp_init(pol, seeds)
    e.mlp_act()
    _assert_last(e, R.act(pol, np.zeros((N, 5 * K + 2), F), R.normals(keys, [0] * N, K + 1)), what="first day")
    e.step_device()
    obs = R.flat_obs(e.fetch())
    e.mlp_act()
    _assert_last(e, R.act(pol, obs, R.normals(keys, [1] * N, K + 1)), what="after a step")
    e.close()


def test_refusals_that_need_an_engine(amd):
    N, K = 2, 4
    rng = np.random.default_rng(1)
    e = _engine(amd, N, K, seed=1)
    for call in (lambda: e.run_days("mlp", 1), lambda: e.mlp_act(), lambda: e.mlp_step(), lambda: e.rollout_enable(4)):
        with pytest.raises(AssertionError, match="mlp_init"):
            call()
    with pytest.raises(ValueError, match="inputs"):
        e.mlp_init(R.random_policy(rng, K + 1, (8,)))
    pol = R.random_policy(rng, K, (8,), value=False)
    e.mlp_init(pol)
    with pytest.raises(AssertionError, match="value network"):
        e.mlp_bootstrap_value()
    with pytest.raises(AssertionError, match="rollout_enable"):
        e.rollout_fetch()
    for other in (R.random_policy(rng, K, (16,)), R.random_policy(rng, K, (8, 8)), R.random_policy(rng, K, (8,), two_heads=True),
                  R.random_policy(rng, K, (8,), value=True), R.random_policy(rng, K, (8,), normalize=True)):
        with pytest.raises(ValueError, match="shapes"):
            e.mlp_set_weights(other)                               # (not the shapes of mlp_init: nothing is uploaded)
    e.mlp_set_weights(R.random_policy(rng, K, (8,)))
    e.rollout_enable(2)
    e.run_days("mlp", 2)
    with pytest.raises(ValueError, match="rollout"):
        e.run_days("mlp", 1)
    e.rollout_enable(0)
    e.run_days("mlp", 3)                                           # no record: no horizon
    e.close()


# ---- the refusals that pass through the helpers the learned agent's host files share (parts/mlp_core.inc: mlp_have,
# population_member_check, learners_ready, the layer upload's callers; parts/mlp_api.inc: squash_set, bounds_set), by their whole
# sentence, two set up at once wherever a shared helper could put them in another order -------------------------------------------
SAID = dict(
    null="engine handle is NULL",
    no_init="adc_engine_mlp_init has not been called",
    network="network: 0 (policy) or 1 (value)",
    layer="no such layer",
    weights="weights or bias is NULL",
    no_population="adc_engine_mlp_population has not been called",
    no_learners="adc_engine_mlp_learners has not been called",
    member="no such member",
    flat_null="flat_p is NULL",
    theta_null="theta_q is NULL",
    log_std_null="log_std is NULL",
    two_heads="a two-headed policy has no log_std vector",
    squash_pair="lo and hi: both vectors, or both NULL (squash off)",
    squash_population="the squashed action with a population active is not supported (adc_engine_mlp_population(0) first)",
    squash_learners="the squashed action with learners active is not supported (adc_engine_mlp_learners(0) first)",
    squash_bounded="the squashed action together with the bounded act is not supported (adc_engine_mlp_set_bounds(NULL, NULL) first)",
    squash_needs_learners="the learners' squashed action needs learners (adc_engine_mlp_learners)",
    squash_learners_bounded="the squashed action together with the bounded act is not supported (adc_engine_mlp_learners_set_bounds(NULL, NULL) first)",
    squash_order="squash bounds: finite, hi > lo",
    squash_overflow="squash bounds: hi - lo overflows",
    bounds_pair="lo and hi: both vectors, or both NULL (bounds off)",
    bounds_population="the bounded act with a population active is not supported (adc_engine_mlp_population(0) first)",
    bounds_learners="learners are active: their bounds are set through adc_engine_mlp_learners_set_bounds",
    bounds_needs_learners="the learners' bounded act needs learners (adc_engine_mlp_learners)",
    bounds_squashed="the bounded act together with the squashed action is not supported (adc_engine_mlp_set_squash(NULL, NULL) first)",
    bounds_two_heads="the bounded act needs the policy with the free log_std head: a two-headed policy (2A outputs) is not supported",
    bounds_order="action bounds: finite, hi > lo",
    bounds_overflow="action bounds: hi - lo overflows or vanishes",
    py_no_init="mlp_init has not been called",
)


def _refused(kind, text, call):
    with pytest.raises(kind) as info:
        call()
    assert str(info.value) == text, (str(info.value), text)


def _walk_the_refusals(e, pol, two, seeds, refused):
    """every successful call in order, on any engine; the refusals between them only where `refused` is _refused"""
    from adcraft_amd import _ffi
    STATE, VALUE = _ffi.EngineStateError, ValueError
    K = e.num_keywords
    lo, hi, big = np.full(K + 1, 0.5, F), np.full(K + 1, 2.0, F), np.full(K + 1, 3.0e38, F)
    LO, HI = lo.ctypes.data, hi.ctypes.data
    (w, b), out = pol.layers[0], np.zeros(4096, F)
    W, B, OUT = w.ctypes.data, b.ctypes.data, out.ctypes.data

    def c(name, *args, h=True):
        return lambda: _ffi.check(getattr(e._lib, "adc_engine_mlp_" + name)(e._h if h else None, *args))

    # the handle, then the policy, before anything else that is wrong with the call
    first = (("set_layer", 2, -1, None, None), ("set_member_layer", -1, -1, None, None), ("get_member_params", -1, None),
             ("set_learner_layer", -1, 2, -1, None, None), ("set_learner_log_std", -1, None), ("get_learner_params", -1, None),
             ("set_squash", LO, None), ("learners_set_squash", LO, None), ("set_bounds", LO, None), ("learners_set_bounds", LO, None))
    for name, *args in first:
        refused(VALUE, SAID["null"], c(name, *args, h=False))
        refused(STATE, SAID["no_init"], c(name, *args))
    for call in (lambda: e.mlp_set_weights(pol), lambda: e.mlp_set_member(0, pol), lambda: e.mlp_set_learner(0, pol), lambda: e.mlp_learner_param_count()):
        refused(STATE, SAID["py_no_init"], call)
    # a two-headed policy: no log_std vector (named before the NULL vector, after the member), no bounded act
    e.mlp_init(two, seeds)
    e.mlp_learners(2)
    refused(VALUE, SAID["member"], c("set_learner_log_std", 2, None))
    refused(VALUE, SAID["two_heads"], c("set_learner_log_std", 0, None))
    refused(STATE, SAID["bounds_two_heads"], lambda: e.mlp_learners_set_bounds(lo, hi))
    # the single policy
    e.mlp_init(pol, seeds)
    refused(VALUE, SAID["network"], c("set_layer", 2, -1, None, None))
    for net, layer in ((0, -1), (0, 3), (1, 2)):
        refused(VALUE, SAID["layer"], c("set_layer", net, layer, None, None))
    for pair in ((None, B), (W, None)):
        refused(VALUE, SAID["weights"], c("set_layer", 0, 0, *pair))
    for name, *args in first[1:3]:
        refused(STATE, SAID["no_population"], c(name, *args))
    for name, *args in first[3:6]:
        refused(STATE, SAID["no_learners"], c(name, *args))
    for name in ("mlp_set_squash", "mlp_learners_set_squash", "mlp_set_bounds", "mlp_learners_set_bounds"):
        refused(VALUE, name + ": lo and hi, or neither", lambda: getattr(e, name)(lo, None))
        refused(VALUE, name + ": lo and hi, or neither", lambda: getattr(e, name)(None, hi))
    refused(STATE, SAID["squash_needs_learners"], c("learners_set_squash", LO, None))
    refused(VALUE, SAID["bounds_pair"], c("learners_set_bounds", LO, None))
    refused(STATE, SAID["bounds_needs_learners"], lambda: e.mlp_learners_set_bounds(lo, hi))
    refused(VALUE, SAID["squash_order"], lambda: e.mlp_set_squash(hi, lo))
    refused(VALUE, SAID["squash_overflow"], lambda: e.mlp_set_squash(-big, big))
    refused(VALUE, SAID["bounds_order"], lambda: e.mlp_set_bounds(hi, lo))
    refused(VALUE, SAID["bounds_overflow"], lambda: e.mlp_set_bounds(-big, big))
    e.mlp_set_bounds(lo, hi)
    refused(VALUE, SAID["squash_pair"], c("set_squash", LO, None))              # (the lone vector before the bounded act)
    refused(STATE, SAID["squash_bounded"], lambda: e.mlp_set_squash(lo, hi))
    e.mlp_set_bounds()
    e.mlp_set_squash(lo, hi)
    refused(STATE, SAID["bounds_squashed"], lambda: e.mlp_set_bounds(lo, hi))
    e.mlp_set_squash()
    # a population
    e.mlp_population(2)
    refused(VALUE, SAID["squash_pair"], c("set_squash", LO, None))              # (the lone vector before the population)
    refused(STATE, SAID["squash_population"], lambda: e.mlp_set_squash(lo, hi))
    refused(VALUE, SAID["bounds_pair"], c("set_bounds", LO, None))
    refused(STATE, SAID["bounds_population"], lambda: e.mlp_set_bounds(lo, hi))
    refused(STATE, SAID["squash_needs_learners"], c("learners_set_squash", LO, None))
    for member in (-1, 2):
        refused(VALUE, SAID["member"], c("set_member_layer", member, -1, None, None))
        refused(VALUE, SAID["member"], c("get_member_params", member, None))
    for layer in (-1, 3):
        refused(VALUE, SAID["layer"], c("set_member_layer", 0, layer, None, None))
    for pair in ((None, B), (W, None)):
        refused(VALUE, SAID["weights"], c("set_member_layer", 1, 0, *pair))
    refused(VALUE, SAID["flat_null"], c("get_member_params", 1, None))
    for name, *args in first[3:6]:
        refused(STATE, SAID["no_learners"], c(name, *args))
    e.mlp_population(0)
    # learners
    e.mlp_learners(2)
    for member in (-1, 2):
        refused(VALUE, SAID["member"], c("set_learner_layer", member, 2, -1, None, None))
        refused(VALUE, SAID["member"], c("set_learner_log_std", member, None))
        refused(VALUE, SAID["member"], c("get_learner_params", member, None))
    refused(VALUE, SAID["network"], c("set_learner_layer", 0, 2, -1, None, None))
    for net, layer in ((0, -1), (0, 3), (1, 2)):
        refused(VALUE, SAID["layer"], c("set_learner_layer", 1, net, layer, None, None))
    for pair in ((None, B), (W, None)):
        refused(VALUE, SAID["weights"], c("set_learner_layer", 1, 0, 0, *pair))
    refused(VALUE, SAID["log_std_null"], c("set_learner_log_std", 1, None))
    refused(VALUE, SAID["theta_null"], c("get_learner_params", 1, None))
    refused(STATE, SAID["no_population"], c("set_member_layer", 0, 0, W, B))
    refused(STATE, SAID["no_population"], c("get_member_params", 0, OUT))
    refused(VALUE, SAID["squash_pair"], c("set_squash", LO, None))              # (the lone vector before the learners)
    refused(STATE, SAID["squash_learners"], lambda: e.mlp_set_squash(lo, hi))
    refused(STATE, SAID["bounds_learners"], lambda: e.mlp_set_bounds(lo, hi))
    refused(VALUE, SAID["squash_pair"], c("learners_set_squash", LO, None))
    refused(VALUE, SAID["squash_order"], lambda: e.mlp_learners_set_squash(hi, lo))
    refused(VALUE, SAID["bounds_order"], lambda: e.mlp_learners_set_bounds(hi, lo))
    e.mlp_learners_set_bounds(lo, hi)
    refused(STATE, SAID["squash_learners_bounded"], c("learners_set_squash", LO, None))     # (the bounded act before the lone vector ...)
    refused(VALUE, SAID["squash_pair"], c("learners_set_squash", None, HI))                 # (... which is named where no lo asks for a squash)
    refused(STATE, SAID["squash_learners_bounded"], lambda: e.mlp_learners_set_squash(lo, hi))
    e.mlp_learners_set_bounds()
    e.mlp_learners_set_squash(lo, hi)
    refused(STATE, SAID["bounds_squashed"], lambda: e.mlp_learners_set_bounds(lo, hi))
    e.mlp_learners_set_squash()
    e.mlp_learners(0)


def test_every_shared_refusal_by_its_whole_sentence_and_which_one_wins(amd):
    """4 envs, 3 keywords, policy hidden (5, 3) and value hidden (6,), free log_std (two-headed where the sentence is about it).
    Every expectation is the parent commit's sentence and order, read off its code"""
    N, K = 4, 3
    rng = np.random.default_rng(7)
    pol, two = R.ragged_policy(rng, K), R.ragged_policy(rng, K, two_heads=True)
    seeds = np.arange(N, dtype=np.uint64) + 5
    e, twin = (_engine(amd, N, K, seed=19) for _ in range(2))
    _walk_the_refusals(e, pol, two, seeds, _refused)
    _walk_the_refusals(twin, pol, two, seeds, lambda *a: None)
    # after all of it the engine acts, and as the twin that saw no refusal
    for x in (e, twin):
        x.mlp_step()
        x.mlp_act()
    a, b = e.mlp_last(), twin.mlp_last()
    for k in a:
        assert _same(a[k], b[k]), k
    for x, y in zip(e.get_actions(), twin.get_actions()):
        assert _same(x, y)
    assert np.abs(a["action"]).sum() > 0
    e.close()
    twin.close()
