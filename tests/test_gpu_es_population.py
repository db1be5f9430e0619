"""GPU tests of policy populations (per-member weights of the MLP policy kernel) and of the evolution strategy over them
(parts/kernel_es.inc) against the host twin adc_mlp_act_host and the numpy restatement tests/es_ref.py, bit for bit; env
groups, resumed state, a learning run, refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import es_ref as E
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


def _engine(amd, N, K, seed=3, mean_volume=24, **kw):
    e = amd.StepEngine(N, K, seed=seed, **kw)
    e.set_all_params(H.implicit_params(N, K, seed + 1, mean_volume=mean_volume, cvr=0.5))
    e.reset()
    return e


STEP_FIELDS = ("impressions", "buyside_clicks", "sellside_conversions", "cost", "revenue", "reward", "cumulative_profit", "days_passed",
               "terminated", "truncated")


@pytest.mark.parametrize("members", [4, 3, 12])
def test_members_equal_to_the_centre_change_nothing(amd, members):
    """3 recorded days of run_days("mlp"): a population whose members all hold the centre gives the bits of no population"""
    N, K = 12, 20
    rng = np.random.default_rng(5)
    pol = R.random_policy(rng, K, (32, 32), "tanh", value=True, normalize=True, scale=1.0)
    pol.shift, pol.scale = R.realistic_norm(K)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    runs = []
    for M in (0, members):
        e = _engine(amd, N, K, seed=31)
        e.mlp_init(pol, seeds)
        if M:
            e.mlp_population(M, rng.integers(0, M, N) if N % M or M == 4 else None)
            assert all(_same(e.mlp_member_params(m), E.flat_params(pol)) for m in range(M))
        assert _same(e.mlp_params(), E.flat_params(pol))
        e.rollout_enable(3, obs=True)
        e.run_days("mlp", 3, 0.0)
        out = e.fetch()
        rec = e.rollout_fetch(bootstrap=True)
        last = e.mlp_last()
        runs.append((out, rec, last))
        e.close()
    (o0, r0, l0), (o1, r1, l1) = runs
    for k in STEP_FIELDS:
        assert _same(o0[k], o1[k]), k
    assert sorted(r0) == sorted(r1) and float(np.abs(r0["action"]).sum()) > 0
    for k in r0:
        assert _same(r0[k], r1[k]), k
    for k in l0:
        assert _same(l0[k], l1[k]), k


@pytest.mark.parametrize("K,hidden", [(10, (32, 32)), (100, (32, 32)), (300, (16,))])
def test_every_env_acts_on_its_members_weights(amd, K, hidden):
    """distinct random members and a scattered map: action, bids, log-probability, value of every env equal the host twin on
    its member's weights, on the first day and on the observation a step left"""
    from adcraft_amd import _ffi
    from adcraft_amd.baselines.es_trainer import policy_from_flat
    lib = _ffi.lib()
    N, M = 7, 3
    rng = np.random.default_rng(K)
    centre = R.random_policy(rng, K, hidden, "tanh", value=True, normalize=True, scale=1.0)
    centre.shift, centre.scale = R.realistic_norm(K)
    mem = [policy_from_flat(centre, (rng.standard_normal(E.flat_params(centre).size) * 0.05).astype(F)) for _ in range(M)]
    member_of_env = np.array([2, 0, 1, 1, 0, 2, 1], np.int32)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    keys = [R.agent_key(s) for s in seeds]
    e = _engine(amd, N, K, seed=41)
    e.mlp_init(centre, seeds)
    e.mlp_population(M, member_of_env)
    for m in range(M):
        e.mlp_set_member(m, mem[m])
        assert _same(e.mlp_member_params(m), E.flat_params(mem[m]))
    assert _same(e.mlp_params(), E.flat_params(centre))            # (the centre is untouched)
    obs = None
    for tick in range(2):
        e.mlp_act()
        st = e.mlp_last()
        st["bids"], st["budget"] = e.get_actions()
        for env in range(N):
            ref = R.twin_act(lib, mem[member_of_env[env]], None if obs is None else obs[env], key=keys[env], tick=tick)
            for k in ("mean", "log_std", "action", "logp", "value", "bids", "budget"):
                assert _same(st[k][env], ref[k][0]), (tick, env, k, st[k][env], ref[k][0])
        # members differ: the same env under another member's weights acts otherwise
        other = R.twin_act(lib, mem[(member_of_env[0] + 1) % M], None if obs is None else obs[0], key=keys[0], tick=tick)
        assert not _same(other["action"][0], st["action"][0])
        e.step_device()
        obs = R.flat_obs(e.fetch())
    e.close()


def _returns_of(e, days):
    """`days` days of mlp_step, the rewards the step outputs reported summed per env in float64, day by day from +0"""
    ret, ended = np.zeros(e.num_envs, np.float64), 0
    for _ in range(days):
        e.mlp_step(1000.0)
        out = e.fetch()
        ret = ret + np.asarray(out["reward"], np.float64)
        ended += int(np.asarray(out["terminated"]).sum() + np.asarray(out["truncated"]).sum())
    return ret, ended


ES_KW = [dict(sigma=0.05, lr=0.02, seed=99), dict(sigma=0.02, lr=0.05, optimiser="sgd", shaping="raw", l2=0.001, seed=0)]


@pytest.mark.parametrize("case", range(len(ES_KW)))
def test_three_generations_equal_the_restatement(amd, case):
    """perturbed members, device fitness (through auto-resets), the update from it: three generations, bit for bit; then the
    same run through run_days arrives at the same theta"""
    kw = dict(ES_KW[case])
    N, K, M, days = 8, 10, 4, 3
    rng = np.random.default_rng(50 + case)
    pol = R.random_policy(rng, K, (8,), "tanh", scale=0.3)
    agent_seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    member_of_env = np.repeat(np.arange(M), N // M)
    e = _engine(amd, N, K, seed=61, max_days=4, auto_reset=True)
    e.mlp_init(pol, agent_seeds)
    e.mlp_population(M)
    e.es_init(**kw)
    noise_seed = kw["seed"] or 61                               # (seed 0: the engine's)
    law = {k: v for k, v in kw.items() if k != "seed"}
    theta, m, v = E.flat_params(pol), np.zeros(E.flat_params(pol).size, F), np.zeros(E.flat_params(pol).size, F)
    st = e.es_state()
    assert _same(st["theta"], theta) and st["generation"] == 0 and not st["m"].any() and not st["v"].any()
    resets = 0
    for g in range(3):
        e.es_perturb()
        ref_members = E.members(theta, noise_seed, g, M, kw["sigma"])
        for mem in range(M):
            assert _same(e.mlp_member_params(mem), ref_members[mem]), (g, mem)
        assert _same(e.mlp_params(), theta)
        ret, ended = _returns_of(e, days)
        resets += ended
        fit = e.es_fitness()
        assert _same(fit, E.fitness(ret, member_of_env, M)), (g, fit)
        stats = e.es_update()
        theta, m, v, grad = E.update(theta, m, v, fit, noise_seed, g, **law)
        st = e.es_state()
        assert _same(st["theta"], theta) and _same(st["m"], m) and _same(st["v"], v), g
        assert st["generation"] == g + 1 == stats["generation"]
        assert _same(e.mlp_params(), theta)                         # (the centre follows theta)
        assert stats["fitness_max"] == fit.max() and stats["fitness_min"] == fit.min() and abs(stats["fitness_mean"] - fit.mean()) < 1e-9
        assert abs(stats["grad_norm"] - np.linalg.norm(grad.astype(np.float64))) < 1e-9 * (1 + stats["grad_norm"])
        assert abs(stats["theta_norm"] - np.linalg.norm(theta.astype(np.float64))) < 1e-9 * (1 + stats["theta_norm"])
    assert resets > 0, "the run was meant to cross auto-resets"
    e.close()
    # the same three generations in run_days
    e = _engine(amd, N, K, seed=61, max_days=4, auto_reset=True)
    e.mlp_init(pol, agent_seeds)
    e.mlp_population(M)
    e.es_init(**kw)
    for g in range(3):
        e.es_perturb()
        e.run_days("mlp", days, 1000.0)
        e.es_update()
    assert _same(e.es_state()["theta"], theta)
    e.close()


def _es_run(amd, N, K, M, generations, days, deterministic, resume_at=None, member_of_env=None):
    """a seeded training run (reset with fixed seeds every generation); returns (fitness per generation, final state, the env
    groups the last day ran as)"""
    rng = np.random.default_rng(70)
    pol = R.random_policy(rng, K, (16, 16), "tanh", value=True, scale=0.3)
    agent_seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    reset_seeds = rng.integers(0, 2 ** 63, (generations, N)).astype(np.uint64)

    def fresh():
        e = _engine(amd, N, K, seed=71, max_days=1 << 20, loss_threshold=1e12)
        e.mlp_init(pol, agent_seeds, deterministic=deterministic)
        e.mlp_population(M, member_of_env)
        e.es_init(sigma=0.05, lr=0.02, seed=5)
        return e

    e, fits, groups = fresh(), [], 0
    for g in range(generations):
        if resume_at == g:
            st = e.es_state()
            e.close()
            e = fresh()
            e.es_state(st)
            assert _same(e.mlp_params(), st["theta"])
        e.es_perturb()
        e.reset(seeds=reset_seeds[g])
        e.run_days("mlp", days, 1000.0)
        groups = e.env_groups()
        fits.append(e.es_fitness())
        e.es_update()
    st = e.es_state()
    e.close()
    return fits, st, groups


def test_env_groups_and_twin_engines_give_the_same_bits(amd, monkeypatch):
    N, K, M = 16, 24, 8
    member_of_env = np.random.default_rng(1).permutation(np.repeat(np.arange(M), N // M)).astype(np.int32)
    runs = []
    for groups in (1, 2, 4, 1):                                     # (the second run of 1: another engine from the same seeds)
        monkeypatch.setenv("ADCRAFT_STREAM_GROUPS", str(groups))
        runs.append(_es_run(amd, N, K, M, 3, 6, deterministic=False, member_of_env=member_of_env))
        assert runs[-1][2] == groups, "the forced env groups did not engage"
    fits0, st0, _ = runs[0]
    assert all(np.isfinite(f).all() for f in fits0) and not _same(fits0[0], fits0[1])
    for fits, st, _ in runs[1:]:
        for a, b in zip(fits0, fits):
            assert _same(a, b)
        for k in ("theta", "m", "v"):
            assert _same(st0[k], st[k]), k
        assert st["generation"] == 3


def test_a_resumed_state_continues_to_the_same_theta(amd):
    N, K, M = 8, 10, 4
    fits0, st0, _ = _es_run(amd, N, K, M, 4, 4, deterministic=True)
    fits1, st1, _ = _es_run(amd, N, K, M, 4, 4, deterministic=True, resume_at=2)
    for a, b in zip(fits0, fits1):
        assert _same(a, b)
    for k in ("theta", "m", "v"):
        assert _same(st0[k], st1[k]), k
    assert st0["generation"] == st1["generation"] == 4


def _episode_returns(amd, policy, planes, reset_seeds, days, budget):
    """deterministic evaluation of one policy (no population): the float64 sum over the days of every env's reward"""
    N, K = planes.shape[1:]
    e = amd.StepEngine(N, K, seed=1234, max_days=days)
    e.set_all_params(planes)
    e.reset(seeds=reset_seeds)
    e.mlp_init(policy, deterministic=True)
    ret = np.zeros(N, np.float64)
    for _ in range(days):
        e.mlp_step(budget)
        ret = ret + np.asarray(e.fetch()["reward"], np.float64)
    e.close()
    return ret


LEARN = dict(N=1024, K=25, members=256, days=10, generations=40, budget=100000.0, mean_volume=8.0)


def learning_run(amd, log=print, **over):
    """train the example's policy at a small shape; returns (curve of mean fitness, paired differences of held-out returns)"""
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import ESTrainer, default_policy
    c = dict(LEARN, **over)
    N, K, days = c["N"], c["K"], c["days"]
    rng = np.random.default_rng(2024)
    pol0 = default_policy(K, days=days, seed=0)
    e = amd.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=c["mean_volume"]))
    e.reset()
    tr = ESTrainer(e, pol0, c["members"], seed=11)
    curve = []
    for g in range(c["generations"]):
        s = tr.generation(days, c["budget"], reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        curve.append(s["fitness_mean"])
        log(f"generation {s['generation']:3d}  fitness mean {s['fitness_mean']:10.3f}  max {s['fitness_max']:10.3f}  "
            f"|g| {s['grad_norm']:8.4f}  |theta| {s['theta_norm']:8.4f}")
    polG = tr.policy()
    e.close()
    held_planes = synthetic.implicit_keyword_planes(N, K, seed=999, mean_volume=c["mean_volume"])      # other keyword sets, other streams
    held_seeds = np.random.default_rng(4048).integers(0, 2 ** 63, N).astype(np.uint64)
    r0 = _episode_returns(amd, pol0, held_planes, held_seeds, days, c["budget"])
    rG = _episode_returns(amd, polG, held_planes, held_seeds, days, c["budget"])
    d = rG - r0
    log(f"held-out episode return: theta_0 {r0.mean():.3f}  theta_G {rG.mean():.3f}  paired difference {d.mean():.3f} "
        f"+- {d.std(ddof=1) / np.sqrt(d.size):.3f} (standard error, {d.size} envs)")
    return curve, d


def test_the_strategy_learns(amd):
    """40 generations of 256 members x 4 envs x 10 days on 25 sparse keywords, the paper's defaults (sigma 0.02, Adam lr 0.01):
    on held-out keyword sets and seeds the trained centre's episode return exceeds the untrained one's by more than three
    standard errors of the paired difference.  Measured curve and margin: profiles/pr_es_population.txt."""
    curve, d = learning_run(amd)
    assert np.isfinite(curve).all()
    se = d.std(ddof=1) / np.sqrt(d.size)
    assert d.mean() > 3.0 * se, (d.mean(), se)


def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd import _ffi
    N, K = 8, 6
    rng = np.random.default_rng(9)
    pol = R.random_policy(rng, K, (8,), "tanh", scale=0.3)
    e = _engine(amd, N, K, seed=81)
    # before mlp_init
    for call in (lambda: e.mlp_population(2), lambda: e.es_init(), lambda: e.mlp_params(), lambda: e.mlp_param_count()):
        with pytest.raises(_ffi.EngineStateError):
            call()
    e.mlp_init(pol)
    # the strategy without a population; its calls before es_init
    for call in (lambda: e.es_init(), lambda: e.es_perturb(), lambda: e.es_update(np.zeros(2)), lambda: e.es_state(),
                 lambda: e.mlp_member_params(0), lambda: e.mlp_set_member(0, pol)):
        with pytest.raises(_ffi.EngineStateError):
            call()
    # populations
    for bad in (lambda: e.mlp_population(3), lambda: e.mlp_population(-1), lambda: e.mlp_population(2, np.array([0, 1, 2, 0, 0, 0, 0, 0])),
                lambda: e.mlp_population(2, np.array([0, 1, -1, 0, 0, 0, 0, 0])), lambda: e.mlp_population(2, np.zeros(5, np.int32)),
                lambda: e.mlp_population(1 << 20)):
        with pytest.raises(ValueError):
            bad()
    e.run_days("mlp", 1, 1000.0)                                   # (no population came of those)
    with pytest.raises(_ffi.EngineStateError):
        e.mlp_member_params(0)
    e.mlp_population(3, np.array([0, 1, 2, 0, 1, 2, 0, 1]))        # a plain population may be odd ...
    with pytest.raises(ValueError):
        e.mlp_member_params(3)
    with pytest.raises(ValueError):
        e.es_init()                                                # ... the strategy's may not
    e.run_days("mlp", 1, 1000.0)
    e.mlp_population(4, np.array([0, 1, 2, 0, 1, 2, 0, 1]))        # member 3 has no env
    for bad in (dict(sigma=0.0), dict(sigma=-0.1)):
        with pytest.raises(ValueError):
            e.es_init(**bad)
    cfg = amd.StepEngine.es_config()
    cfg.sigma = 0.0
    assert e._lib.adc_engine_es_init(e._h, C.byref(cfg)) == _ffi.ADC_EINVAL
    with pytest.raises(_ffi.EngineStateError):
        e.es_perturb()                                             # (the refused es_init left no strategy)
    e.es_init()
    e.es_perturb()
    e.run_days("mlp", 2, 1000.0)
    for call in (lambda: e.es_fitness(), lambda: e.es_update(), lambda: e.es_update(np.zeros(4))):
        with pytest.raises(ValueError):
            call()                                                 # a member without envs has no fitness
    assert e.es_state()["generation"] == 0
    e.mlp_population(4)
    with pytest.raises(_ffi.EngineStateError):
        e.es_perturb()                                             # (a new population drops the strategy over the old one)
    e.es_init()
    e.es_perturb()
    with pytest.raises(ValueError):
        e.es_update()                                              # no day stepped, no fitness handed in
    with pytest.raises(ValueError):
        e.es_update(np.zeros(3))
    assert e.es_state()["generation"] == 0
    theta0 = e.es_state()["theta"]
    e.es_update(np.array([1.0, 0.0, 3.0, 2.0]))                    # a caller's fitness needs no day
    st = e.es_state()
    assert st["generation"] == 1 and not _same(st["theta"], theta0)
    with pytest.raises(ValueError):
        e.es_state(dict(st, theta=st["theta"][:-1]))
    with pytest.raises(ValueError):
        e.es_state(dict(st, generation=-1))
    e.es_perturb()
    e.run_days("mlp", 2, 1000.0)
    assert e.es_update()["generation"] == 2
    # neither survives a re-initialisation of the policy
    e.mlp_init(pol)
    for call in (lambda: e.mlp_member_params(0), lambda: e.es_perturb()):
        with pytest.raises(_ffi.EngineStateError):
            call()
    e.rollout_enable(2)
    e.run_days("mlp", 2, 1000.0)
    assert e.rollout_fetch()["action"].shape == (2, N, K + 1)
    e.close()
