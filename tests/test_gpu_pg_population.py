"""GPU tests of learner populations (adc_engine_mlp_learners, adc_engine_pg_pop_*): M PPO / A2C learners in lock-step on one
engine.  The law is the single learner's: member m of M learners on N envs owns the envs [m n, (m + 1) n), n = N / M, and
everything it computes equals, bit for bit, (a) the numpy restatement tests/pg_ref.py on its slice of the fetched record and
(b) a solo engine of n envs at env_id_base + m n run through PGTrainer.  None of these symbols exists before this feature:
every test here fails on the parent commit."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import pg_pop_ref as PP
from tests import pg_ref as P

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(autouse=True)
def time_limit(request):
    """every test under its own time limit.  The alarm's handler runs when the interpreter next regains control: it ends a test
    that loops or waits in Python; a call that hangs inside the library is for the runner's outer limit to end."""
    seconds = 120

    def expired(*_):
        raise TimeoutError(f"{request.node.name} ran longer than {seconds} s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(seconds)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


SEED, BUDGET = 41, 1000.0
RESETS = dict(max_days=4, auto_reset=True)
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)


def _planes(N, K, seed=SEED):
    return H.implicit_params(N, K, seed + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, seed=SEED, env_id_base=0, **kw):
    _, N, K = planes.shape
    e = amd.StepEngine(N, K, seed=seed, env_id_base=env_id_base, **kw)
    e.set_all_params(planes)
    e.reset()
    return e


def _policies(rng, K, M, hidden=(20, 9), act="tanh", two=False, **kw):
    """M policies of one shape with different policy layers, value layers and log_std; the normalisation is shared"""
    pols = []
    for _ in range(M):
        pol = R.random_policy(rng, K, hidden, act, two_heads=two, value=True, normalize=True, scale=0.6, **kw)
        pol.shift, pol.scale = R.realistic_norm(K)
        pols.append(pol)
    return pols


def _without_norm(pol):
    """the policy on an input that is already normalised (the record's)"""
    import copy
    out = copy.copy(pol)
    out.shift = out.scale = None
    return out


def _assert_state(got, ref, what=""):
    for k in ("theta", "m", "v"):
        assert _same(got[k], ref[k]), (k, what)
    assert got["steps"] == ref["steps"], what


def _assert_stats(got, ref, what=""):
    for k in P.STAT_KEYS:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


# ---- 1. acting -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True])
def test_members_act_as_the_restatement_and_as_solo_engines(amd, two):
    """N = 12, K = 5, M = 3: one recorded episode through an auto-reset.  Every member's actions, log-probabilities, values and
    bootstrap values equal tests/mlp_ref.py on that member's weights (on the recorded input, with the member's agents' own
    normals), and everything recorded equals a solo engine of 4 envs at env_id_base = 4 m."""
    N, K, M, T = 12, 5, 3, 6
    n, A = N // M, K + 1
    rng = np.random.default_rng(101 + two)
    pols = _policies(rng, K, M, two=two)
    planes = _planes(N, K)
    e = _engine(amd, planes, **RESETS)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    for m in range(M):
        assert _same(e.mlp_learner_params(m), P.flat_params(pols[0])), "every member starts as the centre"
    for m in range(1, M):
        e.mlp_set_learner(m, pols[m])
    for m in range(M):
        assert _same(e.mlp_learner_params(m), P.flat_params(pols[m]))
    assert _same(e.mlp_params(), P.flat_params(pols[0])[:e.mlp_param_count()])
    e.rollout_enable(T, obs=True)
    e.run_days("mlp", T, BUDGET)
    rec, last, out = e.rollout_fetch(bootstrap=True), e.mlp_last(), e.fetch()
    done = rec["terminated"] | rec["truncated"]
    assert done[3].all() and not done[2].any(), "the record was meant to cross an auto-reset"
    obs_last = R.flat_obs(out)
    obs_last[done[-1]] = 0.0
    keys, ticks = e.mlp_agent_state()
    assert np.all(ticks == T)
    for m in range(M):
        sl = PP.member_slice(m, n)
        assert _same(keys[sl], np.array([R.default_agent_key(SEED, env) for env in range(m * n, (m + 1) * n)], np.uint64))
        plain = _without_norm(pols[m])
        for t in range(T):
            ref = R.act(plain, rec["obs"][t, sl], R.normals([int(k) for k in keys[sl]], [t] * n, A), deterministic=False)
            for k in ("action", "logp", "value"):
                assert _same(rec[k][t, sl], ref[k]), (k, m, t)
        for k in ("action", "logp", "value", "mean", "log_std"):
            assert _same(last[k][sl], ref[k]), (k, m, "the last act")
        assert _same(rec["bootstrap_value"][sl], R.act(pols[m], obs_last[sl], None, deterministic=True)["value"]), m
        # the solo engine on the member's envs
        s = _engine(amd, planes[:, sl], env_id_base=m * n, **RESETS)
        s.mlp_init(pols[m], deterministic=False)
        s.rollout_enable(T, obs=True)
        s.run_days("mlp", T, BUDGET)
        srec = s.rollout_fetch(bootstrap=True)
        for k in srec:
            assert _same(srec[k], PP.member_record(rec, m, n)[k]), (k, m)
        slast = s.mlp_last()
        for k in slast:
            assert _same(slast[k], last[k][sl]), (k, m)
        s.close()
    # members differ, or the test would show nothing
    assert not _same(rec["value"][:, :n], rec["value"][:, n:2 * n])
    assert two or not _same(last["log_std"][0], last["log_std"][n])
    e.close()


# ---- 2. training equals solo -----------------------------------------------------------------------------------------------------
M3, N3, K3, T3 = 3, 480, 3, 7
CONFIGS = (dict(eps_clip=0.2, normalize_advantages=True, lr=3e-3),                                                       # PPO
           dict(eps_clip=0.0, lam=1.0, normalize_advantages=False, optimiser="sgd", lr=0.01, max_grad_norm=0.0, reward_scale=0.05),   # A2C
           dict(eps_clip=0.2, normalize_advantages=True, lr=0.0))                                                        # PPO that stands still
CASES = {"tanh-1": dict(minibatches=1), "tanh-2": dict(minibatches=2),
         "relu-two-heads-clamp": dict(minibatches=1, act="relu", two=True, log_std_clamp=(-2.0, -0.5))}
EPOCHS, ITERATIONS = 2, 3


def _case(name):
    c = dict(CASES[name])
    minibatches = c.pop("minibatches")
    rng = np.random.default_rng(201)
    pols = _policies(rng, K3, M3, **c)
    n = N3 // M3
    opts = [P.options(minibatch_envs=n // minibatches, **cfg) for cfg in CONFIGS]
    return pols, opts, minibatches, n


def _population(amd, pols, opts, planes, **engine_kw):
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer
    e = _engine(amd, planes, **engine_kw)
    configs = [dict({k: v for k, v in o.items() if k != "minibatch_envs"}, epochs=EPOCHS, minibatches=(N3 // M3) // o["minibatch_envs"]) for o in opts]
    return e, PGPopulationTrainer(e, pols, T3, configs)


_RUNS = {}


def _population_run(amd, name, check, groups=None):
    """ITERATIONS iterations of the population of case `name`; returns per iteration the members' states, their statistics and
    (first iteration) the advantages and returns.  check: compare with the numpy restatement on the way."""
    pols, opts, minibatches, n = _case(name)
    e, tr = _population(amd, pols, opts, _planes(N3, K3), **RESETS)
    states = [PP.fresh_state(p) for p in pols]
    for m in range(M3):
        _assert_state(e.pg_pop_state(m), states[m], "theta starts as the member's device weights")
    out = []
    for it in range(ITERATIONS):
        e.rollout_reset()
        e.run_days("mlp", T3, BUDGET)
        if groups is not None:
            assert e.env_groups() == groups, "the forced env groups did not engage"
        rec = e.rollout_fetch(bootstrap=True) if check else None
        adv = e.pg_pop_advantages(fetch=True) if it == 0 else None
        stats = e.pg_pop_update(EPOCHS)
        got = [e.pg_pop_state(m) for m in range(M3)]
        if check:
            assert (rec["terminated"] | rec["truncated"]).any()
            for m in range(M3):
                if it == 0:
                    radv, rret = PP.member_gae(rec, m, n, opts[m])
                    sl = PP.member_slice(m, n)
                    assert _same(adv[0][:, sl], radv) and _same(adv[1][:, sl], rret), m
                states[m], rstats = PP.member_update(pols[m], states[m], rec, m, n, EPOCHS, opts[m])
                _assert_state(got[m], states[m], (name, it, m))
                _assert_stats(stats[m], rstats, (name, it, m))
                assert stats[m]["steps"] == states[m]["steps"] == (it + 1) * EPOCHS * minibatches
                assert stats[m]["samples"] == T3 * n // minibatches
                assert _same(e.mlp_learner_params(m), states[m]["theta"]), "the member's device weights follow its theta"
        out.append((got, stats, adv))
    for m in range(M3):                                             # (the trainer hands a member's trained policy out)
        assert _same(P.flat_params(tr.policy(m)), out[-1][0][m]["theta"]), m
    returns = tr.returns()
    assert returns.shape == (M3,) and np.isfinite(returns).all()
    e.close()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_training_equals_the_restatement_and_solo_engines(amd, name):
    """M = 3 members of 160 envs, K = 3, T = 7: a member's minibatch is 1120 samples (one full chunk plus a partial one whose
    length is no multiple of 64; the members' chunk boundaries do not line up in the joint launch), or two minibatches of 80
    envs.  Three configurations: PPO with clip and normalisation, A2C with SGD, no norm clip and a reward scale, PPO with
    lr = 0.  After every one of three iterations of two epochs, every member's theta, m, v, steps, statistics and (first
    iteration) advantages and returns equal the numpy restatement on its slice of the record and a solo PGTrainer twin."""
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    pols, opts, minibatches, n = _case(name)
    run = _RUNS[name] = _population_run(amd, name, check=True)
    planes = _planes(N3, K3)
    for m in range(M3):
        s = _engine(amd, planes[:, PP.member_slice(m, n)], env_id_base=m * n, **RESETS)
        cfg = {k: v for k, v in opts[m].items() if k != "minibatch_envs"}
        tr = PGTrainer(s, pols[m], T3, epochs=EPOCHS, minibatches=minibatches, **cfg)
        for it in range(ITERATIONS):
            s.rollout_reset()
            s.run_days("mlp", T3, BUDGET)
            if it == 0:
                adv, ret = s.pg_advantages(fetch=True)
                sl = PP.member_slice(m, n)
                assert _same(run[0][2][0][:, sl], adv) and _same(run[0][2][1][:, sl], ret), m
            stats = s.pg_update(EPOCHS)
            _assert_state(run[it][0][m], s.pg_state(), ("solo twin", name, it, m))
            _assert_stats(run[it][1][m], stats, ("solo twin", name, it, m))
            assert run[it][1][m]["steps"] == stats["steps"] and run[it][1][m]["samples"] == stats["samples"]
        s.close()
    # the lr = 0 member stands exactly still; the others moved
    assert _same(run[-1][0][2]["theta"], P.flat_params(pols[2]))
    assert not _same(run[-1][0][0]["theta"], P.flat_params(pols[0])) and not _same(run[-1][0][1]["theta"], P.flat_params(pols[1]))
    assert not np.any(run[-1][0][1]["m"]) and np.any(run[-1][0][0]["m"]), "SGD keeps no moments"


# ---- 3. env groups ---------------------------------------------------------------------------------------------------------------
def test_env_groups_give_the_same_bits(amd, monkeypatch):
    """the first case again with the days run as three env groups: nothing of the grouping enters any member's bits"""
    name = "tanh-1"
    # (the one-group run is the training test's when that ran before - only to save its time; alone, this test makes its own.
    #  Neither run is compared with the restatement here: this test compares groupings, the training test the law)
    one = _RUNS.get(name) or _population_run(amd, name, check=False)
    monkeypatch.setenv("ADCRAFT_STREAM_GROUPS", "3")
    three = _population_run(amd, name, check=False, groups=3)
    for it in range(ITERATIONS):
        for m in range(M3):
            _assert_state(one[it][0][m], three[it][0][m], (it, m))
            _assert_stats(one[it][1][m], three[it][1][m], (it, m))
    assert _same(one[0][2][0], three[0][2][0]) and _same(one[0][2][1], three[0][2][1])


# ---- 4. state, copy, set_config ----------------------------------------------------------------------------------------------------
def _small(amd, M=3, n=8, K=3, T=5, minibatches=2, seed=301, engine_kw=NO_RESETS, configs=CONFIGS):
    rng = np.random.default_rng(seed)
    pols = _policies(rng, K, M, hidden=(12,))
    opts = [P.options(minibatch_envs=n // minibatches, **cfg) for cfg in configs]
    e = _engine(amd, _planes(M * n, K), **engine_kw)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    for m in range(M):
        e.mlp_set_learner(m, pols[m])
    e.rollout_enable(T, obs=True)
    e.pg_pop_init(opts)
    return e, pols, opts


def test_a_resumed_state_continues_to_the_same_theta(amd):
    M, n, T = 3, 8, 5
    e, pols, opts = _small(amd)
    full = []
    for it in range(3):
        e.rollout_reset()
        e.run_days("mlp", T, BUDGET)
        e.pg_pop_update(2)
        full.append([e.pg_pop_state(m) for m in range(M)])
    e.close()
    # a fresh engine stepped to the env position after iteration 1, given every member's state of then
    e, _, _ = _small(amd)
    e.run_days("mlp", T, BUDGET)
    for m in range(M):
        e.pg_pop_state(m, full[0][m])
        _assert_state(e.pg_pop_state(m), full[0][m])
        assert _same(e.mlp_learner_params(m), full[0][m]["theta"])
    for it in (1, 2):
        e.rollout_reset()
        e.run_days("mlp", T, BUDGET)
        e.pg_pop_update(2)
        for m in range(M):
            _assert_state(e.pg_pop_state(m), full[it][m], (it, m))
    e.close()


def test_copy_and_set_config(amd):
    M, n, K, T = 3, 8, 3, 5
    A = K + 1
    e, pols, opts = _small(amd)
    e.run_days("mlp", T, BUDGET)
    e.pg_pop_update(2)
    before = [e.pg_pop_state(m) for m in range(M)]
    # copy: member 2 becomes member 0 - state, step count and the weights it acts with; members 0 and 1 are untouched
    e.pg_pop_copy(0, 2)
    _assert_state(e.pg_pop_state(2), before[0])
    _assert_state(e.pg_pop_state(0), before[0])
    _assert_state(e.pg_pop_state(1), before[1])
    assert _same(e.mlp_learner_params(2), before[0]["theta"]) and not _same(before[2]["theta"], before[0]["theta"])
    e.rollout_reset()
    e.run_days("mlp", 1, BUDGET)
    rec = e.rollout_fetch()
    keys, _ = e.mlp_agent_state()
    sl = PP.member_slice(2, n)
    ref = R.act(_without_norm(P.with_params(pols[0], before[0]["theta"])), rec["obs"][0, sl], R.normals([int(k) for k in keys[sl]], [T] * n, A), deterministic=False)
    for k in ("action", "logp", "value"):
        assert _same(rec[k][0, sl], ref[k]), k
    # set_config: member 1 turns from A2C with SGD to PPO with Adam; its next step is the restatement's under the new options
    states = [before[0], before[1], before[0]]
    new = P.options(minibatch_envs=opts[1]["minibatch_envs"], eps_clip=0.1, lr=1e-3, gamma=0.9, lam=0.8, ent_coef=0.01, normalize_advantages=True)
    e.pg_pop_set_config(1, **new)
    now = [opts[0], new, opts[2]]
    with pytest.raises(Exception, match="pg_pop_advantages"):
        e.pg_pop_minibatch(0)                                       # (advantages under the old gamma are stale)
    rec = e.rollout_fetch(bootstrap=True)
    adv, ret = e.pg_pop_advantages(fetch=True)
    for m in range(M):
        radv, rret = PP.member_gae(rec, m, n, now[m])
        assert _same(adv[:, PP.member_slice(m, n)], radv) and _same(ret[:, PP.member_slice(m, n)], rret), m
    for index in (0, 1):
        stats = e.pg_pop_minibatch(index)
        for m, pol in enumerate((pols[0], pols[1], pols[0])):
            states[m], rstats = PP.member_minibatch(pol, states[m], rec, adv, ret, m, n, index, now[m])
            _assert_state(e.pg_pop_state(m), states[m], (index, m))
            _assert_stats(stats[m], rstats, (index, m))
    assert np.any(states[1]["m"]), "member 1 runs Adam now"
    with pytest.raises(ValueError, match="minibatch_envs"):
        e.pg_pop_set_config(1, **dict(new, minibatch_envs=n))
    e.close()


# ---- 5. nothing else moved ---------------------------------------------------------------------------------------------------------
def test_nothing_else_moved(amd):
    """training draws nothing: the env streams, the agents' keys and ticks and the centre weights are where they are without the
    updates; and a solo trainer on a second engine gives its usual bits while a population trains on the first"""
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    M, n, K, T = 3, 8, 3, 5
    ends = []
    for updates in (False, True):
        e, pols, opts = _small(amd)
        centre = e.mlp_params()
        for _ in range(2):
            e.rollout_reset()
            e.run_days("mlp", T, BUDGET)
            if updates:
                e.pg_pop_update(2)
        ends.append((e.get_rng_state(), e.mlp_agent_state()))
        assert _same(e.mlp_params(), centre)
        if not updates:
            e.close()
    (sa, aa), (sb, ab) = ends
    assert _same(sa[0], sb[0]) and _same(sa[1], sb[1])
    assert _same(aa[0], ab[0]) and _same(aa[1], ab[1]) and np.all(aa[1] == 2 * T)
    # (the population's engine is still open and trains between the solo trainer's calls)
    solo_opts = P.options(lr=3e-3, minibatch_envs=4)
    runs = []
    for interleaved in (False, True):
        rng = np.random.default_rng(77)
        pol = _policies(rng, K, 1, hidden=(12,))[0]
        s = _engine(amd, _planes(8, K, seed=5), seed=5, **NO_RESETS)
        tr = PGTrainer(s, pol, T, epochs=2, minibatches=2, **{k: v for k, v in solo_opts.items() if k != "minibatch_envs"})
        for _ in range(2):
            tr.iteration(T, BUDGET)
            if interleaved:
                e.rollout_reset()
                e.run_days("mlp", T, BUDGET)
                e.pg_pop_update(1)
        runs.append(s.pg_state())
        s.close()
    _assert_state(runs[0], runs[1])
    e.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd import _ffi
    M, n, K, T = 2, 4, 3, 3
    N = M * n
    rng = np.random.default_rng(401)
    pols = _policies(rng, K, M, hidden=(8,))
    e = _engine(amd, _planes(N, K), **NO_RESETS)
    opts = P.options(minibatch_envs=2)
    with pytest.raises(_ffi.EngineStateError, match="mlp_init"):
        e.mlp_learners(M)
    e.mlp_init(pols[0], deterministic=False)
    for call in (lambda: e.mlp_set_learner(0, pols[0]), lambda: e.mlp_learner_params(0)):
        with pytest.raises(_ffi.EngineStateError, match="mlp_learners"):
            call()
    with pytest.raises(ValueError, match="divide"):
        e.mlp_learners(3)
    e.rollout_enable(T, obs=True)
    # without learners; with an ES population instead
    with pytest.raises(_ffi.EngineStateError, match="learners"):
        e.pg_pop_init(opts)
    e.mlp_population(2)
    with pytest.raises(_ffi.EngineStateError, match="learners"):
        e.pg_pop_init(opts)
    e.mlp_learners(M)                                               # (drops the population)
    with pytest.raises(_ffi.EngineStateError, match="population"):
        e.es_init()
    for call in (lambda: e.pg_pop_update(1), lambda: e.pg_pop_advantages(), lambda: e.pg_pop_minibatch(0), lambda: e.pg_pop_state(0),
                 lambda: e.pg_pop_copy(0, 1), lambda: e.pg_pop_set_config(0)):
        with pytest.raises(_ffi.EngineStateError, match="pg_pop_init"):
            call()
    # the other trainers with learners active
    with pytest.raises(_ffi.EngineStateError, match="learners"):
        e.pg_init()
    with pytest.raises(_ffi.EngineStateError, match="learners"):
        e.td3_init(batch_size=8, capacity=64, critic_widths=(8, 1))
    # without a record; without the recorded input
    e.rollout_enable(0)
    with pytest.raises(_ffi.EngineStateError, match="rollout record"):
        e.pg_pop_init(opts)
    e.rollout_enable(T)
    with pytest.raises(_ffi.EngineStateError, match="ADC_ROLLOUT_OBS"):
        e.pg_pop_init(opts)
    e.rollout_enable(T, obs=True)
    # bad configurations
    for bad in (dict(opts, minibatch_envs=3), [opts] * 3, [opts, dict(opts, minibatch_envs=4)], dict(opts, gamma=2.0)):
        with pytest.raises(ValueError):
            e.pg_pop_init(bad)
    # a solo trainer or TD3 alive (on the centre policy, before the learners)
    e.mlp_learners(0)
    e.pg_init()
    e.mlp_learners(M)
    with pytest.raises(_ffi.EngineStateError, match="single-learner"):
        e.pg_pop_init(opts)
    e.mlp_learners(0)
    e.rollout_enable(T, obs=True)                                   # (drops the solo trainer)
    e.td3_init(batch_size=8, capacity=64, critic_widths=(8, 1))
    e.mlp_learners(M)
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.pg_pop_init(opts)
    e.rollout_enable(T, obs=True)                                   # (drops TD3)
    for m in range(M):
        e.mlp_set_learner(m, pols[m])
    e.pg_pop_init(opts)
    # no recorded day; a deterministic record
    for call in (lambda: e.pg_pop_update(1), lambda: e.pg_pop_advantages(), lambda: e.pg_pop_minibatch(0)):
        with pytest.raises(_ffi.EngineStateError, match="no day"):
            call()
    e.mlp_set_deterministic(True)
    e.run_days("mlp", 1, BUDGET)
    e.mlp_set_deterministic(False)
    for call in (lambda: e.pg_pop_update(1), lambda: e.pg_pop_advantages()):
        with pytest.raises(_ffi.EngineStateError, match="deterministic"):
            call()
    e.rollout_reset()
    e.run_days("mlp", 2, BUDGET)
    with pytest.raises(_ffi.EngineStateError, match="pg_pop_advantages"):
        e.pg_pop_minibatch(0)
    # bad member indices, minibatch indices, epochs, states
    st = e.pg_pop_state(0)
    for member in (-1, M):
        for call in (lambda: e.pg_pop_state(member), lambda: e.pg_pop_state(member, st), lambda: e.pg_pop_copy(0, member),
                     lambda: e.pg_pop_copy(member, 0), lambda: e.pg_pop_set_config(member, **opts), lambda: e.mlp_learner_params(member),
                     lambda: e.mlp_set_learner(member, pols[0])):
            with pytest.raises(ValueError, match="member"):
                call()
    e.pg_pop_advantages()
    for index in (-1, n // 2):
        with pytest.raises(ValueError, match="minibatch"):
            e.pg_pop_minibatch(index)
    for epochs in (0, -1):
        with pytest.raises(ValueError):
            e.pg_pop_update(epochs)
    with pytest.raises(ValueError):
        e.pg_pop_state(0, dict(st, theta=st["theta"][:-1]))
    with pytest.raises(ValueError):
        e.pg_pop_state(0, dict(st, steps=-1))
    # after all of it a valid update works, and the members' step counts say so
    assert [s["steps"] for s in e.pg_pop_update(1)] == [2, 2]
    assert [s["steps"] for s in e.pg_pop_minibatch(1)] == [3, 3]
    # the trainer survives neither new learners, a new record nor a re-initialisation of the policy
    e.mlp_learners(M)
    with pytest.raises(_ffi.EngineStateError, match="pg_pop_init"):
        e.pg_pop_update(1)
    e.pg_pop_init(opts)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="pg_pop_init"):
        e.pg_pop_update(1)
    e.pg_pop_init(opts)
    e.mlp_init(pols[0], deterministic=False)
    with pytest.raises(_ffi.EngineStateError, match="mlp_learners"):
        e.mlp_learner_params(0)
    # ... and the engine is a plain single-policy engine again
    e.rollout_enable(T, obs=True)
    e.pg_init()
    e.run_days("mlp", T, BUDGET)
    assert e.pg_update(1)["steps"] == 1
    e.close()


# ---- 7. the refusals the policy-gradient host files share (parts/pg_core.inc), by their whole sentence: a fragment such as "pg_init"
# or "learners" is also part of the single learner's sentences ------------------------------------------------------------------------
SAID = dict(
    not_initialised="adc_engine_pg_pop_init has not been called (or the policy, the learners or the record were re-initialised since)",
    no_learners="population training needs learners (adc_engine_mlp_learners)",
    no_record="policy-gradient training needs a rollout record (adc_engine_rollout_enable)",
    no_input="policy-gradient training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)",
    no_day="no day has been recorded (adc_engine_mlp_step / adc_engine_run_days with ADC_POLICY_MLP)",
    deterministic="the record holds days collected with the deterministic policy: their log-probabilities mean nothing "
                  "(adc_engine_mlp_set_deterministic(0), adc_engine_rollout_reset, collect again)",
    no_advantages="adc_engine_pg_pop_advantages has not been called since the last recorded day",
    td3="an off-policy (TD3) trainer is alive on this engine: one trainer at a time owns the policy's weights",
    solo="a single-learner trainer is alive on this engine (adc_engine_pg_init)",
    epochs="epochs: 1 to 65536",
    minibatch="no such minibatch: 0 to envs of a member / minibatch_envs - 1",
    shuffled_minibatch="no such minibatch: 0 to ceil(samples of a member / minibatch_samples) - 1",
    member="no such member",
    state_null="theta, m or v is NULL",
    state_steps="steps: 0 to 2^31 - 2",
    lds_keywords="num_keywords too large for policy-gradient training (LDS)",
    lds_frames="frames: the stacked input row is too large for policy-gradient training (LDS); fewer frames fit",
    kl_lds_keywords="num_keywords too large for the KL penalty (LDS)",
)


def _refused(kind, text, call):
    with pytest.raises(kind) as info:
        call()
    assert str(info.value) == text, (str(info.value), text)


def test_every_shared_refusal_by_its_whole_sentence_and_which_one_wins(amd):
    from adcraft_amd import _ffi
    M, n, K, T = 2, 2, 3, 2
    N = M * n
    STATE, VALUE = _ffi.EngineStateError, ValueError
    pols = _policies(np.random.default_rng(411), K, M, hidden=(8,))
    opts = P.options(minibatch_envs=1)
    e = _engine(amd, _planes(N, K), **NO_RESETS)
    e.mlp_init(pols[0], deterministic=False)
    # the state an init needs; two at once: the missing learners are named before the missing record
    _refused(STATE, SAID["no_learners"], lambda: e.pg_pop_init(opts))
    e.mlp_learners(M)
    _refused(STATE, SAID["no_record"], lambda: e.pg_pop_init(opts))
    e.rollout_enable(T)
    _refused(STATE, SAID["no_input"], lambda: e.pg_pop_init(opts))
    for call in (lambda: e.pg_pop_advantages(), lambda: e.pg_pop_advantages(fetch=True), lambda: e.pg_pop_minibatch(0), lambda: e.pg_pop_update(1),
                 lambda: e.pg_pop_update(1, queued=True), lambda: e.pg_pop_state(0), lambda: e.pg_pop_state(M), lambda: e.pg_pop_copy(0, M),
                 lambda: e.pg_pop_set_config(M), lambda: _ffi.check(e._lib.adc_engine_pg_pop_advantages_fetch(e._h, None, None)),
                 lambda: _ffi.check(e._lib.adc_engine_pg_pop_state_set(e._h, M, None, None, None, -1))):
        _refused(STATE, SAID["not_initialised"], call)
    # another trainer alive: TD3, the single learner (each on the centre policy, before the learners)
    e.mlp_learners(0)
    e.rollout_enable(T, obs=True)
    e.td3_init(batch_size=8, capacity=64, critic_widths=(8, 1))
    e.mlp_learners(M)
    _refused(STATE, SAID["td3"], lambda: e.pg_pop_init(opts))
    e.mlp_learners(0)
    e.rollout_enable(T, obs=True)                                   # (drops TD3)
    e.pg_init()
    e.mlp_learners(M)
    _refused(STATE, SAID["solo"], lambda: e.pg_pop_init(opts))
    _refused(STATE, SAID["not_initialised"], lambda: e.pg_pop_update(1))       # (the single learner is not a population)
    e.mlp_learners(0)
    e.rollout_enable(T, obs=True)                                   # (drops the single learner)
    e.mlp_learners(M)
    for m in range(M):
        e.mlp_set_learner(m, pols[m])
    e.pg_pop_init(opts)
    # the record; two at once: no day is named before the epochs, before the missing advantages and before the index
    for call in (lambda: e.pg_pop_advantages(), lambda: e.pg_pop_update(1), lambda: e.pg_pop_update(0), lambda: e.pg_pop_update(1, queued=True),
                 lambda: e.pg_pop_update(0, queued=True), lambda: e.pg_pop_minibatch(0), lambda: e.pg_pop_minibatch(-1)):
        _refused(STATE, SAID["no_day"], call)
    e.mlp_set_deterministic(True)
    e.run_days("mlp", 1, BUDGET)
    e.mlp_set_deterministic(False)
    for call in (lambda: e.pg_pop_advantages(), lambda: e.pg_pop_update(1), lambda: e.pg_pop_update(1, queued=True), lambda: e.pg_pop_minibatch(0)):
        _refused(STATE, SAID["deterministic"], call)
    e.rollout_reset()
    e.run_days("mlp", 1, BUDGET)
    # the advantages (named before a bad index), the index, the epochs
    for call in (lambda: e.pg_pop_minibatch(0), lambda: e.pg_pop_minibatch(-1),
                 lambda: _ffi.check(e._lib.adc_engine_pg_pop_advantages_fetch(e._h, None, None))):
        _refused(STATE, SAID["no_advantages"], call)
    for epochs in (0, 65537):
        _refused(VALUE, SAID["epochs"], lambda: e.pg_pop_update(epochs))
        _refused(VALUE, SAID["epochs"], lambda: e.pg_pop_update(epochs, queued=True))
    e.pg_pop_advantages()
    for index in (-1, n):
        _refused(VALUE, SAID["minibatch"], lambda: e.pg_pop_minibatch(index))
    # the member, the state's arguments; two at once: the member is named before the arrays, a missing array before the step count
    st = e.pg_pop_state(0)
    three = [st[k].ctypes.data for k in ("theta", "m", "v")]
    for member in (-1, M):
        for call in (lambda: e.pg_pop_state(member), lambda: e.pg_pop_state(member, st), lambda: e.pg_pop_copy(0, member), lambda: e.pg_pop_copy(member, 0),
                     lambda: e.pg_pop_set_config(member, **opts),
                     lambda: _ffi.check(e._lib.adc_engine_pg_pop_state_set(e._h, member, None, None, None, -1))):
            _refused(VALUE, SAID["member"], call)
    _refused(VALUE, SAID["state_null"], lambda: _ffi.check(e._lib.adc_engine_pg_pop_state_set(e._h, 1, three[0], three[1], None, -1)))
    for steps in (-1, 2 ** 31 - 1):
        _refused(VALUE, SAID["state_steps"], lambda: e.pg_pop_state(1, dict(st, steps=steps)))
    # the add-ons' member and minibatch indices over the shared count of members
    e.pg_kl_init()
    for member in (-1, M):
        _refused(VALUE, SAID["member"], lambda: e.pg_kl_coef(member))
        _refused(VALUE, SAID["member"], lambda: e.pg_kl_coef(member, 0.5))
    e.pg_shuffle_init(minibatch_samples=2)
    e.pg_pop_advantages()
    e.pg_shuffle_epoch()
    for index in (-1, 1):
        _refused(VALUE, SAID["shuffled_minibatch"], lambda: e.pg_shuffle_minibatch(index))
    # after all of it the trainer works, and the members' step counts say what was taken
    assert [e.pg_pop_state(m)["steps"] for m in range(M)] == [0, 0]
    assert [s["steps"] for s in e.pg_pop_update(1)] == [1, 1]
    assert [s["steps"] for s in e.pg_pop_update(1, queued=True)] == [2, 2]
    e.close()


def _lds_floats(K, frames, hidden, kl):
    """kernel_pg.inc's pg_lds_floats for a free-head policy and a value network of one hidden layer each"""
    D, A = frames * (5 * K + 2), K + 1
    return D + 2 * max(hidden, A) + (5 if kl else 3) * A + (hidden + A) + (hidden + 1)


@pytest.mark.parametrize("K,frames,kl,said", [(1488, 1, False, "lds_keywords"), (1023, 2, False, "lds_frames"), (1259, 1, True, "kl_lds_keywords")])
def test_the_first_shape_past_64_kib_of_lds_is_refused_in_the_right_words(amd, K, frames, kl, said):
    """a sample's workgroup holds 11 K + 25 floats (13 K + 27 under the KL penalty) for one frame and one hidden layer of 8:
    K is the first that passes 16384 floats, K - 1 fits; with two frames one frame of that K still fits, so the frames are named.
    Two learners of one env each, one recorded day"""
    from adcraft_amd import _ffi
    from tests import stack_ref as S
    M, T, hidden = 2, 1, 8
    assert _lds_floats(K, frames, hidden, kl) > 16384 >= _lds_floats(K - 1, frames, hidden, kl)
    assert frames == 1 or _lds_floats(K, 1, hidden, kl) <= 16384   # (one frame of it fits)
    assert not kl or _lds_floats(K, frames, hidden, False) <= 16384    # (the trainer itself fits: the add-on's two vectors do not)
    pol = S.random_policy(np.random.default_rng(431), K, frames, (hidden,), value=True)
    e = _engine(amd, H.implicit_params(M, K, SEED + 1, mean_volume=4, cvr=0.5), **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    e.mlp_learners(M)
    e.rollout_enable(T, obs=True)
    if kl:
        e.pg_pop_init(P.options())
        _refused(ValueError, SAID[said], lambda: e.pg_kl_init())
        e.run_days("mlp", 1, BUDGET)
        assert [s["steps"] for s in e.pg_pop_update(1)] == [1, 1]   # (the trainer goes on without the add-on)
    else:
        _refused(ValueError, SAID[said], lambda: e.pg_pop_init(P.options()))
        _refused(_ffi.EngineStateError, SAID["not_initialised"], lambda: e.pg_pop_state(0))    # (the refused init left no trainer)
    e.close()


# ---- 8. a population of one member is the single learner: the case in which "one configuration" and "one per member" coincide and
# the per-member vectors of length one are read from both front ends ---------------------------------------------------------------
@pytest.mark.parametrize("queued", [False, True])
@pytest.mark.parametrize("addons", [False, True])
def test_a_population_of_one_is_the_single_learner_bit_for_bit(amd, addons, queued):
    """4 envs, 3 keywords, horizon 3, minibatches of 2 envs, two iterations of two epochs on twin engines; addons: the KL penalty and
    shuffled minibatches of 5 of the 12 samples (5, 5 and a tail of 2)"""
    N, K, T = 4, 3, 3
    pol = _policies(np.random.default_rng(421), K, 1, hidden=(8,))[0]
    opts = P.options(minibatch_envs=2)

    def run(pop):
        e = _engine(amd, _planes(N, K), **NO_RESETS)
        e.mlp_init(pol, deterministic=False)
        if pop:
            e.mlp_learners(1)
            e.mlp_set_learner(0, pol)
        e.rollout_enable(T, obs=True)
        e.pg_pop_init(opts) if pop else e.pg_init(**opts)
        if addons:
            e.pg_kl_init(kl_coef=0.3, kl_target=0.001)
            e.pg_shuffle_init(minibatch_samples=5)
        one = (lambda x: x[0]) if pop else (lambda x: x)
        out = []
        for _ in range(2):
            e.rollout_reset()
            e.run_days("mlp", T, BUDGET)
            stats = one(e.pg_pop_update(2, queued=queued) if pop else e.pg_update(2, queued=queued))
            it = dict(state=e.pg_pop_state(0) if pop else e.pg_state(), stats=stats)
            if addons:
                it.update(kl=one(e.pg_kl_stats()), coef=e.pg_kl_coef(0), shuffle=one(e.pg_shuffle_stats()))
            out.append(it)
        e.close()
        return out

    solo, pop = run(False), run(True)
    for it, (a, b) in enumerate(zip(solo, pop)):
        _assert_state(b["state"], a["state"], it)
        assert a["state"]["steps"] == (it + 1) * 2 * (3 if addons else 2), a["state"]["steps"]
        assert set(a["stats"]) == set(b["stats"]) and len(a["stats"]) >= 9
        for k in a["stats"]:
            assert _same(np.float64(a["stats"][k]), np.float64(b["stats"][k])), (k, a["stats"][k], b["stats"][k], it)
        if addons:
            for k in a["kl"]:
                assert _same(np.float64(a["kl"][k]), np.float64(b["kl"][k])), (k, a["kl"][k], b["kl"][k], it)
            assert _same(a["coef"], b["coef"]) and a["shuffle"] == b["shuffle"], (a["coef"], b["coef"], a["shuffle"], b["shuffle"])
    assert not _same(solo[0]["state"]["theta"], solo[1]["state"]["theta"])


def test_the_three_layer_uploads_round_trip_at_a_ragged_shape(amd):
    """the one layer upload under mlp_set_weights, mlp_set_member and mlp_set_learner (parts/mlp_core.inc mlp_layer_upload): 4 envs,
    3 keywords, policy hidden (5, 3), value hidden (6,), free log_std - the two networks differ in depth and no hidden width is a
    multiple of the 4 floats the stores are padded to.  Three different policies go in; each comes back in the host's flat order
    bit for bit, and the member nothing was uploaded to is still the centre"""
    from tests import es_ref as E
    N, K = 4, 3
    rng = np.random.default_rng(611)
    centre, member, learner = (R.ragged_policy(rng, K) for _ in range(3))
    planes = _planes(N, K)
    e, l = _engine(amd, planes), _engine(amd, planes)
    e.mlp_init(centre)
    e.mlp_population(2)
    e.mlp_set_member(1, member)
    assert _same(e.mlp_params(), E.flat_params(centre))
    assert _same(e.mlp_member_params(1), E.flat_params(member)) and not _same(E.flat_params(member), E.flat_params(centre))
    assert _same(e.mlp_member_params(0), E.flat_params(centre)), "the untouched member is the centre"
    l.mlp_init(centre)
    l.mlp_learners(2)
    l.mlp_set_learner(1, learner)
    assert l.mlp_learner_param_count() == P.flat_params(learner).size
    assert _same(l.mlp_learner_params(1), P.flat_params(learner)) and not _same(P.flat_params(learner), P.flat_params(centre))
    assert _same(l.mlp_learner_params(0), P.flat_params(centre)), "the untouched learner is the centre"
    assert _same(l.mlp_params(), E.flat_params(centre))
    # a second upload of the centre's weights: what was there goes
    other = R.ragged_policy(rng, K)
    e.mlp_set_weights(other)
    assert _same(e.mlp_params(), E.flat_params(other)) and _same(e.mlp_member_params(1), E.flat_params(member))
    e.close()
    l.close()
