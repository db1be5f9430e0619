"""GPU tests of policy-gradient training on the device (parts/kernel_pg.inc, parts/pg_api.inc) against the numpy restatement
tests/pg_ref.py, bit for bit: advantages through auto-resets, one minibatch step, full iterations, independence of the launch
shape, resumed state, that nothing else moved, every refusal, and a learning run.  None of these symbols exists before this
feature: every test here fails on the parent commit."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
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
    seconds = 420 if "learns" in request.node.name else 120

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


def _engine(amd, N, K, seed=3, mean_volume=24, **kw):
    e = amd.StepEngine(N, K, seed=seed, **kw)
    e.set_all_params(H.implicit_params(N, K, seed + 1, mean_volume=mean_volume, cvr=0.5))
    e.reset()
    return e


def _policy(rng, K, hidden=(16, 8), act="tanh", two=False, value=True, **kw):
    pol = R.random_policy(rng, K, hidden, act, two_heads=two, value=value, normalize=True, scale=0.6, **kw)
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _trainer(amd, pol, N, K, T, opts, agent_seeds, seed=41, **engine_kw):
    e = _engine(amd, N, K, seed=seed, **engine_kw)
    e.mlp_init(pol, agent_seeds, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.pg_init(**opts)
    return e


def _fresh_state(pol):
    theta = P.flat_params(pol)
    return dict(theta=theta, m=np.zeros_like(theta), v=np.zeros_like(theta), steps=0)


def _assert_state(got, ref, what=""):
    for k in ("theta", "m", "v"):
        assert _same(got[k], ref[k]), (k, what)
    assert got["steps"] == ref["steps"], what


def _assert_stats(got, ref, what=""):
    for k in P.STAT_KEYS:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


RESETS = dict(max_days=4, auto_reset=True)
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)


@pytest.mark.parametrize("kw", [dict(), dict(normalize_advantages=False, gamma=0.9, lam=0.8, reward_scale=0.05)])
def test_advantages_equal_the_restatement_through_auto_resets(amd, kw):
    N, K, T = 12, 8, 7
    rng = np.random.default_rng(11)
    pol = _policy(rng, K)
    opts = P.options(**kw)
    e = _trainer(amd, pol, N, K, T, opts, rng.integers(0, 2 ** 63, N).astype(np.uint64), **RESETS)
    e.run_days("mlp", T, 1000.0)
    rec = e.rollout_fetch(bootstrap=True)
    done = rec["terminated"] | rec["truncated"]
    assert done[:-1].any() and not done.all(), "the record was meant to cross auto-resets"
    adv, ret = e.pg_advantages(fetch=True)
    radv, rret = P.gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], rec["bootstrap_value"], **opts)
    assert _same(adv, radv) and _same(ret, rret)
    assert np.isfinite(adv).all() and float(np.abs(adv).max()) > 0
    e.close()


@pytest.mark.parametrize("case", [dict(act="tanh"), dict(act="relu", two=True, log_std_clamp=(-2.0, -0.5), opts=dict(ent_coef=0.01, optimiser="sgd", lr=0.01)),
                                  dict(act="tanh", value=False, hidden=(), opts=dict(eps_clip=0.0, max_grad_norm=0.0))])
def test_one_minibatch_step_equals_the_restatement(amd, case):
    case = dict(case)
    opts = P.options(**case.pop("opts", {}))
    N, K, T = 10, 9, 5
    rng = np.random.default_rng(21)
    pol = _policy(rng, K, **case)
    e = _trainer(amd, pol, N, K, T, opts, rng.integers(0, 2 ** 63, N).astype(np.uint64), **NO_RESETS)
    st0 = e.pg_state()
    _assert_state(st0, _fresh_state(pol), "theta starts as the device's weights")
    assert e.pg_param_count() == st0["theta"].size
    e.run_days("mlp", T, 1000.0)
    rec = e.rollout_fetch()
    adv, ret = e.pg_advantages(fetch=True)
    boot = e.mlp_bootstrap_value() if pol.value_layers else np.zeros(N, F)      # (without a value network every value is +0)
    radv, rret = P.gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], boot, **opts)
    assert _same(adv, radv) and _same(ret, rret)
    # two steps on the same record: the second sees ratios away from 1
    state = _fresh_state(pol)
    for n0, B in ((0, N), (2, 5)):
        stats = e.pg_minibatch(n0, B)
        state, rstats = P.minibatch(pol, state, rec, adv, ret, n0, B, opts)
        _assert_state(e.pg_state(), state, (n0, B))
        _assert_stats(stats, rstats, (n0, B))
        assert stats["steps"] == state["steps"] and stats["samples"] == T * B
    assert not _same(state["theta"], st0["theta"])
    # the next act uses the new weights
    new = P.with_params(pol, state["theta"])
    assert _same(e.mlp_params(), P.flat_params(new)[:e.mlp_param_count()])
    z = rng.standard_normal((N, K + 1)).astype(F)
    obs = R.flat_obs(e.fetch())
    e.mlp_act(1000.0, replay_normals=z)
    last, ref = e.mlp_last(), R.act(new, obs, z, deterministic=False)
    for k in ("mean", "log_std", "action", "logp", "value"):
        assert _same(last[k], ref[k]), k
    e.close()


def _iterations(amd, pol, N, K, T, opts, epochs, iterations, agent_seeds, check=False, **engine_kw):
    """collect T days, update, `iterations` times; returns (the state after each iteration, env groups of the last day)"""
    e = _trainer(amd, pol, N, K, T, opts, agent_seeds, **engine_kw)
    state, states, groups = _fresh_state(pol), [], 0
    for it in range(iterations):
        e.rollout_reset()
        e.run_days("mlp", T, 1000.0)
        groups = e.env_groups()
        if check:
            rec = e.rollout_fetch(bootstrap=True)
        stats = e.pg_update(epochs)
        if check:
            state, rstats = P.update(pol, state, rec, rec["bootstrap_value"], epochs, opts)
            _assert_state(e.pg_state(), state, it)
            _assert_stats(stats, rstats, it)
            assert (rec["terminated"] | rec["truncated"]).any() or "auto_reset" not in engine_kw
        states.append(e.pg_state())
    e.close()
    return states, groups


@pytest.mark.parametrize("act,minibatches", [("tanh", 2), ("relu", 2), ("tanh", 1)])
def test_three_iterations_equal_the_restatement(amd, act, minibatches):
    """collect through auto-resets, update with 2 epochs x the minibatches, three times over"""
    N, K, T = 8, 8, 5
    rng = np.random.default_rng(31)
    pol = _policy(rng, K, (12, 12), act)
    opts = P.options(lr=3e-3, minibatch_envs=N // minibatches)
    states, _ = _iterations(amd, pol, N, K, T, opts, 2, 3, rng.integers(0, 2 ** 63, N).astype(np.uint64), check=True, **RESETS)
    assert states[-1]["steps"] == 3 * 2 * minibatches
    assert not _same(states[0]["theta"], states[-1]["theta"])


def test_env_groups_and_twin_engines_give_the_same_bits(amd, monkeypatch):
    N, K, T = 16, 24, 4
    rng = np.random.default_rng(41)
    pol = _policy(rng, K, (16, 16))
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = P.options(lr=3e-3, minibatch_envs=N // 2)
    runs = []
    for groups in (1, 2, 4, 1):                                     # (the second run of 1: another engine from the same seeds)
        monkeypatch.setenv("ADCRAFT_STREAM_GROUPS", str(groups))
        runs.append(_iterations(amd, pol, N, K, T, opts, 2, 3, seeds, **RESETS))
        assert runs[-1][1] == groups, "the forced env groups did not engage"
    for states, _ in runs[1:]:
        for a, b in zip(runs[0][0], states):
            _assert_state(a, b)


def test_a_resumed_state_continues_to_the_same_theta(amd):
    """the trainer's state saved after iteration 1 and restored into a fresh engine (given the env's position too) reaches
    iteration 3's theta exactly"""
    N, K, T = 8, 8, 4
    rng = np.random.default_rng(51)
    pol = _policy(rng, K, (12,))
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = P.options(lr=3e-3, minibatch_envs=N // 2)
    full, _ = _iterations(amd, pol, N, K, T, opts, 2, 3, seeds, **NO_RESETS)
    # a straight run of one iteration, then its state alone carried into a fresh engine stepped to the same env position
    e = _trainer(amd, pol, N, K, T, opts, seeds, **NO_RESETS)
    e.run_days("mlp", T, 1000.0)
    e.pg_update(2)
    saved = e.pg_state()
    _assert_state(saved, full[0])
    e.close()
    e = _trainer(amd, pol, N, K, T, opts, seeds, **NO_RESETS)
    e.run_days("mlp", T, 1000.0)                                    # (the env's and agents' streams, as after iteration 1)
    e.pg_state(saved)
    assert _same(e.pg_state()["theta"], saved["theta"]) and e.pg_state()["steps"] == saved["steps"]
    assert _same(e.mlp_params(), saved["theta"][:e.mlp_param_count()])
    for it in (1, 2):
        e.rollout_reset()
        e.run_days("mlp", T, 1000.0)
        e.pg_update(2)
        _assert_state(e.pg_state(), full[it], it)
    e.close()


STEP_FIELDS = ("impressions", "buyside_clicks", "sellside_conversions", "cost", "revenue", "reward", "cumulative_profit", "days_passed",
               "terminated", "truncated")


def test_nothing_else_moved(amd):
    N, K, T = 12, 10, 4
    rng = np.random.default_rng(61)
    pol = _policy(rng, K)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = P.options(lr=3e-3)
    # after pg_init and before any update a day is what it is without it
    runs = []
    for with_pg in (False, True):
        e = _engine(amd, N, K, seed=41, **RESETS)
        e.mlp_init(pol, seeds, deterministic=False)
        e.rollout_enable(T, obs=True)
        if with_pg:
            e.pg_init(**opts)
        e.run_days("mlp", T, 1000.0)
        runs.append((e.fetch(), e.rollout_fetch(bootstrap=True), e.mlp_last(), e.get_rng_state()))
        e.close()
    (o0, r0, l0, s0), (o1, r1, l1, s1) = runs
    for k in STEP_FIELDS:
        assert _same(o0[k], o1[k]), k
    for k in r0:
        assert _same(r0[k], r1[k]), k
    for k in l0:
        assert _same(l0[k], l1[k]), k
    assert _same(s0[0], s1[0]) and _same(s0[1], s1[1])
    # training takes no draws: with updates in between, the envs' streams and the agents' (key and tick of every env's
    # agent) are where they are without; and the next act's normals are the same ones (z = (action - mean) / exp(log_std), up
    # to that expression's rounding under the two different policies)
    ends = []
    for updates in (False, True):
        e = _trainer(amd, pol, N, K, T, opts, seeds, **NO_RESETS)
        for _ in range(2):
            e.rollout_reset()
            e.run_days("mlp", T, 1000.0)
            if updates:
                e.pg_update(2)
        e.mlp_act(1000.0)
        last = e.mlp_last()
        ends.append((e.get_rng_state(), (last["action"] - last["mean"]) / np.exp(last["log_std"]), e.mlp_agent_state()))
        e.close()
    (sa, za, aa), (sb, zb, ab) = ends
    assert _same(sa[0], sb[0]) and _same(sa[1], sb[1])
    assert _same(aa[0], ab[0]) and _same(aa[1], ab[1]) and np.all(aa[1] == 2 * T + 1)
    assert np.abs(za - zb).max() < 1e-3 and np.abs(za).max() > 0.5


def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd import _ffi
    N, K, T = 8, 6, 3
    rng = np.random.default_rng(71)
    pol = _policy(rng, K, (8,))
    e = _engine(amd, N, K, seed=81, **NO_RESETS)
    calls = (lambda: e.pg_advantages(), lambda: e.pg_minibatch(0, N), lambda: e.pg_update(1), lambda: e.pg_state(), lambda: e.pg_param_count())
    # before mlp_init; without a record; without the recorded input
    with pytest.raises(_ffi.EngineStateError, match="mlp_init"):
        e.pg_init()
    e.mlp_init(pol, deterministic=False)
    with pytest.raises(_ffi.EngineStateError, match="rollout record"):
        e.pg_init()
    e.rollout_enable(T)
    with pytest.raises(_ffi.EngineStateError, match="ADC_ROLLOUT_OBS"):
        e.pg_init()
    for call in calls:
        with pytest.raises(_ffi.EngineStateError, match="pg_init"):
            call()
    e.rollout_enable(T, obs=True)
    # a bad configuration
    for bad in (dict(minibatch_envs=3), dict(minibatch_envs=2 * N), dict(gamma=2.0), dict(lr=-1.0)):
        with pytest.raises(ValueError):
            e.pg_init(**bad)
    cfg = amd.StepEngine.pg_config()
    cfg.reward_scale = 0.0
    assert e._lib.adc_engine_pg_init(e._h, C.byref(cfg)) == _ffi.ADC_EINVAL
    with pytest.raises(_ffi.EngineStateError, match="pg_init"):
        e.pg_state()                                               # (the refused pg_init left no trainer)
    # a population
    e.mlp_population(2)
    with pytest.raises(_ffi.EngineStateError, match="population"):
        e.pg_init()
    e.mlp_population(0)
    e.pg_init(minibatch_envs=N // 2)
    # zero recorded days
    for call in (lambda: e.pg_advantages(), lambda: e.pg_update(1), lambda: e.pg_minibatch(0, 4)):
        with pytest.raises(_ffi.EngineStateError, match="no day"):
            call()
    e.run_days("mlp", 2, 1000.0)
    # a minibatch before the advantages; bad ranges; bad epochs
    with pytest.raises(_ffi.EngineStateError, match="pg_advantages"):
        e.pg_minibatch(0, 4)
    e.pg_advantages()
    for n0, B in ((-1, 4), (0, 0), (6, 4), (0, N)):
        with pytest.raises(ValueError):
            e.pg_minibatch(n0, B)
    for epochs in (0, -1):
        with pytest.raises(ValueError):
            e.pg_update(epochs)
    assert e.pg_state()["steps"] == 0
    assert e.pg_minibatch(4, 4)["steps"] == 1
    # another recorded day makes the advantages stale
    e.run_days("mlp", 1, 1000.0)
    with pytest.raises(_ffi.EngineStateError, match="pg_advantages"):
        e.pg_minibatch(0, 4)
    # a population while the trainer exists
    e.mlp_population(2)
    with pytest.raises(_ffi.EngineStateError, match="population"):
        e.pg_update(1)
    e.mlp_population(0)
    assert e.pg_update(1)["steps"] == 3
    # a deterministic policy at collection time
    e.rollout_reset()
    e.mlp_set_deterministic(True)
    e.run_days("mlp", 1, 1000.0)
    e.mlp_set_deterministic(False)
    e.run_days("mlp", 1, 1000.0)
    for call in (lambda: e.pg_advantages(), lambda: e.pg_update(1)):
        with pytest.raises(_ffi.EngineStateError, match="deterministic"):
            call()
    e.rollout_reset()
    e.run_days("mlp", 2, 1000.0)
    assert e.pg_update(1)["steps"] == 5
    # bad state
    st = e.pg_state()
    with pytest.raises(ValueError):
        e.pg_state(dict(st, theta=st["theta"][:-1]))
    with pytest.raises(ValueError):
        e.pg_state(dict(st, steps=-1))
    e.pg_state(st)
    # the trainer survives neither a new record nor a re-initialisation of the policy
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="pg_init"):
        e.pg_update(1)
    e.pg_init()
    e.mlp_init(pol, deterministic=False)
    with pytest.raises(_ffi.EngineStateError, match="pg_init"):
        e.pg_state()
    e.rollout_enable(T, obs=True)
    e.pg_init()
    e.run_days("mlp", T, 1000.0)
    assert e.pg_update(2)["steps"] == 2
    e.close()
    # a sharded engine
    s = amd.ShardedStepEngine(N, K, shards=2, seed=5)
    with pytest.raises(NotImplementedError, match="engine_shards=1"):
        s.pg_init()
    s.close()


# ---- the refusals the three policy-gradient host files share (parts/pg_core.inc), by their whole sentence: a fragment such as
# "pg_init" is also part of the population's sentences --------------------------------------------------------------------------
SAID = dict(
    not_initialised="adc_engine_pg_init has not been called (or the policy / the record was re-initialised since)",
    population="policy-gradient training with a population active is not supported (adc_engine_mlp_population(0) first)",
    learners="learners are active: they train through adc_engine_pg_pop_init (adc_engine_mlp_learners(0) first)",
    no_record="policy-gradient training needs a rollout record (adc_engine_rollout_enable)",
    no_input="policy-gradient training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)",
    no_day="no day has been recorded (adc_engine_mlp_step / adc_engine_run_days with ADC_POLICY_MLP)",
    deterministic="the record holds days collected with the deterministic policy: their log-probabilities mean nothing "
                  "(adc_engine_mlp_set_deterministic(0), adc_engine_rollout_reset, collect again)",
    no_advantages="adc_engine_pg_advantages has not been called since the last recorded day",
    td3="an off-policy (TD3) trainer is alive on this engine: one trainer at a time owns the policy's weights",
    epochs="epochs: 1 to 65536",
    env_range="the env range is not inside [0, num_envs)",
    env_count="env_count exceeds the configuration's minibatch_envs (the scratch was sized for it)",
    minibatch="no such minibatch: 0 to ceil(samples of a member / minibatch_samples) - 1",
    member="no such member",
    state_null="theta, m or v is NULL",
    state_steps="steps: 0 to 2^31 - 2",
    lds_keywords="num_keywords too large for policy-gradient training (LDS)",
    lds_frames="frames: the stacked input row is too large for policy-gradient training (LDS); fewer frames fit",
    kl_lds_keywords="num_keywords too large for the KL penalty (LDS)",
    kl_lds_frames="frames: the stacked input row is too large for the KL penalty (LDS); fewer frames fit",
)


def _refused(kind, text, call):
    with pytest.raises(kind) as info:
        call()
    assert str(info.value) == text, (str(info.value), text)


def test_every_shared_refusal_by_its_whole_sentence_and_which_one_wins(amd):
    from adcraft_amd import _ffi
    N, K, T = 4, 3, 2
    STATE, VALUE = _ffi.EngineStateError, ValueError
    pol = _policy(np.random.default_rng(91), K, (8,))
    e = _engine(amd, N, K, seed=83, **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    # the state an init needs; two at once: the population is named before the missing record
    _refused(STATE, SAID["no_record"], lambda: e.pg_init())
    e.mlp_population(2)
    _refused(STATE, SAID["population"], lambda: e.pg_init())
    e.mlp_population(0)
    e.rollout_enable(T)
    _refused(STATE, SAID["no_input"], lambda: e.pg_init())
    for call in (lambda: e.pg_advantages(), lambda: e.pg_advantages(fetch=True), lambda: e.pg_minibatch(0, N), lambda: e.pg_update(1),
                 lambda: e.pg_update(1, queued=True), lambda: e.pg_state(), lambda: e.pg_param_count(),
                 lambda: _ffi.check(e._lib.adc_engine_pg_advantages_fetch(e._h, None, None)),
                 lambda: _ffi.check(e._lib.adc_engine_pg_state_set(e._h, None, None, None, 0))):
        _refused(STATE, SAID["not_initialised"], call)
    e.rollout_enable(T, obs=True)
    # another trainer alive
    e.td3_init(batch_size=8, capacity=64, critic_widths=(8, 1))
    _refused(STATE, SAID["td3"], lambda: e.pg_init())
    e.rollout_enable(T, obs=True)                                   # (drops TD3)
    e.pg_init(minibatch_envs=N // 2)
    # the record; two at once: no day is named before the epochs, before the missing advantages and before the range
    for call in (lambda: e.pg_advantages(), lambda: e.pg_update(1), lambda: e.pg_update(0), lambda: e.pg_update(1, queued=True),
                 lambda: e.pg_update(0, queued=True), lambda: e.pg_minibatch(0, 2), lambda: e.pg_minibatch(-1, 2)):
        _refused(STATE, SAID["no_day"], call)
    e.mlp_set_deterministic(True)
    e.run_days("mlp", 1, 1000.0)
    e.mlp_set_deterministic(False)
    for call in (lambda: e.pg_advantages(), lambda: e.pg_update(1), lambda: e.pg_update(1, queued=True), lambda: e.pg_minibatch(0, 2)):
        _refused(STATE, SAID["deterministic"], call)
    e.rollout_reset()
    e.run_days("mlp", 1, 1000.0)
    # the advantages (named before a bad range), the ranges, the epochs
    for call in (lambda: e.pg_minibatch(0, 2), lambda: e.pg_minibatch(-1, 2),
                 lambda: _ffi.check(e._lib.adc_engine_pg_advantages_fetch(e._h, None, None))):
        _refused(STATE, SAID["no_advantages"], call)
    for epochs in (0, 65537):
        _refused(VALUE, SAID["epochs"], lambda: e.pg_update(epochs))
        _refused(VALUE, SAID["epochs"], lambda: e.pg_update(epochs, queued=True))
    e.pg_advantages()
    for n0, B in ((-1, 2), (0, 0), (3, 2)):
        _refused(VALUE, SAID["env_range"], lambda: e.pg_minibatch(n0, B))
    _refused(VALUE, SAID["env_count"], lambda: e.pg_minibatch(0, N))
    # the state's arguments; two at once: the missing array is named before the step count
    st = e.pg_state()
    three = [st[k].ctypes.data for k in ("theta", "m", "v")]
    _refused(VALUE, SAID["state_null"], lambda: _ffi.check(e._lib.adc_engine_pg_state_set(e._h, three[0], None, three[2], -1)))
    for steps in (-1, 2 ** 31 - 1):
        _refused(VALUE, SAID["state_steps"], lambda: e.pg_state(dict(st, steps=steps)))
    # the add-ons' member and minibatch indices over the shared count of members; learners with the trainer alive
    e.pg_kl_init()
    for member in (-1, 1):
        _refused(VALUE, SAID["member"], lambda: e.pg_kl_coef(member))
        _refused(VALUE, SAID["member"], lambda: e.pg_kl_coef(member, 0.5))
    e.pg_shuffle_init(minibatch_samples=3)
    e.pg_advantages()
    e.pg_shuffle_epoch()
    for index in (-1, 2):
        _refused(VALUE, SAID["minibatch"], lambda: e.pg_shuffle_minibatch(index))
    e.mlp_learners(2)
    for call in (lambda: e.pg_update(1), lambda: e.pg_update(0, queued=True), lambda: e.pg_advantages(), lambda: e.pg_minibatch(-1, 2)):
        _refused(STATE, SAID["learners"], call)
    e.mlp_learners(0)
    # after all of it the trainer works, and its step count says what was taken
    assert e.pg_state()["steps"] == 0
    assert e.pg_update(1)["steps"] == 2
    assert e.pg_update(1, queued=True)["steps"] == 4
    e.close()


def _lds_floats(K, frames, hidden, kl):
    """kernel_pg.inc's pg_lds_floats for a free-head policy and a value network of one hidden layer each"""
    D, A = frames * (5 * K + 2), K + 1
    return D + 2 * max(hidden, A) + (5 if kl else 3) * A + (hidden + A) + (hidden + 1)


@pytest.mark.parametrize("K,frames,kl,said", [(1488, 1, False, "lds_keywords"), (1023, 2, False, "lds_frames"),
                                              (1259, 1, True, "kl_lds_keywords"), (909, 2, True, "kl_lds_frames")])
def test_the_first_shape_past_64_kib_of_lds_is_refused_in_the_right_words(amd, K, frames, kl, said):
    """a sample's workgroup holds 11 K + 25 floats (13 K + 27 under the KL penalty) for one frame and one hidden layer of 8:
    K is the first that passes 16384 floats, K - 1 fits; with two frames one frame of that K still fits, so the frames are named"""
    from adcraft_amd import _ffi
    from tests import stack_ref as S
    N, T, hidden = 2, 1, 8
    assert _lds_floats(K, frames, hidden, kl) > 16384 >= _lds_floats(K - 1, frames, hidden, kl)
    assert frames == 1 or _lds_floats(K, 1, hidden, kl) <= 16384   # (one frame of it fits)
    assert not kl or _lds_floats(K, frames, hidden, False) <= 16384    # (the trainer itself fits: the add-on's two vectors do not)
    pol = S.random_policy(np.random.default_rng(97), K, frames, (hidden,), value=True)
    e = _engine(amd, N, K, seed=85, mean_volume=4, **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    if kl:
        e.pg_init()
        _refused(ValueError, SAID[said], lambda: e.pg_kl_init())
        e.run_days("mlp", 1, 1000.0)
        assert e.pg_update(1)["steps"] == 1                         # (the trainer goes on without the add-on)
    else:
        _refused(ValueError, SAID[said], lambda: e.pg_init())
        _refused(_ffi.EngineStateError, SAID["not_initialised"], lambda: e.pg_state())    # (the refused pg_init left no trainer)
    e.close()


# the ES test's small shape (LEARN in tests/test_gpu_es_population.py), and what this trainer was given on it
LEARN = dict(N=1024, K=25, days=10, budget=100000.0, mean_volume=8.0, hidden=(32, 32), iterations=40,
             config=dict(epochs=4, minibatches=4, lr=1e-3, reward_scale=0.1, normalize_advantages=True))


def learning_policy(K, days, hidden):
    """default_policy plus a value network of the same hidden sizes, drawn the same way (its last layer's weights * 0.1, bias 0)"""
    from adcraft_amd.baselines.es_trainer import default_policy
    pol = default_policy(K, hidden=hidden, days=days, seed=0)
    rng = np.random.default_rng(1)
    layers, n_in = [], 5 * K + 2
    for n_out in list(hidden) + [1]:
        bound = 1.0 / np.sqrt(n_in)
        layers.append([rng.uniform(-bound, bound, (n_in, n_out)).astype(F), rng.uniform(-bound, bound, n_out).astype(F)])
        n_in = n_out
    layers[-1][0] *= F(0.1)
    layers[-1][1][:] = 0.0
    pol.value_layers = [tuple(l) for l in layers]
    return pol


def episode_returns(amd, policy, planes, reset_seeds, days, budget):
    """deterministic evaluation of one policy: the float64 sum over the days of every env's reward"""
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


def learning_run(amd, log=print, **over):
    """train at the small shape; returns (curve of the mean recorded reward per day, paired differences of held-out returns)"""
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    c = dict(LEARN, **over)
    N, K, days = c["N"], c["K"], c["days"]
    rng = np.random.default_rng(2024)
    pol0 = learning_policy(K, days, c["hidden"])
    e = amd.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=c["mean_volume"]))
    e.reset()
    tr = PGTrainer(e, pol0, days, **c["config"])
    curve = []
    for it in range(c["iterations"]):
        s = tr.iteration(days, c["budget"], reset=True, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        curve.append(float(e.rollout_fetch()["reward"].astype(np.float64).sum(axis=0).mean()))
        log(f"iteration {it + 1:3d}  episode return {curve[-1]:10.3f}  policy loss {s['policy_loss']:9.5f}  value loss {s['value_loss']:10.4f}  "
            f"entropy {s['entropy']:8.3f}  kl {s['approx_kl']:8.5f}  clip {s['clip_fraction']:6.3f}  |g| {s['grad_norm']:8.4f}  "
            f"ev {s['explained_variance']:6.3f}")
    polT = tr.policy()
    e.close()
    held_planes = synthetic.implicit_keyword_planes(N, K, seed=999, mean_volume=c["mean_volume"])      # other keyword sets, other streams
    held_seeds = np.random.default_rng(4048).integers(0, 2 ** 63, N).astype(np.uint64)
    r0 = episode_returns(amd, pol0, held_planes, held_seeds, days, c["budget"])
    rT = episode_returns(amd, polT, held_planes, held_seeds, days, c["budget"])
    d = rT - r0
    log(f"held-out episode return: untrained {r0.mean():.3f}  trained {rT.mean():.3f}  paired difference {d.mean():.3f} "
        f"+- {d.std(ddof=1) / np.sqrt(d.size):.3f} (standard error, {d.size} envs)")
    return curve, d


def test_it_learns(amd):
    """PPO at the ES test's small shape (1024 envs x 25 sparse keywords, 10-day episodes) from default_policy plus a value
    network, collected stochastically: on held-out keyword sets and seeds, evaluated deterministically, the trained policy's
    episode return exceeds the untrained one's by more than three standard errors of the paired difference.  The
    hyperparameters are LEARN's, written down before any run; curve and measured margin (+8.15 +- 0.27, 30 standard errors), next
    to PPO's textbook defaults and A2C: profiles/pr_pg_trainer.txt."""
    curve, d = learning_run(amd)
    assert np.isfinite(curve).all()
    se = d.std(ddof=1) / np.sqrt(d.size)
    assert d.mean() > 3.0 * se, (d.mean(), se)
