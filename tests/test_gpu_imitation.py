"""GPU tests of imitation learning on the device (parts/kernel_imitation.inc, parts/imitation_api.inc; the law is
csrc/adc_imitation.h): the teacher record against a twin engine stepped by run_days(teacher) and against mlp_ref / stack_ref, every
refusal, the update against tests/im_ref.py bit for bit, the hand-over to pg_update, demonstrations into the TD3 ring, and that
cloning a constant action raises its log-probability.  None of these symbols exists before this feature: every test here fails
on the parent commit."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import im_ref as I
from tests import mlp_ref as R
from tests import pg_ref as P
from tests import stack_ref as S
from tests import td3_ref as T3
from tests.test_imitation_host import CLONE, clone_policy

pytestmark = pytest.mark.gpu
F = np.float32
N0, K0, T0 = 6, 5, 4
RESETS = dict(max_days=3, auto_reset=True)
BUDGET = 1000.0
STEP_FIELDS = ("impressions", "buyside_clicks", "sellside_conversions", "cost", "revenue", "reward", "cumulative_profit", "days_passed",
               "terminated", "truncated")


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(autouse=True)
def time_limit(request):
    """every test under its own time limit (the handler runs when the interpreter next regains control)"""
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


def _engine(amd, N, K, seed=43, **kw):
    e = amd.StepEngine(N, K, seed=seed, **kw)
    e.set_all_params(H.implicit_params(N, K, seed + 1, mean_volume=24, cvr=0.5))
    e.reset()
    return e


def _policy(rng, K, frames=1, hidden=(13, 8), act="tanh", two=False, value=True, **kw):
    pol = S.random_policy(rng, K, frames, hidden, act, two_heads=two, value=value, normalize=True, scale=0.6, **kw)
    shift, scale = R.realistic_norm(K)
    pol.shift = np.concatenate([shift + F(0.25 * f) for f in range(frames)]).astype(F)
    pol.scale = np.concatenate([scale * F(1.0 + 0.125 * f) for f in range(frames)]).astype(F)
    return pol


def _teacher_ready(e, teacher, seeds):
    """what run_days(teacher) needs; "fixed": one set of sampled actions in the action buffers, left there"""
    if teacher == "zero_margin":
        e.agent_init(1.0, seeds)
    elif teacher == "oracle":
        e.bid_curves_build(256)
    elif teacher == "fixed":
        e.sample_actions(0.3, 1.0, 40.0)
    elif teacher == "interpolation":
        e.interp_init(seeds=seeds)


def _interp_same(a, b, what=""):
    """the interpolation agent's own state - caches, last bids, beliefs, interpolation points - of two engines"""
    for sa, sb in ((a.interp_state(), b.interp_state()), (a.interp_entries(), b.interp_entries())):
        for k in sa:
            assert _same(np.asarray(sa[k]), np.asarray(sb[k])), (what, k)


def _now(e):
    """(raw frame 0, episode day) an act would read now"""
    day = e.get_episode_state()[0].astype(np.int64)
    x = R.flat_obs(e.fetch()).astype(F)
    x[day == 0] = 0
    return x, day


def _fresh_state(pol):
    theta = P.flat_params(pol)
    return dict(theta=theta, m=np.zeros_like(theta), v=np.zeros_like(theta), steps=0)


def _assert_state(got, ref, what=""):
    for k in ("theta", "m", "v"):
        assert _same(got[k], ref[k]), (k, what)
    assert got["steps"] == ref["steps"], what


def _assert_stats(got, ref, what=""):
    for k in I.STAT_KEYS:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


# ---- 1. the teacher record -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("teacher", ["fixed", "zero_margin", "oracle", "interpolation"])
def test_the_teacher_record_and_the_env_equal_run_days(amd, teacher, frames):
    N, K, T = N0, K0, T0
    rng = np.random.default_rng(7 + frames)
    pol = _policy(rng, K, frames)
    seeds = np.arange(N, dtype=np.uint64) + 11
    a, b, c = (_engine(amd, N, K, **RESETS) for _ in range(3))       # teacher days one by one; the twin under run_days; teacher days at once
    for e in (a, b, c):
        _teacher_ready(e, teacher, seeds)
    for e in (a, c):
        e.mlp_init(pol, seeds, deterministic=False)
        e.rollout_enable(T, obs=True)
    hist = S.History(N, K, frames)
    rows, values, actions = [], [], []
    for t in range(T):
        row = hist.row(*_now(a))
        rows.append(S.normalized(pol, row))
        values.append(R.act(pol, row, None, deterministic=True)["value"])
        a.teach_days(teacher, 1, BUDGET)
        b.run_days(teacher, 1, BUDGET)
        oa, ob = a.fetch(), b.fetch()
        for k in STEP_FIELDS:
            assert _same(oa[k], ob[k]), (t, k)
        bids, budget = b.get_actions()
        abids, abudget = a.get_actions()
        assert _same(abids, bids) and _same(abudget, budget), "the learner's act reached the engine's action buffers"
        actions.append(np.concatenate([np.asarray(budget, F).reshape(N, 1), np.asarray(bids, F).reshape(N, K)], axis=1))
        assert all(np.array_equal(x, y) for x, y in zip(a.get_rng_state(), b.get_rng_state())), t
        if teacher == "interpolation":
            _interp_same(a, b, t)
    rec = a.rollout_fetch()
    assert rec["reward"].shape == (T, N)
    done = rec["terminated"] | rec["truncated"]
    assert done[:-1].any() and not done.all(), "an auto-reset was meant to fall inside the record"
    assert _same(rec["action"], np.stack(actions))
    assert _same(rec["logp"], np.zeros((T, N), F)), "logp is +0"
    assert _same(rec["obs"], np.stack(rows))
    assert _same(rec["value"], np.stack(values))
    assert np.abs(rec["obs"]).sum() > 0 and (frames == 1 or np.abs(rec["obs"][:, :, 5 * K + 2:]).sum() > 0)
    assert np.array_equal(a.mlp_agent_state()[1], np.full(N, T, np.uint32)), "the agents' ticks move on by one a day"
    if frames > 1:
        st, ref = a.mlp_history_state(), hist.state()
        assert all(_same(st[k], ref[k]) for k in ("hist", "last", "from"))
    # the T days in one call: the same record, the same env
    c.teach_days(teacher, T, BUDGET)
    rc = c.rollout_fetch()
    for k in rec:
        assert _same(rec[k], rc[k]), k
    for k in STEP_FIELDS:
        assert _same(a.fetch()[k], c.fetch()[k]), k
    if teacher == "interpolation":
        _interp_same(c, b, "the days in one call")
        assert c.interp_entries()["n_clicks"].max() > 0, "the interpolation agent was meant to learn from its days"
    with pytest.raises(ValueError, match="overflow"):
        a.teach_days(teacher, 1, BUDGET)
    for e in (a, b, c):
        e.close()


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(kind, text, fn, *args, **kw):
    with pytest.raises(kind, match=text):
        fn(*args, **kw)


def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd._ffi import EngineStateError as State
    N, K, T = N0, K0, T0
    rng = np.random.default_rng(3)
    pol = _policy(rng, K)
    seeds = np.arange(N, dtype=np.uint64) + 5
    e, twin = _engine(amd, N, K, **RESETS), _engine(amd, N, K, **RESETS)
    for x in (e, twin):
        x.sample_actions(0.3, 1.0, 40.0)

    def a_correct_day():
        """a teacher day and the twin's run_days day agree (the record is reset when full)"""
        if e.rollout_fetch()["reward"].shape[0] == T:
            e.rollout_reset()
        e.teach_days("fixed", 1)
        twin.run_days("fixed", 1)
        assert all(_same(e.fetch()[k], twin.fetch()[k]) for k in STEP_FIELDS)

    # --- adc_engine_teach_days
    _refused(State, "mlp_init", e.teach_days, "fixed", 1)
    e.mlp_init(pol, seeds, deterministic=False)
    _refused(State, "rollout record", e.teach_days, "fixed", 1)
    e.rollout_enable(T, obs=False)
    _refused(State, "ADC_ROLLOUT_OBS", e.teach_days, "fixed", 1)
    e.rollout_enable(T, obs=True)
    _refused(ValueError, "own teacher", e.teach_days, "mlp", 1)
    _refused(ValueError, "overflow", e.teach_days, "fixed", T + 1)
    _refused(ValueError, "days < 0", e.teach_days, "fixed", -1)
    _refused(State, "agent_init", e.teach_days, "zero_margin", 1)
    _refused(State, "bid_curves_build", e.teach_days, "oracle", 1)
    _refused(State, "interp_init", e.teach_days, "interpolation", 1)
    e.mlp_population(2)
    _refused(State, "population", e.teach_days, "fixed", 1)
    e.mlp_population(0)
    e.mlp_learners(2)
    _refused(State, "learners", e.teach_days, "fixed", 1)
    e.mlp_learners(0)
    e.mlp_set_squash(np.zeros(K + 1, F), np.ones(K + 1, F))
    _refused(State, "squash", e.teach_days, "fixed", 1)
    e.mlp_set_squash(None, None)
    a_correct_day()
    # --- the policy-gradient calls on a teacher record; adc_engine_im_init
    _refused(State, "pg_init first", e.im_init)
    opts = P.options(minibatch_envs=2)
    e.pg_init(**opts)
    for call in (e.pg_advantages, lambda: e.pg_minibatch(0, 2), e.pg_update):
        _refused(State, "the record holds teacher days", call)
    _refused(State, "im_init has not been called", e.im_advantages)
    e.pg_kl_init()
    _refused(State, "KL penalty", e.im_init)
    e.pg_init(**opts)                                                # (a new trainer: the add-on is gone)
    e.pg_shuffle_init(minibatch_samples=4)
    _refused(State, "shuffled", e.im_init)
    e.pg_init(**opts)
    e.rew_norm_init()
    _refused(State, "normaliser", e.im_init)
    e.pg_init(**opts)
    e.obs_norm_init()
    _refused(State, "normaliser", e.im_init)
    e.rollout_enable(T, obs=True)                                    # (the observation normaliser goes with the record it fed on)
    e.pg_init(**opts)
    _refused(ValueError, "beta", e.im_init, beta=-1.0)
    e.im_init(beta=0.5)
    for init in (e.pg_kl_init, lambda: e.pg_shuffle_init(minibatch_samples=4), e.rew_norm_init, e.obs_norm_init):
        _refused(State, "imitation is alive", init)
    # --- the order of the calls
    _refused(State, "no day has been recorded", e.im_advantages)
    e.teach_days("fixed", 2)
    twin.run_days("fixed", 2)
    assert all(_same(e.fetch()[k], twin.fetch()[k]) for k in STEP_FIELDS)
    _refused(State, "im_advantages has not been called", e.im_minibatch, 0, 2)
    _refused(State, "im_advantages has not been called", e.im_update, 1)
    e.im_advantages()
    _refused(ValueError, "env range", e.im_minibatch, 5, 2)
    _refused(ValueError, "minibatch_envs", e.im_minibatch, 0, 3)
    _refused(ValueError, "epochs", e.im_update, 0)
    st = e.im_minibatch(0, 2)
    assert st["steps"] == 1 and st["samples"] == 4 and np.isfinite(st["logp"])
    a_correct_day()
    _refused(State, "im_advantages has not been called", e.im_minibatch, 0, 2)       # (a day recorded since)
    # --- the record's kind: one of both kinds is neither trainer's; the learner's own days are the trainer's, not imitation's
    e.run_days("mlp", 1, BUDGET)
    _refused(State, "the record holds teacher days", e.pg_update)
    _refused(State, "days the learner collected", e.im_advantages)
    e.rollout_reset()
    e.run_days("mlp", 2, BUDGET)
    _refused(State, "days the learner collected", e.im_advantages)
    _refused(State, "days the learner collected", e.im_minibatch, 0, 2)
    assert np.isfinite(e.pg_update(1)["policy_loss"])
    e.rollout_reset()
    e.teach_days("fixed", 2)
    e.im_advantages()
    st = e.im_update(1)
    assert st["steps"] == 7 and np.isfinite(st["logp"]) and np.isfinite(st["grad_norm"])
    # imitation ends where the trainer ends
    e.rollout_enable(T, obs=True)
    _refused(State, "im_init has not been called", e.im_state)
    e.close()
    twin.close()


# ---- 3. update parity ----------------------------------------------------------------------------------------------------------------
UPDATE_CASES = [
    dict(K=2, N=6, T=4, mb=2, pol=dict(hidden=(13, 8), act="tanh"), im=dict(beta=0.7, w_max=1.5, ma_rate=1.0), by_minibatch=True),
    dict(K=10, N=6, T=4, mb=2, pol=dict(hidden=(), act="relu", two=True, value=False, log_std_clamp=(-1.5, 0.0)), im=dict(beta=0.0, vf_coef=0.0)),
    dict(K=10, N=6, T=4, mb=2, pol=dict(hidden=(13, 8), act="relu", log_std_clamp=(-1.0, 0.5)), im=dict(beta=0.7, train_log_std=False, ma_rate=0.5)),
    dict(K=2, N=130, T=8, mb=130, pol=dict(hidden=(8,), act="tanh"), im=dict(beta=0.7, w_max=1.5, ma_rate=1.0)),
]


def _im_trainer(amd, pol, N, K, T, opts, im, seeds):
    e = _engine(amd, N, K, **RESETS)
    e.sample_actions(0.3, 1.0, 40.0)
    e.mlp_init(pol, seeds, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.pg_init(**opts)
    e.im_init(**{k: v for k, v in im.items()})
    return e


def _im_iteration(e, pol, state, ma, T, epochs, opts, im, by_minibatch=False):
    """one iteration on the device and in the restatement: returns (state, ma, the device's statistics)"""
    e.rollout_reset()
    e.teach_days("fixed", T)
    rec = e.rollout_fetch(bootstrap=bool(pol.value_layers))
    adv, ret = e.im_advantages(fetch=True)
    boot = rec["bootstrap_value"] if pol.value_layers else np.zeros(rec["reward"].shape[1], F)     # (without a value network every value is +0)
    radv, rret = I.returns(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], boot, **opts)
    assert _same(adv, radv) and _same(ret, rret)
    ma, c = I.scale(ma, radv, **im)
    N, mb = rec["reward"].shape[1], opts["minibatch_envs"]
    if by_minibatch:
        for ep in range(epochs):
            for n0 in range(0, N, mb):
                stats = e.im_minibatch(n0, mb)
                state, rstats = I.minibatch(pol, state, rec, radv, rret, c, n0, mb, opts, im)
                _assert_state(e.pg_state(), state, (ep, n0))
                _assert_stats(stats, rstats, (ep, n0))
                assert stats["steps"] == state["steps"] and stats["samples"] == T * mb
    else:
        stats = e.im_update(epochs)
        state, rstats = I.update(pol, state, rec, radv, rret, c, epochs, opts, im)
        _assert_state(e.pg_state(), state)
        _assert_stats(stats, rstats)
    st = e.im_state()
    assert _same(np.float64(st["ma"]), np.float64(ma))
    return state, ma, stats, (radv, c)


@pytest.mark.parametrize("case", range(len(UPDATE_CASES)))
def test_the_update_equals_the_restatement_and_resumes_bit_for_bit(amd, case):
    cs = UPDATE_CASES[case]
    K, N, T = cs["K"], cs["N"], cs["T"]
    rng = np.random.default_rng(100 + case)
    pol = _policy(rng, K, **cs["pol"])
    if cs["pol"].get("log_std_clamp") and not cs["pol"].get("two"):   # (a free log_std with one component the clamp moves)
        lo, hi = cs["pol"]["log_std_clamp"]
        pol.log_std = np.linspace(lo + 0.1, hi - 0.1, K + 1).astype(F)
        pol.log_std[1] = F(lo - 0.5)
    if cs["pol"].get("two"):                                          # (the log-std head's biases on both sides of the clamp)
        lo, hi = cs["pol"]["log_std_clamp"]
        pol.layers[-1][1][K + 1:] = np.linspace(lo - 0.6, hi + 0.6, K + 1).astype(F)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = P.options(lr=3e-3, max_grad_norm=0.5, minibatch_envs=cs["mb"], gamma=0.9, reward_scale=0.05)
    im = I.im_options(**cs["im"])
    e = _im_trainer(amd, pol, N, K, T, opts, im, seeds)
    state, ma = _fresh_state(pol), im["ma_start"]
    _assert_state(e.pg_state(), state, "theta starts as the device's weights")
    state, ma, stats, (radv, c) = _im_iteration(e, pol, state, ma, T, 2, opts, im, cs.get("by_minibatch", False))
    assert stats["steps"] == 2 * (N // cs["mb"]) and e.im_state()["calls"] == 1 and stats["grad_norm"] > 0
    if im["beta"] > 0 and im["w_max"] < 20:
        w = I.weight(radv, c, **im)
        assert (w == F(im["w_max"])).any() and (w < F(im["w_max"])).any(), "the case was meant to cap some weights and not others"
    if not im["train_log_std"] and pol.log_std is not None:
        assert _same(state["theta"][-(K + 1):], pol.log_std)
    # the state saved here and restored into a fresh engine at the same env position continues bit for bit
    saved = dict(e.pg_state(), **e.im_state())
    state, ma, _, _ = _im_iteration(e, pol, state, ma, T, 2, opts, im)
    f = _im_trainer(amd, pol, N, K, T, opts, im, seeds)
    f.teach_days("fixed", T)                                         # (the envs' and agents' streams, as after iteration 1)
    f.pg_state(saved)
    f.im_state(saved)
    assert f.im_state() == dict(ma=saved["ma"], calls=1)
    f.rollout_reset()
    f.teach_days("fixed", T)
    f.im_advantages()
    f.im_update(2)
    _assert_state(f.pg_state(), state, "resumed")
    assert _same(np.float64(f.im_state()["ma"]), np.float64(ma)) and f.im_state()["calls"] == 2
    # 4. the hand-over: the learner's own days and pg_update continue from the imitation's state by the policy-gradient law
    if case == 0:
        start = e.pg_state()
        e.rollout_reset()
        e.run_days("mlp", T, BUDGET)
        rec = e.rollout_fetch(bootstrap=True)
        stats = e.pg_update(2)
        ref, rstats = P.update(pol, start, rec, rec["bootstrap_value"], 2, opts)
        _assert_state(e.pg_state(), ref, "hand-over")
        for k in P.STAT_KEYS:
            assert _same(np.float64(stats[k]), np.float64(rstats[k])), k
    e.close()
    f.close()


# ---- 5. demonstrations ---------------------------------------------------------------------------------------------------------------
def test_demonstrations_fill_the_td3_ring_and_the_sac_store_refuses(amd):
    from adcraft_amd._ffi import EngineStateError as State
    from tests import sac_ref as SR
    N, K, T = N0, K0, T0
    D, A = 5 * K + 2, K + 1
    rng = np.random.default_rng(17)
    pol = _policy(rng, K, value=False)
    crit = T3.random_critics_for_tests(rng, K, (12, 1))
    opts = T3.options(critic_widths=(12, 1), batch_size=8, capacity=100, seed=123)
    e = _engine(amd, N, K, **RESETS)
    e.sample_actions(0.3, 1.0, 40.0)
    e.mlp_init(pol, None, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.td3_init(**opts)
    e.td3_set_critics(crit)
    e.teach_days("fixed", T)
    assert e.td3_store() == T * N
    rec, buf = e.rollout_fetch(), e.td3_buffer()
    assert buf["size"] == T * N
    assert _same(buf["x"], rec["obs"].reshape(T * N, D)) and _same(buf["a"], rec["action"].reshape(T * N, A))
    assert _same(buf["r"], rec["reward"].reshape(-1)) and _same(buf["x2"][:(T - 1) * N][~buf["done"][:(T - 1) * N]],
                                                                 rec["obs"][1:].reshape(-1, D)[~buf["done"][:(T - 1) * N]])
    state = T3.fresh_state(pol, crit)
    stats = e.td3_update(1)
    state, rstats = T3.update(pol, state, buf, None, 123, opts)
    got = e.td3_state()
    for k in T3.STATE_KEYS:
        assert _same(got[k], state[k]), k
    for k in T3.STAT_KEYS:
        assert _same(np.float64(stats[k]), np.float64(rstats[k])), k
    e.close()
    # soft actor-critic: the ring would need the pre-squash action
    spol = SR.sac_policy(rng, K, (8,), "tanh", clamp=(-1.0, -0.5), normalize=True, scale=0.6)
    spol.shift, spol.scale = R.realistic_norm(K)
    e = _engine(amd, N, K, **RESETS)
    e.sample_actions(0.3, 1.0, 40.0)
    e.mlp_init(spol, None, deterministic=False)
    e.rollout_enable(T, obs=True)
    bounds = np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], np.full(K, 3.0)]).astype(F)
    e.mlp_set_squash(*bounds)
    e.sac_init(**SR.options(K, critic_widths=(12, 1), batch_size=8, capacity=100))
    e.sac_set_critics(crit)
    with pytest.raises(State, match="squash"):
        e.teach_days("fixed", 2)
    e.mlp_set_squash(None, None)                                     # (the only way a teacher day gets into a SAC trainer's record)
    e.teach_days("fixed", 2)
    e.mlp_set_squash(*bounds)
    with pytest.raises(State, match="teacher days"):
        e.sac_store()
    e.close()


# ---- 6. it clones ----------------------------------------------------------------------------------------------------------------------
def test_cloning_a_constant_action_raises_its_log_probability(amd):
    """the host test's run (tests/test_imitation_host.py) on the device: a fixed teacher with one constant action, log_std = 0
    left untrained; after 30 updates the mean logp is strictly greater than before the first"""
    N, K, T = N0, K0, T0
    pol = clone_policy(K)
    e = _engine(amd, N, K, **RESETS)
    e.sample_actions(CLONE["bid"], CLONE["bid"], CLONE["budget"])
    e.mlp_init(pol, None, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.pg_init(**P.options(lr=CLONE["lr"]))
    e.im_init(beta=0.0, vf_coef=0.0, train_log_std=False)
    e.teach_days("fixed", T)
    rec = e.rollout_fetch()
    assert len({tuple(a) for a in rec["action"].reshape(-1, K + 1)}) == 1, "one constant action"
    e.im_advantages()
    logps = [e.im_minibatch(0, N)["logp"] for _ in range(CLONE["updates"] + 1)]
    assert logps[-1] > logps[0], logps
    assert np.array_equal(e.pg_state()["theta"][-(K + 1):], np.zeros(K + 1, F))
    e.close()
