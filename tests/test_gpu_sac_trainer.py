"""GPU tests of soft actor-critic on the device (parts/kernel_sac.inc, parts/sac_api.inc) and of the squashed act
(parts/kernel_mlp_policy.inc) against the numpy restatement tests/sac_ref.py, bit for bit: the squashed act with squash on, off
and never set, the replay ring through auto-resets and a wrap, updates with state, statistics and alpha after each, the chunk
boundary, independence of the call shape, a resumed state, that nothing else moved, and every refusal.  None of these symbols
exists before this feature: every test here fails on the parent commit."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import sac_ref as S
from tests import td3_ref as T3

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


def _engine(amd, N, K, seed=3, mean_volume=24, **kw):
    e = amd.StepEngine(N, K, seed=seed, **kw)
    e.set_all_params(H.implicit_params(N, K, seed + 1, mean_volume=mean_volume, cvr=0.5))
    e.reset()
    return e


def _policy(rng, K, hidden=(16, 8), act="tanh", clamp=(-1.0, -0.5), **kw):
    pol = S.sac_policy(rng, K, hidden, act, clamp=clamp, normalize=True, scale=0.6, **kw)
    pol.shift, pol.scale = R.realistic_norm(K)
    # the log-std head's biases from below the clamp's lower bound to above its upper one
    pol.layers[-1][1][K + 1:] = np.linspace(clamp[0] - 0.6, clamp[1] + 0.6, K + 1).astype(F)
    return pol


def _bounds(K):
    """budget in [50, 1500], bids in [0.02, 3 + k / 10]"""
    return np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], 3.0 + np.arange(K) / 10.0]).astype(F)


def _trainer(amd, pol, critics, N, K, T, opts, agent_seeds, seed=41, **engine_kw):
    e = _engine(amd, N, K, seed=seed, **engine_kw)
    e.mlp_init(pol, agent_seeds, deterministic=False)
    e.mlp_set_squash(*_bounds(K))
    e.rollout_enable(T, obs=True)
    e.sac_init(**opts)
    e.sac_set_critics(critics)
    return e


def _assert_state(got, ref, what=""):
    for k in S.STATE_KEYS:
        assert _same(got[k], ref[k]), (k, what, got[k][:4], ref[k][:4])
    assert got["updates"] == ref["updates"], what


def _assert_stats(got, ref, what=""):
    for k in S.STAT_KEYS:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


def _assert_buffer(got, ref, what=""):
    for k in ("x", "a", "r", "done", "x2"):
        assert _same(got[k], ref[k]), (k, what)
    assert (got["size"], got["written"], got["capacity"]) == (ref["size"], ref["written"], ref["capacity"]), what


def _current_input(e, pol):
    return T3.current_input(pol, e.fetch(), e.get_episode_state()[0] == 0)


RESETS = dict(max_days=4, auto_reset=True)
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)
N0, K0, T0 = 12, 9, 7


def _assert_act(e, ref, what):
    st = e.mlp_last()
    st["bids"], st["budget"] = e.get_actions()
    for k in ("mean", "log_std", "action", "logp", "value", "bids", "budget"):
        assert _same(st[k], ref[k]), (what, k, st[k], ref[k])


@pytest.mark.parametrize("K", [1, 9])
def test_the_squashed_act(amd, K):
    """bids and budgets are the restatement's bits, stochastic (replayed normals, the agent's own stream) and deterministic; the
    last act's action and the record's keep u; an engine that never had squash and one that had it turned off again give the act
    without it"""
    N, A = N0, K + 1
    rng = np.random.default_rng(100 + K)
    pol = _policy(rng, K, clamp=(-4.0, 1.0), value=True)
    lo, hi = _bounds(K)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    keys = [R.agent_key(s) for s in seeds]
    e, plain = _engine(amd, N, K, seed=11), _engine(amd, N, K, seed=11)
    e.mlp_init(pol, seeds)
    plain.mlp_init(pol, seeds)
    e.mlp_set_squash(lo, hi)
    e.rollout_enable(2, obs=True)
    zero = np.zeros((N, 5 * K + 2), F)
    z = (rng.standard_normal((N, A)) * 3).astype(F)
    e.mlp_act(0.0, z)                                                   # tick 0 -> 1
    ref = S.squashed_act(pol, zero, z, lo, hi)
    _assert_act(e, ref, "first day")
    assert (ref["bids"] <= hi[1:] + 0.005).all() and (ref["budget"] >= lo[0]).all() and (ref["budget"] <= hi[0]).all()
    assert not _same(ref["bids"], R.act(pol, zero, z)["bids"])
    e.mlp_step()                                                        # tick 1 -> 2, recorded
    rec = e.rollout_fetch()
    z1 = R.normals(keys, [1] * N, A)
    r1 = S.squashed_act(pol, zero, z1, lo, hi)
    assert _same(rec["action"][0], r1["action"]) and _same(rec["logp"][0], r1["logp"]), "the record keeps u and its log-probability"
    obs = R.flat_obs(e.fetch())
    e.mlp_act(0.0, z)
    _assert_act(e, S.squashed_act(pol, obs, z, lo, hi), "replay")
    e.mlp_act(77.25)                                                    # tick 3 -> 4, drawn at tick 3
    _assert_act(e, S.squashed_act(pol, obs, R.normals(keys, [3] * N, A), lo, hi, budget_override=77.25), "own stream")
    e.mlp_set_deterministic(True)
    e.mlp_act()
    ref = S.squashed_act(pol, obs, None, lo, hi, deterministic=True)
    _assert_act(e, ref, "deterministic")
    assert _same(ref["action"], ref["mean"]) and _same(e.mlp_agent_state()[1], np.full(N, 5, np.uint32))
    # off again, and never on: the act without squash
    e.mlp_set_deterministic(False)
    e.mlp_set_squash(None, None)
    e.mlp_act(0.0, z)
    plain.mlp_act(0.0, z)
    _assert_act(plain, R.act(pol, zero, z), "never set")
    _assert_act(e, R.act(pol, obs, z), "turned off")
    # re-initialisation clears it
    e.mlp_set_squash(lo, hi)
    e.mlp_init(pol, seeds)
    e.mlp_act(0.0, z)
    _assert_act(e, R.act(pol, obs, z), "after mlp_init")
    e.close()
    plain.close()


UPDATE_CASES = [("tanh", (12, 1)), ("relu", (12, 1)), ("tanh", (1,)), ("relu", (1,))]


@pytest.mark.parametrize("act,widths", UPDATE_CASES, ids=["tanh-12", "relu-12", "tanh-none", "relu-none"])
def test_store_and_five_updates_equal_the_restatement(amd, act, widths):
    """three collect-and-store rounds of 84 transitions into a ring of 200 through auto-resets (it wraps once), the ring against
    the restatement's; then five updates at batch 7 under the tight clamp [-1, -0.5] (raw log-stds on both sides of it): state,
    statistics and alpha after every update; target_update_interval 2"""
    from adcraft_amd import _ffi
    rng = np.random.default_rng(21)
    pol = _policy(rng, K0, act=act, value=True)
    crit = T3.random_critics_for_tests(rng, K0, widths)
    seeds = rng.integers(0, 2 ** 63, N0).astype(np.uint64)
    opts = S.options(K0, critic_widths=widths, batch_size=7, capacity=200, seed=123, tau=0.05, gamma=0.9, reward_scale=0.01, init_alpha=0.3,
                     alpha_lr=3e-3, actor_lr=3e-3, critic_lr=3e-3, target_update_interval=2)
    e = _trainer(amd, pol, crit, N0, K0, T0, opts, seeds, **RESETS)
    state = S.fresh_state(pol, crit, opts)
    _assert_state(e.sac_state(), state, "theta starts as the device's policy, the target critics as copies")
    assert e.sac_param_counts() == (state["theta"].size, state["psi"].size)
    ring = T3.Ring(200, 5 * K0 + 2, K0 + 1)
    assert e.sac_buffer()["size"] == 0
    for rnd in range(3):
        e.rollout_reset()
        e.run_days("mlp", T0, 1000.0)
        assert e.sac_store() == T0 * N0
        ring.store(e.rollout_fetch(bootstrap=True), _current_input(e, pol))
        _assert_buffer(e.sac_buffer(), ring.buffer(), rnd)
    buf = e.sac_buffer()
    assert buf["size"] == 200 and buf["written"] == 252 and buf["done"].any() and not buf["done"].all()
    assert np.abs(buf["a"]).max() > 1.0, "the ring holds u, not the squashed action"
    for u in range(5):
        idx = e.sac_batch_indices(u)
        assert _same(idx, T3.twin_batch_indices(_ffi.lib(), 123, u, 200, 7))
        before = e.sac_state()
        stats = e.sac_update(1)
        state, rstats = S.update(pol, state, buf, 123, opts)
        after = e.sac_state()
        _assert_state(after, state, u)
        _assert_stats(stats, rstats, u)
        assert (stats["updates"], stats["buffer_size"], stats["samples"]) == (u + 1, 200, 7)
        assert not _same(before["theta"], after["theta"]) and not _same(before["psi"], after["psi"]) and not _same(before["log_alpha"], after["log_alpha"])
        assert (not _same(before["psi_target"], after["psi_target"])) == (u % 2 == 1)
    # the clamp was engaged on both sides, and some log-stds lay inside it
    sh = T3.Shapes(pol, opts)
    raw = T3.forward(buf["x"], sh.actor(state["theta"]), sh.act)[-1][:, K0 + 1:]
    assert (raw < -1.0).any() and (raw > -0.5).any() and ((raw > -1.0) & (raw < -0.5)).any()
    assert _same(e.mlp_params(), state["theta"]), "the device's policy layers follow theta"
    e.close()


def test_identical_critics_tie_takes_critic_one(amd):
    rng = np.random.default_rng(23)
    pol = _policy(rng, K0)
    crit = T3.random_critics_for_tests(rng, K0, (12, 1))
    crit[1] = [(w.copy(), b.copy()) for w, b in crit[0]]
    opts = S.options(K0, critic_widths=(12, 1), batch_size=7, capacity=100, seed=9, reward_scale=0.5, actor_lr=3e-3, critic_lr=3e-3)
    e = _trainer(amd, pol, crit, N0, K0, T0, opts, None, **NO_RESETS)
    buf = _random_buffer(rng, K0, 84)
    e.sac_buffer_load(buf)
    state = S.fresh_state(pol, crit, opts)
    for u in range(2):
        stats = e.sac_update(1)
        state, rstats = S.update(pol, state, buf, 9, opts)
        assert rstats["picked2"] == 0, "identical critics with identical moments stay identical: every element ties"
        _assert_state(e.sac_state(), state, u)
        _assert_stats(stats, rstats, u)
    e.close()


def test_interval_three_gates_polyak_and_alpha_lr_zero_leaves_alpha(amd):
    """target_update_interval 3: the target critics move on updates 3 and 6 alone; alpha_lr 0: no temperature step is launched,
    log_alpha and its moments keep their bits and the statistics report init_alpha's alpha; seven updates against the restatement"""
    rng = np.random.default_rng(27)
    pol = _policy(rng, K0)
    crit = T3.random_critics_for_tests(rng, K0, (12, 1))
    opts = S.options(K0, critic_widths=(12, 1), batch_size=7, capacity=100, seed=19, reward_scale=0.5, actor_lr=3e-3, critic_lr=3e-3, tau=0.05,
                     init_alpha=0.7, alpha_lr=0.0, target_update_interval=3)
    e = _trainer(amd, pol, crit, N0, K0, T0, opts, None, **NO_RESETS)
    buf = _random_buffer(rng, K0, 84)
    e.sac_buffer_load(buf)
    state = S.fresh_state(pol, crit, opts)
    la0, moved = state["log_alpha"].copy(), []
    for u in range(7):
        before = e.sac_state()["psi_target"]
        stats = e.sac_update(1)
        state, rstats = S.update(pol, state, buf, 19, opts)
        after = e.sac_state()
        _assert_state(after, state, u)
        _assert_stats(stats, rstats, u)
        assert _same(after["log_alpha"], la0) and stats["alpha"] == float(S.alpha_of(la0[0]))
        moved.append(not _same(before, after["psi_target"]))
    assert moved == [False, False, True, False, False, True, False]
    # one call over the gate equals the calls of one
    f = _trainer(amd, pol, crit, N0, K0, T0, opts, None, **NO_RESETS)
    f.sac_buffer_load(buf)
    f.sac_update(7)
    _assert_state(f.sac_state(), state, "one call of seven")
    e.close()
    f.close()


def test_the_trainer_exports_the_squash_bounds_with_the_weights(amd):
    """SACTrainer.policy(): the trained actor's layers and the bounds; installed on a fresh engine, its deterministic act is the
    restatement's squashed mean"""
    from adcraft_amd.baselines.sac_trainer import SACTrainer, sac
    N, K, T = 8, 6, 3
    rng = np.random.default_rng(37)
    pol = _policy(rng, K, (8,))
    lo, hi = _bounds(K)
    e = _engine(amd, N, K, seed=41, **NO_RESETS)
    tr = SACTrainer(e, pol, lo, hi, horizon=T, **sac(K, critic_hidden=(8,), learning_starts=T * N, updates_per_iteration=2, batch_size=8, capacity=64,
                                                     reward_scale=0.01))
    assert tr.learning_starts == T * N and tr.updates_per_iteration == 2
    stats = tr.iteration(T, 1000.0)
    assert stats["updates"] == 2 and tr.state()["updates"] == 2
    out = tr.policy()
    assert _same(out.action_lo, lo) and _same(out.action_hi, hi)
    assert _same(T3.flat_of(out.policy.layers), tr.state()["theta"]) and not _same(T3.flat_of(out.policy.layers), T3.flat_of(pol.layers))
    g = _engine(amd, N, K, seed=43, **NO_RESETS)
    out.install(g, deterministic=True)
    g.mlp_act()
    _assert_act(g, S.squashed_act(out.policy, np.zeros((N, 5 * K + 2), F), None, lo, hi, deterministic=True), "installed")
    e.close()
    g.close()


def _random_buffer(rng, K, size):
    D, A = 5 * K + 2, K + 1
    return dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * 1.5).astype(F),
                r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))


def test_a_batch_across_the_chunk_boundary(amd):
    """K = 2, batch 1030: the float64 sums cross a 1024-sample chunk; two updates"""
    K, B = 2, 1030
    rng = np.random.default_rng(33)
    pol = _policy(rng, K, (12,))
    crit = T3.random_critics_for_tests(rng, K, (12, 1))
    opts = S.options(K, critic_widths=(12, 1), batch_size=B, capacity=100, seed=77, reward_scale=0.5)
    e = _trainer(amd, pol, crit, N0, K, T0, opts, None, **NO_RESETS)
    buf = _random_buffer(rng, K, 84)
    e.sac_buffer_load(buf)
    state = S.fresh_state(pol, crit, opts)
    for u in range(2):
        stats = e.sac_update(1)
        state, rstats = S.update(pol, state, buf, 77, opts)
        _assert_state(e.sac_state(), state, u)
        _assert_stats(stats, rstats, u)
        assert 0 < rstats["picked2"] < B
    e.close()


@pytest.mark.parametrize("clip", [0.0, 0.5], ids=["no-clip", "clip"])
def test_one_call_of_three_equals_three_calls_of_one(amd, clip):
    rng = np.random.default_rng(43)
    pol = _policy(rng, K0)
    crit = T3.random_critics_for_tests(rng, K0, (12, 1))
    opts = S.options(K0, critic_widths=(12, 1), batch_size=16, capacity=100, seed=5, max_grad_norm=clip, actor_lr=3e-3, critic_lr=3e-3, alpha_lr=3e-3)
    buf = _random_buffer(rng, K0, 84)
    ends = []
    for calls in ((3,), (1, 1, 1)):
        e = _trainer(amd, pol, crit, N0, K0, T0, opts, None, **NO_RESETS)
        e.sac_buffer_load(buf)
        for n in calls:
            stats = e.sac_update(n)
        ends.append((e.sac_state(), stats))
        e.close()
    _assert_state(ends[0][0], ends[1][0])
    _assert_stats(ends[0][1], ends[1][1])
    state = S.fresh_state(pol, crit, opts)
    for _ in range(3):
        state, rstats = S.update(pol, state, buf, 5, opts)
    _assert_state(ends[0][0], state)
    _assert_stats(ends[0][1], rstats)
    if clip:
        assert rstats["critic_grad_norm"] > clip, "the clip was meant to engage"


def test_a_resumed_state_and_ring_continue_to_the_same_bits(amd):
    rng = np.random.default_rng(51)
    N, K, T = 8, 8, 4
    pol = _policy(rng, K, (12,))
    crit = T3.random_critics_for_tests(rng, K, (12, 1))
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = S.options(K, critic_widths=(12, 1), batch_size=16, capacity=80, seed=9, actor_lr=3e-3, critic_lr=3e-3, alpha_lr=3e-3, reward_scale=0.01)

    def iteration(e):
        e.rollout_reset()
        e.run_days("mlp", T, 1000.0)
        e.sac_store()
        e.sac_update(3)
        return e.sac_state(), e.sac_buffer()

    a = _trainer(amd, pol, crit, N, K, T, opts, seeds, **NO_RESETS)
    full = [iteration(a) for _ in range(3)]
    a.close()
    b = _trainer(amd, pol, T3.random_critics_for_tests(rng, K, (12, 1)), N, K, T, opts, seeds, **NO_RESETS)
    b.run_days("mlp", T, 1000.0)                                      # (the envs' and agents' streams, as after iteration 1; not stored)
    b.rollout_reset()
    b.sac_state(full[0][0])
    b.sac_buffer_load(full[0][1])
    _assert_state(b.sac_state(), full[0][0])
    assert _same(b.mlp_params(), full[0][0]["theta"])
    for it in (1, 2):
        st, ring = iteration(b)
        _assert_state(st, full[it][0], it)
        _assert_buffer(ring, full[it][1], it)
    assert not _same(full[0][0]["log_alpha"], full[2][0]["log_alpha"])
    b.close()


def test_nothing_else_moved(amd):
    """training draws from its own key alone: with updates in between, the envs' state and streams, the agents' keys and ticks sit
    where they sit without"""
    N, K, T = 12, 10, 4
    rng = np.random.default_rng(61)
    pol = _policy(rng, K)
    crit = T3.random_critics_for_tests(rng, K, (8, 1))
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = S.options(K, critic_widths=(8, 1), batch_size=16, capacity=500, actor_lr=3e-3, critic_lr=3e-3, reward_scale=0.01)
    e = _trainer(amd, pol, crit, N, K, T, opts, seeds, **NO_RESETS)
    e.run_days("mlp", T, 1000.0)
    e.sac_store()
    before = (e.fetch(), e.get_rng_state(), e.mlp_agent_state(), e.get_episode_state())
    e.sac_update(4)
    after = (e.fetch(), e.get_rng_state(), e.mlp_agent_state(), e.get_episode_state())
    for k in before[0]:
        assert _same(before[0][k], after[0][k]), k
    for i in (1, 2, 3):
        for x, y in zip(before[i], after[i]):
            assert _same(x, y), i
    assert np.all(after[2][1] == T)
    e.close()


def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd import _ffi
    N, K, T = 8, 6, 3
    rng = np.random.default_rng(71)
    pol = _policy(rng, K, (8,))
    crit = T3.random_critics_for_tests(rng, K, (8, 1))
    base = dict(critic_widths=(8, 1), batch_size=8, capacity=40)
    lo, hi = _bounds(K)
    e = _engine(amd, N, K, seed=81, **NO_RESETS)
    with pytest.raises(_ffi.EngineStateError, match="mlp_init"):
        e.sac_init(**base)
    with pytest.raises(_ffi.EngineStateError, match="mlp_init"):
        e.mlp_set_squash(lo, hi)
    # a free-head policy; the clamp off; squash not set; no record; no recorded input
    e.mlp_init(R.random_policy(rng, K, (8,)), deterministic=False)
    e.mlp_set_squash(lo, hi)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="two-headed"):
        e.sac_init(**base)
    e.mlp_init(R.random_policy(rng, K, (8,), two_heads=True), deterministic=False)
    e.mlp_set_squash(lo, hi)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="clamp_log_std"):
        e.sac_init(**base)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="mlp_set_squash"):
        e.sac_init(**base)
    # squash: bad bounds; a population or learners with it on, and it with them active
    for bad_lo, bad_hi in ((lo, lo), (lo, np.where(np.arange(K + 1) == 1, np.inf, hi)), (np.full(K + 1, np.nan, F), hi)):
        with pytest.raises(ValueError, match="squash bounds"):
            e.mlp_set_squash(bad_lo, bad_hi)
    e.mlp_set_squash(lo, hi)
    with pytest.raises(_ffi.EngineStateError, match="squashed action"):
        e.mlp_population(2)
    with pytest.raises(_ffi.EngineStateError, match="squashed action"):
        e.mlp_learners(2)
    e.mlp_set_squash(None, None)
    e.mlp_population(2)
    with pytest.raises(_ffi.EngineStateError, match="population active"):
        e.mlp_set_squash(lo, hi)
    e.mlp_population(0)
    e.mlp_learners(2)
    with pytest.raises(_ffi.EngineStateError, match="learners active"):
        e.mlp_set_squash(lo, hi)
    e.mlp_learners(0)
    e.mlp_set_squash(lo, hi)
    e.mlp_init(pol, deterministic=False)                               # (the record went with the re-initialisation)
    e.mlp_set_squash(lo, hi)
    with pytest.raises(_ffi.EngineStateError, match="rollout record"):
        e.sac_init(**base)
    e.rollout_enable(T)
    with pytest.raises(_ffi.EngineStateError, match="ADC_ROLLOUT_OBS"):
        e.sac_init(**base)
    e.rollout_enable(T, obs=True)
    # a policy-gradient or TD3 trainer alive, and theirs while SAC lives
    e.pg_init()
    with pytest.raises(_ffi.EngineStateError, match="policy-gradient trainer is alive"):
        e.sac_init(**base)
    e.mlp_init(pol, deterministic=False)
    e.mlp_set_squash(lo, hi)
    e.rollout_enable(T, obs=True)
    for name in ("sac_store", "sac_state", "sac_buffer", "sac_param_counts", "sac_sync_targets"):
        with pytest.raises(_ffi.EngineStateError, match="sac_init"):
            getattr(e, name)()
    with pytest.raises(_ffi.EngineStateError, match="sac_init"):
        e.sac_update(1)
    with pytest.raises(ValueError, match="tau"):
        e.sac_init(tau=0.0, **base)
    e.sac_init(**base)
    with pytest.raises(_ffi.EngineStateError, match="soft actor-critic trainer is alive"):
        e.pg_init()
    with pytest.raises(_ffi.EngineStateError):
        e.td3_init(**base)
    with pytest.raises(_ffi.EngineStateError, match="soft actor-critic trainer is alive"):
        e.obs_norm_init()
    with pytest.raises(_ffi.EngineStateError):
        e.rew_norm_init()
    with pytest.raises(_ffi.EngineStateError):
        e.td3_norm_init(observations=True)
    with pytest.raises(_ffi.EngineStateError):
        e.pbt_init("td3", replace_count=1)
    with pytest.raises(_ffi.EngineStateError, match="adc_engine_td3_init has not been called"):
        e.td3_update(1)
    # an update before the critics were uploaded, and with an empty ring; a population or learners active
    with pytest.raises(_ffi.EngineStateError, match="critic layer"):
        e.sac_update(1)
    e.sac_set_critics(crit)
    with pytest.raises(_ffi.EngineStateError, match="empty"):
        e.sac_update(1)
    with pytest.raises(_ffi.EngineStateError, match="empty"):
        e.sac_batch_indices(0)
    with pytest.raises(_ffi.EngineStateError, match="no unstored day"):
        e.sac_store()
    e.mlp_set_squash(None, None)
    with pytest.raises(_ffi.EngineStateError, match="mlp_set_squash"):
        e.sac_update(1)
    e.mlp_population(2)
    with pytest.raises(_ffi.EngineStateError, match="squash"):
        e.sac_update(1)
    e.mlp_population(0)
    e.mlp_set_squash(lo, hi)
    with pytest.raises(ValueError, match="updates"):
        e.sac_update(0)
    # the engine is usable: collect, store, update
    e.run_days("mlp", T, 1000.0)
    assert e.sac_store() == T * N
    st = e.sac_update(2)
    assert st["updates"] == 2 and np.isfinite(st["critic_loss"]) and np.isfinite(st["actor_loss"]) and st["alpha"] > 0
    # the trainer does not survive a re-initialised policy or record
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="sac_init"):
        e.sac_update(1)
    e.close()


def test_lds_overflow_is_refused(amd):
    """K = 720 with the widest networks: the batch kernels' row, activations, deltas and head vectors do not fit 64 KB"""
    N, K = 1, 720
    rng = np.random.default_rng(5)
    pol = S.sac_policy(rng, K, (256, 256, 256), "tanh", clamp=(-5.0, 2.0))
    e = _engine(amd, N, K, seed=7, mean_volume=8, **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    e.mlp_set_squash(*_bounds(K))
    e.rollout_enable(2, obs=True)
    opts = dict(critic_widths=(256, 256, 256, 1), batch_size=8, capacity=16)
    D, A, maxw = 5 * K + 2, K + 1, 2 * (K + 1)
    floats = (D + A) + (3 * 256 + 2 * A) + 2 * (3 * 256 + 1) + 3 * maxw + 6 * A + 8
    assert floats * 4 > 64 * 1024
    with pytest.raises(ValueError, match="LDS"):
        e.sac_init(**opts)
    e.mlp_act(10.0)                                                    # the engine stays usable
    e.close()


def test_a_wrapped_ring_reloaded_at_a_slot_continues_bit_for_bit_and_the_shared_refusals_say_why(amd):
    """the smallest trainer whose store wraps the ring (4 envs x 3 days into 8 slots): its state and its ring - the ring loaded in
    two pieces, the second at slot 3 - carry a fresh engine through two more updates to the bits of the uninterrupted run; then
    every refusal the off-policy front ends share, by its words, and the engine goes on"""
    from adcraft_amd import _ffi
    N, K, T = 4, 2, 3
    rng = np.random.default_rng(91)
    pol = _policy(rng, K, (8,))
    crit = T3.random_critics_for_tests(rng, K, (8, 1))
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = S.options(K, critic_widths=(8, 1), batch_size=4, capacity=8, seed=9, actor_lr=3e-3, critic_lr=3e-3, alpha_lr=3e-3)
    fresh = lambda: _trainer(amd, pol, crit, N, K, T, opts, seeds, **NO_RESETS)
    a = fresh()
    a.run_days("mlp", T, 1000.0)
    assert a.sac_store() == 12
    a.sac_update(1)
    state, ring = a.sac_state(), a.sac_buffer()
    assert (ring["size"], ring["written"], ring["capacity"]) == (8, 12, 8)
    b = fresh()
    part = lambda lo, hi: {k: ring[k][lo:hi] for k in ("x", "a", "r", "done", "x2")}
    b.sac_buffer_load(part(0, 3))
    assert b.sac_buffer(fetch=False) == dict(size=3, written=3, capacity=8)
    b.sac_buffer_load(part(3, 8), slot=3, written=12)
    b.sac_state(state)
    _assert_buffer(b.sac_buffer(), ring)
    _assert_state(b.sac_state(), state)
    assert b.sac_param_counts() == a.sac_param_counts()
    assert _same(a.sac_batch_indices(1), b.sac_batch_indices(1)) and a.sac_batch_indices(1).shape == (4,)
    _assert_stats(b.sac_update(2), a.sac_update(2))
    _assert_state(b.sac_state(), a.sac_state())
    assert b.sac_state()["updates"] == 3
    a.close()
    lib, h, p = b._lib, b._h, lambda v: v.ctypes.data
    x, ac, r, dn = np.zeros((4, 5 * K + 2), F), np.zeros((4, K + 1), F), np.zeros(4, F), np.zeros(4, np.uint8)
    (w, bias), idx = crit[0][0], np.zeros(4, np.int32)
    last = b.sac_state()
    vec = [p(last[k]) for k in amd.StepEngine.SAC_STATE]
    refused = (
        (r"slot range is not inside \[0, size\)", lambda: lib.adc_engine_sac_buffer_fetch(h, 7, 2, p(x), p(ac), p(r), p(dn), p(x))),
        (r"x, a, r, done or x2 is NULL", lambda: lib.adc_engine_sac_buffer_load(h, 0, 4, p(x), None, p(r), p(dn), p(x), 4)),
        (r"slot range is not inside \[0, capacity\)", lambda: lib.adc_engine_sac_buffer_load(h, 6, 4, p(x), p(ac), p(r), p(dn), p(x), 12)),
        (r"written: at least slot \+ count", lambda: lib.adc_engine_sac_buffer_load(h, 0, 4, p(x), p(ac), p(r), p(dn), p(x), 3)),
        (r"critic: 0 or 1", lambda: lib.adc_engine_sac_set_critic_layer(h, 2, 0, p(w), p(bias))),
        (r"no such critic layer", lambda: lib.adc_engine_sac_set_critic_layer(h, 0, 2, p(w), p(bias))),
        (r"weights or bias is NULL", lambda: lib.adc_engine_sac_set_critic_layer(h, 0, 0, p(w), None)),
        (r"idx_b is NULL", lambda: lib.adc_engine_sac_batch_indices(h, 0, None)),
        (r"update: 0 to 2\^32 - 2", lambda: lib.adc_engine_sac_batch_indices(h, -1, p(idx))),
        (r"updates: 1 to 65536", lambda: lib.adc_engine_sac_update(h, 0, None)),
        (r"a state vector is NULL", lambda: lib.adc_engine_sac_state_set(h, *vec[:-1], None, 0)),
        (r"updates: 0 to 2\^31 - 2", lambda: lib.adc_engine_sac_state_set(h, *vec, 2 ** 31 - 1)),
    )
    for words, call in refused:
        with pytest.raises(ValueError, match=words):
            _ffi.check(call())
    # (SAC's update counter ends at 2^31 - 1: the state's largest count leaves no update)
    b.sac_state(dict(last, updates=2 ** 31 - 2))
    with pytest.raises(_ffi.EngineStateError, match="the update counter is exhausted"):
        b.sac_update(1)
    b.sac_state(last)
    _assert_buffer(b.sac_buffer(), ring)
    _assert_state(b.sac_state(), last)
    assert b.sac_update(1)["updates"] == 4
    assert not _same(b.sac_state()["psi_target"], b.sac_state()["psi"])
    b.sac_sync_targets()
    synced = b.sac_state()
    assert _same(synced["psi_target"], synced["psi"])
    b.replay_prio_init()
    with pytest.raises(_ffi.EngineStateError, match="prioritised replay is alive"):
        b.sac_batch_indices(0)
    b.close()
