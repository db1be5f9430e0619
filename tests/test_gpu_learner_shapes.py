"""GPU tests of the learner kernels at wide, deep and ragged network shapes (the shapes W1-W3 of
tests/learner_shapes.py).  Every per-sample kernel - k_pg_sample, the TD3 and SAC target / critic / actor kernels, their
population, KL, gather and queued instances - runs a sample in one 256-lane workgroup, eight lanes a neuron: a layer loop covers
32 neurons a pass, weights sit in blocks of 32 inputs read in chains of 8, the weight gradient is cut into 16 x 16 tiles, head
loops stride by 256, and every buffer is laid out by hand in dynamic LDS.  The other GPU tests train hidden widths of at most
33 and K <= 24; here only the network varies: 8 envs, 5 days, 40 samples, below one 1024-sample chunk.

1. the device against the numpy restatements (tests/pg_ref.py, td3_ref.py, sac_ref.py and the add-ons') bit for bit at W1-W3;
2. the device's gradient - read exactly from the first moment after one Adam step with beta1 = 0 - against PyTorch float64
   autograd under the yardstick of tests/test_pg_host.py, float32 autograd's own error on the same arrays;
3. the last K each family's LDS limit accepts, trained bit for bit, and the refusal one keyword (or one frame's worth) further.
Measured figures: profiles/pr_learner_shapes.txt."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import learner_shapes as W
from tests import mlp_ref as R
from tests import pg_kl_ref as KR
from tests import pg_pop_ref as PP
from tests import pg_ref as P
from tests import pg_shuffle_ref as SR
from tests import sac_ref as S
from tests import td3_pop_ref as TP
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F = np.float32
N, T, BUDGET = 8, 5, 1000.0
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)
NAMES = ("W1", "W2", "W3")
# one seed a case: the policy's and critics' draws, the engine's streams and the agents'
PG_SEED = dict(W1=111, W2=113, W3=13)
TD3_SEED = dict(W1=21, W2=22)
SAC_SEED = dict(W1=31, W2=32, W3=33)


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


def _engine(amd, K, seed, envs=N, **kw):
    """a small engine: few auctions a day, no binding budget"""
    e = amd.StepEngine(envs, K, seed=seed, **dict(NO_RESETS, **kw))
    e.set_all_params(H.implicit_params(envs, K, seed + 1, mean_volume=4, cvr=0.5))
    e.reset()
    return e


def _normed(pol, K):
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


# ======================================================================================================================================
# PPO / A2C
# ======================================================================================================================================
def _pg_policy(rng, name):
    return _normed(W.pg_policy(rng, name, normalize=True), W.SHAPES[name]["K"])


def _pg_fresh(pol):
    theta = P.flat_params(pol)
    return dict(theta=theta, m=np.zeros_like(theta), v=np.zeros_like(theta), steps=0)


def _assert_pg_state(got, ref, what=""):
    for k in ("theta", "m", "v"):
        assert _same(got[k], ref[k]), (k, what)
    assert got["steps"] == ref["steps"], what


def _assert_pg_stats(got, ref, what=""):
    for k in P.STAT_KEYS:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


def _pg_collected(amd, pol, K, opts, seed, days=T):
    """an engine with the trainer alive and `days` recorded: (engine, record with the bootstrap values, adv, ret)"""
    rng = np.random.default_rng(seed)
    e = _engine(amd, K, seed)
    e.mlp_init(pol, rng.integers(0, 2 ** 63, N).astype(np.uint64), deterministic=False)
    e.rollout_enable(days, obs=True)
    e.pg_init(**opts)
    _assert_pg_state(e.pg_state(), _pg_fresh(pol), "theta starts as the device's weights: the flat <-> chain-major mapping")
    assert e.pg_param_count() == P.flat_params(pol).size
    e.run_days("mlp", days, BUDGET)
    rec = e.rollout_fetch(bootstrap=bool(pol.value_layers))
    if not pol.value_layers:
        rec["bootstrap_value"] = np.zeros(N, F)                         # (without a value network every value is +0)
    adv, ret = e.pg_advantages(fetch=True)
    radv, rret = P.gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], rec["bootstrap_value"], **opts)
    assert _same(adv, radv) and _same(ret, rret)
    return e, rec, adv, ret


def _samples(rec, adv, ret, n0=0, B=N):
    """pg_ref.grad's sample arrays of the envs [n0, n0 + B): sample s = t * B + (env - n0)"""
    flat = lambda a: np.ascontiguousarray(a[:, n0:n0 + B]).reshape((-1,) + a.shape[2:])
    return flat(rec["obs"]), flat(rec["action"]), flat(rec["logp"]), flat(adv), flat(ret), flat(rec["value"])


def _assert_pg_alive(pol, rec, adv, ret, opts, what):
    g, _, _ = P.grad(pol, P.flat_params(pol), *_samples(rec, adv, ret), **opts)
    W.assert_terms_alive(g, W.pg_terms(pol), what)
    return g


@pytest.mark.parametrize("name", NAMES)
def test_ppo_two_minibatch_steps_equal_the_restatement(amd, name):
    """all envs, then the inner range (2, 5) whose ratios lie away from 1: theta, m, v and every statistic after each; the
    device's chain-major layers follow theta; the next act on replayed normals runs the new weights"""
    K = W.SHAPES[name]["K"]
    rng = np.random.default_rng(PG_SEED[name])
    pol = _pg_policy(rng, name)
    opts = P.options(ent_coef=0.01, vf_coef=1.0)
    e, rec, adv, ret = _pg_collected(amd, pol, K, opts, PG_SEED[name])
    _assert_pg_alive(pol, rec, adv, ret, opts, name)
    state = _pg_fresh(pol)
    for n0, B in ((0, N), (2, 5)):
        stats = e.pg_minibatch(n0, B)
        state, rstats = P.minibatch(pol, state, rec, adv, ret, n0, B, opts)
        _assert_pg_state(e.pg_state(), state, (n0, B))
        _assert_pg_stats(stats, rstats, (n0, B))
        assert stats["steps"] == state["steps"] and stats["samples"] == T * B
    assert rstats["approx_kl"] != 0.0, "the second step was meant to see ratios away from 1"
    new = P.with_params(pol, state["theta"])
    assert _same(e.mlp_params(), P.flat_params(new)[:e.mlp_param_count()])
    z = rng.standard_normal((N, K + 1)).astype(F)
    obs = R.flat_obs(e.fetch())
    e.mlp_act(BUDGET, replay_normals=z)
    last, ref = e.mlp_last(), R.act(new, obs, z, deterministic=False)
    for k in ("mean", "log_std", "action", "logp", "value"):
        assert _same(last[k], ref[k]), k
    if W.SHAPES[name]["clamp"] is not None:
        moved = (new.log_std < F(new.log_std_clamp[0])) | (new.log_std > F(new.log_std_clamp[1]))
        assert moved.any() and not moved.all(), "the clamp was meant to move some components and not others"
    e.close()


@pytest.mark.parametrize("name", NAMES)
def test_ppo_device_gradient_against_pytorch_autograd(amd, name):
    """One Adam step with beta1 = 0 and no norm clip from fresh moments: m = 0 * 0 + 1 * g, the kernels' gradient itself.  It
    is the restatement's bit for bit, and against float64 autograd on the record the device produced it meets the yardstick of
    tests/test_pg_host.py over the whole vector and in every term: at most twice float32 autograd's own error."""
    import torch
    from tests.test_pg_host import _torch_grad
    K = W.SHAPES[name]["K"]
    pol = _pg_policy(np.random.default_rng(PG_SEED[name]), name)
    opts = P.options(ent_coef=0.01, vf_coef=1.0, beta1=0.0, max_grad_norm=0.0)
    e, rec, adv, ret = _pg_collected(amd, pol, K, opts, PG_SEED[name])
    e.pg_minibatch(0, N)
    g = e.pg_state()["m"]
    e.close()
    batch = _samples(rec, adv, ret)
    theta = P.flat_params(pol)
    rg, _, _ = P.grad(pol, theta, *batch, **opts)
    assert np.array_equal(g, rg)
    W.assert_terms_alive(g, W.pg_terms(pol), name)
    if pol.activation == "relu":
        assert W.relu_margin(batch[0], pol.layers, pol.value_layers) > 1e-6, "a relu pre-activation sits on its kink: choose another seed"
    g64, g32 = _torch_grad(pol, theta, *batch, torch.float64, opts), _torch_grad(pol, theta, *batch, torch.float32, opts)
    W.yardstick(f"{name} PPO device", g, g64, g32, W.pg_terms(pol))


def test_ppo_kl_penalty_at_w1(amd):
    """the KL add-on's instantiation (5 A head floats of LDS, not 3 A): two minibatches of 4 envs at kl_coef = 1, value clip on"""
    name, mb = "W1", 4
    K = W.SHAPES[name]["K"]
    pol = _pg_policy(np.random.default_rng(14), name)
    opts = P.options(lr=1e-3, vf_coef=1.0, ent_coef=0.01, minibatch_envs=mb)
    e, rec, adv, ret = _pg_collected(amd, pol, K, opts, 14)
    dv = (rec["value"] - ret).astype(F)
    kl_opts = KR.kl_options(kl_coef=1.0, adaptive=False, vf_clip=float(F(np.median((dv * dv).astype(np.float64)))))
    e.pg_kl_init(**kl_opts)
    adv, ret = e.pg_advantages(fetch=True)                              # (the add-on's snapshot is taken with the advantages)
    state = _pg_fresh(pol)
    snap = KR.snapshot(pol, state["theta"], rec)
    mean_old, ls_old = e.pg_kl_old_dist()
    assert _same(mean_old, snap[0]) and _same(ls_old, snap[1][None, :])
    fractions = []
    for n0 in (0, mb):
        stats, kst = e.pg_minibatch(n0, mb), e.pg_kl_stats()
        state, rstats, rkst = KR.minibatch(pol, state, rec, adv, ret, snap, n0, mb, opts, kl_opts, 1.0)
        _assert_pg_state(e.pg_state(), state, n0)
        _assert_pg_stats(stats, rstats, n0)
        for k in ("kl", "vf_clip_fraction"):
            assert _same(np.float64(kst[k]), np.float64(rkst[k])), (k, kst[k], rkst[k], n0)
        fractions.append(kst["vf_clip_fraction"])
    assert kst["kl"] > 0.0 and any(0.0 < f < 1.0 for f in fractions)
    e.close()


def test_ppo_shuffled_minibatches_at_w1(amd):
    """the gathered instantiation: one epoch's order, its minibatches of 16, 16 and 8 samples"""
    name, mb, seed = "W1", 16, 15
    K = W.SHAPES[name]["K"]
    pol = _pg_policy(np.random.default_rng(seed), name)
    opts = P.options(lr=1e-3, vf_coef=1.0)
    sh = SR.shuffle_options(minibatch_samples=mb)
    e, rec, adv, ret = _pg_collected(amd, pol, K, opts, seed)
    e.pg_shuffle_init(**sh)
    adv, ret = e.pg_advantages(fetch=True)
    e.pg_shuffle_epoch()
    order, rows = e.pg_shuffle_order()
    ref = SR.order(seed, T * N, 0)                                       # (the configuration's seed 0: the engine's)
    assert _same(order[0], ref) and _same(rows[0], SR.rows(ref, N, N))
    state = _pg_fresh(pol)
    for j, (i0, i1) in enumerate(SR.minibatches(T * N, mb)):
        stats = e.pg_shuffle_minibatch(j)
        state, rstats, _, stopped = SR.minibatch(pol, state, rec, adv, ret, ref[i0:i1].astype(np.int64), opts, sh)
        assert not stopped
        _assert_pg_state(e.pg_state(), state, j)
        _assert_pg_stats(stats, rstats, j)
    assert state["steps"] == 3
    e.close()


def test_ppo_queued_update_at_w1(amd):
    """the queued chain: advantages and two epochs of two minibatches with one host wait"""
    name, seed = "W1", 16
    K = W.SHAPES[name]["K"]
    pol = _pg_policy(np.random.default_rng(seed), name)
    opts = P.options(lr=1e-3, vf_coef=1.0, minibatch_envs=N // 2)
    e, rec, _, _ = _pg_collected(amd, pol, K, opts, seed)
    stats = e.pg_update(2, queued=True)
    state, rstats = P.update(pol, _pg_fresh(pol), rec, rec["bootstrap_value"], 2, opts)
    _assert_pg_state(e.pg_state(), state)
    _assert_pg_stats(stats, rstats)
    assert state["steps"] == 4
    e.close()


def test_ppo_population_of_two_at_w1(amd):
    """two learners with different weights, 4 envs each: ragged widths pad each member's store, and a member's bits are the
    restatement's on its own envs"""
    name, M, seed = "W1", 2, 17
    K, n = W.SHAPES[name]["K"], N // 2
    rng = np.random.default_rng(seed)
    pols = [_pg_policy(rng, name) for _ in range(M)]
    opts = P.options(lr=1e-3, vf_coef=1.0, ent_coef=0.01, minibatch_envs=n // 2)
    e = _engine(amd, K, seed)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    e.mlp_set_learner(1, pols[1])
    for m in range(M):
        assert _same(e.mlp_learner_params(m), P.flat_params(pols[m])), m
    e.rollout_enable(T, obs=True)
    e.pg_pop_init(opts)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch(bootstrap=True)
    stats = e.pg_pop_update(1)
    for m in range(M):
        state, rstats = PP.member_update(pols[m], PP.fresh_state(pols[m]), rec, m, n, 1, opts)
        _assert_pg_state(e.pg_pop_state(m), state, m)
        _assert_pg_stats(stats[m], rstats, m)
        assert _same(e.mlp_learner_params(m), state["theta"]), m
    assert not _same(e.pg_pop_state(0)["theta"], e.pg_pop_state(1)["theta"])
    e.close()


# ======================================================================================================================================
# TD3
# ======================================================================================================================================
def _action_norm(K):
    return np.full(K + 1, 0.25, F), np.full(K + 1, 1.5, F)


def _assert_off_state(keys, got, ref, what=""):
    for k in keys:
        assert _same(got[k], ref[k]), (k, what)
    assert got["updates"] == ref["updates"], what


def _assert_off_stats(keys, got, ref, what=""):
    for k in keys:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


def _assert_buffer(got, ref, what=""):
    for k in ("x", "a", "r", "done", "x2"):
        assert _same(got[k], ref[k]), (k, what)
    assert (got["size"], got["written"], got["capacity"]) == (ref["size"], ref["written"], ref["capacity"]), what


def _current_input(e, pol):
    return T3.current_input(pol, e.fetch(), e.get_episode_state()[0] == 0)


def _td3_collected(amd, name, seed, **over):
    """a TD3 trainer at the shape with 40 transitions collected and stored: (engine, policy, critics, options, ring)"""
    K = W.SHAPES[name]["K"]
    rng = np.random.default_rng(seed)
    pol = _normed(W.td3_policy(rng, name, normalize=True), K)
    crit = W.critics(rng, name)
    opts = T3.options(critic_widths=W.SHAPES[name]["critics"], batch_size=8, capacity=64, seed=seed, policy_delay=1, tau=0.05, gamma=0.9,
                      reward_scale=0.05, target_noise=0.3, target_noise_clip=0.25, **over)
    e = _engine(amd, K, seed)
    e.mlp_init(pol, rng.integers(0, 2 ** 63, N).astype(np.uint64), deterministic=False)
    e.rollout_enable(T, obs=True)
    e.td3_init(**opts)
    e.td3_set_critics(crit, action_norm=_action_norm(K))
    e.run_days("mlp", T, BUDGET)
    assert e.td3_store() == T * N
    ring = T3.Ring(64, 5 * K + 2, K + 1)
    ring.store(e.rollout_fetch(), _current_input(e, pol))
    _assert_buffer(e.td3_buffer(), ring.buffer(), "the ring after the store")
    return e, pol, crit, opts, ring.buffer()


@pytest.mark.parametrize("name", ("W1", "W2"))
def test_td3_store_and_two_updates_equal_the_restatement(amd, name):
    """policy_delay 1: both updates step the actor through critic 1's action inputs and move the targets; the target y through
    y_mean and through everything that follows from it"""
    K, seed = W.SHAPES[name]["K"], TD3_SEED[name]
    e, pol, crit, opts, buf = _td3_collected(amd, name, seed)
    state = T3.fresh_state(pol, crit)
    _assert_off_state(T3.STATE_KEYS, e.td3_state(), state, "theta starts as the device's policy, the targets as copies")
    sh = T3.Shapes(pol, opts)
    ct, at = W.offpolicy_terms(sh)
    for u in range(2):
        if u == 0:
            idx = T3.batch_indices(seed, 0, 40, 8)
            y = T3.target(sh, state["theta_target"], state["psi_target"], _action_norm(K), seed, 0, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
            W.assert_terms_alive(T3.critic_grad(sh, state["psi"], _action_norm(K), buf["x"][idx], buf["a"][idx], y)[0], ct, name)
            W.assert_terms_alive(T3.actor_grad(sh, state["theta"], state["psi"], _action_norm(K), buf["x"][idx])[0], at, name)
        stats = e.td3_update(1)
        state, rstats = T3.update(pol, state, buf, _action_norm(K), seed, opts)
        _assert_off_state(T3.STATE_KEYS, e.td3_state(), state, u)
        _assert_off_stats(T3.STAT_KEYS, stats, rstats, u)
        assert (stats["updates"], stats["actor_steps"], stats["buffer_size"], stats["samples"]) == (u + 1, u + 1, 40, 8)
    assert _same(e.mlp_params(), state["theta"]), "the device's policy layers follow theta"
    assert not _same(state["theta_target"], T3.fresh_state(pol, crit)["theta"])
    e.close()


def test_td3_device_gradients_against_pytorch_autograd_at_w1(amd):
    """beta1 = 0: after the first update m_psi is the critics' gradient and m_theta the actor's (through the stepped critic 1),
    bit for bit the restatement's and under the autograd yardstick of tests/test_td3_host.py"""
    import torch
    from tests.test_td3_host import _torch_grads
    name, seed = "W1", TD3_SEED["W1"]
    K = W.SHAPES[name]["K"]
    e, pol, crit, opts, buf = _td3_collected(amd, name, seed, beta1=0.0)
    e.td3_update(1)
    got = e.td3_state()
    e.close()
    nrm, sh, st0 = _action_norm(K), T3.Shapes(pol, opts), T3.fresh_state(pol, crit)
    idx = T3.batch_indices(seed, 0, 40, 8)
    x, a = buf["x"][idx], buf["a"][idx]
    y = T3.target(sh, st0["theta_target"], st0["psi_target"], nrm, seed, 0, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
    st1, _ = T3.update(pol, st0, buf, nrm, seed, opts)
    assert np.array_equal(got["m_psi"], T3.critic_grad(sh, st0["psi"], nrm, x, a, y)[0])
    assert np.array_equal(got["m_theta"], T3.actor_grad(sh, st0["theta"], st1["psi"], nrm, x)[0])
    ct, at = W.offpolicy_terms(sh)
    gc64, _ = _torch_grads(sh, st0, nrm, x, a, y, torch.float64)
    gc32, _ = _torch_grads(sh, st0, nrm, x, a, y, torch.float32)
    W.yardstick("W1 TD3 critic device", got["m_psi"], gc64, gc32, ct)
    mid = dict(theta=st0["theta"], psi=st1["psi"])
    _, ga64 = _torch_grads(sh, mid, nrm, x, a, y, torch.float64)
    _, ga32 = _torch_grads(sh, mid, nrm, x, a, y, torch.float32)
    W.yardstick("W1 TD3 actor device", got["m_theta"], ga64, ga32, at)


def _random_buffer(rng, K, size, a_scale=0.5, a_shift=0.4):
    D, A = 5 * K + 2, K + 1
    return dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * a_scale + a_shift).astype(F),
                r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))


def test_td3_population_of_two_at_w1(amd):
    """two learners with different actors and critics on loaded rings: a member's two updates are the restatement's under its
    own options and key"""
    name, M, seed = "W1", 2, 23
    K, n = W.SHAPES[name]["K"], N // 2
    rng = np.random.default_rng(seed)
    pols = [_normed(W.td3_policy(rng, name, normalize=True), K) for _ in range(M)]
    crits = [W.critics(rng, name) for _ in range(M)]
    shared = dict(critic_widths=W.SHAPES[name]["critics"], batch_size=8, capacity=32, policy_delay=1)
    opts = [T3.options(**dict(shared, gamma=0.9, tau=0.05, target_noise=0.3, target_noise_clip=0.25, reward_scale=0.5, seed=0)),
            T3.options(**dict(shared, gamma=0.95, tau=0.1, actor_lr=3e-3, critic_lr=3e-3, seed=77, max_grad_norm=0.5))]
    e = _engine(amd, K, seed)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    e.mlp_set_learner(1, pols[1])
    e.rollout_enable(T, obs=True)
    e.td3_pop_init(opts)
    for m in range(M):
        e.td3_pop_set_critics(m, crits[m], action_norm=_action_norm(K) if m == 0 else None)
    bufs = [_random_buffer(rng, K, 20) for _ in range(M)]
    for m in range(M):
        e.td3_pop_buffer_load(m, bufs[m])
    states = [T3.fresh_state(pols[m], crits[m]) for m in range(M)]
    for u in range(2):
        stats = e.td3_pop_update(1)
        for m in range(M):
            states[m], rstats = TP.member_update(pols[m], states[m], bufs[m], _action_norm(K), opts[m], seed)
            _assert_off_state(T3.STATE_KEYS, e.td3_pop_state(m), states[m], (u, m))
            _assert_off_stats(T3.STAT_KEYS, stats[m], rstats, (u, m))
    assert not _same(states[0]["theta"], states[1]["theta"])
    e.close()


# ======================================================================================================================================
# SAC
# ======================================================================================================================================
def _bounds(K):
    """budget in [50, 1500], bids in [0.02, 3 + k / 100]"""
    return np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], 3.0 + np.arange(K) / 100.0]).astype(F)


def _sac_collected(amd, name, seed, **over):
    """a SAC trainer at the shape with 40 transitions collected and stored: (engine, policy, critics, options, ring)"""
    K = W.SHAPES[name]["K"]
    rng = np.random.default_rng(seed)
    pol = _normed(W.sac_policy(rng, name, normalize=True), K)
    crit = W.critics(rng, name)
    opts = S.options(K, critic_widths=W.SHAPES[name]["critics"], batch_size=8, capacity=64, seed=seed, tau=0.05, gamma=0.9, reward_scale=0.01,
                     init_alpha=0.3, alpha_lr=3e-3, actor_lr=1e-3, critic_lr=1e-3, **over)
    e = _engine(amd, K, seed)
    e.mlp_init(pol, rng.integers(0, 2 ** 63, N).astype(np.uint64), deterministic=False)
    e.mlp_set_squash(*_bounds(K))
    e.rollout_enable(T, obs=True)
    e.sac_init(**opts)
    e.sac_set_critics(crit)
    e.run_days("mlp", T, BUDGET)
    assert e.sac_store() == T * N
    ring = T3.Ring(64, 5 * K + 2, K + 1)
    ring.store(e.rollout_fetch(), _current_input(e, pol))
    _assert_buffer(e.sac_buffer(), ring.buffer(), "the ring after the store")
    return e, pol, crit, opts, ring.buffer()


@pytest.mark.parametrize("name", NAMES)
def test_sac_store_and_two_updates_equal_the_restatement(amd, name):
    """state, log_alpha and statistics after each of two updates; the clamp moves some log-stds and not others"""
    K, seed = W.SHAPES[name]["K"], SAC_SEED[name]
    e, pol, crit, opts, buf = _sac_collected(amd, name, seed)
    state = S.fresh_state(pol, crit, opts)
    _assert_off_state(S.STATE_KEYS, e.sac_state(), state, "theta starts as the device's policy, the target critics as copies")
    sh = T3.Shapes(pol, opts)
    ct, at = W.offpolicy_terms(sh)
    idx = T3.batch_indices(seed, 0, 40, 8)
    alpha = S.alpha_of(state["log_alpha"][0])
    y, _ = S.target(sh, pol.log_std_clamp, state["theta"], state["psi_target"], alpha, seed, 0, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
    W.assert_terms_alive(S.critic_grad(sh, state["psi"], buf["x"][idx], buf["a"][idx], y)[0], ct, name)
    W.assert_terms_alive(S.actor_grad(sh, pol.log_std_clamp, state["theta"], state["psi"], alpha, seed, 0, buf["x"][idx], opts)[0], at, name)
    for u in range(2):
        stats = e.sac_update(1)
        state, rstats = S.update(pol, state, buf, seed, opts)
        _assert_off_state(S.STATE_KEYS, e.sac_state(), state, u)
        _assert_off_stats(S.STAT_KEYS, stats, rstats, u)
        assert (stats["updates"], stats["buffer_size"], stats["samples"]) == (u + 1, 40, 8)
    raw = T3.forward(buf["x"], sh.actor(state["theta"]), sh.act)[-1][:, K + 1:]
    lo, hi = pol.log_std_clamp
    assert (raw < lo).any() and (raw > hi).any() and ((raw > lo) & (raw < hi)).any()
    assert _same(e.mlp_params(), state["theta"]), "the device's policy layers follow theta"
    e.close()


def test_sac_device_gradients_against_pytorch_autograd_at_w1(amd):
    """beta1 = 0: after the first update m_psi is the critics' gradient and m_theta the actor's (through the stepped critics),
    bit for bit the restatement's and under the autograd yardstick of tests/test_sac_host.py, its kink checks first"""
    import torch
    from tests.test_sac_host import _torch_grads
    name, seed = "W1", SAC_SEED["W1"]
    e, pol, crit, opts, buf = _sac_collected(amd, name, seed, beta1=0.0)
    e.sac_update(1)
    got = e.sac_state()
    e.close()
    sh, st0, clamp = T3.Shapes(pol, opts), S.fresh_state(pol, crit, opts), pol.log_std_clamp
    alpha = S.alpha_of(st0["log_alpha"][0])
    idx = T3.batch_indices(seed, 0, 40, 8)
    x, u = buf["x"][idx], buf["a"][idx]
    y, _ = S.target(sh, clamp, st0["theta"], st0["psi_target"], alpha, seed, 0, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
    st1, _ = S.update(pol, st0, buf, seed, opts)
    assert np.array_equal(got["m_psi"], S.critic_grad(sh, st0["psi"], x, u, y)[0])
    assert np.array_equal(got["m_theta"], S.actor_grad(sh, clamp, st0["theta"], st1["psi"], alpha, seed, 0, x, opts)[0])
    z = S.noise(seed, S.ST_SAC_PI, 0, 8, sh.A)
    ct, at = W.offpolicy_terms(sh)
    gc64, _ = _torch_grads(sh, st0, clamp, alpha, opts["eps_sq"], x, u, y, z, torch.float64)
    gc32, _ = _torch_grads(sh, st0, clamp, alpha, opts["eps_sq"], x, u, y, z, torch.float32)
    W.yardstick("W1 SAC critic device", got["m_psi"], gc64, gc32, ct)
    mid, checks = dict(theta=st0["theta"], psi=st1["psi"]), {}
    _, ga64 = _torch_grads(sh, mid, clamp, alpha, opts["eps_sq"], x, u, y, z, torch.float64, checks)
    assert checks["dq"] > 1e-6, "two critic values tie: choose another seed"
    raw = checks["raw"]
    assert min(np.abs(raw - float(F(clamp[0]))).min(), np.abs(raw - float(F(clamp[1]))).min()) > 1e-6, "a raw log-std sits on the clamp"
    _, ga32 = _torch_grads(sh, mid, clamp, alpha, opts["eps_sq"], x, u, y, z, torch.float32)
    W.yardstick("W1 SAC actor device", got["m_theta"], ga64, ga32, at)


def test_sac_population_of_two_at_w1(amd):
    """two learners with different actors, critics and temperatures on loaded rings: a member's two updates are the
    restatement's under its own options and key"""
    from tests import sac_pop_ref as SP
    name, M, seed = "W1", 2, 34
    K = W.SHAPES[name]["K"]
    rng = np.random.default_rng(seed)
    pols = [_normed(W.sac_policy(rng, name, normalize=True), K) for _ in range(M)]
    crits = [W.critics(rng, name) for _ in range(M)]
    shared = dict(critic_widths=W.SHAPES[name]["critics"], batch_size=8, capacity=32, target_update_interval=1)
    opts = [S.options(K, **dict(shared, gamma=0.9, tau=0.05, init_alpha=0.3, alpha_lr=3e-3, reward_scale=0.5, seed=0)),
            S.options(K, **dict(shared, gamma=0.95, tau=0.1, init_alpha=0.7, actor_lr=1e-3, critic_lr=1e-3, seed=77, max_grad_norm=0.5))]
    e = _engine(amd, K, seed)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    e.mlp_set_learner(1, pols[1])
    e.mlp_learners_set_squash(*_bounds(K))
    e.rollout_enable(T, obs=True)
    e.sac_pop_init(opts)
    for m in range(M):
        e.sac_pop_set_critics(m, crits[m])
    bufs = [_random_buffer(rng, K, 20, a_scale=1.5, a_shift=0.0) for _ in range(M)]
    for m in range(M):
        e.sac_pop_buffer_load(m, bufs[m])
    states = [SP.member_fresh_state(pols[m], crits[m], opts[m]) for m in range(M)]
    for u in range(2):
        stats = e.sac_pop_update(1)
        for m in range(M):
            states[m], rstats = SP.member_update(pols[m], states[m], bufs[m], opts[m], seed)
            _assert_off_state(S.STATE_KEYS, e.sac_pop_state(m), states[m], (u, m))
            _assert_off_stats(S.STAT_KEYS, stats[m], rstats, (u, m))
    assert not _same(states[0]["theta"], states[1]["theta"])
    e.close()


# ======================================================================================================================================
# one step from the LDS refusal
# ======================================================================================================================================
SAID = dict(
    pg="num_keywords too large for policy-gradient training (LDS)",
    pg_frames="frames: the stacked input row is too large for policy-gradient training (LDS); fewer frames fit",
    pg_kl="num_keywords too large for the KL penalty (LDS)",
    not_initialised="adc_engine_pg_init has not been called (or the policy / the record was re-initialised since)",
)


def _refused(kind, text, call):
    with pytest.raises(kind) as info:
        call()
    assert str(info.value) == text, (str(info.value), text)


@pytest.mark.parametrize("family,frames", [("pg", 1), ("pg_kl", 1), ("pg", 8)], ids=["keywords", "kl-keywords", "frames"])
def test_ppo_trains_at_the_last_k_that_fits_and_refuses_the_next(amd, family, frames):
    """hidden (256, 256, 256) for the policy and the value network, two heads: a sample's workgroup holds 14 K + 1548 floats
    (16 K + 1550 under the KL penalty; 49 K + 1562 with 8 frames).  At the largest K within 16384 floats - the dynamic region
    within a few bytes of 64 KiB, behind k_pg_sample's 8 static bytes - one day of 8 envs is collected and one minibatch of 8
    samples equals the restatement bit for bit; at K + 1 the init is refused in the existing words and the engine goes on"""
    from adcraft_amd import _ffi
    kl = family == "pg_kl"
    K = W.boundary_K(family, frames)
    assert W.widest_count(family, K, frames) <= W.LDS_FLOATS < W.widest_count(family, K + 1, frames)
    assert frames == 1 or W.widest_count(family, K + 1, 1) <= W.LDS_FLOATS     # (one frame of K + 1 fits: the frames are to blame)
    assert not kl or W.widest_count("pg", K + 1) <= W.LDS_FLOATS                # (the trainer itself fits: the add-on's two vectors do not)
    opts = P.options(lr=1e-3, vf_coef=1.0, ent_coef=0.01)
    # the last K that fits
    seed = 41 + frames + kl
    pol = W.widest_policy(np.random.default_rng(seed), K, two=True, value=True, frames=frames, log_std_clamp=(-2.0, -0.5))
    pol.layers[-1][1][K + 1:] += F(-1.25)
    e, rec, adv, ret = _pg_collected(amd, pol, K, opts, seed, days=1)
    assert rec["obs"].shape == (1, N, frames * (5 * K + 2))
    state = _pg_fresh(pol)
    if kl:
        kl_opts = KR.kl_options(kl_coef=1.0, adaptive=False)
        e.pg_kl_init(**kl_opts)
        adv, ret = e.pg_advantages(fetch=True)
        snap = KR.snapshot(pol, state["theta"], rec)
    for step in range(2):                                               # (the second from moved weights: a KL that is not zero)
        stats = e.pg_minibatch(0, N)
        if kl:
            state, rstats, rkst = KR.minibatch(pol, state, rec, adv, ret, snap, 0, N, opts, kl_opts, 1.0)
            assert _same(np.float64(e.pg_kl_stats()["kl"]), np.float64(rkst["kl"])), step
        else:
            state, rstats = P.minibatch(pol, state, rec, adv, ret, 0, N, opts)
        _assert_pg_state(e.pg_state(), state, step)
        _assert_pg_stats(stats, rstats, step)
    assert np.isfinite(state["theta"]).all() and not _same(state["theta"], P.flat_params(pol))
    e.close()
    # one keyword further
    pol = W.widest_policy(np.random.default_rng(seed), K + 1, two=True, value=True, frames=frames)
    e = _engine(amd, K + 1, seed, envs=2)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(1, obs=True)
    if kl:
        e.pg_init()
        _refused(ValueError, SAID["pg_kl"], lambda: e.pg_kl_init())
        e.run_days("mlp", 1, BUDGET)
        assert e.pg_update(1)["steps"] == 1                             # (the trainer goes on without the add-on)
    else:
        _refused(ValueError, SAID["pg_frames" if frames > 1 else "pg"], lambda: e.pg_init())
        _refused(_ffi.EngineStateError, SAID["not_initialised"], lambda: e.pg_state())
        e.run_days("mlp", 1, BUDGET)                                    # (the engine goes on: the policy acts and the day is recorded)
        assert e.rollout_fetch()["reward"].shape == (1, 2)
    e.close()


@pytest.mark.parametrize("family", ["td3", "sac"])
def test_offpolicy_trains_at_the_last_k_that_fits_and_refuses_the_next(amd, family):
    """actor hidden (256, 256, 256), critics (256, 256, 256, 1): TD3 holds 10 K + 1548 floats, SAC (two heads) 20 K + 2331.  At
    the largest K within 16384 floats one update at batch 8 on a loaded ring equals the restatement bit for bit - the
    target, the critics, the actor step and Polyak; at K + 1 the init is refused with the existing "LDS" message and the engine
    goes on"""
    td3 = family == "td3"
    K = W.boundary_K(family)
    assert W.widest_count(family, K) <= W.LDS_FLOATS < W.widest_count(family, K + 1)
    seed, widths = 51 + td3, W.WIDEST["critics"]
    rng = np.random.default_rng(seed)
    if td3:
        pol = W.widest_policy(rng, K, two=False, value=False)
        opts = T3.options(critic_widths=widths, batch_size=8, capacity=16, seed=seed, policy_delay=1, tau=0.05, gamma=0.9, reward_scale=0.5)
    else:
        pol = W.widest_policy(rng, K, two=True, value=False, log_std_clamp=(-1.0, -0.5))
        pol.layers[-1][1][K + 1:] = np.linspace(-1.6, 0.1, K + 1).astype(F)
        opts = S.options(K, critic_widths=widths, batch_size=8, capacity=16, seed=seed, tau=0.05, gamma=0.9, reward_scale=0.5, init_alpha=0.3,
                         alpha_lr=3e-3)
    crit = T3.random_critics_for_tests(rng, K, widths)
    buf = _random_buffer(rng, K, 12, *((0.5, 0.4) if td3 else (1.5, 0.0)))
    e = _engine(amd, K, seed, envs=2)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(1, obs=True)
    if td3:
        e.td3_init(**opts)
        e.td3_set_critics(crit, action_norm=_action_norm(K))
        e.td3_buffer_load(buf)
        stats = e.td3_update(1)
        state, rstats = T3.update(pol, T3.fresh_state(pol, crit), buf, _action_norm(K), seed, opts)
        _assert_off_state(T3.STATE_KEYS, e.td3_state(), state)
        _assert_off_stats(T3.STAT_KEYS, stats, rstats)
        assert state["actor_steps"] == 1
    else:
        e.mlp_set_squash(*_bounds(K))
        e.sac_init(**opts)
        e.sac_set_critics(crit)
        e.sac_buffer_load(buf)
        stats = e.sac_update(1)
        state, rstats = S.update(pol, S.fresh_state(pol, crit, opts), buf, seed, opts)
        _assert_off_state(S.STATE_KEYS, e.sac_state(), state)
        _assert_off_stats(S.STAT_KEYS, stats, rstats)
    assert np.isfinite(state["theta"]).all() and np.isfinite(state["psi"]).all()
    e.close()
    # one keyword further
    pol = W.widest_policy(np.random.default_rng(seed), K + 1, two=not td3, value=False, **({} if td3 else dict(log_std_clamp=(-1.0, -0.5))))
    e = _engine(amd, K + 1, seed, envs=2)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(1, obs=True)
    if not td3:
        e.mlp_set_squash(*_bounds(K + 1))
    with pytest.raises(ValueError, match="LDS"):
        (e.td3_init if td3 else e.sac_init)(critic_widths=widths, batch_size=8, capacity=16)
    e.run_days("mlp", 1, BUDGET)
    assert e.rollout_fetch()["reward"].shape == (1, 2)
    e.close()
