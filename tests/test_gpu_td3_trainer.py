"""GPU tests of off-policy (TD3) training on the device (parts/kernel_td3.inc, parts/td3_api.inc) against the numpy restatement
tests/td3_ref.py, bit for bit: the replay ring through auto-resets and a wrap, updates with the delayed actor and target
steps, full trainer iterations, independence of the launch shape, a resumed state, that nothing else moved, every refusal, and
a learning run.  None of these symbols exists before this feature: every test here fails on the parent commit."""
import ctypes as C
import signal
import time

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
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


def _policy(rng, K, hidden=(16, 8), act="tanh", **kw):
    pol = R.random_policy(rng, K, hidden, act, normalize=True, scale=0.6, **kw)
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _action_norm(K):
    return np.full(K + 1, 0.25, F), np.full(K + 1, 1.5, F)


def _trainer(amd, pol, critics, N, K, T, opts, agent_seeds, norm=None, seed=41, **engine_kw):
    e = _engine(amd, N, K, seed=seed, **engine_kw)
    e.mlp_init(pol, agent_seeds, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.td3_init(**opts)
    e.td3_set_critics(critics, action_norm=norm)
    return e


def _assert_state(got, ref, what=""):
    for k in T3.STATE_KEYS:
        assert _same(got[k], ref[k]), (k, what)
    assert (got["updates"], got["actor_steps"]) == (ref["updates"], ref["actor_steps"]), what


def _assert_stats(got, ref, what=""):
    for k in T3.STAT_KEYS:
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


def test_store_through_auto_resets_and_a_wrap(amd):
    """three collect-and-store rounds of 84 transitions into a ring of 200: it wraps once; stored at once or day by day, the
    ring is the restatement's built from the fetched record plus the current input row"""
    rng = np.random.default_rng(11)
    pol = _policy(rng, K0, value=True)                              # (a value network is ignored by TD3; rollout_fetch's bootstrap needs one)
    crit = T3.random_critics_for_tests(rng, K0, (12, 1))
    seeds = rng.integers(0, 2 ** 63, N0).astype(np.uint64)
    opts = T3.options(critic_widths=(12, 1), batch_size=8, capacity=200)
    a = _trainer(amd, pol, crit, N0, K0, T0, opts, seeds, **RESETS)
    b = _trainer(amd, pol, crit, N0, K0, T0, opts, seeds, **RESETS)
    ring = T3.Ring(200, 5 * K0 + 2, K0 + 1)
    assert a.td3_buffer()["size"] == 0
    for rnd in range(3):
        a.rollout_reset()
        a.run_days("mlp", T0, 1000.0)
        assert a.td3_store() == T0 * N0
        rec = a.rollout_fetch(bootstrap=True)
        ring.store(rec, _current_input(a, pol))
        _assert_buffer(a.td3_buffer(), ring.buffer(), rnd)
        b.rollout_reset()
        for _ in range(T0):
            b.run_days("mlp", 1, 1000.0)
            assert b.td3_store() == N0
        _assert_buffer(b.td3_buffer(), ring.buffer(), ("day by day", rnd))
    buf = a.td3_buffer()
    assert buf["size"] == 200 and buf["written"] == 3 * T0 * N0 and buf["done"].any() and not buf["done"].all()
    # after an auto-reset the next input is the zero row, normalised
    zero_row = T3.current_input(pol, {k: np.zeros_like(v) for k, v in a.fetch().items()}, np.ones(N0, bool))[0]
    assert all(_same(row, zero_row) for row in buf["x2"][buf["done"]])
    # half a record, then the rest: the days not yet stored, and no more
    a.rollout_reset()
    a.run_days("mlp", 3, 1000.0)
    assert a.td3_store() == 3 * N0
    a.run_days("mlp", 2, 1000.0)
    assert a.td3_store() == 2 * N0
    rec = a.rollout_fetch()
    ring.store(rec, _current_input(a, pol))
    _assert_buffer(a.td3_buffer(), ring.buffer(), "in two parts")
    a.close()
    b.close()


def _random_buffer(rng, K, size):
    D, A = 5 * K + 2, K + 1
    buf = dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * 0.5 + 0.4).astype(F),
               r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))
    return buf


UPDATE_CASES = [
    dict(act="tanh", widths=(12, 1), norm=True, opts=dict(seed=123, max_grad_norm=0.5)),
    dict(act="relu", widths=(7, 33, 5, 1), norm=False, opts=dict(action_lo=0.05, action_hi=0.9, optimiser="sgd", actor_lr=0.01, critic_lr=0.01)),
    dict(act="tanh", widths=(1,), norm=True, opts=dict(seed=5)),
    dict(act="relu", widths=(12, 1), norm=True, batch=1100, opts=dict(seed=77)),
]


@pytest.mark.parametrize("case", UPDATE_CASES, ids=["tanh-12", "relu-7-33-5-clamp-sgd", "no-hidden", "batch-1100"])
def test_three_updates_equal_the_restatement(amd, case):
    """policy_delay 2 on a loaded ring of 84 rows: update 2 steps the actor and moves the targets, updates 1 and 3 do not; state
    and statistics after each; the batch indices are the host twin's; the next act runs the new actor.  seed 0 (the second
    case) takes the engine's seed"""
    from adcraft_amd import _ffi
    rng = np.random.default_rng(21)
    B = case.get("batch", 16)
    pol = _policy(rng, K0, act=case["act"])
    crit = T3.random_critics_for_tests(rng, K0, case["widths"])
    norm = _action_norm(K0) if case["norm"] else None
    opts = T3.options(critic_widths=case["widths"], batch_size=B, capacity=100, tau=0.05, target_noise=0.3, target_noise_clip=0.25, gamma=0.9,
                      reward_scale=0.5, **case["opts"])
    seed = opts["seed"] or 41
    e = _trainer(amd, pol, crit, N0, K0, T0, opts, None, norm=norm, **NO_RESETS)
    state = T3.fresh_state(pol, crit)
    _assert_state(e.td3_state(), state, "theta starts as the device's policy, the targets as copies")
    assert e.td3_param_counts() == (state["theta"].size, state["psi"].size)
    buf = _random_buffer(rng, K0, 84)
    e.td3_buffer_load(buf)
    _assert_buffer(e.td3_buffer(), dict(buf, size=84, written=84, capacity=100))
    for u in range(3):
        idx = e.td3_batch_indices(u)
        assert _same(idx, T3.twin_batch_indices(_ffi.lib(), seed, u, 84, B)) and idx.min() >= 0 and idx.max() < 84
        before = e.td3_state()
        stats = e.td3_update(1)
        state, rstats = T3.update(pol, state, buf, norm, seed, opts)
        after = e.td3_state()
        _assert_state(after, state, u)
        _assert_stats(stats, rstats, u)
        assert (stats["updates"], stats["actor_steps"], stats["buffer_size"], stats["samples"]) == (u + 1, (u + 1) // 2, 84, B)
        moved = not _same(before["theta"], after["theta"])
        assert moved == (u == 1) and (not _same(before["theta_target"], after["theta_target"])) == (u == 1)
        assert (not _same(before["psi_target"], after["psi_target"])) == (u == 1) and not _same(before["psi"], after["psi"])
    if B > 84:
        assert len(set(idx.tolist())) < B
    # the next act uses the new actor
    new = R.random_policy(rng, K0, (16, 8), case["act"])
    new.layers, new.log_std, new.shift, new.scale = T3.Shapes(pol, opts).actor(state["theta"]), pol.log_std, pol.shift, pol.scale
    assert _same(e.mlp_params(), state["theta"])
    z = rng.standard_normal((N0, K0 + 1)).astype(F)
    obs = R.flat_obs(e.fetch())
    obs[:] = 0                                                         # (no day stepped since the reset: the first day's zero row)
    e.mlp_act(1000.0, replay_normals=z)
    last, ref = e.mlp_last(), R.act(new, obs, z, deterministic=False)
    for k in ("mean", "log_std", "action", "logp"):
        assert _same(last[k], ref[k]), k
    e.close()


def _loop(amd, pol, crit, N, K, T, opts, iterations, seeds, updates=3, check=False, resume_from=None, **engine_kw):
    """TD3Trainer iterations; returns (the state after each iteration, the ring after each, env groups of the last day)"""
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    e = _engine(amd, N, K, seed=41, **engine_kw)
    cfg = {k: v for k, v in opts.items() if k != "critic_widths"}
    tr = TD3Trainer(e, pol, critic_hidden=opts["critic_widths"][:-1], horizon=T, exploration_sigma=0.2, learning_starts=T * N, updates_per_iteration=updates,
                    agent_seeds=seeds, critics=crit, action_norm=_action_norm(K), **cfg)
    tpl = tr._template
    state, ring, out = T3.fresh_state(tpl, crit), T3.Ring(opts["capacity"], 5 * K + 2, K + 1), []
    groups = 0
    for it in range(iterations):
        stats = tr.iteration(T, 1000.0)
        groups = e.env_groups()
        if check:
            ring.store(e.rollout_fetch(), _current_input(e, tpl))
            _assert_buffer(e.td3_buffer(), ring.buffer(), it)
            actor = dict(actor_loss=-np.float64(0.0), actor_grad_norm=np.float64(0.0))
            for _ in range(updates):
                steps = state["actor_steps"]
                state, rstats = T3.update(tpl, state, ring.buffer(), _action_norm(K), opts["seed"], opts)
                if state["actor_steps"] > steps:                      # (a call reports its last actor step's loss and norm)
                    actor = {k: rstats[k] for k in actor}
            rstats.update(actor)
            _assert_state(tr.state(), state, it)
            _assert_stats(stats, rstats, it)
            assert _same(e.mlp_params(), state["theta"]) and _same(T3.flat_of(tr.policy().layers), state["theta"])
        out.append((tr.state(), e.td3_buffer()))
    e.close()
    return out, groups


def test_three_trainer_iterations_equal_the_restatement(amd):
    """collect through auto-resets under the exploration noise, store, three updates (one actor step among them), three times
    over; the ring of 200 wraps in the third iteration"""
    N, K, T = 12, 9, 7
    rng = np.random.default_rng(31)
    pol = _policy(rng, K, (12, 12))
    crit = T3.random_critics_for_tests(rng, K, (12, 7, 1))
    opts = T3.options(critic_widths=(12, 7, 1), batch_size=16, capacity=200, seed=9, tau=0.05, reward_scale=0.5, actor_lr=3e-3, critic_lr=3e-3)
    out, _ = _loop(amd, pol, crit, N, K, T, opts, 3, rng.integers(0, 2 ** 63, N).astype(np.uint64), check=True, **RESETS)
    assert out[-1][0]["updates"] == 9 and out[-1][0]["actor_steps"] == 4 and out[-1][1]["written"] == 252
    assert not _same(out[0][0]["theta"], out[-1][0]["theta"])


def test_env_groups_and_twin_engines_give_the_same_bits(amd, monkeypatch):
    N, K, T = 16, 24, 4
    rng = np.random.default_rng(41)
    pol = _policy(rng, K, (16, 16))
    crit = T3.random_critics_for_tests(rng, K, (16, 1))
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = T3.options(critic_widths=(16, 1), batch_size=32, capacity=150, seed=9, actor_lr=3e-3, critic_lr=3e-3)
    runs = []
    for groups in (1, 2, 4, 1):                                     # (the second run of 1: another engine from the same seeds)
        monkeypatch.setenv("ADCRAFT_STREAM_GROUPS", str(groups))
        runs.append(_loop(amd, pol, crit, N, K, T, opts, 3, seeds, **RESETS))
        assert runs[-1][1] == groups, "the forced env groups did not engage"
    for out, _ in runs[1:]:
        for (sa, ba), (sb, bb) in zip(runs[0][0], out):
            _assert_state(sa, sb)
            _assert_buffer(ba, bb)


def test_a_resumed_state_and_ring_continue_to_the_same_bits(amd):
    """state plus ring saved after iteration 1, loaded into a fresh engine (stepped to the same env position), reaches iteration
    3's state and ring exactly"""
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    N, K, T = 8, 8, 4
    rng = np.random.default_rng(51)
    pol = _policy(rng, K, (12,))
    crit = T3.random_critics_for_tests(rng, K, (12, 1))
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = T3.options(critic_widths=(12, 1), batch_size=16, capacity=80, seed=9, actor_lr=3e-3, critic_lr=3e-3)
    full, _ = _loop(amd, pol, crit, N, K, T, opts, 3, seeds, **NO_RESETS)
    saved_state, saved_ring = full[0]
    e = _engine(amd, N, K, seed=41, **NO_RESETS)
    cfg = {k: v for k, v in opts.items() if k != "critic_widths"}
    tr = TD3Trainer(e, pol, critic_hidden=(12,), horizon=T, exploration_sigma=0.2, learning_starts=T * N, updates_per_iteration=3, agent_seeds=seeds,
                    critics=T3.random_critics_for_tests(rng, K, (12, 1)), action_norm=_action_norm(K), **cfg)
    e.run_days("mlp", T, 1000.0)                                    # (the env's and agents' streams, as after iteration 1; not stored)
    tr.state(saved_state)
    e.td3_buffer_load(saved_ring)
    _assert_state(tr.state(), saved_state)
    _assert_buffer(e.td3_buffer(), saved_ring)
    assert _same(e.mlp_params(), saved_state["theta"])
    for it in (1, 2):
        tr.iteration(T, 1000.0)
        _assert_state(tr.state(), full[it][0], it)
        _assert_buffer(e.td3_buffer(), full[it][1], it)
    e.close()


STEP_FIELDS = ("impressions", "buyside_clicks", "sellside_conversions", "cost", "revenue", "reward", "cumulative_profit", "days_passed",
               "terminated", "truncated")


def test_nothing_else_moved(amd):
    N, K, T = 12, 10, 4
    rng = np.random.default_rng(61)
    pol = _policy(rng, K)
    crit = T3.random_critics_for_tests(rng, K, (8, 1))
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    opts = T3.options(critic_widths=(8, 1), batch_size=16, capacity=500, actor_lr=3e-3, critic_lr=3e-3)
    # after td3_init (and stores) and before any update a day is what it is without it
    runs = []
    for with_td3 in (False, True):
        e = _engine(amd, N, K, seed=41, **RESETS)
        e.mlp_init(pol, seeds, deterministic=False)
        e.rollout_enable(T, obs=True)
        if with_td3:
            e.td3_init(**opts)
            e.td3_set_critics(crit)
        e.run_days("mlp", T, 1000.0)
        if with_td3:
            e.td3_store()
        runs.append((e.fetch(), e.rollout_fetch(bootstrap=False), e.mlp_last(), e.get_rng_state()))
        e.close()
    (o0, r0, l0, s0), (o1, r1, l1, s1) = runs
    for k in STEP_FIELDS:
        assert _same(o0[k], o1[k]), k
    for k in r0:
        assert _same(r0[k], r1[k]), k
    for k in l0:
        assert _same(l0[k], l1[k]), k
    assert _same(s0[0], s1[0]) and _same(s0[1], s1[1])
    # training draws from its own key alone: with updates in between, the envs' streams and the agents' sit where they sit without
    ends = []
    for updates in (False, True):
        e = _trainer(amd, pol, crit, N, K, T, opts, seeds, **NO_RESETS)
        for _ in range(2):
            e.rollout_reset()
            e.run_days("mlp", T, 1000.0)
            e.td3_store()
            if updates:
                e.td3_update(4)
        e.mlp_act(1000.0)
        last = e.mlp_last()
        ends.append((e.get_rng_state(), (last["action"] - last["mean"]) / np.exp(last["log_std"]), e.mlp_agent_state(), e.td3_state()["theta"]))
        e.close()
    (sa, za, aa, ta), (sb, zb, ab, tb) = ends
    assert _same(sa[0], sb[0]) and _same(sa[1], sb[1])
    assert _same(aa[0], ab[0]) and _same(aa[1], ab[1]) and np.all(aa[1] == 2 * T + 1)
    assert np.abs(za - zb).max() < 1e-3 and np.abs(za).max() > 0.5 and not _same(ta, tb)


def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd import _ffi
    N, K, T = 8, 6, 3
    rng = np.random.default_rng(71)
    pol = _policy(rng, K, (8,))
    crit = T3.random_critics_for_tests(rng, K, (8, 1))
    base = dict(critic_widths=(8, 1), batch_size=8, capacity=40)
    e = _engine(amd, N, K, seed=81, **NO_RESETS)
    calls = (lambda: e.td3_store(), lambda: e.td3_update(1), lambda: e.td3_state(), lambda: e.td3_buffer(), lambda: e.td3_batch_indices(0),
             lambda: e.td3_set_critics(crit), lambda: e.td3_param_counts(), lambda: e.td3_sync_targets())
    # before mlp_init; a two-headed policy; without a record; without the recorded input
    with pytest.raises(_ffi.EngineStateError, match="mlp_init"):
        e.td3_init(**base)
    e.mlp_init(R.random_policy(rng, K, (8,), two_heads=True), deterministic=False)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="two-headed"):
        e.td3_init(**base)
    e.mlp_init(pol, deterministic=False)
    with pytest.raises(_ffi.EngineStateError, match="rollout record"):
        e.td3_init(**base)
    e.rollout_enable(T)
    with pytest.raises(_ffi.EngineStateError, match="ADC_ROLLOUT_OBS"):
        e.td3_init(**base)
    for call in calls:
        with pytest.raises(_ffi.EngineStateError, match="td3_init"):
            call()
    e.rollout_enable(T, obs=True)
    # bad configurations (the Python surface checks them first; the C entry point does too)
    for bad in (dict(gamma=2.0), dict(tau=0.0), dict(tau=1.5), dict(policy_delay=0), dict(target_noise=-1.0), dict(actor_lr=-1.0), dict(critic_lr=-1.0),
                dict(reward_scale=0.0), dict(reward_scale=float("inf")), dict(batch_size=0), dict(capacity=0), dict(critic_widths=(8, 2)),
                dict(critic_widths=(300, 1))):
        with pytest.raises(ValueError):
            e.td3_init(**dict(base, **bad))
    cfg = amd.StepEngine.td3_config(**base)
    cfg.tau = 0.0
    assert e._lib.adc_engine_td3_init(e._h, C.byref(cfg)) == _ffi.ADC_EINVAL
    with pytest.raises(_ffi.EngineStateError, match="td3_init"):
        e.td3_state()                                              # (the refused td3_init left no trainer)
    # a population; a policy-gradient trainer alive, and the reverse
    e.mlp_population(2)
    with pytest.raises(_ffi.EngineStateError, match="population"):
        e.td3_init(**base)
    e.mlp_population(0)
    e.pg_init()
    with pytest.raises(_ffi.EngineStateError, match="policy-gradient"):
        e.td3_init(**base)
    e.rollout_enable(T, obs=True)                                  # (ends the policy-gradient trainer)
    e.td3_init(**base)
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.pg_init()
    # an update before the critics are uploaded, with an empty ring; a store with no unstored day
    with pytest.raises(_ffi.EngineStateError, match="critic layer"):
        e.td3_update(1)
    e.td3_set_critics(crit)
    for call in (lambda: e.td3_update(1), lambda: e.td3_batch_indices(0)):
        with pytest.raises(_ffi.EngineStateError, match="empty"):
            call()
    with pytest.raises(_ffi.EngineStateError, match="no unstored day"):
        e.td3_store()
    with pytest.raises(ValueError):
        e.td3_set_critics([crit[0]])
    for critic, layer in ((2, 0), (0, 2), (-1, 0)):
        w, b = crit[0][0]
        assert e._lib.adc_engine_td3_set_critic_layer(e._h, critic, layer, w.ctypes.data, b.ctypes.data) == _ffi.ADC_EINVAL
    # the envs stepped, or reset, outside the record since the last recorded day
    e.run_days("mlp", 1, 1000.0)
    e.run_days("fixed", 1, 1000.0)
    with pytest.raises(_ffi.EngineStateError, match="outside the record"):
        e.td3_store()
    e.rollout_reset()
    e.run_days("mlp", 1, 1000.0)
    e.reset()
    with pytest.raises(_ffi.EngineStateError, match="outside the record"):
        e.td3_store()
    e.rollout_reset()
    e.run_days("mlp", 1, 1000.0)
    e.run_days("fixed", 1, 1000.0)
    e.run_days("mlp", 1, 1000.0)                                   # (the second recorded day does not follow the first)
    with pytest.raises(_ffi.EngineStateError, match="outside the record"):
        e.td3_store()
    e.rollout_reset()
    e.run_days("mlp", 2, 1000.0)
    assert e.td3_store() == 2 * N
    # bad updates counts, fetch and load ranges, bad state
    for n in (0, -1):
        with pytest.raises(ValueError):
            e.td3_update(n)
    D, A = 5 * K + 2, K + 1
    x, a, r, dn = np.zeros((4, D), F), np.zeros((4, A), F), np.zeros(4, F), np.zeros(4, np.uint8)
    for slot, count in ((-1, 2), (0, 0), (15, 2), (16, 1)):
        assert e._lib.adc_engine_td3_buffer_fetch(e._h, slot, count, x.ctypes.data, a.ctypes.data, r.ctypes.data, dn.ctypes.data, x.ctypes.data) == _ffi.ADC_EINVAL
    for slot, count, written in ((-1, 2, 10), (0, 0, 10), (38, 4, 50), (0, 4, 3)):
        assert e._lib.adc_engine_td3_buffer_load(e._h, slot, count, x.ctypes.data, a.ctypes.data, r.ctypes.data, dn.ctypes.data, x.ctypes.data,
                                                 written) == _ffi.ADC_EINVAL
    with pytest.raises(ValueError):
        e.td3_buffer_load(dict(x=x, a=a[:, :-1], r=r, done=dn, x2=x))
    assert e.td3_buffer(fetch=False) == dict(size=2 * N, written=2 * N, capacity=40)
    assert e.td3_update(2)["updates"] == 2
    st = e.td3_state()
    for bad in (dict(theta=st["theta"][:-1]), dict(psi=st["psi"][:-1]), dict(m_psi=st["theta"]), dict(updates=-1), dict(actor_steps=5)):
        with pytest.raises(ValueError):
            e.td3_state(dict(st, **bad))
    e.td3_state(st)
    # a population while the trainer exists
    e.mlp_population(2)
    for call in (lambda: e.td3_update(1), lambda: e.td3_store()):
        with pytest.raises(_ffi.EngineStateError, match="population"):
            call()
    e.mlp_population(0)
    assert e.td3_update(1)["updates"] == 3
    # the trainer survives neither a new record nor a re-initialisation of the policy
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="td3_init"):
        e.td3_update(1)
    e.td3_init(**base)
    e.mlp_init(pol, deterministic=False)
    with pytest.raises(_ffi.EngineStateError, match="td3_init"):
        e.td3_state()
    e.rollout_enable(T, obs=True)
    e.td3_init(**base)
    e.td3_set_critics(crit)
    e.run_days("mlp", T, 1000.0)
    assert e.td3_store() == T * N
    assert e.td3_update(2)["updates"] == 2
    e.close()
    # a sharded engine
    s = amd.ShardedStepEngine(N, K, shards=2, seed=5)
    with pytest.raises(NotImplementedError, match="engine_shards=1"):
        s.td3_init()
    s.close()


# the small shape of the issue, and what this trainer was given on it (chosen on the training planes: profiles/pr_td3_trainer.txt)
LEARN = dict(N=256, K=25, days=10, budget=100000.0, mean_volume=8.0, hidden=(32, 32), iterations=60,
             config=dict(critic_hidden=(64, 64), exploration_sigma=0.1, learning_starts=2560, updates_per_iteration=100, gamma=0.9, tau=0.01,
                         policy_delay=2, target_noise=0.05, target_noise_clip=0.1, batch_size=256, capacity=100000, actor_lr=1e-5, critic_lr=1e-3,
                         reward_scale=0.1, action_lo=0.01, action_hi=3.0, seed=7, critic_seed=1))


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


def learning_run(amd, log=print, held_out=True, **over):
    """train at the small shape; returns (curve of the mean recorded episode return, paired differences of held-out returns)"""
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    c = dict(LEARN, **over)
    N, K, days = c["N"], c["K"], c["days"]
    rng = np.random.default_rng(2024)
    pol0 = default_policy(K, hidden=c["hidden"], days=days, seed=0)
    e = amd.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=c["mean_volume"]))
    e.reset()
    tr = TD3Trainer(e, pol0, horizon=days, action_norm=(np.full(K + 1, 0.5, F), np.full(K + 1, 2.0, F)), **c["config"])
    curve = []
    for it in range(c["iterations"]):
        s = tr.iteration(days, c["budget"], reset=True, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        curve.append(float(e.rollout_fetch()["reward"].astype(np.float64).sum(axis=0).mean()))
        if s.get("updates"):
            log(f"iteration {it + 1:3d}  episode return {curve[-1]:10.3f}  critic loss {s['critic_loss']:10.4f}  Q1 {s['q1_mean']:8.3f}  y {s['y_mean']:8.3f}  "
                f"actor loss {s['actor_loss']:8.3f}  |g critic| {s['critic_grad_norm']:8.4f}  |g actor| {s['actor_grad_norm']:8.5f}")
        else:
            log(f"iteration {it + 1:3d}  episode return {curve[-1]:10.3f}  (collecting: {s['buffer_size']} transitions)")
    polT = tr.policy()
    e.close()
    if not held_out:
        return curve, None
    held_planes = synthetic.implicit_keyword_planes(N, K, seed=999, mean_volume=c["mean_volume"])      # other keyword sets, other streams
    held_seeds = np.random.default_rng(4048).integers(0, 2 ** 63, N).astype(np.uint64)
    r0 = episode_returns(amd, pol0, held_planes, held_seeds, days, c["budget"])
    rT = episode_returns(amd, polT, held_planes, held_seeds, days, c["budget"])
    d = rT - r0
    log(f"held-out episode return: untrained {r0.mean():.3f}  trained {rT.mean():.3f}  paired difference {d.mean():.3f} "
        f"+- {d.std(ddof=1) / np.sqrt(d.size):.3f} (standard error, {d.size} envs)")
    return curve, d


def test_it_learns(amd):
    """TD3 at the small shape (256 envs x 25 sparse keywords, 10-day episodes) from default_policy, collected under exploration
    noise 0.1: on held-out keyword sets and seeds, evaluated deterministically, the trained policy's episode return exceeds the
    untrained one's by more than three standard errors of the paired difference.  The hyperparameters are LEARN's, chosen by the
    training planes' curves alone (the actor's learning rate decides: at 1e-3, Fujimoto et al.'s, the actor outruns the critics
    and the return falls; at 1e-5 it rises steadily); the held-out set was looked at twice in all: for the first configuration kept
    (actor 1e-3: -76.3 +- 3.0, a failure) and for this one (+43.0 +- 1.9, 22.8 standard errors).  Every
    configuration tried, its curve, the measured margin and the run time: profiles/pr_td3_trainer.txt."""
    t0 = time.perf_counter()
    curve, d = learning_run(amd)
    print(f"learning run: {time.perf_counter() - t0:.1f} s")
    assert np.isfinite(curve).all()
    se = d.std(ddof=1) / np.sqrt(d.size)
    assert d.mean() > 3.0 * se, (d.mean(), se)


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
    opts = T3.options(critic_widths=(8, 1), batch_size=4, capacity=8, seed=9, actor_lr=3e-3, critic_lr=3e-3)
    fresh = lambda: _trainer(amd, pol, crit, N, K, T, opts, seeds, norm=_action_norm(K), **NO_RESETS)
    a = fresh()
    a.run_days("mlp", T, 1000.0)
    assert a.td3_store() == 12
    a.td3_update(1)
    state, ring = a.td3_state(), a.td3_buffer()
    assert (ring["size"], ring["written"], ring["capacity"]) == (8, 12, 8)
    b = fresh()
    part = lambda lo, hi: {k: ring[k][lo:hi] for k in ("x", "a", "r", "done", "x2")}
    b.td3_buffer_load(part(0, 3))
    assert b.td3_buffer(fetch=False) == dict(size=3, written=3, capacity=8)
    b.td3_buffer_load(part(3, 8), slot=3, written=12)
    b.td3_state(state)
    _assert_buffer(b.td3_buffer(), ring)
    _assert_state(b.td3_state(), state)
    assert b.td3_param_counts() == a.td3_param_counts()
    assert _same(a.td3_batch_indices(1), b.td3_batch_indices(1)) and a.td3_batch_indices(1).shape == (4,)
    _assert_stats(b.td3_update(2), a.td3_update(2))
    _assert_state(b.td3_state(), a.td3_state())
    assert b.td3_state()["updates"] == 3
    a.close()
    lib, h, p = b._lib, b._h, lambda v: v.ctypes.data
    x, ac, r, dn = np.zeros((4, 5 * K + 2), F), np.zeros((4, K + 1), F), np.zeros(4, F), np.zeros(4, np.uint8)
    (w, bias), idx = crit[0][0], np.zeros(4, np.int32)
    last = b.td3_state()
    vec = [p(last[k]) for k in amd.StepEngine.TD3_STATE]
    refused = (
        (r"slot range is not inside \[0, size\)", lambda: lib.adc_engine_td3_buffer_fetch(h, 7, 2, p(x), p(ac), p(r), p(dn), p(x))),
        (r"x, a, r, done or x2 is NULL", lambda: lib.adc_engine_td3_buffer_load(h, 0, 4, p(x), None, p(r), p(dn), p(x), 4)),
        (r"slot range is not inside \[0, capacity\)", lambda: lib.adc_engine_td3_buffer_load(h, 6, 4, p(x), p(ac), p(r), p(dn), p(x), 12)),
        (r"written: at least slot \+ count", lambda: lib.adc_engine_td3_buffer_load(h, 0, 4, p(x), p(ac), p(r), p(dn), p(x), 3)),
        (r"critic: 0 or 1", lambda: lib.adc_engine_td3_set_critic_layer(h, 2, 0, p(w), p(bias))),
        (r"no such critic layer", lambda: lib.adc_engine_td3_set_critic_layer(h, 0, 2, p(w), p(bias))),
        (r"weights or bias is NULL", lambda: lib.adc_engine_td3_set_critic_layer(h, 0, 0, p(w), None)),
        (r"idx_b is NULL", lambda: lib.adc_engine_td3_batch_indices(h, 0, None)),
        (r"update: 0 to 2\^32 - 2", lambda: lib.adc_engine_td3_batch_indices(h, -1, p(idx))),
        (r"updates: 1 to 65536", lambda: lib.adc_engine_td3_update(h, 0, None)),
        (r"a state vector is NULL", lambda: lib.adc_engine_td3_state_set(h, *vec[:-1], None, 0, 0)),
        (r"updates: 0 to 2\^31 - 2", lambda: lib.adc_engine_td3_state_set(h, *vec, 2 ** 31 - 1, 0)),
    )
    for words, call in refused:
        with pytest.raises(ValueError, match=words):
            _ffi.check(call())
    _assert_buffer(b.td3_buffer(), ring)
    _assert_state(b.td3_state(), last)
    assert b.td3_update(1)["updates"] == 4
    assert not _same(b.td3_state()["psi_target"], b.td3_state()["psi"])
    b.td3_sync_targets()
    synced = b.td3_state()
    assert _same(synced["psi_target"], synced["psi"])
    assert _same(synced["theta_target"], synced["theta"])
    b.replay_prio_init()
    with pytest.raises(_ffi.EngineStateError, match="prioritised replay is alive"):
        b.td3_batch_indices(0)
    b.close()
