"""GPU tests of the bounded act and bounded TD3 (k_mlp_policy's kBounded forms, k_teach_record_bounded, the kBounded forms of the TD3
target and actor bodies, parts/td3_bounded_api.inc) against the numpy restatement tests/td3_bounded_ref.py, bit for bit: the act
in its three modes, store and updates, a population against solo engines, a composed trainer and its resumed state, the box
invariant, teacher days, the warm-up's switch, and every refusal by its message.  None of these symbols exists before this
feature: every test here fails on the parent commit."""
import copy
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import stack_ref as S
from tests import td3_bounded_ref as BR
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F = np.float32
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)
RESETS = dict(max_days=2, auto_reset=True)
SEED = 41


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(autouse=True)
def time_limit(request):
    """every test under its own time limit (the alarm ends a test that loops or waits in Python)"""
    def expired(*_):
        raise TimeoutError(f"{request.node.name} ran longer than 120 s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _planes(N, K):
    return H.implicit_params(N, K, SEED + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, env_id_base=0, **kw):
    e = amd.StepEngine(planes.shape[1], planes.shape[2], seed=SEED, env_id_base=env_id_base, **kw)
    e.set_all_params(planes)
    e.reset()
    return e


def _case(name, frames=1, sigma=0.8):
    """td3_bounded_ref.case, with a stacked policy and critics under an observation history; sigma in units of the half-range"""
    c = BR.case(name)
    K, rng = c["K"], c["rng"]
    if frames > 1:
        c["pol"] = S.random_policy(rng, K, frames, c["hidden"], c["act"], normalize=True, scale=0.6)
        shift, scale = R.realistic_norm(K)
        c["pol"].shift = np.concatenate([shift + F(0.25 * f) for f in range(frames)]).astype(F)
        c["pol"].scale = np.concatenate([scale * F(1.0 + 0.125 * f) for f in range(frames)]).astype(F)
        c["crit"] = S.random_critics(rng, K, frames, c["critics"])
    c["pol"].log_std = np.full(K + 1, np.log(sigma), F)
    c["seeds"] = np.arange(c["N"], dtype=np.uint64) + 5
    return c


def _bounded_engine(amd, c, days, resets=NO_RESETS, learner=True, planes=None, env_id_base=0):
    e = _engine(amd, _planes(c["N"], c["K"]) if planes is None else planes, env_id_base, **resets)
    e.mlp_init(c["pol"], c["seeds"], deterministic=False)
    e.mlp_set_bounds(c["lo"], c["hi"])
    e.rollout_enable(days, obs=True)
    if learner:
        e.td3_init(**c["opts"])
        e.td3_set_critics(c["crit"])
        e.td3_set_bounded(True)
    return e


def _on_input(pol):
    """`pol` as a function of the network's input row (the record's obs): no normalisation left to do"""
    p = copy.copy(pol)
    p.shift = p.scale = None
    return p


# ---- 5. the act ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frames", [("B1", 1), ("B1", 2), ("B2", 1), ("B3", 1)], ids=["B1", "B1-frames2", "B2", "B3"])
def test_the_act_equals_the_restatement_in_the_three_modes(amd, name, frames):
    """five recorded days - gaussian, random, deterministic, gaussian, random -: the last act's mean, action, logp, the bids and
    budgets the env got and the record's action are the restatement's on the row the kernel read (the record's obs; on the first
    day the normalised zero row); the ticks move by one whatever the mode"""
    c = _case(name, frames)
    N, K, pol, lo, hi = c["N"], c["K"], c["pol"], c["lo"], c["hi"]
    A = K + 1
    e = _bounded_engine(amd, c, 5, learner=False)
    assert e.mlp_bounds()["bounded"] and _same(e.mlp_bounds()["lo"], lo) and _same(e.mlp_bounds()["hi"], hi) and e.mlp_bounds()["explore"] == "gaussian"
    net = _on_input(pol)
    plan = [("gaussian", BR.GAUSSIAN), ("random", BR.RANDOM), ("deterministic", BR.DETERMINISTIC), ("gaussian", BR.GAUSSIAN), ("random", BR.RANDOM)]
    for day, (how, mode) in enumerate(plan):
        e.mlp_set_deterministic(how == "deterministic")
        e.mlp_set_explore("random" if how == "random" else "gaussian")
        keys, ticks = e.mlp_agent_state()
        assert np.all(ticks == day)
        z, w = R.normals(keys, ticks, A), BR.words(keys, ticks, A)
        e.mlp_step(0.0)
        last, (bids, budget), rec = e.mlp_last(), e.get_actions(), e.rollout_fetch()
        x = rec["obs"][day]
        if day == 0:
            zero = np.zeros((N, pol.layers[0][0].shape[0]), F)
            assert _same(x, R.act(pol, zero, np.zeros((N, A), F), deterministic=True)["x"])
        ref = BR.act(net, x, lo, hi, mode, z=z, w=w)
        for k in ("mean", "action", "logp"):
            assert _same(last[k], ref[k]), (name, how, k)
        assert _same(bids, ref["bids"]) and _same(budget, ref["budget"]), (name, how)
        assert _same(rec["action"][day], ref["action"]) and not rec["logp"][day].any() and np.signbit(rec["logp"][day]).sum() == 0
        assert np.all(np.abs(ref["action"]) <= 1) and np.all(ref["env"] >= lo) and np.all(ref["env"] <= hi)
        if mode == BR.RANDOM:
            assert np.all(np.abs(ref["action"]) < 1)
    e.close()


def test_handed_in_normals_and_the_clip(amd):
    """mlp_act with handed-in normals at B1: large normals drive components onto both faces of the box; the random mode does not
    read them"""
    c = _case("B1")
    N, K, pol, lo, hi = c["N"], c["K"], c["pol"], c["lo"], c["hi"]
    e = _bounded_engine(amd, c, 2, learner=False)
    z = (np.random.default_rng(2).standard_normal((N, K + 1)) * 3).astype(F)
    zero = np.zeros((N, 5 * K + 2), F)
    e.mlp_act(0.0, replay_normals=z)
    ref = BR.act(pol, zero, lo, hi, BR.GAUSSIAN, z=z)
    last, (bids, budget) = e.mlp_last(), e.get_actions()
    assert _same(last["action"], ref["action"]) and _same(bids, ref["bids"]) and _same(budget, ref["budget"])
    assert (ref["action"] == 1).any() and (ref["action"] == -1).any()
    e.mlp_set_explore("random")
    keys, ticks = e.mlp_agent_state()
    e.mlp_act(0.0, replay_normals=z)
    assert _same(e.mlp_last()["action"], BR.act(pol, zero, lo, hi, BR.RANDOM, w=BR.words(keys, ticks, K + 1))["action"])
    e.close()


@pytest.mark.parametrize("name", ["B1", "B3"])
def test_a_deterministic_bounded_act_gives_the_env_the_squash_bits(amd, name):
    """three deterministic days on two engines, one bounded, one with mlp_set_squash: the same bids and budgets, the same days"""
    c = _case(name)
    a = _bounded_engine(amd, c, 3, learner=False)
    b = _engine(amd, _planes(c["N"], c["K"]), **NO_RESETS)
    b.mlp_init(c["pol"], c["seeds"], deterministic=True)
    b.mlp_set_squash(c["lo"], c["hi"])
    a.mlp_set_deterministic(True)
    for day in range(3):
        a.mlp_step(0.0)
        b.mlp_step(0.0)
        (ba, ua), (bb, ub) = a.get_actions(), b.get_actions()
        assert _same(ba, bb) and _same(ua, ub), day
        assert _same(a.fetch()["reward"], b.fetch()["reward"])
        assert _same(a.mlp_last()["action"], R.tanh32(b.mlp_last()["action"]))
    a.close()
    b.close()


# ---- 6. store and updates -----------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("name,updates", [("B1", 2), ("B2", 2), ("B3", 1)])
def test_store_and_updates_equal_the_restatement(amd, name, updates):
    """the shape's days collected under the bounded act (through an auto-reset at B1, whose 15 samples wrap the ring of 12), the
    store, and `updates` updates with policy_delay 2 (the second steps the actor and moves the targets; B3's one has policy_delay 1):
    the ring, theta, psi, both targets, the moments and the statistics are the restatement's"""
    c = _case(name, sigma=0.3)
    if updates == 1:
        c["opts"] = dict(c["opts"], policy_delay=1)
    N, K, pol, opts, days = c["N"], c["K"], c["pol"], c["opts"], c["days"]
    e = _bounded_engine(amd, c, days, resets=RESETS if name == "B1" else NO_RESETS)
    assert e.td3_bounded()
    e.run_days("mlp", days, 1000.0)
    assert e.td3_store() == days * N
    rec = e.rollout_fetch()
    assert np.all(np.abs(rec["action"]) <= 1)
    ring = T3.Ring(opts["capacity"], 5 * K + 2, K + 1)
    ring.store(rec, T3.current_input(pol, e.fetch(), e.get_episode_state()[0] == 0))
    buf = ring.buffer()
    _assert_buffer(e.td3_buffer(), buf, name)
    if name == "B1":
        assert buf["written"] == 15 and buf["size"] == 12 and buf["done"].any()
    state = T3.fresh_state(pol, c["crit"])
    for u in range(updates):
        stats = e.td3_update(1)
        state, rstats = BR.update(pol, state, buf, opts["seed"], opts)
        _assert_state(e.td3_state(), state, (name, u))
        _assert_stats(stats, rstats, (name, u))
    assert state["actor_steps"] == 1 and _same(e.mlp_params(), state["theta"])
    # the unbounded law on the same ring gives other bits: the mode is not a no-op
    other, _ = T3.update(pol, T3.fresh_state(pol, c["crit"]), buf, None, opts["seed"], dict(opts, policy_delay=1))
    mine, _ = BR.update(pol, T3.fresh_state(pol, c["crit"]), buf, opts["seed"], dict(opts, policy_delay=1))
    assert not _same(other["psi"], mine["psi"]) and not _same(other["theta"], mine["theta"])
    e.close()


# ---- 7. a population ------------------------------------------------------------------------------------------------------------------
def test_a_population_of_two_equals_two_solo_engines(amd):
    """TD3PopulationTrainer at B1 with two members of different sigmas and seeds against two TD3Trainers on engines of a member's
    envs: after each of two iterations every member's ring and state are the solo trainer's"""
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer, TD3Trainer
    c = _case("B1")
    M, n, K = 2, c["N"], c["K"]
    rng = c["rng"]
    pols = [c["pol"], R.random_policy(rng, K, c["hidden"], c["act"], normalize=True, scale=0.6)]
    pols[1].shift, pols[1].scale = pols[0].shift, pols[0].scale
    crits = [c["crit"], T3.random_critics_for_tests(rng, K, c["critics"])]
    sigmas, seeds = [0.2, 0.6], np.arange(M * n, dtype=np.uint64) + 5
    base = dict(critic_hidden=c["critics"][:-1], learning_starts=8, updates_per_iteration=2, batch_size=8, capacity=24, policy_delay=2, gamma=0.9)
    cfgs = [dict(base, seed=123, critics=crits[0]), dict(base, seed=321, critics=crits[1], tau=0.02)]
    planes = _planes(M * n, K)
    bounds = (c["lo"], c["hi"])
    pop = TD3PopulationTrainer(_engine(amd, planes, **RESETS), pols, sigmas, cfgs, horizon=3, agent_seeds=seeds, action_bounds=bounds, random_timesteps=n * 3)
    solos = [TD3Trainer(_engine(amd, planes[:, m * n:(m + 1) * n], env_id_base=m * n, **RESETS), pols[m], horizon=3, exploration_sigma=sigmas[m],
                        agent_seeds=seeds[m * n:(m + 1) * n], action_bounds=bounds, random_timesteps=n * 3, **cfgs[m]) for m in range(M)]
    assert pop.engine.td3_bounded() and pop.engine.mlp_bounds()["bounded"]
    for it in range(3):
        pop.iteration(budget=1000.0)
        assert pop.engine.mlp_bounds()["explore"] == ("random" if it == 0 else "gaussian")
        for m, s in enumerate(solos):
            s.iteration(budget=1000.0)
            got, ref = pop.engine.td3_pop_buffer(m), s.engine.td3_buffer()
            for k in ("x", "a", "r", "done", "x2"):
                assert _same(got[k], ref[k]), (it, m, k)
            gs, rs = pop.state(m), s.state()
            for k in T3.STATE_KEYS:
                assert _same(gs[k], rs[k]), (it, m, k)
            assert gs["updates"] == rs["updates"] == 2 * (it + 1)
    a0, a1 = pop.engine.td3_pop_buffer(0)["a"], pop.engine.td3_pop_buffer(1)["a"]
    assert not _same(a0, a1) and np.all(np.abs(a0) <= 1) and np.all(np.abs(a1) <= 1)
    from adcraft_amd.baselines.sac_trainer import SquashedPolicy
    assert isinstance(pop.policy(1), SquashedPolicy) and _same(pop.policy(1).action_hi, c["hi"])
    for t in [pop] + solos:
        t.engine.close()


# ---- 8. composed, and a resumed state -------------------------------------------------------------------------------------------------
def _loaded(c, size, gamma):
    """a ring of known arrays at the case's shape: actions in the box's units, gn a mix of gamma, gamma^2 and gamma^3"""
    rng, K = c["rng"], c["K"]
    D, A = 5 * K + 2, K + 1
    g1 = F(gamma)
    g2 = F(g1 * g1)
    g3 = F(g2 * g1)
    buf = dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=np.clip(rng.standard_normal((size, A)) * 0.7, -1, 1).astype(F),
               r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))
    buf["gn"] = np.array([g1, g2, g3], F)[rng.integers(0, 3, size)]
    return buf


@pytest.mark.parametrize("addon", ["prioritised", "reward-normaliser"])
def test_composed_bounded_updates_equal_the_composed_restatement(amd, addon):
    """B1, bounded, n_step = 3 on a loaded ring whose slots carry their own discounts, with prioritised replay (importance weights,
    the leaves updated from |d|) or with the reward normaliser (a multiplier != 1 and a clip that binds): two updates with
    policy_delay 2 against nstep_ref.td3_update - the composed restatement that exists - under the bounded law"""
    from tests import nstep_ref as NS
    from tests import per_ref as PR
    c = _case("B1")
    pol, crit, opts = c["pol"], c["crit"], dict(c["opts"], capacity=40)
    c["opts"] = opts
    buf = _loaded(c, 20, opts["gamma"])
    e = _bounded_engine(amd, c, 3)
    state, kw = T3.fresh_state(pol, crit), {}
    if addon == "prioritised":
        per = PR.options()
        e.replay_prio_init(**per)
        kw = dict(tree=PR.Tree(40, np.ones(20, F)), per=per)
    else:
        e.td3_norm_init(rewards=True, rew_clip=0.8)
        st = e.td3_norm_state()
        st.update(rew_count=np.float64(50.0), rew_mean=np.float64(0.5), rew_M2=np.float64(50.0 * 7.3), rew_scale=F(0.37))
        e.td3_norm_state(0, st)
        kw = dict(rew_scale=e.td3_norm_state()["rew_scale"], rew_clip=0.8)
        assert kw["rew_scale"] != 1
    e.replay_nstep_init(3)
    e.td3_buffer_load(buf)
    e.replay_nstep_load(buf["gn"])
    e.td3_update(2)
    with BR.bounded_law():
        for _ in range(2):
            state, _ = NS.td3_update(pol, state, buf, None, opts["seed"], opts, **kw)
    _assert_state(e.td3_state(), state, addon)
    assert state["actor_steps"] == 1
    if addon == "prioritised":
        assert _same(e.replay_prio_fetch(), kw["tree"].leaf[:20]) and not np.all(kw["tree"].leaf[:20] == 1)
    e.close()


def test_all_add_ons_at_once_equal_the_composed_restatement(amd):
    """B1, bounded, with prioritised replay, n_step = 3, the running observation normaliser (the ring holds raw rows, normalised as
    they are gathered) and the reward normaliser (multiplier != 1, a clip that binds) all alive: two updates with policy_delay 2 on
    a loaded ring against td3_bounded_ref.composed_update, which chains the add-ons' own restatements; state, statistics and the
    tree's leaves"""
    from tests import per_ref as PR
    c = _case("B1")
    pol, crit, opts = c["pol"], c["crit"], dict(c["opts"], capacity=40)
    c["opts"] = opts
    buf = _loaded(c, 20, opts["gamma"])
    buf["x"], buf["x2"] = (R.realistic_obs(c["rng"], 20, c["K"]) for _ in range(2))       # (raw rows)
    e = _bounded_engine(amd, c, 3)
    per = PR.options()
    e.replay_prio_init(**per)
    e.td3_norm_init(observations=True, rewards=True, rew_clip=0.8)
    st = e.td3_norm_state()
    st.update(rew_count=np.float64(50.0), rew_mean=np.float64(0.5), rew_M2=np.float64(50.0 * 7.3), rew_scale=F(0.37))
    e.td3_norm_state(0, st)
    st = e.td3_norm_state()
    vectors, mult = (st["shift"], st["scale"]), st["rew_scale"]
    assert mult != 1 and _same(vectors[0], pol.shift)
    e.replay_nstep_init(3)
    e.td3_buffer_load(buf)
    e.replay_nstep_load(buf["gn"])
    tree, state = PR.Tree(40, np.ones(20, F)), T3.fresh_state(pol, crit)
    for u in range(2):
        stats = e.td3_update(1)
        state, rstats = BR.composed_update(pol, state, buf, opts["seed"], opts, tree, per, vectors, mult, 0.8)
        _assert_state(e.td3_state(), state, u)
        _assert_stats(stats, rstats, u)
    assert state["actor_steps"] == 1 and _same(e.replay_prio_fetch(), tree.leaf[:20]) and not np.all(tree.leaf[:20] == 1)
    rs = buf["r"] * F(opts["reward_scale"]) * F(mult)
    assert (np.abs(rs) > 0.8).any() and (np.abs(rs) < 0.8).any(), "the clip binds for some elements"
    e.close()


def test_a_composed_bounded_trainer_resumes_bit_for_bit(amd):
    """TD3Trainer at B1 under bounds with prioritised replay, n_step = 3 and both running normalisers: three iterations in one go;
    two iterations, then state(), norm_state() and the ring into a fresh trainer on an engine driven through the same two
    iterations whose ring was then wiped, and the third: the same bits.  The first iteration is the warm-up's"""
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    c = _case("B1")
    N, K = c["N"], c["K"]

    def make():
        return TD3Trainer(_engine(amd, _planes(N, K), **RESETS), c["pol"], critic_hidden=c["critics"][:-1], horizon=3, exploration_sigma=0.4,
                          learning_starts=10, updates_per_iteration=2, agent_seeds=c["seeds"], critics=c["crit"], batch_size=8, capacity=24, seed=123,
                          gamma=0.9, policy_delay=2, n_step=3, prioritized_replay=dict(alpha=0.6, beta=0.4), normalize_observations=True,
                          normalize_rewards=True, action_bounds=(c["lo"], c["hi"]), random_timesteps=N * 3)

    def snapshot(t):
        st, buf, nrm = t.state(), t.engine.td3_buffer(), t.norm_state()
        return ([st[k] for k in T3.STATE_KEYS] + [st["replay_nstep"]["gn"], buf["x"], buf["a"], buf["r"], buf["done"], buf["x2"]]
                + [np.asarray(nrm[k]) for k in sorted(nrm) if isinstance(nrm[k], np.ndarray)])
    a = make()
    modes = []
    for _ in range(3):
        a.iteration(budget=1000.0)
        modes.append(a.engine.mlp_bounds()["explore"])
    assert modes == ["random", "gaussian", "gaussian"]
    want = snapshot(a)
    b = make()
    for _ in range(2):
        b.iteration(budget=1000.0)
    saved, norm, ring = copy.deepcopy(b.state()), copy.deepcopy(b.norm_state()), b.engine.td3_buffer()
    assert saved["bounded"]["random_timesteps"] == N * 3 and saved["bounded"]["explore"] == "gaussian" and _same(saved["bounded"]["hi"], c["hi"])
    assert np.all(np.abs(ring["a"]) <= 1)
    d = make()
    for _ in range(2):
        d.iteration(budget=1000.0)                                 # (the envs, the agents' ticks and the record's position)
    wiped = {k: np.zeros_like(ring[k]) for k in ("x", "a", "r", "done", "x2")}
    d.engine.td3_buffer_load(wiped, written=ring["written"])
    d.engine.td3_buffer_load(ring)
    d.engine.mlp_set_explore("random")                             # (the state brings the mode back)
    d.norm_state(norm)
    d.load_state(saved)
    assert d.engine.mlp_bounds()["explore"] == "gaussian"
    d.iteration(budget=1000.0)
    got = snapshot(d)
    assert all(_same(g, w) for g, w in zip(got, want)), [_same(g, w) for g, w in zip(got, want)]
    with pytest.raises(ValueError, match="other action_bounds"):
        d.load_state(dict(saved, bounded=dict(saved["bounded"], hi=saved["bounded"]["hi"] + 1)))
    for t in (a, b, d):
        t.engine.close()


# ---- 9. the invariant -----------------------------------------------------------------------------------------------------------------
def test_with_sigma_5_everything_stays_in_the_box(amd):
    """sigma 5 (in units of the half-range) over three days at B1: every recorded n is in [-1, 1], and every bid and budget the
    env consumed is inside [lo, hi] (bids: the box's cent image; most components sit on a face)"""
    c = _case("B1", sigma=5.0)
    K, lo, hi = c["K"], c["lo"], c["hi"]
    e = _bounded_engine(amd, c, 3, learner=False)
    faces = 0
    for day in range(3):
        e.mlp_step(0.0)
        bids, budget = e.get_actions()
        assert np.all(budget >= lo[0]) and np.all(budget <= hi[0])
        assert np.all(bids >= R.cent_bids(lo[None, 1:])) and np.all(bids <= R.cent_bids(hi[None, 1:]))
        n = e.rollout_fetch()["action"][day]
        assert np.all(n >= -1) and np.all(n <= 1)
        faces += int((np.abs(n) == 1).sum())
    assert faces > 3 * c["N"] * (K + 1) // 2
    e.close()


# ---- 10. teacher days -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,envs", [("B1", 5), ("B3", 5)], ids=["5x6", "5x256"])
def test_teacher_days_record_the_mapping_of_the_buffers_actions(amd, name, envs):
    """TD3Trainer.demonstrate("fixed") under bounds at B1: the sampled bids (30 cents to 4 dollars: some above the box) and the budget
    (above its bound) stay in the action buffers; the record's and the ring's actions are their mapping, faces included.  And at
    B3's network with 5 envs: k_teach_record_bounded's 5 x 257 = 1285 lanes are six blocks, the last one partial - the split
    i / A, i % A across blocks and the read of lo / inv_half at a = 256, under the box's ragged bounds"""
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    c = _case(name)
    c["N"], c["seeds"] = envs, np.arange(envs, dtype=np.uint64) + 5
    assert (c["N"], c["K"]) in ((5, 6), (5, 256))
    N, K, lo, hi = c["N"], c["K"], c["lo"], c["hi"]
    t = TD3Trainer(_engine(amd, _planes(N, K), **NO_RESETS), c["pol"], critic_hidden=c["critics"][:-1], horizon=3, agent_seeds=c["seeds"], critics=c["crit"],
                   batch_size=8, capacity=24, action_bounds=(lo, hi))
    e = t.engine
    e.sample_actions(0.3, 4.0, 400.0)
    bids, budget = e.get_actions()
    assert t.demonstrate("fixed", budget=400.0) == 3 * N
    want = BR.unbox(np.concatenate([budget[:, None], bids], axis=1), lo[None, :], hi[None, :])
    rec, buf = e.rollout_fetch(), e.td3_buffer()
    for day in range(3):
        assert _same(rec["action"][day], want), day
    assert _same(buf["a"], np.concatenate([want] * 3)) and not rec["logp"].any()
    assert np.all(want[:, 0] == 1) and (want[:, 1:] == 1).any() and (np.abs(want[:, 1:]) < 1).any()
    assert len(set(want[:, K].tolist())) > 1, "component a = K of the label was meant to differ between envs"
    e.td3_update(1)                                                 # (the critics read such a ring)
    e.close()


# ---- 11. the warm-up ------------------------------------------------------------------------------------------------------------------
def test_the_mode_flips_where_the_ring_reaches_random_timesteps(amd):
    """random_timesteps = 25 at N = 5, horizon 2: the ring holds 0, 10, 20 before the first three collections (random) and 30 before
    the fourth (gaussian).  A twin trainer without a warm-up collects the same days in the gaussian mode: the agents' ticks advance
    identically; its actions differ while the modes differ"""
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    c = _case("B1")
    N, K = c["N"], c["K"]

    def make(random_timesteps):
        return TD3Trainer(_engine(amd, _planes(N, K), **NO_RESETS), c["pol"], critic_hidden=c["critics"][:-1], horizon=2, exploration_sigma=0.3,
                          learning_starts=1000, agent_seeds=c["seeds"], critics=c["crit"], batch_size=8, capacity=100, action_bounds=(c["lo"], c["hi"]),
                          random_timesteps=random_timesteps)
    a, b = make(25), make(0)
    modes = []
    for it in range(4):
        before = a.engine.td3_buffer(fetch=False)["size"]
        a.iteration(budget=1000.0)
        b.iteration(budget=1000.0)
        modes.append((before, a.engine.mlp_bounds()["explore"]))
        ta, tb = a.engine.mlp_agent_state()[1], b.engine.mlp_agent_state()[1]
        assert _same(ta, tb) and np.all(ta == 2 * (it + 1))
        na, nb = a.engine.rollout_fetch()["action"], b.engine.rollout_fetch()["action"]
        assert np.all(np.abs(na) < 1) if it < 3 else True
        assert not _same(na, nb)                                    # (before the flip the modes differ; after it the envs do)
    assert modes == [(0, "random"), (10, "random"), (20, "random"), (30, "gaussian")]
    assert b.engine.mlp_bounds()["explore"] == "gaussian"
    a.engine.close()
    b.engine.close()


# ---- the refusals, by their messages ----------------------------------------------------------------------------------------------------
def _refused(kind, text, fn, *args, **kw):
    with pytest.raises(kind, match=text):
        fn(*args, **kw)


def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd._ffi import EngineStateError as State
    c = _case("B1")
    N, K, pol, lo, hi, opts = c["N"], c["K"], c["pol"], c["lo"], c["hi"], c["opts"]
    e = _engine(amd, _planes(N, K), **NO_RESETS)
    _refused(State, "mlp_init", e.mlp_set_bounds, lo, hi)
    _refused(State, "mlp_init", e.mlp_set_explore, "random")
    # bounds with a two-headed policy
    two = R.random_policy(c["rng"], K, c["hidden"], c["act"], two_heads=True)
    e.mlp_init(two, c["seeds"])
    _refused(State, "two-headed", e.mlp_set_bounds, lo, hi)
    e.mlp_init(pol, c["seeds"], deterministic=False)
    # the bounds themselves, the mode without bounds
    _refused(ValueError, "lo and hi, or neither", e.mlp_set_bounds, lo, None)
    _refused(ValueError, "finite, hi > lo", e.mlp_set_bounds, hi, lo)
    _refused(ValueError, "finite, hi > lo", e.mlp_set_bounds, lo, np.full(K + 1, np.inf, F))
    _refused(State, "needs the bounded act", e.mlp_set_explore, "random")
    _refused(ValueError, "unknown exploration mode", e.mlp_set_explore, "ou")
    _refused(State, "needs learners", e.mlp_learners_set_bounds, lo, hi)
    # bounds together with the squash, either order
    e.mlp_set_squash(lo, hi)
    _refused(State, "together with the squashed action", e.mlp_set_bounds, lo, hi)
    e.mlp_set_squash(None, None)
    e.mlp_set_bounds(lo, hi)
    _refused(State, "together with the bounded act", e.mlp_set_squash, lo, hi)
    # what needs a log-probability: the policy-gradient trainer (imitation lives on it), SAC, the evolution strategy's population
    e.rollout_enable(3, obs=True)
    _refused(State, "policy-gradient training under the bounded act", e.pg_init)
    _refused(State, "soft actor-critic training under the bounded act", e.sac_init, num_keywords=K)
    _refused(State, "population with the bounded act", e.mlp_population, 2)
    _refused(State, "single policy's bounded act", e.mlp_learners, N)
    # bounded TD3: without the bounded act, with an action normalisation, with action_lo / action_hi
    e.mlp_set_bounds(None, None)
    assert not e.mlp_bounds()["bounded"]
    _refused(State, "td3_init", e.td3_set_bounded, True)
    e.td3_init(**opts)
    e.td3_set_critics(c["crit"])
    _refused(State, "bounded TD3 needs the bounded act", e.td3_set_bounded, True)
    e.mlp_set_bounds(lo, hi)
    _refused(State, "learner must be bounded too", e.td3_store)
    e.td3_set_critics(c["crit"], action_norm=(np.zeros(K + 1, F), np.ones(K + 1, F)))
    _refused(State, "with an action normalisation", e.td3_set_bounded, True)
    e.td3_init(**dict(opts, action_lo=0.1, action_hi=0.9))
    e.td3_set_critics(c["crit"])
    _refused(State, "action_lo / action_hi set", e.td3_set_bounded, True)
    e.td3_init(**opts)
    e.td3_set_critics(c["crit"])
    assert not e.td3_bounded()
    e.td3_set_bounded(True)
    _refused(State, "with an action normalisation", e.td3_set_critics, c["crit"], action_norm=(np.zeros(K + 1, F), np.ones(K + 1, F)))
    # the act and the learner must agree; the bounds may not change under a filled ring
    e.run_days("mlp", 3, 1000.0)
    assert e.td3_store() == 3 * N
    _refused(State, "ring holds transitions", e.mlp_set_bounds, lo, hi + F(1))
    _refused(State, "ring holds transitions", e.mlp_set_bounds, None, None)
    _refused(State, "ring holds transitions", e.td3_set_bounded, False)
    stats = e.td3_update(2)                                         # (the engine still works)
    assert stats["updates"] == 2 and stats["actor_steps"] == 1
    # a new trainer starts unbounded on an empty ring: the bounds may change again
    e.td3_init(**opts)
    assert not e.td3_bounded()
    e.mlp_set_bounds(lo, hi + F(1))
    e.mlp_set_bounds(None, None)
    e.close()
    # a population: the learners' own entry points
    e = _engine(amd, _planes(2 * N, K), **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    e.mlp_learners(2)
    _refused(State, "adc_engine_mlp_learners_set_bounds", e.mlp_set_bounds, lo, hi)
    e.rollout_enable(3, obs=True)
    e.td3_pop_init([dict(opts), dict(opts, seed=7)])
    _refused(State, "bounded TD3 needs the bounded act", e.td3_pop_set_bounded, True)
    e.mlp_learners_set_bounds(lo, hi)
    e.td3_pop_set_bounded(True)
    _refused(State, "action_lo / action_hi set", lambda: (e.td3_pop_set_config(1, **dict(opts, seed=7, action_lo=0.1, action_hi=0.9)), e.td3_pop_store()))
    e.mlp_learners(0)                                               # (the learners' bounds go with them)
    assert not e.mlp_bounds()["bounded"]
    e.close()
