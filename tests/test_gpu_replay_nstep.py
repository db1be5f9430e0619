"""GPU tests of n-step returns for the TD3 / SAC learners (parts/nstep_api.inc, the n-step forms of the store in
parts/kernel_td3.inc, the targets' read of gn) against the numpy restatement tests/nstep_ref.py, bit for bit: the store through
auto-resets, a second store and a wrapping ring, with and without an observation history; TD3 and SAC updates on a loaded ring with
mixed discounts; the reward normaliser's multiplier and clip; prioritised replay; populations against solo engines, member copies
and a PBT round with rings; n = 1 and off; the refusals; a resumed trainer.  3 envs per learner x 2 keywords, policy (8,), critics
(8, 1), batch 8.  The entry points do not exist before this feature: every test but the off-means-off one fails on the parent
commit.  The wide shapes live in tests/test_gpu_replay_shapes.py: the four forms of the store and the population's at K = 256,
where a row takes six passes of 256 lanes (twelve with two frames) and an action two."""
import copy
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import nstep_ref as NS
from tests import per_ref as PR
from tests import sac_ref as S
from tests import stack_ref as ST
from tests import td3_pop_ref as TP
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F = np.float32
N, K, B, HIDDEN, WIDTHS, SEED, BUDGET = 3, 2, 8, (8,), (8, 1), 47, 1000.0
D, A = 5 * K + 2, K + 1
RESETS = dict(max_days=4, auto_reset=True)
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)
GAMMA = 0.9


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


def _planes(envs=N):
    return H.implicit_params(envs, K, SEED + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, env_id_base=0, **kw):
    e = amd.StepEngine(planes.shape[1], K, seed=SEED, env_id_base=env_id_base, **kw)
    e.set_all_params(planes)
    e.reset()
    return e


def _td3_policy(rng):
    pol = R.random_policy(rng, K, HIDDEN, "tanh", normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(K)
    pol.layers[-1][1][1:K + 1] += F(0.8)                           # bids around 80 cents: auctions are won, rewards are not zero
    return pol


def _sac_policy(rng):
    pol = S.sac_policy(rng, K, HIDDEN, "tanh", clamp=(-1.0, -0.5), normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _bounds():
    return np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], 3.0 + np.arange(K) / 10.0]).astype(F)


def _td3_opts(capacity, **kw):
    return T3.options(**dict(dict(critic_widths=WIDTHS, batch_size=B, capacity=capacity, policy_delay=1, tau=0.05, target_noise=0.3, target_noise_clip=0.25,
                                  gamma=GAMMA, reward_scale=0.5, critic_lr=3e-3, seed=123), **kw))


def _sac_opts(capacity, **kw):
    return S.options(K, **dict(dict(critic_widths=WIDTHS, batch_size=B, capacity=capacity, tau=0.05, gamma=GAMMA, reward_scale=0.5, init_alpha=0.3,
                                    critic_lr=3e-3, seed=123), **kw))


def _td3(amd, pol, crit, opts, horizon=5, env_id_base=0, planes=None, resets=NO_RESETS):
    e = _engine(amd, _planes() if planes is None else planes, env_id_base, **resets)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(horizon, obs=True)
    e.td3_init(**opts)
    e.td3_set_critics(crit)
    return e


def _sac(amd, pol, crit, opts, horizon=5, env_id_base=0, planes=None, resets=NO_RESETS):
    e = _engine(amd, _planes() if planes is None else planes, env_id_base, **resets)
    e.mlp_init(pol, deterministic=False)
    e.mlp_set_squash(*_bounds())
    e.rollout_enable(horizon, obs=True)
    e.sac_init(**opts)
    e.sac_set_critics(crit)
    return e


def _collect(e, store, days):
    e.rollout_reset()
    e.run_days("mlp", days, BUDGET)
    return store()


def _peek(e, pol):
    return T3.current_input(pol, e.fetch(), e.get_episode_state()[0] == 0)


def _assert_ring(e, ring, what, fam="td3", member=None):
    buf = getattr(e, fam + "_buffer")() if member is None else getattr(e, fam + "_pop_buffer")(member)
    ref = ring.buffer()
    assert (buf["size"], buf["written"]) == (ref["size"], ref["written"]), what
    for k in ("x", "a", "r", "done", "x2"):
        assert _same(buf[k], ref[k]), (k, what)
    assert _same(e.replay_nstep_fetch(0 if member is None else member), ref["gn"]), ("gn", what)
    return buf


def _loaded(rng, size, gamma=GAMMA):
    """a ring of known arrays: gn a mix of gamma, gamma^2 and gamma^3 (as the store forms them), dones mixed"""
    g1 = F(gamma)
    g2 = F(g1 * g1)
    g3 = F(g2 * g1)
    buf = dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * 0.5 + 0.4).astype(F),
               r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))
    buf["gn"] = np.array([g1, g2, g3], F)[rng.integers(0, 3, size)]
    assert len(set(buf["gn"].tolist())) == 3 and buf["done"].any() and not buf["done"].all()
    return buf


def _assert_keys(got, ref, keys, what=""):
    for k in keys:
        assert _same(got[k], ref[k]), (k, what)


# ---- 1. the store, solo TD3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [40, 7], ids=["appending", "wrapping"])
def test_store_equals_the_restatement(amd, capacity):
    """max_days 4, T = 5, n = 3: an auto-reset falls inside the record.  After td3_store the ring and gn are the restatement's built
    from rollout_fetch of the same record and the row an act would read now; a second store appends behind the first.  Capacity 7 is
    less than the 15 samples of a store: the ring wraps and the samples with s + C < count are skipped"""
    rng = np.random.default_rng(1)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _td3_opts(capacity)
    e = _td3(amd, pol, crit, opts, resets=RESETS)
    assert e.replay_nstep_info() == 0
    e.replay_nstep_init(3)
    assert e.replay_nstep_info() == 3
    ring = NS.Ring(capacity, D, A, 3, GAMMA)
    for rnd in range(2):
        assert _collect(e, e.td3_store, 5) == 5 * N
        rec, peek = e.rollout_fetch(), _peek(e, pol)
        ring.store(rec, peek)
        buf = _assert_ring(e, ring, (capacity, rnd))
        done = rec["terminated"] | rec["truncated"]
        assert done.any() and not done.all(), "an episode ends inside the record"
        w = NS.windows(3, GAMMA, rec["reward"], rec["terminated"], rec["truncated"])
        assert set(w["m"].tolist()) == {1, 2, 3} and w["done"].any() and np.count_nonzero(rec["reward"]) > 5 * N // 2
        if capacity == 40:
            at = rnd * 5 * N
            m, t = w["m"], np.repeat(np.arange(5), N)
            assert _same(buf["r"][at:at + 5 * N], w["R"]) and not _same(w["R"], rec["reward"].reshape(-1))
            reach = t + m >= 5                                  # windows that reach the fragment's end: x' is the peeked row
            assert reach.sum() >= N
            assert all(_same(buf["x2"][at + s], peek[s % N]) for s in np.flatnonzero(reach))
            assert all(_same(buf["x2"][at + s], rec["obs"][t[s] + m[s], s % N]) for s in np.flatnonzero(~reach))
    e.close()


# ---- 2. the store with an observation history ----------------------------------------------------------------------------------------------
def test_store_with_an_observation_history(amd):
    """frames = 2: the _hist form of the n-step store.  x' of a window that reaches the fragment's end is the peeked stacked row"""
    frames, T, C = 2, 5, 11
    Dh = frames * D
    rng = np.random.default_rng(2)
    pol = ST.random_policy(rng, K, frames, HIDDEN, "tanh", value=False, normalize=True, scale=0.6)
    shift, scale = R.realistic_norm(K)
    pol.shift, pol.scale = np.concatenate([shift, shift + F(0.25)]).astype(F), np.concatenate([scale, scale * F(1.125)]).astype(F)
    pol.layers[-1][1][1:K + 1] += F(0.8)                           # bids around 80 cents: auctions are won
    crit = ST.random_critics(rng, K, frames, WIDTHS)
    e = _engine(amd, _planes(), **RESETS)
    e.mlp_init(pol, np.arange(N, dtype=np.uint64) + 11, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.td3_init(**_td3_opts(C))
    e.td3_set_critics(crit)
    e.replay_nstep_init(3)
    hist = ST.History(N, K, frames)

    def now():
        day = e.get_episode_state()[0].astype(np.int64)
        x = R.flat_obs(e.fetch()).astype(F)
        x[day == 0] = 0
        return x, day
    ring = NS.Ring(C, Dh, A, 3, GAMMA)
    for rnd in range(2):
        e.rollout_reset()
        for _ in range(T):
            hist.row(*now())
            e.mlp_step(BUDGET)
        assert e.td3_store() == T * N
        rec = e.rollout_fetch()
        peek = ST.normalized(pol, hist.row(*now(), commit=False))
        # (round 0 ends on the second day of an episode, whose older frame is the first day's zero row; round 1 on the third)
        assert rnd == 0 or np.abs(hist.row(*now(), commit=False)[:, D:]).sum() > 0, "the peeked row has an older frame"
        ring.store(rec, peek)
        buf = _assert_ring(e, ring, rnd)
        assert buf["done"].any() and not buf["done"].all() and buf["x"].shape[1] == Dh and np.count_nonzero(buf["r"]) > C // 2
    e.close()


# ---- 3. updates on a loaded ring ---------------------------------------------------------------------------------------------------------
def test_td3_updates_equal_the_restatement(amd):
    rng = np.random.default_rng(3)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _td3_opts(40)
    buf = _loaded(rng, 20)
    e = _td3(amd, pol, crit, opts)
    e.replay_nstep_init(3)
    e.td3_buffer_load(buf)
    e.replay_nstep_load(buf["gn"])
    assert _same(e.replay_nstep_fetch(), buf["gn"])
    stats = e.td3_update(2)
    state = T3.fresh_state(pol, crit)
    for _ in range(2):
        state, rstats = NS.td3_update(pol, state, buf, None, 123, opts)
    got = e.td3_state()
    _assert_keys(got, state, T3.STATE_KEYS)
    assert (got["updates"], got["actor_steps"]) == (2, 2)
    for k in T3.STAT_KEYS:
        assert _same(np.float64(stats[k]), np.float64(rstats[k])), (k, stats[k], rstats[k])
    # the discounts matter: the one-step target on the same ring gives other bits
    one = T3.update(pol, T3.fresh_state(pol, crit), buf, None, 123, opts)[0]
    two = NS.td3_update(pol, T3.fresh_state(pol, crit), buf, None, 123, opts)[0]
    assert not _same(one["psi"], two["psi"])
    e.close()


def test_sac_updates_equal_the_restatement(amd):
    rng = np.random.default_rng(4)
    pol, crit = _sac_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _sac_opts(40)
    buf = _loaded(rng, 20)
    e = _sac(amd, pol, crit, opts)
    e.replay_nstep_init(3)
    e.sac_buffer_load(buf)
    e.replay_nstep_load(buf["gn"], member=-1)                     # (-1 or 0 for a solo trainer)
    stats = e.sac_update(2)
    state = S.fresh_state(pol, crit, opts)
    for _ in range(2):
        state, rstats = NS.sac_update(pol, state, buf, 123, opts)
    got = e.sac_state()
    _assert_keys(got, state, S.STATE_KEYS)                      # (log_alpha, the temperature's cell, among them)
    for k in S.STAT_KEYS:
        assert _same(np.float64(stats[k]), np.float64(rstats[k])), (k, stats[k], rstats[k])
    one = S.update(pol, S.update(pol, S.fresh_state(pol, crit, opts), buf, 123, opts)[0], buf, 123, opts)[0]
    assert not _same(one["psi"], state["psi"]), "the discounts matter"
    e.close()


# ---- 4. the reward normaliser, prioritised replay ------------------------------------------------------------------------------------------
def test_td3_update_under_the_reward_normaliser(amd):
    """normalize_rewards with a multiplier != 1 and rew_clip > 0: the multiplier and the clip apply to R as they applied to r"""
    rng = np.random.default_rng(5)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _td3_opts(40)
    buf = _loaded(rng, 20)
    e = _td3(amd, pol, crit, opts)
    e.td3_norm_init(rewards=True, rew_clip=0.8)
    st = e.td3_norm_state()
    st.update(rew_count=np.float64(50.0), rew_mean=np.float64(0.5), rew_M2=np.float64(50.0 * 7.3), rew_scale=F(0.37))
    e.td3_norm_state(0, st)
    mult = e.td3_norm_state()["rew_scale"]
    print("multiplier in force", mult)
    assert mult != 1 and np.isfinite(mult) and mult > 0
    e.replay_nstep_init(3)
    e.td3_buffer_load(buf)
    e.replay_nstep_load(buf["gn"])
    e.td3_update(2)
    state = T3.fresh_state(pol, crit)
    for _ in range(2):
        state, _ = NS.td3_update(pol, state, buf, None, 123, opts, rew_scale=mult, rew_clip=0.8)
    _assert_keys(e.td3_state(), state, T3.STATE_KEYS)
    rs = buf["r"] * F(0.5) * F(mult)
    assert (np.abs(rs) > 0.8).any() and (np.abs(rs) < 0.8).any(), "the clip binds for some elements"
    e.close()


def test_td3_update_under_prioritised_replay(amd):
    rng = np.random.default_rng(6)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _td3_opts(40)
    buf = _loaded(rng, 20)
    per = PR.options()
    e = _td3(amd, pol, crit, opts)
    e.replay_prio_init(**per)
    e.replay_nstep_init(3)
    e.td3_buffer_load(buf)
    e.replay_nstep_load(buf["gn"])
    tree = PR.Tree(40, np.ones(20, F))
    e.td3_update(2)
    state = T3.fresh_state(pol, crit)
    for _ in range(2):
        state, _ = NS.td3_update(pol, state, buf, None, 123, opts, tree=tree, per=per)
    _assert_keys(e.td3_state(), state, T3.STATE_KEYS)
    assert _same(e.replay_prio_fetch(), tree.leaf[:20]) and not np.all(tree.leaf[:20] == 1)
    e.close()


# ---- 5. populations ----------------------------------------------------------------------------------------------------------------------
M, NP = 2, 6
n = NP // M
TD3_OWN = (dict(seed=0, gamma=0.9), dict(seed=77, gamma=0.97, critic_lr=1e-3))
SAC_OWN = (dict(seed=0, gamma=0.9), dict(seed=77, gamma=0.97, init_alpha=0.1))


def _pop(amd, kind, pols, crits, opts, horizon=5):
    e = _engine(amd, _planes(NP), **RESETS)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    for m in range(1, M):
        e.mlp_set_learner(m, pols[m])
    if kind == "sac":
        e.mlp_learners_set_squash(*_bounds())
    e.rollout_enable(horizon, obs=True)
    getattr(e, kind + "_pop_init")(opts)
    for m in range(M):
        getattr(e, kind + "_pop_set_critics")(m, crits[m])
    return e


def _members(rng, kind):
    make = _td3_policy if kind == "td3" else _sac_policy
    pols, crits = [make(rng) for _ in range(M)], [T3.random_critics_for_tests(rng, K, WIDTHS) for _ in range(M)]
    own = TD3_OWN if kind == "td3" else SAC_OWN
    return pols, crits, [(_td3_opts if kind == "td3" else _sac_opts)(40, **o) for o in own]


@pytest.mark.parametrize("kind", ["td3", "sac"])
def test_a_population_member_equals_a_solo_engine_on_its_envs(amd, kind):
    """M = 2 learners with different gamma on 6 envs, n = 3, two collections of five days through auto-resets with one update after
    each: every member's ring, gn and state are those of a solo engine of its three envs under its own gamma"""
    rng = np.random.default_rng(7)
    pols, crits, opts = _members(rng, kind)
    e = _pop(amd, kind, pols, crits, opts)
    e.replay_nstep_init(3)
    solos = []
    for m in range(M):
        s = (_td3 if kind == "td3" else _sac)(amd, pols[m], crits[m], opts[m], env_id_base=m * n, planes=_planes(NP)[:, TP.member_slice(m, n)], resets=RESETS)
        s.replay_nstep_init(3)
        solos.append(s)
    keys = T3.STATE_KEYS if kind == "td3" else S.STATE_KEYS
    for rnd in range(2):
        assert _collect(e, getattr(e, kind + "_pop_store"), 5) == 5 * n
        getattr(e, kind + "_pop_update")(1)
        for m, s in enumerate(solos):
            assert _collect(s, getattr(s, kind + "_store"), 5) == 5 * n
            getattr(s, kind + "_update")(1)
            got, ref = getattr(e, kind + "_pop_buffer")(m), getattr(s, kind + "_buffer")()
            _assert_keys(got, ref, ("x", "a", "r", "done", "x2"), (rnd, m))
            assert np.count_nonzero(got["r"]) > len(got["r"]) // 2 and got["done"].any()
            assert _same(e.replay_nstep_fetch(m), s.replay_nstep_fetch()), (rnd, m)
            _assert_keys(getattr(e, kind + "_pop_state")(m), getattr(s, kind + "_state")(), keys, (rnd, m))
    g = [e.replay_nstep_fetch(m) for m in range(M)]
    assert set(g[0].tolist()) <= {F(0.9), F(F(0.9) * F(0.9)), F(F(F(0.9) * F(0.9)) * F(0.9))} and len(set(g[0].tolist())) == 3
    assert F(0.97) in g[1] and not _same(g[0], g[1]), "every member discounts by its own gamma"
    for s in solos:
        s.close()
    e.close()


@pytest.mark.parametrize("kind", ["td3", "sac"])
def test_copies_carry_gn_with_the_ring(amd, kind):
    rng = np.random.default_rng(8)
    pols, crits, opts = _members(rng, kind)
    e = _pop(amd, kind, pols, crits, opts)
    e.replay_nstep_init(3)
    _collect(e, getattr(e, kind + "_pop_store"), 5)
    before = [e.replay_nstep_fetch(m) for m in range(M)]
    rings = [getattr(e, kind + "_pop_buffer")(m) for m in range(M)]
    assert not _same(before[0], before[1])
    copy_ = getattr(e, kind + "_pop_copy")
    copy_(0, 1, with_ring=False)
    assert _same(e.replay_nstep_fetch(1), before[1]), "without the ring gn stays"
    copy_(0, 1, with_ring=True)
    assert _same(e.replay_nstep_fetch(1), before[0]) and _same(e.replay_nstep_fetch(0), before[0]), "with the ring gn is the donor's"
    _assert_keys(getattr(e, kind + "_pop_buffer")(1), rings[0], ("x", "a", "r", "done", "x2"))
    # a PBT round with rings: member 0 becomes member 1, whose gn is given a pattern of its own first
    mark = (before[1] * F(0.5)).astype(F)
    e.replay_nstep_load(mark, member=1)
    e.pbt_init(kind, replace_count=1, with_ring=True)
    e.pbt_exploit([1, -1])
    assert _same(e.replay_nstep_fetch(0), mark) and _same(e.replay_nstep_fetch(1), mark), "an exploit with rings carries gn"
    getattr(e, kind + "_pop_update")(1)                          # (the copied rings are whole: an update runs on them)
    e.close()


# ---- 6. n = 1 and off ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["td3", "sac"])
def test_n_1_gives_the_bits_of_an_engine_without_the_add_on(amd, kind):
    rng = np.random.default_rng(9)
    td3 = kind == "td3"
    pol, crit = (_td3_policy if td3 else _sac_policy)(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = (_td3_opts if td3 else _sac_opts)(40)
    make = _td3 if td3 else _sac
    off, one = make(amd, pol, crit, opts, resets=RESETS), make(amd, pol, crit, opts, resets=RESETS)
    one.replay_nstep_init(1)
    assert off.replay_nstep_info() == 0 and one.replay_nstep_info() == 1
    for rnd in range(2):
        for e in (off, one):
            assert _collect(e, getattr(e, kind + "_store"), 5) == 5 * N
            getattr(e, kind + "_update")(2)
        a, b = getattr(off, kind + "_buffer")(), getattr(one, kind + "_buffer")()
        _assert_keys(b, a, ("x", "a", "r", "done", "x2"), rnd)
        assert a["done"].any() and np.count_nonzero(a["r"]) > len(a["r"]) // 2
        _assert_keys(getattr(one, kind + "_state")(), getattr(off, kind + "_state")(), T3.STATE_KEYS if td3 else S.STATE_KEYS, rnd)
        assert np.all(one.replay_nstep_fetch() == F(GAMMA))
    off.close()
    one.close()


def test_init_on_a_filled_ring_and_a_second_init(amd):
    """a ring that holds one-step transitions gets gn = gamma; a second init changes the window from the next store on and leaves
    the stored slots alone"""
    rng = np.random.default_rng(10)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    e = _td3(amd, pol, crit, _td3_opts(50), resets=RESETS)
    ring = NS.Ring(50, D, A, 1, GAMMA)
    for n_now in (None, 2, 3):
        if n_now is not None:
            e.replay_nstep_init(n_now)
            ring.n = n_now
        assert _collect(e, e.td3_store, 5) == 5 * N
        ring.store(e.rollout_fetch(), _peek(e, pol))
        if n_now is not None:
            _assert_ring(e, ring, n_now)
    gn = e.replay_nstep_fetch()
    assert np.all(gn[:5 * N] == F(GAMMA)) and F(F(GAMMA) * F(GAMMA)) in gn[5 * N:10 * N] and F(F(F(GAMMA) * F(GAMMA)) * F(GAMMA)) in gn[10 * N:]
    assert F(F(F(GAMMA) * F(GAMMA)) * F(GAMMA)) not in gn[:10 * N]
    e.close()


def test_refusals(amd):
    from adcraft_amd import _ffi
    rng = np.random.default_rng(11)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    e = _engine(amd, _planes(), **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(5, obs=True)
    assert e.replay_nstep_info() == 0
    with pytest.raises(_ffi.EngineStateError, match="TD3 or SAC trainer"):
        e.replay_nstep_init(3)
    e.td3_init(**_td3_opts(40))
    e.td3_set_critics(crit)
    with pytest.raises(_ffi.EngineStateError, match="replay_nstep_init"):
        e.replay_nstep_fetch(0, 0, 1)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="1 to 16"):
            e.replay_nstep_init(bad)
    assert e.replay_nstep_info() == 0
    e.replay_nstep_init(16)
    buf = _loaded(rng, 10)
    e.td3_buffer_load(buf)
    for bad in (np.nan, np.inf, -0.5):
        g = buf["gn"].copy()
        g[3] = bad
        with pytest.raises(ValueError, match="finite"):
            e.replay_nstep_load(g)
    with pytest.raises(ValueError, match="member"):
        e.replay_nstep_fetch(1, 0, 1)
    with pytest.raises(ValueError, match="slot range"):
        e.replay_nstep_fetch(0, 5, 6)
    with pytest.raises(ValueError, match="slot range"):
        e.replay_nstep_load(np.ones(41, F))
    e.replay_nstep_load(buf["gn"])
    e.td3_update(1)                                              # (the engine still works)
    # a new trainer starts without the add-on
    e.td3_init(**_td3_opts(40))
    assert e.replay_nstep_info() == 0
    e.close()


# ---- 7. resume -----------------------------------------------------------------------------------------------------------------------------
def test_a_resumed_td3_trainer_continues_bit_for_bit(amd):
    """TD3Trainer(n_step=3): three iterations in one go; two iterations, state() and the ring into a fresh trainer on an engine
    driven through the same two iterations whose ring and gn were then wiped, and the third: the same bits"""
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    rng = np.random.default_rng(12)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    seeds = np.arange(N, dtype=np.uint64) + 5

    def make():
        return TD3Trainer(_engine(amd, _planes(), **RESETS), pol, critic_hidden=HIDDEN, horizon=5, learning_starts=10, updates_per_iteration=2, agent_seeds=seeds,
                          critics=crit, batch_size=B, capacity=40, seed=123, gamma=GAMMA, policy_delay=1, n_step=3)

    def snapshot(t):
        st, buf = t.state(), t.engine.td3_buffer()
        return [st[k] for k in T3.STATE_KEYS] + [st["replay_nstep"]["gn"], buf["x"], buf["r"], buf["done"], buf["x2"]]
    a = make()
    assert a.engine.replay_nstep_info() == 3
    for _ in range(3):
        a.iteration(budget=BUDGET)
    want = snapshot(a)
    b = make()
    for _ in range(2):
        b.iteration(budget=BUDGET)
    saved, ring = copy.deepcopy(b.state()), b.engine.td3_buffer()
    assert saved["replay_nstep"]["n"] == 3 and len(set(saved["replay_nstep"]["gn"].tolist())) == 3
    c = make()
    for _ in range(2):
        c.iteration(budget=BUDGET)                                 # (the envs, the agents' ticks and the record's position)
    wiped = {k: np.zeros_like(ring[k]) for k in ("x", "a", "r", "done", "x2")}
    c.engine.td3_buffer_load(wiped, written=ring["written"])
    c.engine.replay_nstep_load(np.zeros(ring["size"], F))
    c.engine.td3_buffer_load(ring)
    c.load_state(saved)
    c.iteration(budget=BUDGET)
    got = snapshot(c)
    assert all(_same(g, w) for g, w in zip(got, want)), [_same(g, w) for g, w in zip(got, want)]
    # without n_step the trainer never initialises the add-on
    d = TD3Trainer(_engine(amd, _planes(), **RESETS), pol, critic_hidden=HIDDEN, horizon=5, critics=crit, batch_size=B, capacity=40)
    assert d.engine.replay_nstep_info() == 0 and "replay_nstep" not in d.state()
    for x in (a, b, c, d):
        x.engine.close()
