"""GPU tests of prioritised replay on the device (parts/kernel_per.inc, parts/per_api.inc) against the numpy restatement
tests/per_ref.py, bit for bit: the tree and the sampler on one, two and three levels, solo TD3 and SAC updates with certain
duplicates, the ring's wrap, populations against solo engines, member copies and a PBT exploit with rings, a checkpoint,
set_beta, every refusal, and the four trainers.  8 envs x 3 keywords, policy (8,), critics (8, 8, 1), batch 16; the
population tests take 9 envs, so that three members own three each.  None of these symbols exists before this feature:
every test here fails on the parent commit.  The wide shapes live in tests/test_gpu_replay_shapes.py: a three-level tree
(capacity 4200) under TD3, SAC and population updates and under a wrapping store."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import per_ref as PR
from tests import sac_ref as S
from tests import td3_pop_ref as TP
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F = np.float32
N, K, B, HIDDEN, WIDTHS, SEED, BUDGET = 8, 3, 16, (8,), (8, 8, 1), 41, 1000.0
D, A = 5 * K + 2, K + 1
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)
PER = PR.options()


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


def _planes(envs):
    return H.implicit_params(envs, K, SEED + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, env_id_base=0, **kw):
    e = amd.StepEngine(planes.shape[1], K, seed=SEED, env_id_base=env_id_base, **dict(NO_RESETS, **kw))
    e.set_all_params(planes)
    e.reset()
    return e


def _td3_policy(rng):
    pol = R.random_policy(rng, K, HIDDEN, "tanh", normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _sac_policy(rng):
    pol = S.sac_policy(rng, K, HIDDEN, "tanh", clamp=(-1.0, -0.5), normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _bounds():
    return np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], 3.0 + np.arange(K) / 10.0]).astype(F)


def _action_norm():
    return np.full(A, 0.25, F), np.full(A, 1.5, F)


def _td3_opts(capacity, **kw):
    return T3.options(**dict(dict(critic_widths=WIDTHS, batch_size=B, capacity=capacity, policy_delay=2, tau=0.05, target_noise=0.3, target_noise_clip=0.25,
                                  gamma=0.9, reward_scale=0.5, critic_lr=3e-3, seed=123), **kw))


def _sac_opts(capacity, **kw):
    return S.options(K, **dict(dict(critic_widths=WIDTHS, batch_size=B, capacity=capacity, tau=0.05, gamma=0.9, reward_scale=0.5, init_alpha=0.3,
                                    critic_lr=3e-3, seed=123), **kw))


def _td3(amd, pol, crit, opts, envs=N, env_id_base=0, planes=None, horizon=2):
    e = _engine(amd, _planes(envs) if planes is None else planes, env_id_base)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(horizon, obs=True)
    e.td3_init(**opts)
    e.td3_set_critics(crit, action_norm=_action_norm())
    return e


def _sac(amd, pol, crit, opts, envs=N, env_id_base=0, planes=None, horizon=2):
    e = _engine(amd, _planes(envs) if planes is None else planes, env_id_base)
    e.mlp_init(pol, deterministic=False)
    e.mlp_set_squash(*_bounds())
    e.rollout_enable(horizon, obs=True)
    e.sac_init(**opts)
    e.sac_set_critics(crit)
    return e


def _random_buffer(rng, size):
    return dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * 0.5 + 0.4).astype(F),
                r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))


def _assert_tree(e, tree, size, what="", member=0):
    info = e.replay_prio_info(member)
    assert _same(e.replay_prio_fetch(member), tree.leaf[:size]), ("leaf", what)
    assert _same(info["top"], F(tree.top)), ("top", what, info["top"], tree.top)
    assert _same(info["total"], np.float64(tree.total)), ("total", what, info["total"], tree.total)


def _assert_keys(got, ref, keys, what=""):
    for k in keys:
        assert _same(got[k], ref[k]), (k, what)


# ---- 1. the tree and the sampler -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,size", [(64, 64), (100, 70), (4100, 4100)], ids=["one-level", "padded-second-level", "three-levels"])
def test_tree_and_sampling_equal_the_restatement(amd, capacity, size):
    rng = np.random.default_rng(capacity)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    e = _td3(amd, pol, crit, _td3_opts(capacity))
    e.td3_buffer_load(_random_buffer(rng, size))
    e.replay_prio_init(**PER)
    tree = PR.Tree(capacity, np.ones(size, F))
    _assert_tree(e, tree, size, "a loaded ring starts at leaf 1")
    leaf = (10.0 ** rng.uniform(-2, 1, size)).astype(F)
    e.replay_prio_load(leaf, 7.5)
    tree = PR.Tree(capacity, leaf, top=7.5)
    _assert_tree(e, tree, size, "loaded leaves")
    for update in (0, 5, 2 ** 32 - 2):
        idx, w = e.replay_prio_batch(update)
        ridx, rw = PR.sample(tree, 123, update, B, size, PER["beta"])
        assert _same(idx, ridx) and _same(w, rw), update
        assert idx.min() >= 0 and idx.max() < size and w.max() == 1 and w.min() > 0
    # a part of the range: only the nodes above it are rebuilt, and the rest still stands
    part = (10.0 ** rng.uniform(-2, 1, 30)).astype(F)
    e.replay_prio_load(part, 9.0, slot=size - 40)
    leaf[size - 40:size - 10] = part
    tree = PR.Tree(capacity, leaf, top=9.0)
    _assert_tree(e, tree, size, "a part")
    idx, w = e.replay_prio_batch(3)
    ridx, rw = PR.sample(tree, 123, 3, B, size, PER["beta"])
    assert _same(idx, ridx) and _same(w, rw)
    e.close()


# ---- 2., 3. solo learners ----------------------------------------------------------------------------------------------------------------
def _collect(e, store, days=1):
    e.rollout_reset()
    e.run_days("mlp", days, BUDGET)
    return store()


def test_td3_updates_equal_the_restatement(amd):
    """one day of 8 envs stored: size 8 < B 16, so every batch holds duplicates.  Five updates at policy_delay 2 against td3_ref
    driven by per_ref's slots and weights; then the add-on starts over with alpha = beta = 0: all weights 1, all leaves 1"""
    rng = np.random.default_rng(2)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _td3_opts(100)
    e = _td3(amd, pol, crit, opts)
    e.replay_prio_init(**PER)
    assert _collect(e, e.td3_store) == 8
    buf = e.td3_buffer()
    tree = PR.Tree(100)
    tree.fill(range(8))
    _assert_tree(e, tree, 8, "stored transitions get top")
    state = T3.fresh_state(pol, crit)
    for u in range(5):
        idx, w = e.replay_prio_batch(u)
        assert len(set(idx.tolist())) < B
        stats = e.td3_update(1)
        state, rstats = PR.td3_update(pol, state, buf, _action_norm(), 123, opts, tree, PER)
        got = e.td3_state()
        _assert_keys(got, state, T3.STATE_KEYS, u)
        assert (got["updates"], got["actor_steps"]) == (u + 1, (u + 1) // 2)
        for k in T3.STAT_KEYS:
            assert _same(np.float64(stats[k]), np.float64(rstats[k])), (k, u, stats[k], rstats[k])
        _assert_tree(e, tree, 8, u)
    assert not np.all(tree.leaf[:8] == 1), "the priorities moved"
    e.replay_prio_init(alpha=0.0, beta=0.0)
    tree = PR.Tree(100, np.ones(8, F))
    per0 = PR.options(alpha=0.0, beta=0.0)
    for u in range(5, 7):
        assert np.all(e.replay_prio_batch(u)[1] == 1)
        e.td3_update(1)
        state, _ = PR.td3_update(pol, state, buf, _action_norm(), 123, opts, tree, per0)
        _assert_keys(e.td3_state(), state, T3.STATE_KEYS, u)
        _assert_tree(e, tree, 8, u)
        assert np.all(e.replay_prio_fetch() == 1) and e.replay_prio_info()["top"] == 1
    e.close()


def test_sac_updates_equal_the_restatement(amd):
    rng = np.random.default_rng(3)
    pol, crit = _sac_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _sac_opts(100)
    e = _sac(amd, pol, crit, opts)
    e.replay_prio_init(**PER)
    assert _collect(e, e.sac_store) == 8
    buf = e.sac_buffer()
    tree = PR.Tree(100)
    tree.fill(range(8))
    state = S.fresh_state(pol, crit, opts)
    for u in range(5):
        stats = e.sac_update(1)
        state, rstats = PR.sac_update(pol, state, buf, 123, opts, tree, PER)
        got = e.sac_state()
        _assert_keys(got, state, S.STATE_KEYS, u)
        for k in S.STAT_KEYS:
            assert _same(np.float64(stats[k]), np.float64(rstats[k])), (k, u, stats[k], rstats[k])
        _assert_tree(e, tree, 8, u)
    assert not np.all(tree.leaf[:8] == 1), "the priorities moved"
    e.replay_prio_init(alpha=0.0, beta=0.0)
    tree = PR.Tree(100, np.ones(8, F))
    for u in range(5, 7):
        assert np.all(e.replay_prio_batch(u)[1] == 1)
        e.sac_update(1)
        state, _ = PR.sac_update(pol, state, buf, 123, opts, tree, PR.options(alpha=0.0, beta=0.0))
        _assert_keys(e.sac_state(), state, S.STATE_KEYS, u)
        assert np.all(e.replay_prio_fetch() == 1) and e.replay_prio_info()["top"] == 1
    e.close()


def test_a_batch_longer_than_a_tile_of_the_leaf_update(amd):
    """batch 1100 over 84 loaded rows: the leaf update's maximum over duplicates passes the batch through LDS in tiles of 1024,
    and the batch-wide minimum and maximum run over more than one round of a workgroup; two updates against the restatement"""
    rng = np.random.default_rng(15)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _td3_opts(100, batch_size=1100)
    e = _td3(amd, pol, crit, opts)
    buf = _random_buffer(rng, 84)
    e.td3_buffer_load(buf)
    e.replay_prio_init(**PER)
    tree = PR.Tree(100, np.ones(84, F))
    state = T3.fresh_state(pol, crit)
    for u in range(2):
        idx, w = e.replay_prio_batch(u)
        ridx, rw = PR.sample(tree, 123, u, 1100, 84, PER["beta"])
        assert _same(idx, ridx) and _same(w, rw), u
        e.td3_update(1)
        state, _ = PR.td3_update(pol, state, buf, _action_norm(), 123, opts, tree, PER)
        _assert_keys(e.td3_state(), state, T3.STATE_KEYS, u)
        _assert_tree(e, tree, 84, u)
    e.close()


# ---- 4. the wrap ---------------------------------------------------------------------------------------------------------------------------
def test_a_wrapping_store_gives_the_overwritten_slots_the_top_of_that_moment(amd):
    """capacity 16: two days stored (full), three updates, one more day stored: slots 0 .. 7 are overwritten and hold the top the
    updates left; the root (the tree's only node) is the restatement's; the next update is too"""
    rng = np.random.default_rng(4)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _td3_opts(16)
    e = _td3(amd, pol, crit, opts)
    e.replay_prio_init(**PER)
    assert _collect(e, e.td3_store, 2) == 16
    buf = e.td3_buffer()
    tree = PR.Tree(16)
    tree.fill(range(16))
    state = T3.fresh_state(pol, crit)
    for u in range(3):
        e.td3_update(1)
        state, _ = PR.td3_update(pol, state, buf, _action_norm(), 123, opts, tree, PER)
    _assert_tree(e, tree, 16, "before the wrap")
    top = tree.top
    assert _collect(e, e.td3_store, 1) == 8
    buf = e.td3_buffer()
    assert buf["written"] == 24 and buf["size"] == 16
    tree.fill(range(8))
    _assert_tree(e, tree, 16, "after the wrap")
    assert np.all(e.replay_prio_fetch()[:8] == top)
    e.td3_update(1)
    state, _ = PR.td3_update(pol, state, buf, _action_norm(), 123, opts, tree, PER)
    _assert_keys(e.td3_state(), state, T3.STATE_KEYS, "after the wrap")
    _assert_tree(e, tree, 16, "an update after the wrap")
    e.close()


# ---- 5., 6. populations ------------------------------------------------------------------------------------------------------------------
M, NP = 3, 9
n = NP // M
TD3_OWN = (dict(seed=0, gamma=0.9), dict(seed=77, gamma=0.99, critic_lr=1e-3), dict(seed=5, gamma=0.8, tau=0.2))
SAC_OWN = (dict(seed=0, gamma=0.9), dict(seed=77, gamma=0.99, init_alpha=0.1), dict(seed=5, gamma=0.8, tau=0.2))


def _td3_pop(amd, pols, crits, opts):
    e = _engine(amd, _planes(NP))
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    for m in range(1, M):
        e.mlp_set_learner(m, pols[m])
    e.rollout_enable(2, obs=True)
    e.td3_pop_init(opts)
    for m in range(M):
        e.td3_pop_set_critics(m, crits[m], action_norm=_action_norm() if m == 0 else None)
    return e


def _sac_pop(amd, pols, crits, opts):
    e = _engine(amd, _planes(NP))
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    for m in range(1, M):
        e.mlp_set_learner(m, pols[m])
    e.mlp_learners_set_squash(*_bounds())
    e.rollout_enable(2, obs=True)
    e.sac_pop_init(opts)
    for m in range(M):
        e.sac_pop_set_critics(m, crits[m])
    return e


def _members(rng, make_policy):
    return [make_policy(rng) for _ in range(M)], [T3.random_critics_for_tests(rng, K, WIDTHS) for _ in range(M)]


@pytest.mark.parametrize("kind", ["td3", "sac"])
def test_a_population_member_equals_a_solo_engine_on_its_envs(amd, kind):
    """M = 3 on 9 envs, two collections of one day (3 transitions per member each) with two updates after each: every member's
    state, leaves, top, total and next batch are those of a solo engine of its three envs"""
    rng = np.random.default_rng(5)
    td3 = kind == "td3"
    pols, crits = _members(rng, _td3_policy if td3 else _sac_policy)
    opts = [(_td3_opts if td3 else _sac_opts)(40, **own) for own in (TD3_OWN if td3 else SAC_OWN)]
    e = (_td3_pop if td3 else _sac_pop)(amd, pols, crits, opts)
    e.replay_prio_init(**PER)
    solos = []
    for m in range(M):
        s = (_td3 if td3 else _sac)(amd, pols[m], crits[m], opts[m], env_id_base=m * n, planes=_planes(NP)[:, TP.member_slice(m, n)])
        s.replay_prio_init(**PER)
        solos.append(s)
    keys = T3.STATE_KEYS if td3 else S.STATE_KEYS
    for rnd in range(2):
        assert _collect(e, e.td3_pop_store if td3 else e.sac_pop_store) == n
        (e.td3_pop_update if td3 else e.sac_pop_update)(2)
        for m, s in enumerate(solos):
            assert _collect(s, s.td3_store if td3 else s.sac_store) == n
            (s.td3_update if td3 else s.sac_update)(2)
            got = (e.td3_pop_state if td3 else e.sac_pop_state)(m)
            _assert_keys(got, (s.td3_state if td3 else s.sac_state)(), keys, (rnd, m))
            assert _same(e.replay_prio_fetch(m), s.replay_prio_fetch()), (rnd, m)
            assert e.replay_prio_info(m) == s.replay_prio_info(), (rnd, m)
            a, b = e.replay_prio_batch(2 * rnd + 2, m), s.replay_prio_batch(2 * rnd + 2)
            assert _same(a[0], b[0]) and _same(a[1], b[1]), (rnd, m)
    assert not _same(e.replay_prio_fetch(0), e.replay_prio_fetch(1)), "the members' priorities are their own"
    for s in solos:
        s.close()
    e.close()


@pytest.mark.parametrize("kind", ["td3", "sac"])
def test_a_member_under_replay_and_its_own_normalisers_equals_a_solo_engine(amd, kind):
    """the population test above with both running normalisers on, one per member, and moved after every store: a batch kernel then
    takes the member's slots and weights, its vectors and its multiplier in one pass.  Every member's state, normaliser state (the
    vectors and the multiplier with it), running returns, leaves, top, total and next batch are those of a solo engine of its three
    envs under the same two add-ons"""
    rng = np.random.default_rng(16)
    td3 = kind == "td3"
    fam = "td3" if td3 else "sac"
    pols, crits = _members(rng, _td3_policy if td3 else _sac_policy)
    opts = [(_td3_opts if td3 else _sac_opts)(40, **own) for own in (TD3_OWN if td3 else SAC_OWN)]
    norm = dict(observations=True, rewards=True, rew_clip=0.8)
    e = (_td3_pop if td3 else _sac_pop)(amd, pols, crits, opts)
    getattr(e, fam + "_norm_init")(per_member=True, **norm)
    e.replay_prio_init(**PER)
    solos = []
    for m in range(M):
        s = (_td3 if td3 else _sac)(amd, pols[m], crits[m], opts[m], env_id_base=m * n, planes=_planes(NP)[:, TP.member_slice(m, n)])
        getattr(s, fam + "_norm_init")(**norm)
        s.replay_prio_init(**PER)
        solos.append(s)
    keys = T3.STATE_KEYS if td3 else S.STATE_KEYS
    for rnd in range(2):
        assert _collect(e, getattr(e, fam + "_pop_store")) == n
        assert getattr(e, fam + "_norm_update")() == n
        getattr(e, fam + "_pop_update")(2)
        returns = getattr(e, fam + "_norm_returns")()
        for m, s in enumerate(solos):
            assert _collect(s, getattr(s, fam + "_store")) == n
            assert getattr(s, fam + "_norm_update")() == n
            getattr(s, fam + "_update")(2)
            _assert_keys(getattr(e, fam + "_pop_state")(m), getattr(s, fam + "_state")(), keys, (rnd, m))
            got, ref = getattr(e, fam + "_norm_state")(m), getattr(s, fam + "_norm_state")()
            assert set(got) == set(ref) >= {"shift", "scale", "rew_scale"}, (rnd, m)
            _assert_keys({k: np.asarray(v) for k, v in got.items()}, {k: np.asarray(v) for k, v in ref.items()}, sorted(ref), (rnd, m))
            assert _same(returns[m * n:(m + 1) * n], getattr(s, fam + "_norm_returns")()), (rnd, m)
            assert _same(e.replay_prio_fetch(m), s.replay_prio_fetch()), (rnd, m)
            assert e.replay_prio_info(m) == s.replay_prio_info(), (rnd, m)
            a, b = e.replay_prio_batch(2 * rnd + 2, m), s.replay_prio_batch(2 * rnd + 2)
            assert _same(a[0], b[0]) and _same(a[1], b[1]), (rnd, m)
    v = [getattr(e, fam + "_norm_state")(m) for m in range(M)]
    assert not _same(v[0]["shift"], v[1]["shift"]) and v[0]["rew_scale"] != v[1]["rew_scale"], "the members' normalisers are their own"
    assert not _same(v[0]["shift"], pols[0].shift), "the vectors moved"
    assert not _same(e.replay_prio_fetch(0), e.replay_prio_fetch(1)), "the members' priorities are their own"
    for s in solos:
        s.close()
    e.close()


@pytest.mark.parametrize("kind", ["td3", "sac"])
def test_copies_carry_the_tree_with_the_ring_and_only_with_it(amd, kind):
    """*_pop_copy without the ring leaves the destination's leaves, total and top alone; with it they are the donor's, and the
    destination's next batch is the restatement's on the donor's leaves under its own key; a PBT exploit with rings does the same"""
    rng = np.random.default_rng(6)
    td3 = kind == "td3"
    pols, crits = _members(rng, _td3_policy if td3 else _sac_policy)
    own = TD3_OWN if td3 else SAC_OWN
    opts = [(_td3_opts if td3 else _sac_opts)(40, **o) for o in own]
    e = (_td3_pop if td3 else _sac_pop)(amd, pols, crits, opts)
    e.replay_prio_init(**PER)
    for _ in range(2):
        _collect(e, e.td3_pop_store if td3 else e.sac_pop_store)
        (e.td3_pop_update if td3 else e.sac_pop_update)(2)
    size = 2 * n
    snap = lambda m: (e.replay_prio_fetch(m), e.replay_prio_info(m))
    before = [snap(m) for m in range(M)]
    assert not _same(before[0][0], before[1][0]) and not _same(before[0][0], before[2][0])
    copy = e.td3_pop_copy if td3 else e.sac_pop_copy
    copy(1, 0, with_ring=False)
    assert _same(snap(0)[0], before[0][0]) and snap(0)[1] == before[0][1], "without the ring the tree stays"
    copy(1, 0, with_ring=True)
    assert _same(snap(0)[0], before[1][0]) and snap(0)[1] == before[1][1], "with the ring the tree is the donor's"
    assert _same(snap(1)[0], before[1][0]) and snap(1)[1] == before[1][1] and _same(snap(2)[0], before[2][0])
    tree = PR.Tree(40, before[1][0], top=before[1][1]["top"])
    assert _same(np.float64(tree.total), before[1][1]["total"])
    seed0 = own[0]["seed"] or SEED
    idx, w = e.replay_prio_batch(4, 0)
    ridx, rw = PR.sample(tree, seed0, 4, B, size, PER["beta"])
    assert _same(idx, ridx) and _same(w, rw)
    # one exploit round with rings: member 1 becomes member 2
    e.pbt_init(kind, replace_count=1, with_ring=True)
    e.pbt_exploit([-1, 2, -1])
    assert _same(snap(1)[0], before[2][0]) and snap(1)[1] == before[2][1], "an exploit with rings carries the tree"
    assert _same(snap(0)[0], before[1][0]) and _same(snap(2)[0], before[2][0])
    tree = PR.Tree(40, before[2][0], top=before[2][1]["top"])
    idx, w = e.replay_prio_batch(4, 1)
    ridx, rw = PR.sample(tree, own[1]["seed"], 4, B, size, PER["beta"])
    assert _same(idx, ridx) and _same(w, rw)
    (e.td3_pop_update if td3 else e.sac_pop_update)(1)                   # (the copied trees are whole: an update runs on them)
    e.close()


def test_an_exploit_without_rings_leaves_the_trees_alone(amd):
    rng = np.random.default_rng(7)
    pols, crits = _members(rng, _td3_policy)
    e = _td3_pop(amd, pols, crits, [_td3_opts(40, **o) for o in TD3_OWN])
    e.replay_prio_init(**PER)
    _collect(e, e.td3_pop_store)
    e.td3_pop_update(2)
    before = [e.replay_prio_fetch(m) for m in range(M)]
    e.pbt_init("td3", replace_count=1, with_ring=False)
    e.pbt_exploit([-1, 2, -1])
    assert all(_same(e.replay_prio_fetch(m), before[m]) for m in range(M))
    e.close()


# ---- 7., 8. a checkpoint, set_beta --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["td3", "sac"])
def test_a_checkpoint_continues_bit_for_bit(amd, kind):
    """state + ring + the fetched leaves and top into a fresh engine: its next three updates are the first engine's"""
    rng = np.random.default_rng(8)
    td3 = kind == "td3"
    pol, crit = (_td3_policy if td3 else _sac_policy)(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = (_td3_opts if td3 else _sac_opts)(100)
    make = _td3 if td3 else _sac
    a, b = make(amd, pol, crit, opts), make(amd, pol, crit, opts)
    a.replay_prio_init(**PER)
    _collect(a, a.td3_store if td3 else a.sac_store, 2)
    (a.td3_update if td3 else a.sac_update)(3)
    b.replay_prio_init(**PER)
    (b.td3_buffer_load if td3 else b.sac_buffer_load)((a.td3_buffer if td3 else a.sac_buffer)())
    (b.td3_state if td3 else b.sac_state)((a.td3_state if td3 else a.sac_state)())
    st = a.replay_prio_state()
    assert st["leaf"].shape == (16,) and not np.all(st["leaf"] == 1)
    b.replay_prio_state(0, st)
    assert b.replay_prio_info() == a.replay_prio_info()
    for u in range(3):
        sa, sb = (a.td3_update if td3 else a.sac_update)(1), (b.td3_update if td3 else b.sac_update)(1)
        assert sa == sb, u
        _assert_keys((b.td3_state if td3 else b.sac_state)(), (a.td3_state if td3 else a.sac_state)(), T3.STATE_KEYS if td3 else S.STATE_KEYS, u)
        assert _same(a.replay_prio_fetch(), b.replay_prio_fetch()) and a.replay_prio_info() == b.replay_prio_info()
    a.close()
    b.close()


def test_set_beta_takes_effect_on_the_next_update_only(amd):
    rng = np.random.default_rng(9)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    opts = _td3_opts(100)
    e = _td3(amd, pol, crit, opts)
    e.replay_prio_init(**PER)
    _collect(e, e.td3_store)
    buf = e.td3_buffer()
    tree = PR.Tree(100)
    tree.fill(range(8))
    state = T3.fresh_state(pol, crit)
    betas = (0.4, 0.4, 1.0, 0.0)
    for u, beta in enumerate(betas):
        if u >= 2:
            e.replay_prio_set_beta(beta)
        e.td3_update(1)
        state, _ = PR.td3_update(pol, state, buf, _action_norm(), 123, opts, tree, dict(PER, beta=beta))
        _assert_keys(e.td3_state(), state, T3.STATE_KEYS, u)
        _assert_tree(e, tree, 8, u)
    # a value set between two calls reaches the updates enqueued after it: two updates in one call under beta 0.7
    e.replay_prio_set_beta(0.7)
    e.td3_update(2)
    for _ in range(2):
        state, _ = PR.td3_update(pol, state, buf, _action_norm(), 123, opts, tree, dict(PER, beta=0.7))
    _assert_keys(e.td3_state(), state, T3.STATE_KEYS, "two queued updates")
    assert _same(e.replay_prio_batch(6)[1], PR.sample(tree, 123, 6, B, 8, 0.7)[1])
    e.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(amd):
    rng = np.random.default_rng(10)
    pol, crit = _td3_policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    e = _engine(amd, _planes(N))
    with pytest.raises(AssertionError):
        e.replay_prio_init()                                            # no trainer
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(2, obs=True)
    with pytest.raises(AssertionError):
        e.replay_prio_init()                                            # still none
    e.td3_init(**_td3_opts(100))
    e.td3_set_critics(crit, action_norm=_action_norm())
    for call in (lambda: e.replay_prio_set_beta(0.5), lambda: e.replay_prio_info(), lambda: e.replay_prio_fetch(0, 0, 1),
                 lambda: e.replay_prio_load(np.ones(1, F), 1.0), lambda: e.replay_prio_batch(0)):
        with pytest.raises(AssertionError):
            call()                                                      # no add-on yet
    with pytest.raises(ValueError):
        e.replay_prio_init(alpha=1.5)
    e.td3_buffer_load(_random_buffer(rng, 10))
    assert e.td3_batch_indices(0).shape == (B,)
    e.replay_prio_init(**PER)
    with pytest.raises(AssertionError):
        e.td3_batch_indices(0)                                          # the uniform law's voice
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            e.replay_prio_set_beta(bad)
    for call in (lambda: e.replay_prio_info(1), lambda: e.replay_prio_fetch(0, 5, 6), lambda: e.replay_prio_fetch(0, -1, 2),
                 lambda: e.replay_prio_load(np.ones(11, F), 1.0), lambda: e.replay_prio_load(np.ones(2, F), 1.0, slot=9),
                 lambda: e.replay_prio_load(np.array([1, 0], F), 1.0), lambda: e.replay_prio_load(np.array([1, -2], F), 1.0),
                 lambda: e.replay_prio_load(np.array([1, np.inf], F), 1.0), lambda: e.replay_prio_load(np.array([1, np.nan], F), 1.0),
                 lambda: e.replay_prio_load(np.ones(2, F), 0.0), lambda: e.replay_prio_load(np.ones(2, F), float("inf")),
                 lambda: e.replay_prio_batch(-1), lambda: e.replay_prio_batch(2 ** 32 - 1), lambda: e.replay_prio_batch(0, member=1)):
        with pytest.raises(ValueError):
            call()
    # the engine stayed usable, and a refused load changed nothing
    assert np.all(e.replay_prio_fetch() == 1) and e.replay_prio_info()["top"] == 1
    e.td3_update(1)
    # the add-on ends with its trainer
    e.td3_init(**_td3_opts(100))
    with pytest.raises(AssertionError):
        e.replay_prio_info()
    e.td3_set_critics(crit, action_norm=_action_norm())
    e.td3_buffer_load(_random_buffer(rng, 10))
    assert e.td3_batch_indices(0).shape == (B,)
    # an empty ring has no batch
    e.td3_init(**_td3_opts(100))
    e.replay_prio_init(**PER)
    with pytest.raises(AssertionError):
        e.replay_prio_batch(0)
    e.close()
    # SAC and the populations refuse their batch_indices alike
    s = _sac(amd, _sac_policy(rng), crit, _sac_opts(100))
    s.sac_buffer_load(_random_buffer(rng, 10))
    s.replay_prio_init(**PER)
    with pytest.raises(AssertionError):
        s.sac_batch_indices(0)
    s.close()
    pols, crits = _members(rng, _td3_policy)
    p = _td3_pop(amd, pols, crits, [_td3_opts(40, **o) for o in TD3_OWN])
    p.td3_pop_buffer_load(0, _random_buffer(rng, 10))
    p.replay_prio_init(**PER)
    with pytest.raises(AssertionError):
        p.td3_pop_batch_indices(0, 0)
    with pytest.raises(ValueError):
        p.replay_prio_info(M)
    # (one member's load moved every ring's size: the other members' slots are stored ones now, and have leaves)
    assert all(np.all(p.replay_prio_fetch(m) == 1) for m in range(M))
    p.close()
    pols, crits = _members(rng, _sac_policy)
    p = _sac_pop(amd, pols, crits, [_sac_opts(40, **o) for o in SAC_OWN])
    p.sac_pop_buffer_load(0, _random_buffer(rng, 10))
    p.replay_prio_init(**PER)
    with pytest.raises(AssertionError):
        p.sac_pop_batch_indices(0, 0)
    p.close()


# ---- 10. the trainers --------------------------------------------------------------------------------------------------------------------
PRIO = dict(alpha=0.7, beta=0.5, beta_final=1.0, beta_iterations=2)


def _two_iterations_and_a_round_trip(make, members=None):
    """trainers a and b start from different critics (make's argument is the critics' seed) and run the same first iteration; then
    a's state() - the priorities with it - and ring go into b, and the second iteration of both is the same bit for bit"""
    a, b = make(1), make(2)
    ms = [None] if members is None else list(range(members))
    a.iteration(budget=BUDGET)
    b.iteration(budget=BUDGET)                                          # (the same days: the collection runs before the first update)
    pop = members is not None
    ea, eb = a.engine, b.engine
    name = type(a).__name__
    kind = "td3" if "TD3" in name else "sac"
    for m in ms:
        st = a.state() if not pop else a.state(m)
        assert "replay_prio" in st and st["replay_prio"]["iterations"] == 1 and st["replay_prio"]["leaf"].size > 0
        if pop:
            getattr(eb, f"{kind}_pop_buffer_load")(m, getattr(ea, f"{kind}_pop_buffer")(m))
            b.state(m, st)
        else:
            getattr(eb, f"{kind}_buffer_load")(getattr(ea, f"{kind}_buffer")())
            b.state(st)
    sa, sb = a.iteration(budget=BUDGET), b.iteration(budget=BUDGET)
    assert sa == sb
    for m in ms:
        x, y = (a.state(), b.state()) if not pop else (a.state(m), b.state(m))
        for k in x:
            if k == "replay_prio":
                assert _same(x[k]["leaf"], y[k]["leaf"]) and _same(x[k]["top"], y[k]["top"]) and x[k]["iterations"] == y[k]["iterations"] == 2
            else:
                assert _same(np.asarray(x[k]), np.asarray(y[k])), (k, m)
        assert not np.all(x["replay_prio"]["leaf"] == 1)
    ea.close()
    eb.close()


def test_td3_trainer_with_prioritized_replay(amd):
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    pol = _td3_policy(np.random.default_rng(11))
    _two_iterations_and_a_round_trip(lambda cs: TD3Trainer(_engine(amd, _planes(N)), pol, critic_hidden=WIDTHS[:-1], horizon=2, learning_starts=8,
                                                        updates_per_iteration=3, batch_size=B, capacity=100, critic_seed=cs, prioritized_replay=PRIO))
    with pytest.raises(ValueError):
        TD3Trainer(_engine(amd, _planes(N)), pol, critic_hidden=WIDTHS[:-1], horizon=2, batch_size=B, capacity=100, prioritized_replay=dict(gamma=1))


def test_sac_trainer_with_prioritized_replay(amd):
    from adcraft_amd.baselines.sac_trainer import SACTrainer
    pol = _sac_policy(np.random.default_rng(12))
    lo, hi = _bounds()
    _two_iterations_and_a_round_trip(lambda cs: SACTrainer(_engine(amd, _planes(N)), pol, lo, hi, critic_hidden=WIDTHS[:-1], horizon=2, learning_starts=8,
                                                        updates_per_iteration=3, batch_size=B, capacity=100, critic_seed=cs, prioritized_replay=PRIO))


def test_td3_population_trainer_with_prioritized_replay(amd):
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer
    pol = _td3_policy(np.random.default_rng(13))
    cfg = dict(critic_hidden=WIDTHS[:-1], learning_starts=3, updates_per_iteration=3, batch_size=B, capacity=40)
    _two_iterations_and_a_round_trip(lambda cs: TD3PopulationTrainer(_engine(amd, _planes(NP)), pol, [0.1, 0.2, 0.3], dict(cfg, critic_seed=cs), horizon=2, members=M,
                                                                  prioritized_replay=PRIO), members=M)


def test_sac_population_trainer_with_prioritized_replay(amd):
    from adcraft_amd.baselines.sac_trainer import SACPopulationTrainer
    pol = _sac_policy(np.random.default_rng(14))
    lo, hi = _bounds()
    cfg = dict(critic_hidden=WIDTHS[:-1], learning_starts=3, updates_per_iteration=3, batch_size=B, capacity=40)
    _two_iterations_and_a_round_trip(lambda cs: SACPopulationTrainer(_engine(amd, _planes(NP)), pol, dict(cfg, critic_seed=cs), lo, hi, horizon=2, members=M,
                                                                  prioritized_replay=PRIO), members=M)
