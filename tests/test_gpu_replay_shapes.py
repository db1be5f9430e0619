"""GPU tests of the device code between the rollout record and the learner's batch at the shapes where its hand-written index
arithmetic takes another path (the shapes and their preconditions are tests/replay_shapes.py's):

1. the four forms of the replay store and their population twins at K = 256 (rows of 1282 and 2564 floats, actions of 257: every
   loop j = tid; j < D; j += 256 takes more than one pass), through auto-resets, the skip rule and a wrapping ring;
2. the prioritised-replay tree on three levels (capacity 4200) under TD3, SAC and population updates and a wrapping store;
3. the running normalisers with members, two chunks of samples and two column tiles at once (K = 52, 7 envs a member, 150 days);
4. more than one 1024-sample chunk at the wide networks W1 and W3 of tests/learner_shapes.py;
5. frames with the off-policy learners at the last K their LDS limit accepts, and the refusal one keyword further.
Every device result is compared bit for bit with the numpy restatements; every case first asserts, on the restatement alone, the
precondition that makes it able to fail, and prints what it measured.  Measured figures: profiles/pr_replay_shapes.txt."""
import copy
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import learner_shapes as W
from tests import mlp_ref as R
from tests import norm_ref as NR
from tests import nstep_ref as NS
from tests import per_ref as PR
from tests import pg_pop_ref as PP
from tests import pg_ref as P
from tests import replay_shapes as RS
from tests import rew_norm_ref as RR
from tests import sac_norm_ref as SN
from tests import sac_ref as S
from tests import stack_ref as ST
from tests import td3_norm_ref as TN
from tests import td3_pop_ref as TP
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F, D64 = np.float32, np.float64
SEED, BUDGET = 47, 1000.0
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


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


def _planes(envs, K, seed=SEED, mean_volume=24):
    return H.implicit_params(envs, K, seed + 1, mean_volume=mean_volume, cvr=0.5)


def _engine(amd, planes, env_id_base=0, seed=SEED, **kw):
    e = amd.StepEngine(planes.shape[1], planes.shape[2], seed=seed, env_id_base=env_id_base, **kw)
    e.set_all_params(planes)
    e.reset()
    return e


def _assert_keys(got, ref, keys, what=""):
    for k in keys:
        assert _same(got[k], ref[k]), (k, what)


def _assert_stats(keys, got, ref, what=""):
    for k in keys:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


def _bounds(K, step=100.0):
    """budget in [50, 1500], bids in [0.02, 3 + k / step]"""
    return np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], 3.0 + np.arange(K) / step]).astype(F)


def _stacked_norm(K, frames):
    """realistic_norm per frame, older frames a little different, so that a frame in the wrong place shows"""
    shift, scale = R.realistic_norm(K)
    return (np.concatenate([shift + F(0.25 * f) for f in range(frames)]).astype(F),
            np.concatenate([scale * F(1.0 + 0.125 * f) for f in range(frames)]).astype(F))


def _now(e):
    """(raw frame 0, episode day) an act would read now"""
    day = e.get_episode_state()[0].astype(np.int64)
    x = R.flat_obs(e.fetch()).astype(F)
    x[day == 0] = 0
    return x, day


# ======================================================================================================================================
# 1. the store at wide rows
# ======================================================================================================================================
ST_K, ST_N, ST_T, ST_C, ST_GAMMA = (RS.STORE[k] for k in ("K", "N", "T", "C", "gamma"))
ST_HIDDEN, ST_WIDTHS = (8,), (8, 1)
ST_D0, ST_A = 5 * ST_K + 2, ST_K + 1


def _store_policy(rng, family, frames):
    K = ST_K
    if family == "sac":
        pol = ST.random_policy(rng, K, frames, ST_HIDDEN, "tanh", two_heads=True, value=False, normalize=True, scale=0.6, log_std_clamp=(-1.0, -0.5))
        pol.layers[-1][1][K + 1:] = np.linspace(-1.6, 0.1, K + 1).astype(F)
    else:
        pol = ST.random_policy(rng, K, frames, ST_HIDDEN, "tanh", value=False, normalize=True, scale=0.6)
        pol.layers[-1][1][1:K + 1] += F(0.8)                       # bids around 80 cents: auctions are won, rewards are not zero
    pol.shift, pol.scale = _stacked_norm(K, frames)
    return pol


def _store_options(family, capacity=ST_C, **kw):
    common = dict(critic_widths=ST_WIDTHS, batch_size=8, capacity=capacity, tau=0.05, gamma=ST_GAMMA, reward_scale=0.5, seed=123)
    if family == "sac":
        return S.options(ST_K, **dict(dict(common, init_alpha=0.3), **kw))
    return T3.options(**dict(dict(common, policy_delay=1, target_noise=0.3, target_noise_clip=0.25), **kw))


def _store_engine(amd, family, pol, crit, opts, planes, env_id_base=0):
    e = _engine(amd, planes, env_id_base, **RS.RESETS)
    e.mlp_init(pol, deterministic=False)
    if family == "sac":
        e.mlp_set_squash(*_bounds(ST_K))
    e.rollout_enable(ST_T, obs=True)
    getattr(e, family + "_init")(**opts)
    getattr(e, family + "_set_critics")(crit)
    return e


def _assert_ring(buf, gn, ring, n, what):
    ref = ring.buffer()
    assert (buf["size"], buf["written"]) == (ref["size"], ref["written"]), what
    _assert_keys(buf, ref, ("x", "a", "r", "done", "x2"), what)
    if n is not None:
        assert _same(gn, ref["gn"]), ("gn", what)


@pytest.mark.parametrize("family,frames,n", [("td3", 1, None), ("td3", 1, 3), ("td3", 2, None), ("td3", 2, 3), ("sac", 2, 3)],
                         ids=["plain", "nstep", "frames", "frames-nstep", "sac-frames-nstep"])
def test_store_at_wide_rows_equals_the_restatement(amd, family, frames, n):
    """K = 256, 6 envs, 5 days, capacity 17, max_days 4 with auto-reset.  The first store of 30 samples is longer than the ring (the
    13 samples with s + C < count are skipped), the second wraps from written = 30.  After each, x, a, r, done, x2, gn, size and
    written are the restatement's ring built from the fetched record (the stacked record with frames) and the row an act would
    read now (the peeked stacked row of stack_ref.History)"""
    case = f"store {family} frames={frames} n={n}"
    D = frames * ST_D0
    rng = np.random.default_rng(1)
    pol = _store_policy(rng, family, frames)
    crit = ST.random_critics(rng, ST_K, frames, ST_WIDTHS)
    e = _store_engine(amd, family, pol, crit, _store_options(family), _planes(ST_N, ST_K))
    if n is not None:
        e.replay_nstep_init(n)
    ring = T3.Ring(ST_C, D, ST_A) if n is None else NS.Ring(ST_C, D, ST_A, n, ST_GAMMA)
    hist = ST.History(ST_N, ST_K, frames)
    for rnd in range(2):
        e.rollout_reset()
        for _ in range(ST_T):
            hist.row(*_now(e))
            e.mlp_step(BUDGET)
        assert getattr(e, family + "_store")() == ST_T * ST_N
        rec = e.rollout_fetch()
        raw = hist.row(*_now(e), commit=False)
        assert rec["obs"].shape == (ST_T, ST_N, D) and raw.shape == (ST_N, D)
        RS.store_windows(f"{case} round {rnd}", rec, n or 1)
        if frames > 1 and rnd == 1:                                 # (round 0 ends on an episode's second day: its older frame is the zero row)
            RS.store_peek(f"{case} round {rnd}", raw, ST_D0)
        ring.store(rec, ST.normalized(pol, raw))
        RS.store_columns(f"{case} round {rnd}", ring.buffer(), D, first_store=rnd == 0)
        buf = getattr(e, family + "_buffer")()
        _assert_ring(buf, e.replay_nstep_fetch() if n is not None else None, ring, n, (case, rnd))
        assert (buf["size"], buf["written"]) == (ST_C, (rnd + 1) * ST_T * ST_N)
    e.close()


def test_population_store_at_wide_rows_equals_solo_engines_and_the_restatement(amd):
    """M = 2 learners over the same 6 envs (3 each) with their own gammas, n = 3, capacity 11 < the 15 samples of a member's store:
    after each of two stores every member's ring and gn are those of a solo engine on its envs at env_id_base = 3 m, and the
    restatement's built from the member's slice of the population's record"""
    M, n_envs, C_, nstep = 2, ST_N // 2, 11, RS.STORE["n"]
    rng = np.random.default_rng(7)
    pols = [_store_policy(rng, "td3", 1) for _ in range(M)]
    crits = [T3.random_critics_for_tests(rng, ST_K, ST_WIDTHS) for _ in range(M)]
    gammas = (0.9, 0.97)
    opts = [_store_options("td3", C_, gamma=gammas[m], seed=(0, 77)[m]) for m in range(M)]
    planes = _planes(ST_N, ST_K)
    e = _engine(amd, planes, **RS.RESETS)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    e.mlp_set_learner(1, pols[1])
    e.rollout_enable(ST_T, obs=True)
    e.td3_pop_init(opts)
    for m in range(M):
        e.td3_pop_set_critics(m, crits[m])
    e.replay_nstep_init(nstep)
    solos = []
    for m in range(M):
        s = _store_engine(amd, "td3", pols[m], crits[m], opts[m], planes[:, TP.member_slice(m, n_envs)], env_id_base=m * n_envs)
        s.replay_nstep_init(nstep)
        solos.append(s)
    rings = [NS.Ring(C_, ST_D0, ST_A, nstep, gammas[m]) for m in range(M)]
    for rnd in range(2):
        e.rollout_reset()
        e.run_days("mlp", ST_T, BUDGET)
        assert e.td3_pop_store() == ST_T * n_envs
        rec = e.rollout_fetch()
        out, first = e.fetch(), e.get_episode_state()[0] == 0
        for m, s in enumerate(solos):
            case = f"store population member {m} round {rnd}"
            sl = TP.member_slice(m, n_envs)
            mrec = TP.member_record(rec, m, n_envs)
            RS.store_windows(case, mrec, nstep, gammas[m])
            rings[m].store(mrec, T3.current_input(pols[m], out, first)[sl])
            RS.store_columns(case, rings[m].buffer(), ST_D0, first_store=rnd == 0)
            got = e.td3_pop_buffer(m)
            _assert_ring(got, e.replay_nstep_fetch(m), rings[m], nstep, case)
            s.rollout_reset()
            s.run_days("mlp", ST_T, BUDGET)
            assert s.td3_store() == ST_T * n_envs
            _assert_keys(got, s.td3_buffer(), ("x", "a", "r", "done", "x2"), case)
            assert _same(e.replay_nstep_fetch(m), s.replay_nstep_fetch()), case
    assert not _same(e.replay_nstep_fetch(0), e.replay_nstep_fetch(1)), "every member discounts by its own gamma"
    for s in solos:
        s.close()
    e.close()


# ======================================================================================================================================
# 2. a three-level tree under updates
# ======================================================================================================================================
TR_K, TR_HIDDEN, TR_WIDTHS = 3, (8,), (8, 8, 1)
TR_D, TR_A = 5 * TR_K + 2, TR_K + 1
TR_C, TR_B, TR_TOP = RS.TREE["C"], RS.TREE["B"], RS.TREE["top"]
PER = PR.options()


def _tr_td3_policy(rng):
    pol = R.random_policy(rng, TR_K, TR_HIDDEN, "tanh", normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(TR_K)
    return pol


def _tr_sac_policy(rng):
    pol = S.sac_policy(rng, TR_K, TR_HIDDEN, "tanh", clamp=(-1.0, -0.5), normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(TR_K)
    return pol


def _tr_action_norm():
    return np.full(TR_A, 0.25, F), np.full(TR_A, 1.5, F)


def _tr_td3_opts(**kw):
    return T3.options(**dict(dict(critic_widths=TR_WIDTHS, batch_size=TR_B, capacity=TR_C, policy_delay=2, tau=0.05, target_noise=0.3, target_noise_clip=0.25,
                                  gamma=0.9, reward_scale=0.5, critic_lr=3e-3, seed=123), **kw))


def _tr_sac_opts(**kw):
    return S.options(TR_K, **dict(dict(critic_widths=TR_WIDTHS, batch_size=TR_B, capacity=TR_C, tau=0.05, gamma=0.9, reward_scale=0.5, init_alpha=0.3,
                                       critic_lr=3e-3, seed=123), **kw))


def _tr_buffer(rng, size):
    return dict(x=(rng.standard_normal((size, TR_D)) * 0.7).astype(F), a=(rng.standard_normal((size, TR_A)) * 0.5 + 0.4).astype(F),
                r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, TR_D)) * 0.7).astype(F))


def _assert_tree(e, tree, size, what="", member=0):
    info = e.replay_prio_info(member)
    assert _same(e.replay_prio_fetch(member), tree.leaf[:size]), ("leaf", what)
    assert _same(info["top"], F(tree.top)), ("top", what, info["top"], tree.top)
    assert _same(info["total"], np.float64(tree.total)), ("total", what, info["total"], tree.total)


def _assert_next_batch(e, tree, seed, update, size, case, member=0):
    """the batch update number `update` would draw: its precondition on the restatement, then the device's slots and weights"""
    ridx, rw = PR.sample(tree, seed, update, TR_B, size, PER["beta"])
    RS.tree_batch(f"{case} batch {update}", ridx)
    idx, w = e.replay_prio_batch(update, member)
    assert _same(idx, ridx) and _same(w, rw), (case, update)
    return ridx


@pytest.mark.parametrize("family,updates", [("td3", 3), ("sac", 2)])
def test_solo_updates_on_a_three_level_tree_equal_the_restatement(amd, family, updates):
    """4200 loaded rows, leaves over three decades with the slots from 4096 on raised, batch 300: after every update (TD3 at
    policy_delay 2) the state, the statistics, the leaves, top, total and the next batch's slots and weights are per_ref's"""
    td3 = family == "td3"
    assert RS.tree_shape(TR_C) == [4200, 66, 2, 1]
    rng = np.random.default_rng(2 + td3)
    pol, crit = (_tr_td3_policy if td3 else _tr_sac_policy)(rng), T3.random_critics_for_tests(rng, TR_K, TR_WIDTHS)
    opts = (_tr_td3_opts if td3 else _tr_sac_opts)()
    buf = _tr_buffer(rng, TR_C)
    leaf = RS.tree_leaves(20 + td3)
    tree = PR.Tree(TR_C, leaf, top=TR_TOP)
    e = _engine(amd, _planes(8, TR_K), **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    if not td3:
        e.mlp_set_squash(*_bounds(TR_K, 10.0))
    e.rollout_enable(2, obs=True)
    if td3:
        e.td3_init(**opts)
        e.td3_set_critics(crit, action_norm=_tr_action_norm())
    else:
        e.sac_init(**opts)
        e.sac_set_critics(crit)
    getattr(e, family + "_buffer_load")(buf)
    e.replay_prio_init(**PER)
    _assert_tree(e, PR.Tree(TR_C, np.ones(TR_C, F)), TR_C, "a loaded ring starts at leaf 1")
    e.replay_prio_load(leaf, TR_TOP)
    _assert_tree(e, tree, TR_C, "loaded leaves")
    state = T3.fresh_state(pol, crit) if td3 else S.fresh_state(pol, crit, opts)
    case = f"tree {family}"
    _assert_next_batch(e, tree, 123, 0, TR_C, case)
    for u in range(updates):
        stats = getattr(e, family + "_update")(1)
        if td3:
            state, rstats = PR.td3_update(pol, state, buf, _tr_action_norm(), 123, opts, tree, PER)
        else:
            state, rstats = PR.sac_update(pol, state, buf, 123, opts, tree, PER)
        _assert_keys(getattr(e, family + "_state")(), state, T3.STATE_KEYS if td3 else S.STATE_KEYS, u)
        _assert_stats(T3.STAT_KEYS if td3 else S.STAT_KEYS, stats, rstats, u)
        _assert_tree(e, tree, TR_C, u)
        _assert_next_batch(e, tree, 123, u + 1, TR_C, case)
    assert not _same(tree.leaf[:TR_C], leaf), "the priorities moved"
    if td3:
        assert state["actor_steps"] == updates // 2
    e.close()


def test_population_updates_on_three_level_trees_equal_the_restatement(amd):
    """two TD3 learners on loaded rings of 4200 rows with different leaves: after each of two updates every member's state, leaves,
    top, total and next batch are the restatement's under its own key and options"""
    M = 2
    rng = np.random.default_rng(5)
    pols = [_tr_td3_policy(rng) for _ in range(M)]
    crits = [T3.random_critics_for_tests(rng, TR_K, TR_WIDTHS) for _ in range(M)]
    opts = [_tr_td3_opts(seed=0, gamma=0.9), _tr_td3_opts(seed=77, gamma=0.99, critic_lr=1e-3)]
    seeds = [TP.member_seed(o, SEED) for o in opts]
    norm = _tr_action_norm()                                       # (the population's: member 0 sets it, None leaves it alone)
    bufs = [_tr_buffer(rng, TR_C) for _ in range(M)]
    leaves = [RS.tree_leaves(30 + m) for m in range(M)]
    trees = [PR.Tree(TR_C, leaves[m], top=TR_TOP) for m in range(M)]
    first = [PR.sample(trees[m], seeds[m], 0, TR_B, TR_C, PER["beta"])[0] for m in range(M)]
    assert not _same(first[0], first[1]), "the members' batches were meant to differ"
    e = _engine(amd, _planes(8, TR_K), **NO_RESETS)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    e.mlp_set_learner(1, pols[1])
    e.rollout_enable(2, obs=True)
    e.td3_pop_init(opts)
    for m in range(M):
        e.td3_pop_set_critics(m, crits[m], action_norm=norm if m == 0 else None)
        e.td3_pop_buffer_load(m, bufs[m])
    e.replay_prio_init(**PER)
    for m in range(M):
        e.replay_prio_load(leaves[m], TR_TOP, member=m)
        _assert_tree(e, trees[m], TR_C, ("loaded leaves", m), m)
        _assert_next_batch(e, trees[m], seeds[m], 0, TR_C, f"tree population member {m}", m)
    states = [T3.fresh_state(pols[m], crits[m]) for m in range(M)]
    for u in range(2):
        stats = e.td3_pop_update(1)
        for m in range(M):
            states[m], rstats = PR.td3_update(pols[m], states[m], bufs[m], norm, seeds[m], opts[m], trees[m], PER)
            _assert_keys(e.td3_pop_state(m), states[m], T3.STATE_KEYS, (u, m))
            _assert_stats(T3.STAT_KEYS, stats[m], rstats, (u, m))
            _assert_tree(e, trees[m], TR_C, (u, m), m)
            _assert_next_batch(e, trees[m], seeds[m], u + 1, TR_C, f"tree population member {m}", m)
    assert not _same(trees[0].leaf, trees[1].leaf) and states[0]["actor_steps"] == 1
    e.close()


def test_a_wrapping_store_on_three_levels(amd):
    """4190 rows loaded, then one day of 16 envs stored: the slots 4190 .. 4199 and 0 .. 5 get top - two ranges under different
    level-1 and level-2 nodes.  Leaves, top, total and the next batch are the restatement's, and so is an update on the wrapped ring"""
    envs, loaded = 16, 4190
    rng = np.random.default_rng(6)
    pol, crit = _tr_td3_policy(rng), T3.random_critics_for_tests(rng, TR_K, TR_WIDTHS)
    opts = _tr_td3_opts()
    leaf = RS.tree_leaves(40, size=loaded)
    slots = [(loaded + s) % TR_C for s in range(envs)]
    assert slots[:10] == list(range(4190, 4200)) and slots[10:] == list(range(6))
    assert len({s >> 6 for s in slots}) == 2 and len({s >> 12 for s in slots}) == 2
    e = _engine(amd, _planes(envs, TR_K), **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(2, obs=True)
    e.td3_init(**opts)
    e.td3_set_critics(crit, action_norm=_tr_action_norm())
    e.td3_buffer_load(_tr_buffer(rng, loaded))
    e.replay_prio_init(**PER)
    e.replay_prio_load(leaf, TR_TOP)
    tree = PR.Tree(TR_C, leaf, top=TR_TOP)
    _assert_tree(e, tree, loaded, "before the wrap")
    e.run_days("mlp", 1, BUDGET)
    assert e.td3_store() == envs
    buf = e.td3_buffer()
    assert (buf["size"], buf["written"]) == (TR_C, loaded + envs)
    tree.fill(slots)
    _assert_tree(e, tree, TR_C, "after the wrap")
    assert np.all(e.replay_prio_fetch()[slots] == F(TR_TOP))
    _assert_next_batch(e, tree, 123, 0, TR_C, "tree wrapping store")
    e.td3_update(1)
    state, _ = PR.td3_update(pol, T3.fresh_state(pol, crit), buf, _tr_action_norm(), 123, opts, tree, PER)
    _assert_keys(e.td3_state(), state, T3.STATE_KEYS, "an update after the wrap")
    _assert_tree(e, tree, TR_C, "an update after the wrap")
    _assert_next_batch(e, tree, 123, 1, TR_C, "tree wrapping store")
    e.close()


# ======================================================================================================================================
# 3. the normalisers with members, chunks and column tiles at once
# ======================================================================================================================================
NM_K, NM_n, NM_T = (RS.NORM[k] for k in ("K", "n", "T"))
NM_D, NM_A, NM_S, NM_COLS = 5 * NM_K + 2, NM_K + 1, NM_n * NM_T, list(RS.NORM["cols"])
NM_RESETS = dict(max_days=7, auto_reset=True)                  # (first-day rows are among the samples)


def _columns(state, cols=NM_COLS):
    return dict(count=state["count"], **{k: np.ascontiguousarray(state[k][cols]) for k in ("mean", "M2", "shift", "scale")})


def _assert_obs_state(got, start, rows, update, twin, lib, what):
    """a member's observation state in full against the host twin and the numpy restatement, and the four columns against the
    restatement run on those columns alone"""
    assert NR.same(got, twin(lib, start, rows)), ("twin", what)
    assert NR.same(got, update(start, rows)), ("restatement", what)
    part = update(_columns(start), rows[:, NM_COLS])
    for k in ("mean", "M2", "shift", "scale"):
        assert _same(np.ascontiguousarray(got[k][NM_COLS]), part[k]), (k, what)
    assert got["count"] == part["count"] == rows.shape[0]


def _nm_pg_policy(rng, vary):
    pol = R.random_policy(rng, NM_K, (12,), "tanh", value=True, normalize=True, scale=0.6)
    shift, scale = R.realistic_norm(NM_K)
    if vary:
        shift = (shift + rng.standard_normal(shift.size).astype(F) * F(vary)).astype(F)
        scale = (scale * np.exp(rng.standard_normal(scale.size) * vary).astype(F)).astype(F)
    pol.shift, pol.scale = shift, scale
    return pol


def test_ppo_normalisers_with_three_members_two_chunks_and_two_tiles(amd, lib):
    """M = 3 learners x 7 envs x 52 keywords x 150 days, per-member observation and reward normalisers in one engine: S = 1050 a
    member (chunks of 1024 and 26, the second starting at env 2 of a day), D = 262 (tiles of 256 and 6).  After one update every
    member's observation state is the twin's and norm_ref.update's, its reward state rew_norm_ref's, and the next act reads the
    new vectors"""
    M, N = 3, 3 * NM_n
    rng = np.random.default_rng(303)
    pols = [_nm_pg_policy(rng, 0.2 * (m > 0)) for m in range(M)]
    configs = [dict(gamma=float(F(g)), lam=0.9) for g in (0.8, 0.9, 0.99)]
    assert RS.norm_shape("norm ppo", NM_S, NM_D, NM_n) == [1024, 26]
    e = _engine(amd, _planes(N, NM_K, seed=43), seed=43, **NM_RESETS)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    for m in range(M):
        e.mlp_set_learner(m, pols[m])
    e.rollout_enable(NM_T, obs=True)
    e.pg_pop_init(configs)
    e.obs_norm_init(per_member=True)
    e.rew_norm_init(per_member=True)
    for m in range(M):
        st = e.obs_norm_state(m)
        st["shift"], st["scale"] = pols[m].shift, pols[m].scale
        e.obs_norm_state(m, st)
    e.run_days("mlp", NM_T, BUDGET)
    e.obs_norm_update()
    e.rew_norm_update()
    rec = e.rollout_fetch()
    done = rec["terminated"] | rec["truncated"]
    assert done.any() and not done.all(), "the record was meant to cross auto-resets"
    states = [e.obs_norm_state(m) for m in range(M)]
    RS.norm_moved("norm ppo observations", states, [p.scale for p in pols])
    carry = e.rew_norm_returns()
    rews = []
    for m in range(M):
        rows = NR.member_rows(rec["obs"], m, NM_n)
        assert rows.shape == (NM_S, NM_D)
        _assert_obs_state(states[m], NR.fresh(NM_D, pols[m].shift, pols[m].scale), rows, NR.update, NR.twin, lib, m)
        got = dict(e.rew_norm_state(m), returns=carry[m * NM_n:(m + 1) * NM_n].copy())
        days = RR.member_days(rec, m, NM_n)
        assert RR.same(got, RR.update(RR.fresh(NM_n), *days, F(configs[m]["gamma"]))), ("rewards, the restatement", m)
        assert RR.same(got, RR.twin(lib, RR.fresh(NM_n), *days, F(configs[m]["gamma"]))), ("rewards, the twin", m)
        rews.append(got)
    RS.log("norm ppo rewards", scales=[float(r["scale"]) for r in rews], counts=[int(r["count"]) for r in rews])
    assert len({float(r["scale"]) for r in rews}) == M and all(r["scale"] != F(1.0) and r["count"] == NM_S for r in rews)
    # the next act runs under the new vectors
    out = e.fetch()
    obs = R.flat_obs(out)
    obs[np.asarray(out["terminated"], bool) | np.asarray(out["truncated"], bool)] = 0.0       # (auto-reset: the reset observation)
    e.mlp_set_deterministic(True)
    e.mlp_act(BUDGET)
    last = e.mlp_last()
    for env in range(N):
        pol = copy.copy(pols[env // NM_n])
        pol.shift, pol.scale = states[env // NM_n]["shift"], states[env // NM_n]["scale"]
        ref = R.twin_act(lib, pol, obs[env], deterministic=True)
        assert _same(last["mean"][env], ref["mean"][0]) and _same(last["value"][env], ref["value"][0]), env
    e.close()


def _nm_off_policy(rng, family, sigma):
    if family == "sac":
        pol = S.sac_policy(rng, NM_K, (8,), "tanh", clamp=(-1.0, -0.5), normalize=True, scale=0.6)
    else:
        pol = R.random_policy(rng, NM_K, (8,), "tanh", normalize=True, scale=0.6)
        pol.log_std = np.full(NM_K + 1, np.log(sigma), F)
    pol.shift, pol.scale = R.realistic_norm(NM_K)
    return pol


@pytest.mark.parametrize("family", ["td3", "sac"])
def test_offpolicy_normalisers_with_two_members_two_chunks_and_two_tiles(amd, lib, family):
    """populations of two x 7 envs x 52 keywords x 150 days under per-member observation and reward normalisers: store, normaliser
    update, two learner updates.  Every member's normaliser states are the twins' and the restatement's on its raw rows; its
    learner state and statistics are the restatement's under its current vectors and multiplier - the batch kernels read
    n_shift[member * n_stride + j] with member 1 and j >= 256"""
    td3 = family == "td3"
    M, N, widths, cap, clip = 2, 2 * NM_n, (8, 8, 1), 1100, 10.0
    rng = np.random.default_rng(25 + td3)
    pols = [_nm_off_policy(rng, family, (0.2, 0.05)[m]) for m in range(M)]
    crits = [T3.random_critics_for_tests(rng, NM_K, widths) for _ in range(M)]
    gammas = [F(0.97), F(0.9)]
    own = [dict(seed=0), dict(seed=77)]
    common = dict(critic_widths=widths, batch_size=16, capacity=cap, tau=0.05, reward_scale=0.5, actor_lr=3e-3, critic_lr=3e-3)
    if td3:
        opts = [T3.options(**dict(common, policy_delay=1, target_noise=0.3, target_noise_clip=0.25, gamma=float(gammas[m]), **own[m])) for m in range(M)]
    else:
        opts = [S.options(NM_K, **dict(common, init_alpha=0.3, alpha_lr=3e-3, gamma=float(gammas[m]), **own[m])) for m in range(M)]
    assert RS.norm_shape(f"norm {family}", NM_S, NM_D, NM_n) == [1024, 26] and cap >= NM_S
    e = _engine(amd, _planes(N, NM_K, seed=41), seed=41, **RS.RESETS)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    e.mlp_set_learner(1, pols[1])
    if not td3:
        e.mlp_learners_set_squash(*_bounds(NM_K))
    e.rollout_enable(NM_T, obs=True)
    getattr(e, family + "_pop_init")(opts)
    for m in range(M):
        getattr(e, family + "_pop_set_critics")(m, crits[m])
    getattr(e, family + "_norm_init")(observations=True, rewards=True, per_member=True, rew_clip=clip)
    e.run_days("mlp", NM_T, BUDGET)
    assert getattr(e, family + "_pop_store")() == NM_S
    assert getattr(e, family + "_norm_update")() == NM_S
    rec = e.rollout_fetch()
    done = rec["terminated"] | rec["truncated"]
    assert done.any() and not done.all() and (rec["obs"][0] == 0).all() and np.abs(rec["obs"]).max() > 10.0, "raw rows through auto-resets"
    returns = getattr(e, family + "_norm_returns")()
    norms = []
    for m in range(M):
        st = getattr(e, family + "_norm_state")(m)
        st["returns"] = returns[m * NM_n:(m + 1) * NM_n].copy()
        o, r = TN.split(st)
        rows = NR.member_rows(rec["obs"], m, NM_n)
        _assert_obs_state(o, TN.obs_fresh(NM_D, pols[m].shift, pols[m].scale), rows, TN.obs_update, TN.twin_obs, lib, (family, m))
        rew = tuple(np.ascontiguousarray(rec[k][:, m * NM_n:(m + 1) * NM_n]) for k in ("reward", "terminated", "truncated"))
        assert TN.rew_same(r, TN.rew_update(TN.rew_fresh(NM_n), *rew, gammas[m])), ("rewards, the restatement", m)
        assert TN.rew_same(r, TN.twin_rew(lib, TN.rew_fresh(NM_n), *rew, gammas[m])), ("rewards, the twin", m)
        norms.append((o, r))
    RS.norm_moved(f"norm {family} observations", [o for o, _ in norms], [p.scale for p in pols])
    assert norms[0][1]["scale"] != norms[1][1]["scale"] and all(r["scale"] != F(1.0) for _, r in norms)
    bufs = [getattr(e, family + "_pop_buffer")(m) for m in range(M)]
    for m in range(M):
        assert bufs[m]["size"] == NM_S and _same(bufs[m]["x"], NR.member_rows(rec["obs"], m, NM_n)), "the ring holds the member's raw rows"
    states = [T3.fresh_state(pols[m], crits[m]) if td3 else S.fresh_state(pols[m], crits[m], opts[m]) for m in range(M)]
    for u in range(2):
        stats = getattr(e, family + "_pop_update")(1)
        for m in range(M):
            (o, r), seed = norms[m], TP.member_seed(opts[m], 41)
            if td3:
                states[m], rstats, _ = TN.update(pols[m], states[m], bufs[m], None, seed, opts[m], (o["shift"], o["scale"]), r["scale"], clip)
            else:
                states[m], rstats, _ = SN.update(pols[m], states[m], bufs[m], seed, opts[m], (o["shift"], o["scale"]), r["scale"], clip)
            _assert_keys(getattr(e, family + "_pop_state")(m), states[m], T3.STATE_KEYS if td3 else S.STATE_KEYS, (u, m))
            _assert_stats(T3.STAT_KEYS if td3 else S.STAT_KEYS, stats[m], rstats, (u, m))
    assert not _same(states[0]["theta"], states[1]["theta"])
    e.close()


# ======================================================================================================================================
# 4. more than one chunk at wide shapes
# ======================================================================================================================================
def _normed(pol, K):
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _pg_fresh(pol):
    theta = P.flat_params(pol)
    return dict(theta=theta, m=np.zeros_like(theta), v=np.zeros_like(theta), steps=0)


def _assert_pg(e_state, stats, state, rstats, what):
    _assert_keys(e_state, state, ("theta", "m", "v"), what)
    assert e_state["steps"] == state["steps"], what
    _assert_stats(P.STAT_KEYS, stats, rstats, what)


def test_ppo_minibatches_of_more_than_one_chunk_at_w1(amd):
    """W1 on 220 envs x 5 days: pg_minibatch(0, 220) is 1100 samples - a second chunk of one whole slab of 64 and 12 samples;
    pg_minibatch(3, 205) is 1025 - a second chunk of one sample.  State and statistics equal the restatement after each"""
    name, envs, T, seed = "W1", 220, 5, 111
    K = W.SHAPES[name]["K"]
    rng = np.random.default_rng(seed)
    pol = _normed(W.pg_policy(rng, name, normalize=True), K)
    opts = P.options(ent_coef=0.01, vf_coef=1.0)
    e = _engine(amd, _planes(envs, K, seed, mean_volume=4), seed=seed, **NO_RESETS)
    e.mlp_init(pol, rng.integers(0, 2 ** 63, envs).astype(np.uint64), deterministic=False)
    e.rollout_enable(T, obs=True)
    e.pg_init(**opts)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch(bootstrap=True)
    adv, ret = e.pg_advantages(fetch=True)
    radv, rret = P.gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], rec["bootstrap_value"], **opts)
    assert _same(adv, radv) and _same(ret, rret)
    state = _pg_fresh(pol)
    for n0, B in ((0, 220), (3, 205)):
        samples = T * B
        RS.log(f"chunks ppo {name} pg_minibatch({n0}, {B})", S=samples, chunk_sizes=RS.chunk_sizes(samples), slabs_of_the_last_chunk=[64] * (RS.chunk_sizes(samples)[-1] // 64)
               + [RS.chunk_sizes(samples)[-1] % 64])
        assert len(RS.chunk_sizes(samples)) == 2
        flat = lambda a: np.ascontiguousarray(a[:, n0:n0 + B]).reshape((-1,) + a.shape[2:])
        g, _, rstats = P.grad(pol, state["theta"], flat(rec["obs"]), flat(rec["action"]), flat(rec["logp"]), flat(adv), flat(ret), flat(rec["value"]), **opts)
        W.assert_terms_alive(g, W.pg_terms(pol), (name, n0, B))
        theta, m, v = P.step(state["theta"], state["m"], state["v"], g, state["steps"], **opts)      # (pg_ref.minibatch's two lines, the gradient kept)
        state = dict(theta=theta, m=m, v=v, steps=state["steps"] + 1)
        stats = e.pg_minibatch(n0, B)
        _assert_pg(e.pg_state(), stats, state, rstats, (n0, B))
        assert stats["samples"] == samples
    e.close()


def test_ppo_population_of_more_than_one_chunk_at_w3(amd):
    """two W3 learners x 206 envs x 5 days: S = 1030 a member, a second chunk of 6 samples behind the other member's partials"""
    name, M, n, T, seed = "W3", 2, 206, 5, 13
    K = W.SHAPES[name]["K"]
    rng = np.random.default_rng(seed)
    pols = [_normed(W.pg_policy(rng, name, normalize=True), K) for _ in range(M)]
    opts = P.options(lr=1e-3, vf_coef=1.0, ent_coef=0.01)
    RS.log(f"chunks ppo population {name}", S=T * n, chunk_sizes=RS.chunk_sizes(T * n))
    assert len(RS.chunk_sizes(T * n)) == 2
    e = _engine(amd, _planes(M * n, K, seed, mean_volume=4), seed=seed, **NO_RESETS)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    e.mlp_set_learner(1, pols[1])
    e.rollout_enable(T, obs=True)
    e.pg_pop_init(opts)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch()
    rec["bootstrap_value"] = np.zeros(M * n, F)                     # (without a value network every value is +0)
    stats = e.pg_pop_update(1)
    for m in range(M):
        state, rstats = PP.member_update(pols[m], PP.fresh_state(pols[m]), rec, m, n, 1, opts)
        _assert_pg(e.pg_pop_state(m), stats[m], state, rstats, m)
        assert _same(e.mlp_learner_params(m), state["theta"]), m
    assert not _same(e.pg_pop_state(0)["theta"], e.pg_pop_state(1)["theta"])
    e.close()


def _wide_buffer(rng, K, size, a_scale, a_shift):
    D, A = 5 * K + 2, K + 1
    return dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * a_scale + a_shift).astype(F),
                r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))


@pytest.mark.parametrize("family,name", [("td3", "W1"), ("sac", "W3")])
def test_offpolicy_batch_of_more_than_one_chunk(amd, family, name):
    """batch 1030 over a loaded ring of 1100 rows: one update with the actor step against the restatement; the weight gradients'
    second chunk holds 6 samples"""
    td3 = family == "td3"
    K, batch, size, seed = W.SHAPES[name]["K"], 1030, 1100, 61 + td3
    rng = np.random.default_rng(seed)
    RS.log(f"chunks {family} {name}", batch=batch, chunk_sizes=RS.chunk_sizes(batch), ring=size)
    assert len(RS.chunk_sizes(batch)) == 2
    crit = W.critics(rng, name)
    e = _engine(amd, _planes(2, K, seed, mean_volume=4), seed=seed, **NO_RESETS)
    if td3:
        pol = _normed(W.td3_policy(rng, name, normalize=True), K)
        norm = (np.full(K + 1, 0.25, F), np.full(K + 1, 1.5, F))
        opts = T3.options(critic_widths=W.SHAPES[name]["critics"], batch_size=batch, capacity=size, seed=seed, policy_delay=1, tau=0.05, gamma=0.9,
                          reward_scale=0.05, target_noise=0.3, target_noise_clip=0.25)
        buf = _wide_buffer(rng, K, size, 0.5, 0.4)
        e.mlp_init(pol, deterministic=False)
        e.rollout_enable(1, obs=True)
        e.td3_init(**opts)
        e.td3_set_critics(crit, action_norm=norm)
        e.td3_buffer_load(buf)
        stats = e.td3_update(1)
        state, rstats = T3.update(pol, T3.fresh_state(pol, crit), buf, norm, seed, opts)
        _assert_keys(e.td3_state(), state, T3.STATE_KEYS)
        _assert_stats(T3.STAT_KEYS, stats, rstats)
        assert state["actor_steps"] == 1 and stats["samples"] == batch
    else:
        pol = _normed(W.sac_policy(rng, name, normalize=True), K)
        opts = S.options(K, critic_widths=W.SHAPES[name]["critics"], batch_size=batch, capacity=size, seed=seed, tau=0.05, gamma=0.9, reward_scale=0.01,
                         init_alpha=0.3, alpha_lr=3e-3, actor_lr=1e-3, critic_lr=1e-3)
        buf = _wide_buffer(rng, K, size, 1.5, 0.0)
        e.mlp_init(pol, deterministic=False)
        e.mlp_set_squash(*_bounds(K))
        e.rollout_enable(1, obs=True)
        e.sac_init(**opts)
        e.sac_set_critics(crit)
        e.sac_buffer_load(buf)
        stats = e.sac_update(1)
        state, rstats = S.update(pol, S.fresh_state(pol, crit, opts), buf, seed, opts)
        _assert_keys(e.sac_state(), state, S.STATE_KEYS)
        _assert_stats(S.STAT_KEYS, stats, rstats)
        assert stats["samples"] == batch
    assert np.isfinite(state["theta"]).all() and np.isfinite(state["psi"]).all()
    e.close()


# ======================================================================================================================================
# 5. frames with the off-policy learners at the LDS boundary
# ======================================================================================================================================
SAID = dict(td3="frames: the stacked input row is too large for off-policy training (LDS); fewer frames fit",
            sac="frames: the stacked input row is too large for soft actor-critic training (LDS); fewer frames fit")


@pytest.mark.parametrize("family", ["td3", "sac"])
def test_offpolicy_with_frames_trains_at_the_last_k_that_fits_and_refuses_the_next(amd, family):
    """actor hidden (256, 256, 256), critics (256, 256, 256, 1), 8 frames: TD3 holds 45 K + 1562 floats (K >= 255), SAC 55 K + 2345.
    At the largest K within 16384 floats three days of 4 envs are stored and one update at batch 8 equals the restatement bit for
    bit; at K + 1 the init is refused in the existing words - one frame of K + 1 fits - and the engine goes on stepping"""
    td3, frames, envs, T = family == "td3", 8, 4, 3
    K = W.boundary_K(family, frames)
    below, above = W.widest_count(family, K, frames), W.widest_count(family, K + 1, frames)
    RS.log(f"boundary {family} frames={frames}", K=K, floats_at_K=below, floats_at_K_plus_1=above, limit=W.LDS_FLOATS,
           one_frame_at_K_plus_1=W.widest_count(family, K + 1, 1))
    assert below <= W.LDS_FLOATS < above and W.widest_count(family, K + 1, 1) <= W.LDS_FLOATS
    assert K == (329 if td3 else 255), "the restated count disagrees with the count by hand"
    D, A, seed, widths = frames * (5 * K + 2), K + 1, 71 + td3, W.WIDEST["critics"]
    rng = np.random.default_rng(seed)
    if td3:
        pol = W.widest_policy(rng, K, two=False, value=False, frames=frames, normalize=True)
        pol.layers[-1][1][1:K + 1] += F(0.8)
        opts = T3.options(critic_widths=widths, batch_size=8, capacity=16, seed=seed, policy_delay=1, tau=0.05, gamma=0.9, reward_scale=0.5)
        norm = (np.full(A, 0.25, F), np.full(A, 1.5, F))
    else:
        pol = W.widest_policy(rng, K, two=True, value=False, frames=frames, normalize=True, log_std_clamp=(-1.0, -0.5))
        pol.layers[-1][1][K + 1:] = np.linspace(-1.6, 0.1, K + 1).astype(F)
        opts = S.options(K, critic_widths=widths, batch_size=8, capacity=16, seed=seed, tau=0.05, gamma=0.9, reward_scale=0.5, init_alpha=0.3, alpha_lr=3e-3)
        norm = None
    pol.shift, pol.scale = _stacked_norm(K, frames)
    crit = ST.random_critics(rng, K, frames, widths)
    e = _engine(amd, _planes(envs, K, seed, mean_volume=4), seed=seed, **NO_RESETS)
    e.mlp_init(pol, np.arange(envs, dtype=np.uint64) + 11, deterministic=False)
    if not td3:
        e.mlp_set_squash(*_bounds(K))
    e.rollout_enable(T, obs=True)
    if td3:
        e.td3_init(**opts)
        e.td3_set_critics(crit, action_norm=norm)
    else:
        e.sac_init(**opts)
        e.sac_set_critics(crit)
    hist = ST.History(envs, K, frames)
    for _ in range(T):
        hist.row(*_now(e))
        e.mlp_step(BUDGET)
    assert getattr(e, family + "_store")() == T * envs
    rec = e.rollout_fetch()
    raw = hist.row(*_now(e), commit=False)
    assert rec["obs"].shape == (T, envs, D) and np.count_nonzero(raw[:, 2 * (5 * K + 2):3 * (5 * K + 2)]) > 0, "the peeked row holds three days"
    ring = T3.Ring(16, D, A)
    ring.store(rec, ST.normalized(pol, raw))
    buf = getattr(e, family + "_buffer")()
    _assert_keys(buf, ring.buffer(), ("x", "a", "r", "done", "x2"), "the ring after the store")
    assert (buf["size"], buf["written"]) == (T * envs, T * envs)
    stats = getattr(e, family + "_update")(1)
    with ST.stacked_shapes():
        if td3:
            state, rstats = T3.update(pol, T3.fresh_state(pol, crit), buf, norm, seed, opts)
        else:
            state, rstats = S.update(pol, S.fresh_state(pol, crit, opts), buf, seed, opts)
    _assert_keys(getattr(e, family + "_state")(), state, T3.STATE_KEYS if td3 else S.STATE_KEYS)
    _assert_stats(T3.STAT_KEYS if td3 else S.STAT_KEYS, stats, rstats)
    assert np.isfinite(state["theta"]).all() and np.isfinite(state["psi"]).all() and not _same(state["theta"], T3.flat_of(pol.layers))
    e.close()
    # one keyword further
    pol = W.widest_policy(np.random.default_rng(seed), K + 1, two=not td3, value=False, frames=frames, **({} if td3 else dict(log_std_clamp=(-1.0, -0.5))))
    e = _engine(amd, _planes(2, K + 1, seed, mean_volume=4), seed=seed, **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(1, obs=True)
    if not td3:
        e.mlp_set_squash(*_bounds(K + 1))
    with pytest.raises(ValueError) as info:
        (e.td3_init if td3 else e.sac_init)(critic_widths=widths, batch_size=8, capacity=16)
    assert str(info.value) == SAID[family], (str(info.value), SAID[family])
    e.run_days("mlp", 1, BUDGET)                                    # (the engine goes on: the policy acts and the day is recorded)
    assert e.rollout_fetch()["reward"].shape == (1, 2)
    e.close()
