"""GPU tests of the TD3 learners' running observation and reward normalisers (parts/kernel_norm.inc, parts/norm_api.inc,
the sample-time normalisation of parts/kernel_td3.inc / kernel_td3_pop.inc) against the numpy restatement tests/td3_norm_ref.py
and the host twins, bit for bit: there is no tolerance anywhere.  None of these entry points exists before this feature: every
test here fails on the parent commit.

Unless a test says otherwise the shape is 8 envs x 3 keywords (D = 17: the tail of a 32-input weight block, A = 4), policy hidden
(8,), critics (8, 8, 1), horizon 3, batch 16, capacity 64."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import norm_ref as NR
from tests import td3_norm_ref as TN
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F, D64 = np.float32, np.float64
N, K, T, B, CAP = 8, 3, 3, 16, 64
D, A = 5 * K + 2, K + 1
HIDDEN, WIDTHS = (8,), (8, 8, 1)
SEED, BUDGET = 41, 1000.0
RESETS = dict(max_days=4, auto_reset=True)


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(autouse=True)
def time_limit(request):
    """every test under its own time limit (the handler runs when the interpreter next regains control)"""
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


def _planes(envs=N, keywords=K):
    return H.implicit_params(envs, keywords, SEED + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, env_id_base=0, **kw):
    e = amd.StepEngine(planes.shape[1], planes.shape[2], seed=SEED, env_id_base=env_id_base, **kw)
    e.set_all_params(planes)
    e.reset()
    return e


def _policy(rng, keywords=K, sigma=0.2):
    pol = R.random_policy(rng, keywords, HIDDEN, "tanh", normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(keywords)
    pol.log_std = np.full(keywords + 1, np.log(sigma), F)
    return pol


def _options(**kw):
    return T3.options(**dict(dict(critic_widths=WIDTHS, batch_size=B, capacity=CAP, policy_delay=2, gamma=0.9, tau=0.05, reward_scale=0.5, actor_lr=3e-3,
                                  critic_lr=3e-3, target_noise=0.3, target_noise_clip=0.25), **kw))


def _solo(amd, pol, crit, opts, planes=None, env_id_base=0, horizon=T, norm=None, engine_kw=RESETS):
    e = _engine(amd, _planes() if planes is None else planes, env_id_base, **engine_kw)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(horizon, obs=True)
    e.td3_init(**opts)
    e.td3_set_critics(crit)
    if norm is not None:
        e.td3_norm_init(**norm)
    return e


def _population(amd, pols, crits, opts, norm=None, planes=None, horizon=T):
    e = _engine(amd, _planes() if planes is None else planes, **RESETS)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(len(pols))
    for m in range(1, len(pols)):
        e.mlp_set_learner(m, pols[m])
    e.rollout_enable(horizon, obs=True)
    e.td3_pop_init(opts)
    for m in range(len(pols)):
        e.td3_pop_set_critics(m, crits[m])
    if norm is not None:
        e.td3_norm_init(**norm)
    return e


def _raw_input(e):
    """the raw row an act would read now: the flat observation, zeros on an episode's first day"""
    x = R.flat_obs(e.fetch()).astype(F)
    x[e.get_episode_state()[0] == 0] = 0
    return x


def _collect(e, days=T, pop=False):
    e.rollout_reset()
    e.run_days("mlp", days, BUDGET)
    return e.td3_pop_store() if pop else e.td3_store()


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


def _norm_state(e, member=0, envs=None):
    """(observation state, reward state with the member's envs' carry) in td3_norm_ref's keys"""
    st = e.td3_norm_state(member)
    if "rew_count" in st:
        g = e.td3_norm_returns()
        st["returns"] = g if envs is None else g[member * envs:(member + 1) * envs].copy()
    return TN.split(st)


def _assert_norm(got, ref, what=""):
    (go, gr), (ro, rr) = got, ref
    assert (go is None) == (ro is None) and (gr is None) == (rr is None), what
    if go is not None:
        assert TN.obs_same(go, ro), ("observations", what)
    if gr is not None:
        assert TN.rew_same(gr, rr), ("rewards", what)


BOTH = dict(observations=True, rewards=True)


# ---- 1. a frozen normaliser is the hand-set one -----------------------------------------------------------------------------------
def test_frozen_normaliser_equals_hand_set_vectors(amd):
    """A: the vectors of mlp_set_norm and no normaliser, rows normalised when they are stored.  B: td3_norm_init, the same vectors
    through mlp_set_norm, never updated (multiplier 1, no clip), raw rows normalised when they are sampled.  Two rounds of collect,
    store and 4 updates: the same bits everywhere, and normalize(B's ring) is A's ring"""
    rng = np.random.default_rng(11)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options()
    a = _solo(amd, pol, crit, opts)
    b = _solo(amd, pol, crit, opts, norm=dict(BOTH, rew_clip=0.0))
    a.mlp_set_norm(pol.shift, pol.scale)
    b.mlp_set_norm(pol.shift, pol.scale)
    fresh = _norm_state(b)
    for rnd in range(2):
        assert _collect(a) == _collect(b) == T * N
        ra, rb = a.rollout_fetch(), b.rollout_fetch()
        for k in ("action", "reward", "terminated", "truncated"):
            assert _same(ra[k], rb[k]), (k, rnd)
        assert not _same(ra["obs"], rb["obs"]) and _same(TN.normalize(rb["obs"].reshape(-1, D), pol.shift, pol.scale), ra["obs"].reshape(-1, D))
        sa, sb = a.td3_update(4), b.td3_update(4)
        _assert_stats(sa, sb, rnd)
        _assert_state(a.td3_state(), b.td3_state(), rnd)
        ba, bb = a.td3_buffer(), b.td3_buffer()
        for k in ("a", "r", "done"):
            assert _same(ba[k], bb[k]), (k, rnd)
        for k in ("x", "x2"):
            assert not _same(ba[k], bb[k]) and _same(TN.normalize(bb[k], pol.shift, pol.scale), ba[k]), (k, rnd)
    assert sb["actor_steps"] == 4 and bb["size"] == 2 * T * N
    # B's rows are the raw observation: counts and dollars, zeros on an episode's first day
    assert (bb["x2"][bb["done"]] == 0).all() and bb["done"].any() and np.abs(bb["x"]).max() > 10.0
    _assert_norm(_norm_state(b), fresh, "nothing moved the moments")
    assert fresh[0]["count"] == 0 and _same(fresh[0]["shift"], pol.shift) and _same(fresh[0]["scale"], pol.scale) and fresh[1]["scale"] == F(1.0)
    assert _same(a.mlp_params(), b.mlp_params())
    a.close()
    b.close()


# ---- 2. the moments -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1500])
def test_moments_equal_the_host_twin_and_the_restatement(amd, cap):
    """64 envs x 1 keyword x 17 days: S = 1088 samples an update, more than one 1024-sample chunk; three updates through auto-resets"""
    from adcraft_amd import _ffi
    n_envs, kw, days = 64, 1, 17
    rng = np.random.default_rng(21)
    pol, crit = _policy(rng, kw), T3.random_critics_for_tests(rng, kw, WIDTHS)
    opts = _options(capacity=4096, gamma=0.97)
    e = _solo(amd, pol, crit, opts, planes=_planes(n_envs, kw), horizon=days,
              norm=dict(BOTH, obs_count_cap=cap, rew_count_cap=cap, obs_min_std=0.05, rew_min_std=0.02))
    d = 5 * kw + 2
    ref_o = twin_o = TN.obs_fresh(d, pol.shift, pol.scale)
    ref_r = twin_r = TN.rew_fresh(n_envs)
    for it in range(3):
        assert _collect(e, days) == days * n_envs
        assert e.td3_norm_update() == days * n_envs
        rec = e.rollout_fetch()
        rows = NR.member_rows(rec["obs"], 0, n_envs)
        rew = (rec["reward"], rec["terminated"], rec["truncated"])
        ref_o, twin_o = TN.obs_update(ref_o, rows, 0.05, cap), TN.twin_obs(_ffi.lib(), twin_o, rows, 0.05, cap)
        ref_r, twin_r = TN.rew_update(ref_r, *rew, F(0.97), 0.02, cap), TN.twin_rew(_ffi.lib(), twin_r, *rew, F(0.97), 0.02, cap)
        got = _norm_state(e)
        _assert_norm(got, (ref_o, ref_r), ("restatement", it))
        _assert_norm(got, (twin_o, twin_r), ("twin", it))
        assert (rec["terminated"] | rec["truncated"]).any() and (rec["obs"][0] == 0).all() == (it == 0)
    assert got[0]["count"] == (cap or 3 * days * n_envs) and got[1]["count"] == (cap or 3 * days * n_envs)
    assert got[1]["scale"] != F(1.0) and not _same(got[0]["shift"], pol.shift) and np.any(got[1]["returns"] != 0)
    with pytest.raises(_ffi.EngineStateError, match="no day has been recorded"):
        e.td3_norm_update()
    e.close()


# ---- 2b. raw observation moments across tile and chunk boundaries ------------------------------------------------------------------
@pytest.mark.parametrize("members", [0, 2])
def test_raw_moments_across_column_tiles_and_chunks(amd, members):
    """8 envs a normaliser x 60 keywords x 130 days: D = 302 is two 256-column tiles, the second partial; S = 1040 is two
    1024-sample chunks, the second partial.  One collect, one update: the raw finish and the scan equal the restatement and the
    host twins.  members = 2: per-member normalisers of two learners over 16 envs, the same S for each"""
    from adcraft_amd import _ffi
    n, kw, days, M = 8, 60, 130, max(members, 1)
    d = 5 * kw + 2
    rng = np.random.default_rng(25)
    pols = [_policy(rng, kw, sigma=(0.2, 0.05)[m]) for m in range(M)]
    crits = [T3.random_critics_for_tests(rng, kw, WIDTHS) for _ in range(M)]
    gammas = [F(0.97), F(0.9)][:M]
    opts = [_options(capacity=2048, gamma=float(g)) for g in gammas]
    if members:
        e = _population(amd, pols, crits, opts, norm=dict(BOTH, per_member=True), planes=_planes(M * n, kw), horizon=days)
    else:
        e = _solo(amd, pols[0], crits[0], opts[0], planes=_planes(n, kw), horizon=days, norm=BOTH)
    assert _collect(e, days, pop=bool(members)) == days * n
    assert e.td3_norm_update() == days * n
    rec = e.rollout_fetch()
    assert (rec["terminated"] | rec["truncated"]).any() and (rec["obs"][0] == 0).all() and np.abs(rec["obs"]).max() > 10.0
    for m in range(M):
        rows = NR.member_rows(rec["obs"], m, n)
        assert rows.shape == (1040, 302)
        rew = tuple(rec[k][:, m * n:(m + 1) * n] for k in ("reward", "terminated", "truncated"))
        o, r = TN.obs_fresh(d, pols[m].shift, pols[m].scale), TN.rew_fresh(n)
        got = _norm_state(e, m, n)
        _assert_norm(got, (TN.obs_update(o, rows), TN.rew_update(r, *rew, gammas[m])), ("restatement", m))
        _assert_norm(got, (TN.twin_obs(_ffi.lib(), o, rows), TN.twin_rew(_ffi.lib(), r, *rew, gammas[m])), ("twin", m))
        assert got[0]["count"] == days * n and not _same(got[0]["shift"], pols[m].shift) and got[1]["scale"] != F(1.0)
    e.close()


# ---- 2c. the batched copy with one part absent -------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["rewards", "observations"])
def test_copy_with_one_part_absent(amd, part):
    """3 members x 2 envs with the rewards' part alone, then with the observations' alone: after an update (the members differ)
    td3_norm_copy([2, -1, 2]) makes member 0's state member 2's, bit for bit, and leaves members 1 and 2 and the envs' carry alone"""
    M, n = 3, 2
    pols, crits = _members(27, M)
    opts = [_options(gamma=float(F(0.9 + 0.03 * m))) for m in range(M)]
    e = _population(amd, pols, crits, opts, norm={part: True, "per_member": True}, planes=_planes(M * n, K))
    assert _collect(e, pop=True) == T * n
    assert e.td3_norm_update() == T * n
    before = [_norm_state(e, m, n) for m in range(M)]
    carry = e.td3_norm_returns() if part == "rewards" else None
    which = 1 if part == "rewards" else 0
    same = (lambda a, b: TN.rew_same(a, b, returns=False)) if part == "rewards" else TN.obs_same
    assert all(st[1 - which] is None for st in before) and not same(before[0][which], before[2][which])
    e.td3_norm_copy([2, -1, 2])
    after = [_norm_state(e, m, n) for m in range(M)]
    assert same(after[0][which], before[2][which]), "member 0 is its donor"
    for m in (1, 2):
        _assert_norm(after[m], before[m], ("untouched", m))
    if part == "rewards":
        assert np.any(carry != 0) and _same(e.td3_norm_returns(), carry), "the carry is the envs' and stays"
    e.close()


# ---- 3. moving vectors reach the batch ----------------------------------------------------------------------------------------------
def _moving_pass(amd, clip):
    rng = np.random.default_rng(31)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options(reward_scale=1.0)
    e = _solo(amd, pol, crit, opts, norm=dict(BOTH, rew_clip=clip))
    _collect(e)
    e.td3_norm_update()
    (o, r), buf = _norm_state(e), e.td3_buffer()
    assert not _same(o["shift"], pol.shift) and r["scale"] != F(1.0)
    state, rs_all = T3.fresh_state(pol, crit), []
    # (what the old vectors would give is something else: the update below is held against the new ones)
    stale, _, _ = TN.update(pol, state, buf, None, SEED, opts, (pol.shift, pol.scale), r["scale"], clip)
    for u in range(2):                                  # (policy_delay 2: the second update steps the actor on normalised rows too)
        stats = e.td3_update(1)
        state, rstats, (rs, _) = TN.update(pol, state, buf, None, SEED, opts, (o["shift"], o["scale"]), r["scale"], clip)
        _assert_state(e.td3_state(), state, (clip, u))
        _assert_stats(stats, rstats, (clip, u))
        assert u > 0 or not _same(stale["psi"], state["psi"])
        rs_all.append(rs)
    e.close()
    return np.abs(np.concatenate(rs_all))


def test_moving_vectors_and_multiplier_reach_the_next_update(amd):
    """after td3_norm_update the next updates equal td3_ref on the fetched raw ring with rows normalised by the NEW vectors and
    targets from td3_y_norm under the new multiplier: once without a clip, once with a clip that binds on some elements only (the
    median of the batch's |scaled reward|, taken from the first pass on the host)"""
    mags = _moving_pass(amd, 0.0)
    clip = float(F(np.median(mags[mags > 0])))
    assert (mags > clip).any() and (mags < clip).any(), "the clip was meant to bind on some elements only"
    _moving_pass(amd, clip)


# ---- 4. the ring wraps with raw rows ------------------------------------------------------------------------------------------------
def test_ring_wrap_keeps_the_skip_rule_and_the_raw_next_row(amd):
    """capacity 20, stores of 24 samples (the first 4 of a store are skipped).  max_days 3: the third day ends every episode and
    auto-resets the env, so the last day's x' is the zero row; a further store of 2 days ends inside an episode: raw counts"""
    rng = np.random.default_rng(41)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options(capacity=20)
    e = _solo(amd, pol, crit, opts, norm=BOTH, engine_kw=dict(max_days=3, auto_reset=True))
    ring = T3.Ring(20, D, A)
    for rnd, days in enumerate((3, 2, 3)):
        assert _collect(e, days) == days * N
        rec, now = e.rollout_fetch(), _raw_input(e)
        ring.store(rec, now)
        _assert_buffer(e.td3_buffer(), ring.buffer(), rnd)
        done_last = rec["terminated"][-1] | rec["truncated"][-1]
        if days == 3 and rnd == 0:
            assert done_last.all() and (now == 0).all() and (rec["obs"][0] == 0).all() and np.abs(rec["obs"][1]).max() > 1.0
        if days == 2:
            assert not done_last.any() and np.abs(now).max() > 1.0 and _same(now, R.flat_obs(e.fetch()).astype(F))
    buf = e.td3_buffer()
    assert buf["size"] == 20 and buf["written"] == 8 * N
    e.td3_norm_update()
    e.td3_update(2)                                                 # (the wrapped ring is sampled)
    e.close()


# ---- 5. populations -----------------------------------------------------------------------------------------------------------------
OWN = (dict(gamma=0.9, reward_scale=0.5, seed=0), dict(gamma=0.99, reward_scale=0.1, seed=77))


def _members(seed, members=2):
    rng = np.random.default_rng(seed)
    pols = [_policy(rng, sigma=(0.2, 0.05, 0.4, 0.1)[m]) for m in range(members)]
    return pols, [T3.random_critics_for_tests(rng, K, WIDTHS) for _ in range(members)]


def test_population_per_member_equals_solo_engines(amd):
    """M = 2 x 4 envs, per-member normalisers, the members' own gamma and reward_scale: after two iterations with normaliser
    updates every member's state, ring, statistics and normalisers are those of a solo engine of its envs at env_id_base = m n"""
    n = N // 2
    pols, crits = _members(51)
    opts = [_options(**OWN[m]) for m in range(2)]
    norm = dict(BOTH, rew_clip=0.8)
    e = _population(amd, pols, crits, opts, norm=dict(norm, per_member=True))
    solos = [_solo(amd, pols[m], crits[m], opts[m], planes=_planes()[:, m * n:(m + 1) * n], env_id_base=m * n, norm=norm) for m in range(2)]
    for it in range(2):
        assert _collect(e, pop=True) == T * n
        assert e.td3_norm_update() == T * n
        stats = e.td3_pop_update(2)
        for m, s in enumerate(solos):
            _collect(s)
            s.td3_norm_update()
            sstats = s.td3_update(2)
            _assert_stats(stats[m], sstats, (it, m))
            _assert_state(e.td3_pop_state(m), s.td3_state(), (it, m))
            _assert_buffer(e.td3_pop_buffer(m), s.td3_buffer(), (it, m))
            _assert_norm(_norm_state(e, m, n), _norm_state(s), (it, m))
    a, b = _norm_state(e, 0, n), _norm_state(e, 1, n)
    assert not _same(a[0]["shift"], b[0]["shift"]) and a[1]["scale"] != b[1]["scale"]
    # mlp_set_norm writes every member's vectors and leaves the moments alone
    e.mlp_set_norm(pols[0].shift, pols[0].scale)
    for m, old in enumerate((a, b)):
        new = _norm_state(e, m, n)
        assert _same(new[0]["shift"], pols[0].shift) and _same(new[0]["scale"], pols[0].scale) and _same(new[0]["mean"], old[0]["mean"])
        assert new[0]["count"] == old[0]["count"] and TN.rew_same(new[1], old[1])
    e.close()
    for s in solos:
        s.close()


def test_population_with_a_shared_normaliser_equals_the_host_twin(amd):
    from adcraft_amd import _ffi
    n = N // 2
    pols, crits = _members(52)
    opts = [_options(**OWN[m]) for m in range(2)]
    e = _population(amd, pols, crits, opts, norm=BOTH)
    gammas = np.repeat(np.array([o["gamma"] for o in opts], F), n)
    o, r = TN.obs_fresh(D, pols[0].shift, pols[0].scale), TN.rew_fresh(N)
    for it in range(2):
        _collect(e, pop=True)
        assert e.td3_norm_update() == T * N
        rec = e.rollout_fetch()
        o = TN.twin_obs(_ffi.lib(), o, NR.member_rows(rec["obs"], 0, N))
        r = TN.twin_rew(_ffi.lib(), r, rec["reward"], rec["terminated"], rec["truncated"], gammas)
        _assert_norm(_norm_state(e), (o, r), it)
        e.td3_pop_update(2)
    with pytest.raises(_ffi.EngineStateError, match="shared"):
        e.td3_norm_copy([-1])
    e.close()


# ---- 6. a PBT round carries the normalisers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ring", [True, False])
def test_pbt_round_copies_the_donors_normalisers(amd, with_ring):
    from adcraft_amd.baselines.pbt import PBTScheduler
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer
    M, n = 4, 2
    pols, crits = _members(61, M)
    e = _engine(amd, _planes(), **RESETS)
    cfgs = [dict(critic_hidden=WIDTHS[:-1], batch_size=B, capacity=CAP, learning_starts=0, updates_per_iteration=2, critics=crits[m], policy_delay=2,
                 gamma=float(F(0.9 + 0.02 * m)), reward_scale=float(F(0.5 / (m + 1))), tau=0.05, actor_lr=3e-3, critic_lr=3e-3) for m in range(M)]
    tr = TD3PopulationTrainer(e, pols, [0.2, 0.05, 0.4, 0.1], cfgs, horizon=T, normalize_observations=True, normalize_rewards=True, norm=dict(rew_clip=0.8))
    sch = PBTScheduler(tr, replace_fraction=0.25, tuned=("tau",), bounds={"tau": (0.01, 0.1)}, factors=(0.5, 2.0), with_ring=with_ring)
    assert sch.replace_count == 1
    tr.iteration(budget=BUDGET)
    before = [_norm_state(e, m, n) for m in range(M)]
    rings = [e.td3_pop_buffer(m) for m in range(M)]
    res = sch.step()
    (dst,) = np.nonzero(res["src"] >= 0)[0]
    src = int(res["src"][dst])
    after = [_norm_state(e, m, n) for m in range(M)]
    assert TN.obs_same(after[dst][0], before[src][0]) and TN.rew_same(after[dst][1], before[src][1], returns=False)
    assert not TN.obs_same(before[dst][0], before[src][0])
    assert _same(after[dst][1]["returns"], before[dst][1]["returns"]), "the carry is the envs' and stays"
    for m in range(M):
        if m != dst:
            _assert_norm(after[m], before[m], ("untouched", m))
    ring = e.td3_pop_buffer(dst)
    _assert_buffer(ring, rings[src if with_ring else dst], "the ring holds raw rows either way")
    # the destination's next update: the reference on its ring under the donor's vectors and multiplier
    opts = T3.options(**dict({k: v for k, v in tr.configs[dst].items()}, seed=0))
    state = e.td3_pop_state(dst)
    e.td3_pop_update(1)
    o, r = after[dst]
    ref, _, _ = TN.update(tr._templates[dst], state, ring, None, SEED, opts, (o["shift"], o["scale"]), r["scale"], 0.8)
    _assert_state(e.td3_pop_state(dst), ref, "after the round")
    assert _same(tr.policy(dst).shift, before[src][0]["shift"]), "policy() exports the current vectors"
    e.close()


# ---- 7. resume ----------------------------------------------------------------------------------------------------------------------
def test_a_resumed_run_continues_to_the_same_bits(amd):
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    rng = np.random.default_rng(71)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options(seed=9)
    cfg = {k: v for k, v in opts.items() if k != "critic_widths"}

    def make():
        e = _engine(amd, _planes(), **RESETS)
        return e, TD3Trainer(e, pol, critic_hidden=WIDTHS[:-1], horizon=T, exploration_sigma=0.2, learning_starts=0, updates_per_iteration=3, critics=crit,
                             normalize_observations=True, normalize_rewards=True, norm=dict(rew_clip=0.8, obs_count_cap=40), **cfg)
    e1, t1 = make()
    t1.iteration(budget=BUDGET)
    saved = t1.norm_state(), t1.state(), e1.td3_buffer()
    s1 = t1.iteration(budget=BUDGET)
    e2, t2 = make()
    e2.run_days("mlp", T, BUDGET)                                   # (the envs' and the agents' streams, as after iteration 1; not stored)
    t2.norm_state(saved[0])
    t2.state(saved[1])
    e2.td3_buffer_load(saved[2])
    _assert_norm(TN.split(t2.norm_state()), TN.split(saved[0]), "loaded")
    s2 = t2.iteration(budget=BUDGET)
    _assert_stats(s1, s2)
    _assert_state(t1.state(), t2.state())
    _assert_buffer(e1.td3_buffer(), e2.td3_buffer())
    _assert_norm(TN.split(t1.norm_state()), TN.split(t2.norm_state()), "after iteration 2")
    assert saved[0]["obs_count"] == T * N and t1.norm_state()["obs_count"] == 40
    assert _same(t1.policy().shift, t1.norm_state()["shift"]) and not _same(t1.policy().shift, pol.shift)
    e1.close()
    e2.close()


# ---- 8. off means off ---------------------------------------------------------------------------------------------------------------
def test_without_a_normaliser_nothing_changed_and_the_record_goes_back(amd):
    rng = np.random.default_rng(81)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options()
    e = _solo(amd, pol, crit, opts)
    ring, state = T3.Ring(CAP, D, A), T3.fresh_state(pol, crit)
    _collect(e)
    rec = e.rollout_fetch()
    ring.store(rec, T3.current_input(pol, e.fetch(), e.get_episode_state()[0] == 0))
    _assert_buffer(e.td3_buffer(), ring.buffer())
    assert _same(rec["obs"][0], TN.normalize(np.zeros((N, D), F), pol.shift, pol.scale)), "network inputs: the first day's row is (0 - shift) * scale"
    for u in range(2):
        stats = e.td3_update(1)
        state, rstats = T3.update(pol, state, ring.buffer(), None, SEED, opts)
        _assert_state(e.td3_state(), state, u)
        _assert_stats(stats, rstats, u)
    # a normaliser that ended through rollout_enable: the record holds network inputs again
    e2 = _solo(amd, pol, crit, opts, norm=BOTH)
    _collect(e2)
    assert (e2.rollout_fetch()["obs"][0] == 0).all()
    e2.rollout_enable(T, obs=True)
    e2.td3_init(**opts)
    e2.td3_set_critics(crit)
    e2.reset()
    _collect(e2)
    assert _same(e2.rollout_fetch()["obs"][0], rec["obs"][0])
    e.close()
    e2.close()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(amd):
    from adcraft_amd import _ffi
    rng = np.random.default_rng(91)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options()
    e = _engine(amd, _planes(), **RESETS)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="td3_init"):
        e.td3_norm_init(**BOTH)                                     # no trainer
    for call in (lambda: e.td3_norm_update(), lambda: e.td3_norm_state(), lambda: e.td3_norm_returns(), lambda: e.td3_norm_copy([-1])):
        with pytest.raises(_ffi.EngineStateError, match="td3_norm_init"):
            call()
    e.td3_init(**opts)
    e.td3_set_critics(crit)
    with pytest.raises(ValueError, match="population"):
        e.td3_norm_init(per_member=True, **BOTH)                    # per_member without a population
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.obs_norm_init()
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.rew_norm_init()
    e.run_days("mlp", 1, BUDGET)
    with pytest.raises(_ffi.EngineStateError, match="must be empty"):
        e.td3_norm_init(**BOTH)                                     # a day already recorded
    e.td3_store()
    e.rollout_reset()
    with pytest.raises(_ffi.EngineStateError, match="must be empty"):
        e.td3_norm_init(**BOTH)                                     # a transition already in the ring
    e.td3_init(**opts)                                              # (a new trainer: an empty ring)
    e.td3_set_critics(crit)
    e.td3_norm_init(**BOTH)
    with pytest.raises(_ffi.EngineStateError, match="no day has been recorded"):
        e.td3_norm_update()                                         # no unconsumed day
    with pytest.raises(_ffi.EngineStateError):
        e.pg_init()                                                 # still refused while TD3 lives
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.obs_norm_init()
    with pytest.raises(_ffi.EngineStateError, match="shared"):
        e.td3_norm_copy([-1])
    with pytest.raises(ValueError, match="no such normaliser"):
        e.td3_norm_state(1)
    with pytest.raises(ValueError, match="one value per env"):
        e.td3_norm_returns(np.zeros(3))
    # the engine is usable after every refusal
    _collect(e)
    assert e.td3_norm_update() == T * N
    e.td3_update(2)
    # the normaliser ends with its trainer
    for end in (lambda: e.td3_init(**opts), lambda: e.rollout_enable(T, obs=True), lambda: e.mlp_init(pol, deterministic=False)):
        end()
        with pytest.raises(_ffi.EngineStateError, match="td3_norm_init"):
            e.td3_norm_state()
        e.mlp_init(pol, deterministic=False)
        e.rollout_enable(T, obs=True)
        e.td3_init(**opts)
        e.td3_set_critics(crit)
        e.td3_norm_init(rewards=True)
        assert "obs_count" not in e.td3_norm_state()
    # a policy without normalisation cannot have its observations normalised; its rewards can
    plain = R.random_policy(rng, K, HIDDEN, "tanh", normalize=False, scale=0.6)
    plain.log_std = np.full(A, np.log(0.2), F)
    e.mlp_init(plain, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.td3_init(**opts)
    e.td3_set_critics(crit)
    with pytest.raises(ValueError, match="without normalisation"):
        e.td3_norm_init(observations=True)
    e.td3_norm_init(rewards=True)
    # chained copies are refused under per-member normalisers
    e.close()
    pols, crits = _members(92, 4)
    p = _population(amd, pols, crits, [_options()] * 4, norm=dict(BOTH, per_member=True))
    with pytest.raises(ValueError, match="also a source"):
        p.td3_norm_copy([1, 2, -1, -1])
    with pytest.raises(ValueError, match="src_of_member_m"):
        p.td3_norm_copy([4, -1, -1, -1])
    with pytest.raises(ValueError, match="one source per member"):
        p.td3_norm_copy([-1])
    p.td3_norm_copy([-1, 0, 2, 0])
    # a population's trainer ends with mlp_learners and with mlp_population, and its normalisers with it
    for end in (lambda: p.mlp_learners(4), lambda: p.mlp_population(2)):
        end()
        with pytest.raises(_ffi.EngineStateError, match="td3_norm_init"):
            p.td3_norm_state()
        with pytest.raises(_ffi.EngineStateError, match="td3_pop_init"):
            p.td3_pop_store()
        p.mlp_population(0)
        p.mlp_learners(4)
        p.td3_pop_init([_options()] * 4)
        p.td3_norm_init(per_member=True, **BOTH)
    p.close()


# ---- 9b. a solo trainer and its normalisers survive learners and a population -------------------------------------------------------
def test_solo_trainer_continues_on_its_raw_ring_after_learners_and_a_population(amd):
    """mlp_learners / mlp_population do not end a single-learner trainer (its calls are refused while they are active), so they may
    not end its normalisers either: the ring is raw.  After mlp_learners(2), mlp_learners(0), mlp_population(2), mlp_population(0)
    the run continues to the bits of a twin that was never interrupted"""
    from adcraft_amd import _ffi
    rng = np.random.default_rng(95)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options()
    norm = dict(BOTH, rew_clip=0.8)
    a, b = _solo(amd, pol, crit, opts, norm=norm), _solo(amd, pol, crit, opts, norm=norm)

    def iteration(e):
        _collect(e)
        e.td3_norm_update()
        return e.td3_update(2)
    _assert_stats(iteration(a), iteration(b), "the twins before")
    before = _norm_state(b)
    for on, off in ((lambda: b.mlp_learners(2), lambda: b.mlp_learners(0)), (lambda: b.mlp_population(2), lambda: b.mlp_population(0))):
        on()
        _assert_norm(_norm_state(b), before, "the normalisers live on")
        for call in (b.td3_update, b.td3_store):
            with pytest.raises(_ffi.EngineStateError, match="not supported"):
                call()
        off()
    for it in range(2):
        _assert_stats(iteration(a), iteration(b), it)
        _assert_state(a.td3_state(), b.td3_state(), it)
        _assert_buffer(a.td3_buffer(), b.td3_buffer(), it)
        _assert_norm(_norm_state(a), _norm_state(b), it)
    assert np.abs(b.td3_buffer()["x"]).max() > 10.0, "the ring is raw throughout"
    # state_set takes finite moments and vectors alone
    st = b.td3_norm_state()
    for key, bad in (("shift", np.nan), ("obs_mean", np.inf), ("obs_M2", -1.0), ("scale", 0.0), ("rew_M2", np.nan), ("rew_mean", np.inf)):
        worse = dict(st)
        worse[key] = np.full(D, bad, st[key].dtype) if np.ndim(st[key]) else type(st[key])(bad)
        with pytest.raises(ValueError, match="finite"):
            b.td3_norm_state(0, worse)
    b.td3_norm_state(0, st)
    _assert_norm(_norm_state(a), _norm_state(b), "refused sets wrote nothing")
    a.close()
    b.close()


# ---- 10. a host reset ends the reset envs' running return ---------------------------------------------------------------------------
def test_host_reset_zeroes_exactly_the_reset_envs_carry(amd):
    rng = np.random.default_rng(101)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options()
    e = _solo(amd, pol, crit, opts, norm=BOTH, engine_kw=dict(max_days=1 << 20, loss_threshold=1e12))
    _collect(e)
    e.td3_norm_update()
    g = e.td3_norm_returns()
    mask = np.arange(N) % 3 == 0
    assert np.any(g[mask] != 0) and np.any(g[~mask] != 0), "running returns to zero, and running returns to keep"
    e.reset(env_mask=mask)
    g2 = e.td3_norm_returns()
    assert np.all(g2[mask] == 0) and _same(g2[~mask], g[~mask])
    e.reset()
    assert np.all(e.td3_norm_returns() == 0)
    e.close()
