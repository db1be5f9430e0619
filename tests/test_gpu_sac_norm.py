"""GPU tests of the SAC learners' running observation and reward normalisers (parts/norm_api.inc's adc_engine_sac_norm_*, the
sample-time normalisation of parts/kernel_sac.inc / kernel_sac_pop.inc, the law csrc/adc_sac_norm.h) against the numpy restatement
tests/sac_norm_ref.py and the host twins, bit for bit: there is no tolerance anywhere.  None of these entry points exists before
this feature: every test here fails on the parent commit.

Unless a test says otherwise the shape is 8 envs x 3 keywords (D = 17: the tail of a 32-input weight block, A = 4), actor hidden
(8,) with two heads, critics (8, 8, 1), horizon 3, batch 16, capacity 64, max_days 4 with auto-reset (so that resets and the zero
first-day row occur)."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import norm_ref as NR
from tests import per_ref as PR
from tests import sac_norm_ref as SN
from tests import sac_ref as S
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F, D64 = np.float32, np.float64
N, K, T, B, CAP = 8, 3, 3, 16, 64
D, A = 5 * K + 2, K + 1
HIDDEN, WIDTHS = (8,), (8, 8, 1)
SEED, BUDGET = 41, 1000.0
RESETS = dict(max_days=4, auto_reset=True)
BOTH = dict(observations=True, rewards=True)


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


def _policy(rng, keywords=K):
    pol = S.sac_policy(rng, keywords, HIDDEN, "tanh", clamp=(-1.0, -0.5), normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(keywords)
    return pol


def _bounds(keywords=K):
    return np.concatenate([[50.0], np.full(keywords, 0.02)]).astype(F), np.concatenate([[1500.0], 3.0 + np.arange(keywords) / 10.0]).astype(F)


def _options(keywords=K, **kw):
    return S.options(keywords, **dict(dict(critic_widths=WIDTHS, batch_size=B, capacity=CAP, gamma=0.9, tau=0.05, reward_scale=0.5, init_alpha=0.3,
                                           alpha_lr=3e-3, actor_lr=3e-3, critic_lr=3e-3), **kw))


def _solo(amd, pol, crit, opts, planes=None, env_id_base=0, horizon=T, norm=None, engine_kw=RESETS):
    e = _engine(amd, _planes() if planes is None else planes, env_id_base, **engine_kw)
    e.mlp_init(pol, deterministic=False)
    e.mlp_set_squash(*_bounds(pol.num_keywords))
    e.rollout_enable(horizon, obs=True)
    e.sac_init(**opts)
    e.sac_set_critics(crit)
    if norm is not None:
        e.sac_norm_init(**norm)
    return e


def _population(amd, pols, crits, opts, norm=None, planes=None, horizon=T, engine_kw=RESETS):
    e = _engine(amd, _planes() if planes is None else planes, **engine_kw)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(len(pols))
    for m in range(1, len(pols)):
        e.mlp_set_learner(m, pols[m])
    e.mlp_learners_set_squash(*_bounds(pols[0].num_keywords))
    e.rollout_enable(horizon, obs=True)
    e.sac_pop_init(opts)
    for m in range(len(pols)):
        e.sac_pop_set_critics(m, crits[m])
    if norm is not None:
        e.sac_norm_init(**norm)
    return e


def _members(seed, members, keywords=K):
    rng = np.random.default_rng(seed)
    pols = [_policy(rng, keywords) for _ in range(members)]
    return pols, [T3.random_critics_for_tests(rng, keywords, WIDTHS) for _ in range(members)]


def _raw_input(e):
    """the raw row an act would read now: the flat observation, zeros on an episode's first day"""
    x = R.flat_obs(e.fetch()).astype(F)
    x[e.get_episode_state()[0] == 0] = 0
    return x


def _collect(e, days=T, pop=False):
    e.rollout_reset()
    e.run_days("mlp", days, BUDGET)
    return e.sac_pop_store() if pop else e.sac_store()


def _assert_state(got, ref, what=""):
    for k in S.STATE_KEYS:
        assert _same(got[k], ref[k]), (k, what)
    assert got["updates"] == ref["updates"], what


def _assert_stats(got, ref, what=""):
    for k in S.STAT_KEYS:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


def _assert_buffer(got, ref, what=""):
    for k in ("x", "a", "r", "done", "x2"):
        assert _same(got[k], ref[k]), (k, what)
    assert (got["size"], got["written"], got["capacity"]) == (ref["size"], ref["written"], ref["capacity"]), what


def _norm_state(e, member=0, envs=None):
    """(observation state, reward state with the member's envs' carry) in sac_norm_ref's keys"""
    st = e.sac_norm_state(member)
    if "rew_count" in st:
        g = e.sac_norm_returns()
        st["returns"] = g if envs is None else g[member * envs:(member + 1) * envs].copy()
    return SN.split(st)


def _assert_norm(got, ref, what=""):
    (go, gr), (ro, rr) = got, ref
    assert (go is None) == (ro is None) and (gr is None) == (rr is None), what
    if go is not None:
        assert SN.obs_same(go, ro), ("observations", what)
    if gr is not None:
        assert SN.rew_same(gr, rr), ("rewards", what)


# ---- 1. a frozen normaliser is the hand-set one -----------------------------------------------------------------------------------
def test_frozen_normaliser_equals_hand_set_vectors(amd):
    """A: the vectors of mlp_set_norm, no normaliser, reward_scale 0.125; rows normalised when they are stored.  B: sac_norm_init,
    the same vectors and the multiplier 0.25 through sac_norm_state (a huge count; reward_scale 0.5, so that (r * 0.5) * 0.25 is
    r * 0.125 exactly), never updated, no clip; raw rows normalised when they are sampled.  Two rounds of collect, store and 2
    updates: the same state and statistics, and normalize(B's ring) is A's ring"""
    rng = np.random.default_rng(11)
    pol, crit = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS)
    a = _solo(amd, pol, crit, _options(reward_scale=0.125))
    b = _solo(amd, pol, crit, _options(reward_scale=0.5), norm=dict(BOTH, rew_clip=0.0))
    a.mlp_set_norm(pol.shift, pol.scale)
    b.mlp_set_norm(pol.shift, pol.scale)
    st = b.sac_norm_state()
    assert st["obs_count"] == 0 and _same(st["shift"], pol.shift) and _same(st["scale"], pol.scale) and st["rew_scale"] == F(1.0)
    b.sac_norm_state(0, dict(st, obs_count=1 << 40, rew_count=1 << 40, rew_scale=F(0.25)))
    frozen = _norm_state(b)
    for rnd in range(2):
        assert _collect(a) == _collect(b) == T * N
        ra, rb = a.rollout_fetch(), b.rollout_fetch()
        for k in ("action", "reward", "terminated", "truncated"):
            assert _same(ra[k], rb[k]), (k, rnd)
        assert not _same(ra["obs"], rb["obs"]) and _same(SN.normalize(rb["obs"].reshape(-1, D), pol.shift, pol.scale), ra["obs"].reshape(-1, D))
        sa, sb = a.sac_update(2), b.sac_update(2)
        _assert_stats(sa, sb, rnd)
        _assert_state(a.sac_state(), b.sac_state(), rnd)
        ba, bb = a.sac_buffer(), b.sac_buffer()
        for k in ("a", "r", "done"):
            assert _same(ba[k], bb[k]), (k, rnd)
        for k in ("x", "x2"):
            assert not _same(ba[k], bb[k]) and _same(SN.normalize(bb[k], pol.shift, pol.scale), ba[k]), (k, rnd)
    assert sb["updates"] == 4 and bb["size"] == 2 * T * N
    # B's rows are the raw observation: counts and dollars, zeros on an episode's first day
    assert (bb["x2"][bb["done"]] == 0).all() and bb["done"].any() and np.abs(bb["x"]).max() > 10.0
    _assert_norm(_norm_state(b), frozen, "nothing moved the moments")
    assert _same(a.mlp_params(), b.mlp_params())
    a.close()
    b.close()


# ---- 2. the moments -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1500])
def test_moments_equal_the_host_twin_and_the_restatement(amd, cap):
    """64 envs x 1 keyword x 17 days: S = 1088 samples an update (more than one 1024-sample chunk, and two updates pass the cap of
    1500); two collect / store / update rounds through auto-resets"""
    from adcraft_amd import _ffi
    n_envs, kw, days = 64, 1, 17
    rng = np.random.default_rng(21)
    pol, crit = _policy(rng, kw), T3.random_critics_for_tests(rng, kw, WIDTHS)
    opts = _options(kw, capacity=4096, gamma=0.97)
    e = _solo(amd, pol, crit, opts, planes=_planes(n_envs, kw), horizon=days,
              norm=dict(BOTH, obs_count_cap=cap, rew_count_cap=cap, obs_min_std=0.05, rew_min_std=0.02))
    d = 5 * kw + 2
    ref_o = twin_o = SN.obs_fresh(d, pol.shift, pol.scale)
    ref_r = twin_r = SN.rew_fresh(n_envs)
    for it in range(2):
        assert _collect(e, days) == days * n_envs
        assert e.sac_norm_update() == days * n_envs
        rec = e.rollout_fetch()
        rows = NR.member_rows(rec["obs"], 0, n_envs)
        rew = (rec["reward"], rec["terminated"], rec["truncated"])
        ref_o, twin_o = SN.obs_update(ref_o, rows, 0.05, cap), SN.twin_obs(_ffi.lib(), twin_o, rows, 0.05, cap)
        ref_r, twin_r = SN.rew_update(ref_r, *rew, F(0.97), 0.02, cap), SN.twin_rew(_ffi.lib(), twin_r, *rew, F(0.97), 0.02, cap)
        got = _norm_state(e)
        _assert_norm(got, (ref_o, ref_r), ("restatement", it))
        _assert_norm(got, (twin_o, twin_r), ("twin", it))
        assert (rec["terminated"] | rec["truncated"]).any() and (rec["obs"][0] == 0).all() == (it == 0)
        e.sac_update(1)
    assert got[0]["count"] == (cap or 2 * days * n_envs) and got[1]["count"] == (cap or 2 * days * n_envs)
    assert got[1]["scale"] != F(1.0) and not _same(got[0]["shift"], pol.shift) and np.any(got[1]["returns"] != 0)
    e.close()


# ---- 3. raw moments across a column tile and a sample chunk -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["solo", "population-shared", "population-per-member"])
def test_raw_moments_across_column_tiles_and_chunks(amd, kind):
    """344 envs x 7 keywords x 3 days: D = 37 is more than two 16-column tiles, the last partial; S = 1032 is two 1024-sample chunks,
    the second partial.  One collect, one update: the raw finish and the scan equal the restatement and the host twins.  With a
    population: 2 members of 172 envs each with their own discounts, under one shared normaliser (S = 1032, the envs' discounts
    their members') and under per-member normalisers (S = 516 each).  max_days 2: the second day ends every episode"""
    from adcraft_amd import _ffi
    kw, days, envs = 7, 3, 344
    d = 5 * kw + 2
    M = 1 if kind == "solo" else 2
    n = envs // M
    pols, crits = _members(25, M, kw)
    gammas = [F(0.97), F(0.9)][:M]
    opts = [_options(kw, capacity=2048, gamma=float(g)) for g in gammas]
    kwargs = dict(planes=_planes(envs, kw), horizon=days, engine_kw=dict(max_days=2, auto_reset=True))
    if kind == "solo":
        e = _solo(amd, pols[0], crits[0], opts[0], norm=BOTH, **kwargs)
    else:
        e = _population(amd, pols, crits, opts, norm=dict(BOTH, per_member=kind.endswith("per-member")), **kwargs)
    assert _collect(e, days, pop=M > 1) == days * n
    per_member = kind.endswith("per-member")
    assert e.sac_norm_update() == days * (n if per_member else envs)
    rec = e.rollout_fetch()
    assert (rec["terminated"] | rec["truncated"]).any() and (rec["obs"][0] == 0).all() and (rec["obs"][2] == 0).all() and np.abs(rec["obs"]).max() > 10.0
    for m in range(M if per_member else 1):
        width = n if per_member else envs
        rows = NR.member_rows(rec["obs"], m, width)
        assert rows.shape == (days * width, d)
        rew = tuple(rec[k][:, m * width:(m + 1) * width] for k in ("reward", "terminated", "truncated"))
        gm = gammas[m] if per_member or M == 1 else np.repeat(np.array(gammas, F), n)
        o, r = SN.obs_fresh(d, pols[0].shift, pols[0].scale), SN.rew_fresh(width)
        got = _norm_state(e, m, width if per_member else None)
        _assert_norm(got, (SN.obs_update(o, rows), SN.rew_update(r, *rew, gm)), ("restatement", m))
        _assert_norm(got, (SN.twin_obs(_ffi.lib(), o, rows), SN.twin_rew(_ffi.lib(), r, *rew, gm)), ("twin", m))
        assert got[0]["count"] == days * width and not _same(got[0]["shift"], pols[0].shift) and got[1]["scale"] != F(1.0)
    e.close()


# ---- 4. moving statistics reach the next update -------------------------------------------------------------------------------------
def _moving_pass(amd, clip):
    rng = np.random.default_rng(31)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options(reward_scale=1.0)
    e = _solo(amd, pol, crit, opts, norm=dict(BOTH, rew_clip=clip))
    state, mags = S.fresh_state(pol, crit, opts), []
    old = (pol.shift, pol.scale, F(1.0))
    for rnd in range(2):
        _collect(e)
        e.sac_norm_update()
        (o, r), buf = _norm_state(e), e.sac_buffer()
        assert not _same(o["shift"], old[0]) and r["scale"] != old[2], "the statistics moved"
        # (what the vectors and the multiplier of before this round's update would give is something else: a kernel that ignored the
        #  pointers, or read stale ones, does not pass)
        stale, _, _ = SN.update(pol, state, buf, SEED, opts, (old[0], old[1]), old[2], clip)
        stats = e.sac_update(1)
        state, rstats, _ = SN.update(pol, state, buf, SEED, opts, (o["shift"], o["scale"]), r["scale"], clip)
        _assert_state(e.sac_state(), state, (clip, rnd))
        _assert_stats(stats, rstats, (clip, rnd))
        assert not _same(stale["psi"], state["psi"]) and not _same(stale["theta"], state["theta"])
        old = (o["shift"], o["scale"], r["scale"])
        with np.errstate(all="ignore"):
            mags.append(np.abs((buf["r"] * F(opts["reward_scale"])) * r["scale"]))
    e.close()
    return np.concatenate(mags)


def test_moving_vectors_and_multiplier_reach_the_next_update(amd):
    """after sac_norm_update the next update equals sac_norm_ref on the fetched raw ring with rows normalised by the NEW vectors and
    targets from sac_y_norm under the new multiplier, two rounds: once without a clip, once with a clip that binds on some
    transitions only (the median of the ring's |scaled reward|, taken from the first pass on the host)"""
    mags = _moving_pass(amd, 0.0)
    clip = float(F(np.median(mags[mags > 0])))
    assert (mags > clip).any() and (mags < clip).any(), "the clip was meant to bind on some transitions only"
    _moving_pass(amd, clip)


# ---- 5. the ring wraps with raw rows ------------------------------------------------------------------------------------------------
def test_ring_wrap_keeps_the_skip_rule_and_the_raw_next_row(amd):
    """capacity 40, a horizon of 6 days: a store of 48 samples skips its first 8.  max_days 3: the third and the sixth day end every
    episode and auto-reset the env, so the last day's x' is the zero row; a further store of 2 days ends inside an episode: raw
    counts"""
    rng = np.random.default_rng(41)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options(capacity=40)
    e = _solo(amd, pol, crit, opts, horizon=6, norm=BOTH, engine_kw=dict(max_days=3, auto_reset=True))
    ring = T3.Ring(40, D, A)
    for rnd, days in enumerate((6, 2, 6)):
        assert _collect(e, days) == days * N
        rec, now = e.rollout_fetch(), _raw_input(e)
        ring.store(rec, now)
        _assert_buffer(e.sac_buffer(), ring.buffer(), rnd)
        done_last = rec["terminated"][-1] | rec["truncated"][-1]
        if days == 6 and rnd == 0:
            assert done_last.all() and (now == 0).all() and (rec["obs"][0] == 0).all() and (rec["obs"][3] == 0).all() and np.abs(rec["obs"][1]).max() > 1.0
        if days == 2:
            assert not done_last.any() and np.abs(now).max() > 1.0 and _same(now, R.flat_obs(e.fetch()).astype(F))
    buf = e.sac_buffer()
    assert buf["size"] == 40 and buf["written"] == 14 * N
    e.sac_norm_update()
    e.sac_update(2)                                                 # (the wrapped ring is sampled)
    e.close()


# ---- 6. populations -----------------------------------------------------------------------------------------------------------------
OWN = (dict(gamma=0.9, reward_scale=0.5, init_alpha=0.3), dict(gamma=0.99, reward_scale=0.1, init_alpha=0.6, seed=77),
       dict(gamma=0.95, reward_scale=0.25, init_alpha=1.0, alpha_lr=0.0))


def test_population_per_member_equals_solo_engines(amd):
    """M = 3 x 4 envs, per-member normalisers, the members' own gamma, reward_scale and temperature: after two iterations with
    normaliser updates every member's state, ring, statistics and normalisers are those of a solo engine of its envs at
    env_id_base = m n"""
    M, n = 3, 4
    pols, crits = _members(51, M)
    opts = [_options(**OWN[m]) for m in range(M)]
    norm = dict(BOTH, rew_clip=0.8)
    planes = _planes(M * n)
    e = _population(amd, pols, crits, opts, norm=dict(norm, per_member=True), planes=planes)
    solos = [_solo(amd, pols[m], crits[m], opts[m], planes=planes[:, m * n:(m + 1) * n], env_id_base=m * n, norm=norm) for m in range(M)]
    for it in range(2):
        assert _collect(e, pop=True) == T * n
        assert e.sac_norm_update() == T * n
        stats = e.sac_pop_update(2)
        for m, s in enumerate(solos):
            _collect(s)
            s.sac_norm_update()
            sstats = s.sac_update(2)
            _assert_stats(stats[m], sstats, (it, m))
            _assert_state(e.sac_pop_state(m), s.sac_state(), (it, m))
            _assert_buffer(e.sac_pop_buffer(m), s.sac_buffer(), (it, m))
            _assert_norm(_norm_state(e, m, n), _norm_state(s), (it, m))
    a, b = _norm_state(e, 0, n), _norm_state(e, 1, n)
    assert not _same(a[0]["shift"], b[0]["shift"]) and a[1]["scale"] != b[1]["scale"]
    # sac_pop_copy leaves the normalisers alone
    e.sac_pop_copy(0, 1)
    _assert_norm(_norm_state(e, 1, n), b, "sac_pop_copy")
    e.close()
    for s in solos:
        s.close()


def test_population_with_a_shared_normaliser_equals_the_restatement(amd):
    from adcraft_amd import _ffi
    M, n = 2, N // 2
    pols, crits = _members(52, M)
    opts = [_options(**OWN[m]) for m in range(M)]
    e = _population(amd, pols, crits, opts, norm=dict(BOTH, rew_clip=0.8))
    gammas = np.repeat(np.array([o["gamma"] for o in opts], F), n)
    o, r = SN.obs_fresh(D, pols[0].shift, pols[0].scale), SN.rew_fresh(N)
    for it in range(2):
        _collect(e, pop=True)
        assert e.sac_norm_update() == T * N
        rec = e.rollout_fetch()
        rows = NR.member_rows(rec["obs"], 0, N)
        o2, r2 = SN.obs_update(o, rows), SN.rew_update(r, rec["reward"], rec["terminated"], rec["truncated"], gammas)
        o = SN.twin_obs(_ffi.lib(), o, rows)
        r = SN.twin_rew(_ffi.lib(), r, rec["reward"], rec["terminated"], rec["truncated"], gammas)
        _assert_norm((o, r), (o2, r2), ("twin against restatement", it))
        _assert_norm(_norm_state(e), (o, r), it)
        # every member's update: the restatement on its raw ring under the shared vectors and multiplier
        states, bufs = [e.sac_pop_state(m) for m in range(M)], [e.sac_pop_buffer(m) for m in range(M)]
        stats = e.sac_pop_update(1)
        for m in range(M):
            ref, rstats, _ = SN.update(pols[m], states[m], bufs[m], opts[m]["seed"] or SEED, opts[m], (o["shift"], o["scale"]), r["scale"], 0.8)
            _assert_state(e.sac_pop_state(m), ref, (it, m))
            _assert_stats(stats[m], rstats, (it, m))
    with pytest.raises(_ffi.EngineStateError, match="shared"):
        e.sac_norm_copy([-1])
    e.close()


# ---- 7. prioritised replay under the normalisers ------------------------------------------------------------------------------------
def test_prioritised_replay_follows_the_normalised_errors(amd):
    """with replay_prio_init over a SAC trainer with live normalisers: the batch slots, the importance weights and the tree's
    leaves, top and total after each of 2 updates equal per_ref.py driven by the |d| of the normalised inputs and target; the
    normaliser's update leaves the tree alone"""
    rng = np.random.default_rng(71)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options()
    per = PR.options()
    e = _solo(amd, pol, crit, opts, norm=dict(BOTH, rew_clip=0.8))
    e.replay_prio_init(**per)
    assert _collect(e) == T * N
    leaves = e.replay_prio_fetch()
    e.sac_norm_update()
    assert _same(e.replay_prio_fetch(), leaves), "the tree is untouched by the normaliser"
    (o, r), buf = _norm_state(e), e.sac_buffer()
    tree = PR.Tree(CAP)
    tree.fill(range(T * N))
    state = S.fresh_state(pol, crit, opts)
    plain = PR.Tree(CAP)
    plain.fill(range(T * N))
    for u in range(2):
        idx, w = e.replay_prio_batch(u)
        stats = e.sac_update(1)
        if u == 0:
            PR.sac_update(pol, state, buf, SEED, opts, plain, per)              # (the raw rows and sac_y: other errors, other leaves)
        state, rstats, extra = SN.update(pol, state, buf, SEED, opts, (o["shift"], o["scale"]), r["scale"], 0.8, tree=tree, per=per)
        assert _same(idx, extra["idx"]) and _same(w, extra["w"]), u
        _assert_state(e.sac_state(), state, u)
        _assert_stats(stats, rstats, u)
        info = e.replay_prio_info()
        assert _same(e.replay_prio_fetch(), tree.leaf[:T * N]), ("leaf", u)
        assert _same(info["top"], F(tree.top)) and _same(info["total"], np.float64(tree.total)), ("top, total", u)
    assert not np.all(tree.leaf[:T * N] == 1) and not _same(plain.leaf[:T * N], tree.leaf[:T * N]), "the priorities are those of the normalised errors"
    e.close()


# ---- 8. a PBT round carries the normalisers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ring", [True, False])
def test_pbt_round_copies_the_donors_normalisers(amd, with_ring):
    from adcraft_amd.baselines.pbt import PBTScheduler
    from adcraft_amd.baselines.sac_trainer import SACPopulationTrainer
    M, n = 4, 2
    pols, crits = _members(61, M)
    e = _engine(amd, _planes(), **RESETS)
    cfgs = [dict(critic_hidden=WIDTHS[:-1], batch_size=B, capacity=CAP, learning_starts=0, updates_per_iteration=2, critics=crits[m],
                 gamma=float(F(0.9 + 0.02 * m)), reward_scale=float(F(0.5 / (m + 1))), tau=0.05, actor_lr=3e-3, critic_lr=3e-3, alpha_lr=3e-3,
                 init_alpha=float(F(0.3 + 0.1 * m))) for m in range(M)]
    tr = SACPopulationTrainer(e, pols, cfgs, *_bounds(), horizon=T, normalize_observations=True, normalize_rewards=True, norm=dict(rew_clip=0.8))
    sch = PBTScheduler(tr, replace_fraction=0.25, tuned=("tau",), bounds={"tau": (0.01, 0.1)}, factors=(0.5, 2.0), with_ring=with_ring)
    assert sch.kind == "sac" and sch.replace_count == 1
    tr.iteration(budget=BUDGET)
    before = [_norm_state(e, m, n) for m in range(M)]
    rings = [e.sac_pop_buffer(m) for m in range(M)]
    res = sch.step()
    (dst,) = np.nonzero(res["src"] >= 0)[0]
    src = int(res["src"][dst])
    after = [_norm_state(e, m, n) for m in range(M)]
    assert SN.obs_same(after[dst][0], before[src][0]) and SN.rew_same(after[dst][1], before[src][1], returns=False)
    assert not SN.obs_same(before[dst][0], before[src][0])
    assert _same(after[dst][1]["returns"], before[dst][1]["returns"]), "the carry is the envs' and stays"
    for m in range(M):
        if m != dst:
            _assert_norm(after[m], before[m], ("untouched", m))
    ring = e.sac_pop_buffer(dst)
    _assert_buffer(ring, rings[src if with_ring else dst], "the ring holds raw rows either way")
    # the destination's next update: the restatement on its ring under the donor's vectors and multiplier
    opts = S.options(K, **dict(tr.configs[dst], seed=0))
    state = e.sac_pop_state(dst)
    e.sac_pop_update(1)
    o, r = after[dst]
    ref, _, _ = SN.update(tr._templates[dst], state, ring, SEED, opts, (o["shift"], o["scale"]), r["scale"], 0.8)
    _assert_state(e.sac_pop_state(dst), ref, "after the round")
    assert _same(tr.policy(dst).policy.shift, before[src][0]["shift"]), "policy() exports the current vectors"
    e.close()


# ---- 9. resume ----------------------------------------------------------------------------------------------------------------------
def test_a_resumed_run_continues_to_the_same_bits(amd):
    from adcraft_amd.baselines.sac_trainer import SACTrainer
    rng = np.random.default_rng(91)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options(seed=9)
    cfg = {k: v for k, v in opts.items() if k != "critic_widths"}

    def make():
        e = _engine(amd, _planes(), **RESETS)
        return e, SACTrainer(e, pol, *_bounds(), critic_hidden=WIDTHS[:-1], horizon=T, learning_starts=0, updates_per_iteration=3, critics=crit,
                             normalize_observations=True, normalize_rewards=True, rew_clip=0.8, obs_count_cap=40, **cfg)
    e1, t1 = make()
    t1.iteration(budget=BUDGET)
    saved = t1.state(), e1.sac_buffer()
    assert {"obs_count", "obs_mean", "obs_M2", "shift", "scale", "rew_count", "rew_mean", "rew_M2", "rew_scale", "returns"} <= set(saved[0]["norm"])
    s1 = t1.iteration(budget=BUDGET)
    e2, t2 = make()
    e2.run_days("mlp", T, BUDGET)                                   # (the envs' and the agents' streams, as after iteration 1; not stored)
    t2.load_state(saved[0])
    e2.sac_buffer_load(saved[1])
    _assert_norm(SN.split(t2.norm_state()), SN.split(saved[0]["norm"]), "loaded")
    s2 = t2.iteration(budget=BUDGET)
    _assert_stats(s1, s2)
    _assert_state(t1.state(), t2.state())
    _assert_buffer(e1.sac_buffer(), e2.sac_buffer())
    _assert_norm(SN.split(t1.norm_state()), SN.split(t2.norm_state()), "after iteration 2")
    assert saved[0]["norm"]["obs_count"] == T * N and t1.norm_state()["obs_count"] == 40
    assert _same(t1.policy().policy.shift, t1.norm_state()["shift"]) and not _same(t1.policy().policy.shift, pol.shift)
    e1.close()
    e2.close()


# ---- 10. off means off --------------------------------------------------------------------------------------------------------------
def test_without_a_normaliser_nothing_changed_and_the_record_goes_back(amd):
    rng = np.random.default_rng(101)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options()
    e = _solo(amd, pol, crit, opts)
    ring, state = T3.Ring(CAP, D, A), S.fresh_state(pol, crit, opts)
    _collect(e)
    rec = e.rollout_fetch()
    ring.store(rec, T3.current_input(pol, e.fetch(), e.get_episode_state()[0] == 0))
    _assert_buffer(e.sac_buffer(), ring.buffer())
    assert _same(rec["obs"][0], SN.normalize(np.zeros((N, D), F), pol.shift, pol.scale)), "network inputs: the first day's row is (0 - shift) * scale"
    for u in range(2):
        stats = e.sac_update(1)
        state, rstats = S.update(pol, state, ring.buffer(), SEED, opts)
        _assert_state(e.sac_state(), state, u)
        _assert_stats(stats, rstats, u)
    # a normaliser that ended through rollout_enable: the record holds network inputs again
    e2 = _solo(amd, pol, crit, opts, norm=BOTH)
    _collect(e2)
    assert (e2.rollout_fetch()["obs"][0] == 0).all()
    e2.rollout_enable(T, obs=True)
    e2.sac_init(**opts)
    e2.sac_set_critics(crit)
    e2.reset()
    _collect(e2)
    assert _same(e2.rollout_fetch()["obs"][0], rec["obs"][0])
    e.close()
    e2.close()


# ---- 11. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(amd):
    from adcraft_amd import _ffi
    rng = np.random.default_rng(111)
    pol, crit, opts = _policy(rng), T3.random_critics_for_tests(rng, K, WIDTHS), _options()
    e = _engine(amd, _planes(), **RESETS)
    e.mlp_init(pol, deterministic=False)
    e.mlp_set_squash(*_bounds())
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="sac_init"):
        e.sac_norm_init(**BOTH)                                     # no trainer
    for call in (lambda: e.sac_norm_update(), lambda: e.sac_norm_state(), lambda: e.sac_norm_returns(), lambda: e.sac_norm_copy([-1])):
        with pytest.raises(_ffi.EngineStateError, match="sac_norm_init"):
            call()
    e.sac_init(**opts)
    e.sac_set_critics(crit)
    with pytest.raises(ValueError, match="population"):
        e.sac_norm_init(per_member=True, **BOTH)                    # per_member without a population
    # the existing refusals over a SAC trainer stay
    with pytest.raises(_ffi.EngineStateError, match="td3_init"):
        e.td3_norm_init(**BOTH)
    with pytest.raises(_ffi.EngineStateError, match="soft actor-critic"):
        e.obs_norm_init()
    with pytest.raises(_ffi.EngineStateError):
        e.rew_norm_init()
    e.run_days("mlp", 1, BUDGET)
    with pytest.raises(_ffi.EngineStateError, match="must be empty"):
        e.sac_norm_init(**BOTH)                                     # a non-empty record
    e.sac_store()
    e.rollout_reset()
    with pytest.raises(_ffi.EngineStateError, match="must be empty"):
        e.sac_norm_init(**BOTH)                                     # a non-empty ring
    e.sac_init(**opts)                                              # (a new trainer: an empty ring)
    e.sac_set_critics(crit)
    e.sac_norm_init(**BOTH)
    with pytest.raises(_ffi.EngineStateError, match="no day has been recorded"):
        e.sac_norm_update()                                         # no new day
    with pytest.raises(_ffi.EngineStateError, match="td3_norm_init"):
        e.td3_norm_state()                                          # the TD3 family does not see a SAC normaliser
    with pytest.raises(_ffi.EngineStateError, match="td3_init"):
        e.td3_norm_init(**BOTH)
    with pytest.raises(_ffi.EngineStateError, match="shared"):
        e.sac_norm_copy([-1])
    with pytest.raises(ValueError, match="no such normaliser"):
        e.sac_norm_state(1)
    with pytest.raises(ValueError, match="one value per env"):
        e.sac_norm_returns(np.zeros(3))
    # the engine is usable after every refusal
    _collect(e)
    assert e.sac_norm_update() == T * N
    e.sac_update(2)
    # the normaliser ends with its trainer
    for end in (lambda: e.sac_init(**opts), lambda: e.rollout_enable(T, obs=True), lambda: e.mlp_init(pol, deterministic=False)):
        end()
        with pytest.raises(_ffi.EngineStateError, match="sac_norm_init"):
            e.sac_norm_state()
        e.mlp_init(pol, deterministic=False)
        e.mlp_set_squash(*_bounds())
        e.rollout_enable(T, obs=True)
        e.sac_init(**opts)
        e.sac_set_critics(crit)
        e.sac_norm_init(rewards=True)
        assert "obs_count" not in e.sac_norm_state()
    # a policy without normalisation cannot have its observations normalised; its rewards can
    plain = S.sac_policy(rng, K, HIDDEN, "tanh", clamp=(-1.0, -0.5), normalize=False, scale=0.6)
    e.mlp_init(plain, deterministic=False)
    e.mlp_set_squash(*_bounds())
    e.rollout_enable(T, obs=True)
    e.sac_init(**opts)
    e.sac_set_critics(crit)
    with pytest.raises(ValueError, match="without normalisation"):
        e.sac_norm_init(observations=True)
    e.sac_norm_init(rewards=True)
    _collect(e)
    assert e.sac_norm_update() == T * N
    e.sac_update(1)
    e.close()
    # the SAC family on a TD3 engine: refused with a message that names sac_init; the engine trains on
    tpol = R.random_policy(rng, K, HIDDEN, "tanh", normalize=True, scale=0.6)
    tpol.shift, tpol.scale = R.realistic_norm(K)
    tpol.log_std = np.full(A, np.log(0.2), F)
    t = _engine(amd, _planes(), **RESETS)
    t.mlp_init(tpol, deterministic=False)
    t.rollout_enable(T, obs=True)
    t.td3_init(**T3.options(critic_widths=WIDTHS, batch_size=B, capacity=CAP))
    t.td3_set_critics(crit)
    with pytest.raises(_ffi.EngineStateError, match="sac_init"):
        t.sac_norm_init(**BOTH)
    t.td3_norm_init(**BOTH)
    for call in (lambda: t.sac_norm_update(), lambda: t.sac_norm_state(), lambda: t.sac_norm_returns(), lambda: t.sac_norm_copy([-1])):
        with pytest.raises(_ffi.EngineStateError, match="sac_init"):
            call()                                                  # (a TD3 normaliser is not a SAC one)
    t.rollout_reset()
    t.run_days("mlp", T, BUDGET)
    t.td3_store()
    assert t.td3_norm_update() == T * N
    t.td3_update(2)
    t.close()
    # chained copies are refused under per-member normalisers
    pols, crits = _members(112, 4)
    p = _population(amd, pols, crits, [_options()] * 4, norm=dict(BOTH, per_member=True))
    with pytest.raises(ValueError, match="also a source"):
        p.sac_norm_copy([1, 2, -1, -1])
    with pytest.raises(ValueError, match="one source per member"):
        p.sac_norm_copy([-1])
    p.sac_norm_copy([-1, 0, 2, 0])
    # a population's trainer ends with mlp_learners, and its normalisers with it
    p.mlp_learners(4)
    with pytest.raises(_ffi.EngineStateError, match="sac_norm_init"):
        p.sac_norm_state()
    p.close()
