"""GPU parity of the observation history (MLPPolicy(frames=H); csrc/adc_mlp.h, "Observation history") with the numpy restatement
tests/stack_ref.py composed with mlp_ref / pg_ref / pg_kl_ref / pg_shuffle_ref / td3_ref / sac_ref / per_ref: the act on stacked
rows through auto-resets (populations and learners), H = 1 through the new entry point, breaks and forgets, env groups, a PPO
update, TD3 and SAC stores and updates, resumed trainers, refusals.  Every comparison is bitwise.  None of the entry points
exists before this feature."""
import copy
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import per_ref as PR
from tests import pg_kl_ref as KR
from tests import pg_ref as P
from tests import pg_shuffle_ref as SH
from tests import sac_ref as SR
from tests import stack_ref as S
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F = np.float32
SEED, BUDGET = 43, 1000.0
RESETS = dict(max_days=4, auto_reset=True)
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)


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


def _planes(N, K, seed=SEED):
    return H.implicit_params(N, K, seed + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, seed=SEED, env_id_base=0, **kw):
    _, N, K = planes.shape
    e = amd.StepEngine(N, K, seed=seed, env_id_base=env_id_base, **kw)
    e.set_all_params(planes)
    e.reset()
    return e


def _stacked_norm(K, frames, rng=None, vary=0.0):
    """realistic_norm per frame (older frames a little different, so that a frame in the wrong place shows)"""
    shift, scale = R.realistic_norm(K)
    shift = np.concatenate([shift + F(0.25 * f) for f in range(frames)]).astype(F)
    scale = np.concatenate([scale * F(1.0 + 0.125 * f) for f in range(frames)]).astype(F)
    if vary:
        shift = (shift + rng.standard_normal(shift.size).astype(F) * F(vary)).astype(F)
        scale = (scale * np.exp(rng.standard_normal(scale.size) * vary).astype(F)).astype(F)
    return shift, scale


def _policy(rng, K, frames, act="tanh", normalize=True, hidden=(16, 8), two=False, value=True, **kw):
    pol = S.random_policy(rng, K, frames, hidden, act, two_heads=two, value=value, normalize=normalize, scale=0.6 if normalize else 0.05, **kw)
    if normalize:
        pol.shift, pol.scale = _stacked_norm(K, frames)
    pol.layers[-1][1][1:K + 1] += F(0.8)                           # bids around 80 cents: auctions are won
    return pol


def _now(e):
    """(raw frame 0, episode day) an act would read now"""
    day = e.get_episode_state()[0].astype(np.int64)
    x = R.flat_obs(e.fetch()).astype(F)
    x[day == 0] = 0
    return x, day


def _days(e, hist, T, budget=BUDGET):
    """T days of mlp_step with the restatement's history alongside: the raw stacked rows [T, N, D] every act read"""
    rows = []
    for _ in range(T):
        rows.append(hist.row(*_now(e)))
        e.mlp_step(budget)
    return np.stack(rows)


def _assert_history(e, hist, what=""):
    st, ref = e.mlp_history_state(), hist.state()
    for k in ("hist", "last", "from"):
        assert _same(st[k], ref[k]), (k, what, st[k], ref[k])


def _with(pol, shift, scale):
    out = copy.copy(pol)
    out.shift, out.scale = shift, scale
    return out


# ---- 1. act parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["population", "learners"])
@pytest.mark.parametrize("frames", [2, 3, 8])
@pytest.mark.parametrize("K", [3, 7])
def test_act_parity_on_stacked_rows(amd, K, frames, kind):
    """D0 = 17 and 37: frame boundaries fall inside a chain block of 32.  max_days 4 and 2H + 3 recorded days: every env passes
    several auto-resets.  The recorded obs rows are the restatement's stacked rows (normalised per position), and actions,
    log-probabilities and values are mlp_ref.act's on them, tanh with and relu without normalisation.  A population
    (k_mlp_policy<1>, 5 envs on 2 members) and learners (k_mlp_policy<2>, M = 2 with a normaliser each; 6 envs, as the members'
    envs must be equally many)."""
    T, A = 2 * frames + 3, K + 1
    N = 5 if kind == "population" else 6
    for act, normalize in (("tanh", True), ("relu", False)):
        rng = np.random.default_rng(1000 * K + 10 * frames + (kind == "learners"))
        pols = [_policy(rng, K, frames, act, normalize) for _ in range(2)]
        seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
        e = _engine(amd, _planes(N, K), **RESETS)
        e.mlp_init(pols[0], seeds, deterministic=False)
        assert e.mlp_frames() == frames and e.mlp_input_size() == frames * (5 * K + 2)
        if kind == "population":
            member = np.array([0, 1, 1, 0, 1], np.int32)
            e.mlp_population(2, member)
            e.mlp_set_member(1, pols[1])
            pols[1] = _with(copy.copy(pols[1]), pols[0].shift, pols[0].scale)       # (value network, log_std and vectors stay shared)
            pols[1].value_layers, pols[1].log_std = pols[0].value_layers, pols[0].log_std
        else:
            member = np.arange(N) // (N // 2)
            e.mlp_learners(2)
            e.mlp_set_learner(1, pols[1])
        e.rollout_enable(T, obs=True)
        if kind == "learners" and normalize:
            e.obs_norm_init(per_member=True)
            sh1, sc1 = _stacked_norm(K, frames, rng, vary=0.2)
            st = e.obs_norm_state(1)
            st["shift"], st["scale"] = sh1, sc1
            e.obs_norm_state(1, st)
            pols[1] = _with(pols[1], sh1, sc1)
        hist = S.History(N, K, frames)
        raw = _days(e, hist, T)
        rec = e.rollout_fetch(bootstrap=True)
        done = rec["terminated"] | rec["truncated"]
        assert (done.sum(axis=0) == T // 4).all() and T // 4 >= 1, "every env passes an auto-reset every four days"
        keys = [R.agent_key(s) for s in seeds]
        for m in range(2):
            envs = np.flatnonzero(member == m)
            for t in range(T):
                x = S.normalized(pols[m], raw[t][envs])
                assert _same(rec["obs"][t][envs], x), (act, m, t)
                ref = R.act(pols[m], raw[t][envs], R.normals([keys[n] for n in envs], [t] * len(envs), A))
                for k in ("action", "logp", "value"):
                    assert _same(rec[k][t][envs], ref[k]), (act, m, t, k)
            # the bootstrap value is the value network on the row an act would read now, and reading it wrote nothing
            peek = hist.row(*_now(e), commit=False)
            assert _same(rec["bootstrap_value"][envs], R.act(pols[m], peek[envs], None, deterministic=True)["value"]), (act, m)
        assert np.abs(raw[:, :, 5 * K + 2:]).sum() > 0 and (raw[done.argmax(axis=0) + 1, np.arange(N), 5 * K + 2:] == 0).all()
        _assert_history(e, hist, (act, kind))
        e.close()


# ---- 2. H = 1 through the new entry point -----------------------------------------------------------------------------------------
def test_one_frame_through_the_new_entry_point_is_mlp_init(amd):
    import ctypes as C
    from adcraft_amd._ffi import check
    N, K, T = 5, 7, 6
    rng = np.random.default_rng(5)
    pol = _policy(rng, K, 1)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    out = []
    for new in (False, True):
        e = _engine(amd, _planes(N, K), **RESETS)
        if new:
            cfg = pol.config(K, False)
            check(e._lib.adc_engine_mlp_init_frames(e._h, C.byref(cfg), seeds.ctypes.data, 1))
            e._mlp, e._frames, e._members, e._learners = pol, 1, 0, 0
            e.mlp_set_weights(pol)
        else:
            e.mlp_init(pol, seeds, deterministic=False)
        assert e.mlp_frames() == 1 and e.mlp_history_state() is None
        e.rollout_enable(T, obs=True)
        e.run_days("mlp", T, BUDGET)
        out.append((e.rollout_fetch(bootstrap=True), e.mlp_last(), e.mlp_agent_state(), e.get_rng_state()))
        e.close()
    (ra, la, aa, sa), (rb, lb, ab, sb) = out
    for k in ra:
        assert _same(ra[k], rb[k]), k
    for k in la:
        assert _same(la[k], lb[k]), k
    assert all(_same(x, y) for x, y in zip(aa, ab)) and all(np.array_equal(x, y) for x, y in zip(sa, sb))


# ---- 3. break and forget ------------------------------------------------------------------------------------------------------------
def test_break_forget_replay_and_peek(amd):
    N, K, frames = 4, 3, 3
    D0, A = 5 * K + 2, K + 1
    rng = np.random.default_rng(9)
    pol = _policy(rng, K, frames)
    e = _engine(amd, _planes(N, K), **NO_RESETS)
    e.mlp_init(pol, deterministic=False)
    hist = S.History(N, K, frames)
    _assert_history(e, hist, "fresh: no env has acted")
    rows = _days(e, hist, 3)
    assert np.abs(rows[2][:, D0:2 * D0]).sum() > 0 and (rows[2][:, 2 * D0:] == 0).all(), "day 2 reads day 1's frame and day 0's zeros"
    _assert_history(e, hist, "three days")
    # mlp_act twice on one day with replayed normals: the same row, the history unchanged
    z = rng.standard_normal((N, A)).astype(F)
    row = hist.row(*_now(e))
    assert np.abs(row[:, 2 * D0:]).sum() > 0
    e.mlp_act(BUDGET, z)
    first = e.mlp_last()
    _assert_history(e, hist, "first act of day 3")
    for k, v in R.act(pol, row, z).items():
        assert k not in first or _same(first[k], v), k
    e.mlp_act(BUDGET, z)
    second = e.mlp_last()
    assert all(_same(first[k], second[k]) for k in first)
    assert _same(hist.row(*_now(e)), row)
    _assert_history(e, hist, "second act of day 3")
    # mlp_bootstrap_value writes nothing
    before = e.mlp_history_state()
    boot = e.mlp_bootstrap_value()
    after = e.mlp_history_state()
    assert all(_same(before[k], after[k]) for k in before)
    assert _same(boot, R.act(pol, hist.row(*_now(e), commit=False), None, deterministic=True)["value"])
    # one day stepped with fixed actions between two acts: older frames read as zeros from then on
    e.step_device()                                                 # day 3 under the last act's actions
    e.step_device()                                                 # day 4 without an act
    row = hist.row(*_now(e))
    assert (row[:, D0:] == 0).all() and np.abs(row[:, :D0]).sum() > 0
    e.mlp_act(BUDGET, z)
    assert _same(e.mlp_last()["mean"], R.act(pol, row, z)["mean"])
    _assert_history(e, hist, "after a day without the agent")
    e.step_device()
    row = hist.row(*_now(e))
    assert np.abs(row[:, D0:2 * D0]).sum() > 0 and (row[:, 2 * D0:] == 0).all()
    e.mlp_act(BUDGET, z)
    assert _same(e.mlp_last()["mean"], R.act(pol, row, z)["mean"])
    # a masked explicit reset: only the reset envs forget
    mask = np.array([1, 0, 0, 1], np.uint8)
    e.reset(env_mask=mask)
    hist.forget(mask)
    _assert_history(e, hist, "masked reset")
    x, day = _now(e)
    assert (day[mask == 1] == 0).all() and (day[mask == 0] > 0).all()
    row = hist.row(x, day)
    assert (row[mask == 1] == 0).all() and np.abs(row[mask == 0][:, D0:2 * D0]).sum() > 0
    e.mlp_act(BUDGET, z)
    assert _same(e.mlp_last()["mean"], R.act(pol, row, z)["mean"])
    _assert_history(e, hist, "the act after the masked reset")
    # the state goes out and back in
    st = e.mlp_history_state()
    e.mlp_set_history_state({"hist": np.zeros_like(st["hist"]), "last": np.full(N, -2, np.int32), "from": np.zeros(N, np.int32)})
    assert not e.mlp_history_state()["hist"].any()
    e.mlp_set_history_state(st)
    _assert_history(e, hist, "restored")
    e.close()


# ---- 4. env groups --------------------------------------------------------------------------------------------------------------------
def test_env_groups_give_the_same_record_and_history(amd):
    N, K, frames, T = 8, 3, 3, 7
    rng = np.random.default_rng(4)
    pol = _policy(rng, K, frames)
    seeds = np.arange(N, dtype=np.uint64) + 1
    out = []
    for groups in (1, 4):
        e = _engine(amd, _planes(N, K), **RESETS)
        e.set_env_groups(groups)
        e.mlp_init(pol, seeds, deterministic=False)
        e.rollout_enable(T, obs=True)
        e.run_days("mlp", T, BUDGET)
        assert e.env_groups() == groups
        out.append((e.rollout_fetch(bootstrap=True), e.mlp_history_state()))
        e.close()
    (ra, ha), (rb, hb) = out
    for k in ra:
        assert _same(ra[k], rb[k]), k
    for k in ha:
        assert _same(ha[k], hb[k]), k
    assert np.abs(ra["obs"][:, :, 5 * K + 2:]).sum() > 0 and len({tuple(r) for r in ha["hist"].reshape(N, -1)}) == N


# ---- 5. PPO ---------------------------------------------------------------------------------------------------------------------------
def _fresh_pg(pol):
    theta = P.flat_params(pol)
    return dict(theta=theta, m=np.zeros_like(theta), v=np.zeros_like(theta), steps=0)


def test_a_ppo_update_on_stacked_rows(amd):
    """K = 3, H = 3, N = 4, T = 5: one pg_update of two epochs with the KL add-on and shuffled minibatches of 7 equals the
    restatements fed the stacked rows; the queued update gives the same bits"""
    N, K, frames, T, mb = 4, 3, 3, 5, 7
    rng = np.random.default_rng(31)
    pol = _policy(rng, K, frames)
    seeds = np.arange(N, dtype=np.uint64) + 7
    opts = P.options(lr=3e-3, vf_coef=1.0)
    kl_opts = KR.kl_options(kl_coef=0.5, adaptive=True, vf_clip=10.0)
    sh = SH.shuffle_options(minibatch_samples=mb)
    got = []
    for queued in (False, True):
        e = _engine(amd, _planes(N, K), **RESETS)
        e.mlp_init(pol, seeds, deterministic=False)
        e.rollout_enable(T, obs=True)
        e.pg_init(**opts)
        e.pg_kl_init(**kl_opts)
        e.pg_shuffle_init(**sh)
        hist = S.History(N, K, frames)
        raw = _days(e, hist, T)
        rec = e.rollout_fetch(bootstrap=True)
        assert _same(rec["obs"], np.stack([S.normalized(pol, r) for r in raw]))
        assert _same(rec["bootstrap_value"], R.act(pol, hist.row(*_now(e), commit=False), None, deterministic=True)["value"])
        stats = e.pg_update(2, queued=queued)
        got.append((e.pg_state(), stats, e.pg_kl_stats(), e.pg_shuffle_stats(), rec))
        _assert_history(e, hist, "the update writes no history")
        e.close()
    (state, stats, kst, sst, rec), (qstate, qstats, qkst, qsst, _) = got
    ref, rstats, rkst, rsst = SH.update(pol, _fresh_pg(pol), rec, rec["bootstrap_value"], 2, opts, sh, SEED, kl_opts, kl_opts["kl_coef"])
    for k in ("theta", "m", "v"):
        assert _same(state[k], ref[k]) and _same(qstate[k], ref[k]), k
    assert state["steps"] == qstate["steps"] == ref["steps"] == 2 * 3
    for k in P.STAT_KEYS:
        assert _same(np.float64(stats[k]), np.float64(rstats[k])) and _same(np.float64(qstats[k]), np.float64(rstats[k])), k
    for k in ("kl", "vf_clip_fraction"):
        assert _same(np.float64(kst[k]), np.float64(rkst[k])) and _same(np.float64(qkst[k]), np.float64(rkst[k])), k
    assert _same(F(kst["kl_coef_next"]), F(rkst["kl_coef_next"])) and sst == qsst == rsst


# ---- 6. TD3 and SAC ------------------------------------------------------------------------------------------------------------------
OFF = dict(N=3, K=3, frames=2, T=6, C=13, B=5)


def _sac_policy(rng, K, frames):
    pol = _policy(rng, K, frames, two=True, value=False, log_std_clamp=(-1.0, -0.5))
    pol.layers[-1][1][K + 1:] = np.linspace(-1.6, 0.1, K + 1).astype(F)
    return pol


def _bounds(K):
    return np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], 3.0 + np.arange(K) / 10.0]).astype(F)


def _off_engine(amd, family, pol, crit, opts, planes, seeds, case=None, env_id_base=0):
    e = _engine(amd, planes, env_id_base=env_id_base, **RESETS)
    e.mlp_init(pol, seeds, deterministic=False)
    if family == "sac":
        e.mlp_set_squash(*_bounds(pol.num_keywords))
    e.rollout_enable(OFF["T"], obs=True)
    getattr(e, family + "_init")(**opts)
    getattr(e, family + "_set_critics")(crit)
    if case == "norm":
        getattr(e, family + "_norm_init")(observations=True)
    if case == "prio":
        e.replay_prio_init(**PR.options())
    return e


def _off_options(family, K):
    common = dict(critic_widths=(12, 1), batch_size=OFF["B"], capacity=OFF["C"], seed=123, tau=0.05, gamma=0.9)
    if family == "sac":
        return SR.options(K, reward_scale=0.01, init_alpha=0.3, alpha_lr=3e-3, actor_lr=3e-3, critic_lr=3e-3, target_update_interval=2, **common)
    return T3.options(target_noise=0.3, target_noise_clip=0.25, reward_scale=0.5, **common)


@pytest.mark.parametrize("case", ["prio", "norm"])
@pytest.mark.parametrize("family", ["td3", "sac"])
def test_store_and_two_updates_on_stacked_rows(amd, family, case):
    """capacity 13, N = 3, T = 6, H = 2, max_days 4: the store passes an auto-reset and wraps the ring.  The ring is the
    restatement's Ring(capacity, H * D0, A) built from the stacked record, its last day's x' the peeked stacked row; two updates
    equal the restatement's.  `prio`: prioritised replay (rows normalised when stored).  `norm`: the family's running observation
    normaliser, never updated - raw stacked rows in the ring, vectors of length D applied as a batch is sampled."""
    N, K, frames, T, C = (OFF[k] for k in ("N", "K", "frames", "T", "C"))
    D, A = frames * (5 * K + 2), K + 1
    rng = np.random.default_rng(61)
    pol = _sac_policy(rng, K, frames) if family == "sac" else _policy(rng, K, frames, value=False)
    crit = S.random_critics(rng, K, frames, (12, 1))
    opts = _off_options(family, K)
    seeds = np.arange(N, dtype=np.uint64) + 11
    e = _off_engine(amd, family, pol, crit, opts, _planes(N, K), seeds, case)
    hist = S.History(N, K, frames)
    raw = _days(e, hist, T)
    assert getattr(e, family + "_store")() == T * N
    rec = e.rollout_fetch()
    peek = hist.row(*_now(e), commit=False)
    _assert_history(e, hist, "the store writes no history")
    stored = (lambda r: np.ascontiguousarray(r, F)) if case == "norm" else (lambda r: S.normalized(pol, r))
    assert _same(rec["obs"], np.stack([stored(r) for r in raw])), "the record holds the stacked rows"
    assert np.abs(peek[:, 5 * K + 2:]).sum() > 0, "the peeked row has an older frame"
    ring = T3.Ring(C, D, A)
    ring.store(rec, stored(peek))
    buf = getattr(e, family + "_buffer")()
    for k in ("x", "a", "r", "done", "x2"):
        assert _same(buf[k], ring.buffer()[k]), k
    assert (buf["size"], buf["written"]) == (C, T * N) and buf["done"].any() and not buf["done"].all()
    ref_buf = dict(buf)
    if case == "norm":
        ref_buf["x"], ref_buf["x2"] = S.normalized(pol, buf["x"]), S.normalized(pol, buf["x2"])
    tree = None
    if case == "prio":
        tree = PR.Tree(C)
        tree.fill([s % C for s in range(T * N)])
    with S.stacked_shapes():
        state = SR.fresh_state(pol, crit, opts) if family == "sac" else T3.fresh_state(pol, crit)
        for u in range(2):
            stats = getattr(e, family + "_update")(1)
            if family == "sac":
                state, rstats = PR.sac_update(pol, state, ref_buf, 123, opts, tree, PR.options()) if tree else SR.update(pol, state, ref_buf, 123, opts)
            else:
                state, rstats = PR.td3_update(pol, state, ref_buf, None, 123, opts, tree, PR.options()) if tree else T3.update(pol, state, ref_buf, None, 123, opts)
            got = getattr(e, family + "_state")()
            for k in (SR if family == "sac" else T3).STATE_KEYS:
                assert _same(got[k], state[k]), (k, u)
            for k in (SR if family == "sac" else T3).STAT_KEYS:
                assert _same(np.float64(stats[k]), np.float64(rstats[k])), (k, u)
    e.close()


@pytest.mark.parametrize("family", ["td3", "sac"])
def test_a_population_of_two_equals_two_solo_engines(amd, family):
    N, K, frames, T, M = 6, OFF["K"], OFF["frames"], OFF["T"], 2
    n = N // M
    rng = np.random.default_rng(71)
    make = (lambda: _sac_policy(rng, K, frames)) if family == "sac" else (lambda: _policy(rng, K, frames, value=False))
    pols = [make() for _ in range(M)]
    for p in pols[1:]:
        p.shift, p.scale = pols[0].shift, pols[0].scale
        if family == "td3":
            p.log_std = pols[0].log_std
    crits = [S.random_critics(rng, K, frames, (12, 1)) for _ in range(M)]
    opts = _off_options(family, K)
    seeds = np.arange(N, dtype=np.uint64) + 21
    planes = _planes(N, K)
    e = _engine(amd, planes, **RESETS)
    e.mlp_init(pols[0], seeds, deterministic=False)
    e.mlp_learners(M)
    e.mlp_set_learner(1, pols[1])
    if family == "sac":
        e.mlp_learners_set_squash(*_bounds(K))
    e.rollout_enable(T, obs=True)
    getattr(e, family + "_pop_init")([dict(opts, seed=123 + m) for m in range(M)])
    for m in range(M):
        getattr(e, family + "_pop_set_critics")(m, crits[m])
    e.run_days("mlp", T, BUDGET)
    getattr(e, family + "_pop_store")()
    getattr(e, family + "_pop_update")(2)
    hist = e.mlp_history_state()
    for m in range(M):
        s = _off_engine(amd, family, pols[m], crits[m], dict(opts, seed=123 + m), planes[:, m * n:(m + 1) * n], seeds[m * n:(m + 1) * n], env_id_base=m * n)
        s.run_days("mlp", T, BUDGET)
        getattr(s, family + "_store")()
        getattr(s, family + "_update")(2)
        got, want = getattr(e, family + "_pop_buffer")(m), getattr(s, family + "_buffer")()
        for k in ("x", "a", "r", "done", "x2"):
            assert _same(got[k], want[k]), (m, k)
        got, want = getattr(e, family + "_pop_state")(m), getattr(s, family + "_state")()
        for k in (SR if family == "sac" else T3).STATE_KEYS:
            assert _same(got[k], want[k]), (m, k)
        sh = s.mlp_history_state()
        for k in sh:
            assert _same(hist[k][m * n:(m + 1) * n], sh[k]), (m, k)
        s.close()
    e.close()


# ---- 7. resume -------------------------------------------------------------------------------------------------------------------------
def _env_state(e):
    return dict(rng=e.get_rng_state(), episode=e.get_episode_state(), agent=e.mlp_agent_state(), out=e.fetch(), params=e.get_all_params())


def _resume_pair(amd, make, iterate, snapshot):
    """three iterations in one go; two iterations, the trainer's state() into a fresh trainer on an engine driven through the same
    two iterations (the env's own state and the ring are the engine's, not the trainer's) whose history was then wiped, and the
    third: the same bits"""
    a = make()
    for _ in range(3):
        iterate(a)
    want = snapshot(a)
    b = make()
    for _ in range(2):
        iterate(b)
    saved = copy.deepcopy(b.state())
    assert "obs_history" in saved and np.abs(saved["obs_history"]["hist"]).sum() > 0
    c = make()
    for _ in range(2):
        iterate(c)                                                 # (the envs, the agents' ticks and the record's position)
    zero = {"hist": np.zeros_like(saved["obs_history"]["hist"]), "last": np.full_like(saved["obs_history"]["last"], -2), "from": saved["obs_history"]["from"] * 0}
    c.engine.mlp_set_history_state(zero)                            # (what a fresh engine would hold: the state must bring it back)
    c.load_state(saved)
    iterate(c)
    got = snapshot(c)
    for x in (a, b, c):
        x.engine.close()
    return got, want


def test_a_resumed_ppo_trainer_continues_bit_for_bit(amd):
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    N, K, frames, T = 4, 3, 3, 5
    pol = _policy(np.random.default_rng(81), K, frames)
    seeds = np.arange(N, dtype=np.uint64) + 3

    def make():
        return PGTrainer(_engine(amd, _planes(N, K), **RESETS), pol, T, agent_seeds=seeds, epochs=2, minibatches=2, lr=3e-3)

    def snapshot(t):
        st = t.state()
        return [st["theta"], st["m"], st["v"], st["obs_history"]["hist"], st["obs_history"]["last"], st["obs_history"]["from"],
                t.engine.rollout_fetch()["obs"]]
    got, want = _resume_pair(amd, make, lambda t: t.iteration(budget=BUDGET), snapshot)
    assert all(_same(g, w) for g, w in zip(got, want)), [_same(g, w) for g, w in zip(got, want)]


def test_a_resumed_sac_trainer_continues_bit_for_bit(amd):
    from adcraft_amd.baselines.sac_trainer import SACTrainer
    N, K, frames, T = 3, 3, 2, 6
    rng = np.random.default_rng(91)
    pol = _sac_policy(rng, K, frames)
    crit = S.random_critics(rng, K, frames, (12, 1))
    seeds = np.arange(N, dtype=np.uint64) + 5
    lo, hi = _bounds(K)

    def make():
        return SACTrainer(_engine(amd, _planes(N, K), **RESETS), pol, lo, hi, critic_hidden=(12,), horizon=T, learning_starts=10, updates_per_iteration=2,
                          agent_seeds=seeds, critics=crit, batch_size=5, capacity=40, seed=123)

    def snapshot(t):
        st, buf = t.state(), t.engine.sac_buffer()
        return [st[k] for k in SR.STATE_KEYS] + [st["obs_history"][k] for k in ("hist", "last", "from")] + [buf["x"], buf["x2"]]
    got, want = _resume_pair(amd, make, lambda t: t.iteration(budget=BUDGET), snapshot)
    assert all(_same(g, w) for g, w in zip(got, want)), [_same(g, w) for g, w in zip(got, want)]


# ---- 8. refusals leave the engine working -------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_working(amd):
    import ctypes as C
    from adcraft_amd import _ffi
    N, K, frames = 2, 3, 2
    D0 = 5 * K + 2
    rng = np.random.default_rng(2)
    e = _engine(amd, _planes(N, K), **NO_RESETS)
    one = _policy(rng, K, 1)
    cfg = one.config(K)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="frames"):
            _ffi.check(e._lib.adc_engine_mlp_init_frames(e._h, C.byref(cfg), None, bad))
    with pytest.raises(_ffi.EngineStateError, match="mlp_init"):
        e.mlp_frames()
    with pytest.raises(ValueError, match="inputs"):
        e.mlp_init(_policy(rng, K + 1, frames))                    # a first layer of the wrong width
    pol = _policy(rng, K, frames)
    e.mlp_init(pol, deterministic=False)
    with pytest.raises(ValueError, match=str(frames * D0)):
        e.mlp_set_norm(np.zeros(D0, F), np.ones(D0, F))            # vectors of length D
    e.mlp_set_norm(pol.shift, pol.scale)
    with pytest.raises(ValueError, match="shapes"):
        e.mlp_set_weights(_policy(rng, K, 1))
    with pytest.raises(ValueError, match="history"):
        e.mlp_set_history_state(None)
    with pytest.raises(ValueError, match="hist"):
        e.mlp_set_history_state({"hist": np.zeros((N, frames + 1, D0), F), "last": np.zeros(N, np.int32), "from": np.zeros(N, np.int32)})
    e.mlp_step(BUDGET)
    e.mlp_step(BUDGET)
    assert np.abs(e.mlp_history_state()["hist"]).sum() > 0
    e.mlp_init(one, deterministic=False)                           # back to one frame: no history
    assert e.mlp_frames() == 1 and e.mlp_history_state() is None
    assert e._lib.adc_engine_mlp_history_get(e._h, None, None, None) == _ffi.ADC_ESTATE
    e.mlp_step(BUDGET)
    e.close()


def test_an_lds_overflow_caused_by_the_frames_is_refused_by_name(amd):
    """K = 1024: one frame fits the act and the trainers; eight do not"""
    from adcraft_amd import _ffi
    N, K = 2, 1024
    rng = np.random.default_rng(3)
    e = _engine(amd, _planes(N, K), **NO_RESETS)
    with pytest.raises(ValueError, match="frames"):
        e.mlp_init(S.random_policy(rng, K, 8, (8,), value=True), deterministic=False)
    with pytest.raises(_ffi.EngineStateError, match="mlp_init"):
        e.mlp_act()                                                # (the refused init left no policy)
    pol = S.random_policy(rng, K, 4, (8,), value=True, scale=0.05)
    e.mlp_init(pol, deterministic=False)                           # 4 frames fit the act (150 KB) ...
    e.rollout_enable(2, obs=True)
    with pytest.raises(ValueError, match="frames"):
        e.pg_init(**P.options())                                   # ... and not the trainer (64 KB)
    with pytest.raises(ValueError, match="frames"):
        e.td3_init(**T3.options(critic_widths=(8, 1), batch_size=4, capacity=16))
    e.run_days("mlp", 2, BUDGET)                                   # the engine still works
    assert e.rollout_fetch()["obs"].shape == (2, N, 4 * (5 * K + 2))
    one = R.random_policy(rng, K, (8,), value=True, scale=0.05)
    e.mlp_init(one, deterministic=False)
    e.rollout_enable(2, obs=True)
    e.pg_init(**P.options())                                       # one frame at this K fits, as it did
    e.close()
