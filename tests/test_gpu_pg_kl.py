"""GPU tests of the PPO learners' KL penalty and value-loss clip (parts/kernel_pg_kl.inc, parts/pg_kl_api.inc) against the numpy
restatement tests/pg_kl_ref.py, bit for bit: the snapshot of the collecting distribution, every minibatch of an update, the
adaptive coefficient through the trainer, a learner population against solo engines, the copies, a resumed run, that nothing else
moved, and every refusal.  None of these symbols exists before this feature: every test here fails on the parent commit."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import pg_kl_ref as KR
from tests import pg_pop_ref as PP
from tests import pg_ref as P

pytestmark = pytest.mark.gpu
F = np.float32
BUDGET = 1000.0
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(autouse=True)
def time_limit(request):
    """every test under its own time limit (test_gpu_pg_trainer.py's)"""
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


def _planes(N, K, seed=41):
    return H.implicit_params(N, K, seed + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, seed=41, env_id_base=0, **kw):
    _, N, K = planes.shape
    e = amd.StepEngine(N, K, seed=seed, env_id_base=env_id_base, **dict(NO_RESETS, **kw))
    e.set_all_params(planes)
    e.reset()
    return e


def _policy(rng, K, hidden=(16, 8), act="tanh", two=False, **kw):
    pol = R.random_policy(rng, K, hidden, act, two_heads=two, value=True, normalize=True, scale=0.6, **kw)
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _trainer(amd, pol, N, K, T, opts, **engine_kw):
    e = _engine(amd, _planes(N, K), **engine_kw)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.pg_init(**opts)
    return e


def _fresh_state(pol):
    theta = P.flat_params(pol)
    return dict(theta=theta, m=np.zeros_like(theta), v=np.zeros_like(theta), steps=0)


def _assert_state(got, ref, what=""):
    for k in ("theta", "m", "v"):
        assert _same(got[k], ref[k]), (k, what)
    assert got["steps"] == ref["steps"], what


def _assert_stats(got, ref, what=""):
    for k in P.STAT_KEYS:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


def _assert_kl_stats(got, ref, what=""):
    for k in ("kl", "vf_clip_fraction"):
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)
    for k in ("kl_coef", "kl_coef_next"):
        assert _same(F(got[k]), F(ref[k])), (k, got[k], ref[k], what)


def _median_sq(pol, rec, opts):
    """the median squared value error of the record under its own value function: a cap that clips about half the samples"""
    adv, ret = P.gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], rec["bootstrap_value"], **opts)
    dv = (rec["value"] - ret).astype(F)
    return float(F(np.median((dv * dv).astype(np.float64))))


# ---- 1. the snapshot ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,K,hidden,two", [(8, 3, 3, (16, 8), False), (8, 3, 3, (16, 8), True), (8, 3, 9, (16, 8), False), (8, 3, 9, (16, 8), True),
                                              (4, 2, 256, (8,), False)])
def test_the_snapshot_is_the_acting_distribution(amd, N, T, K, hidden, two):
    """after run_days and pg_advantages the device's mean_old / ls_old equal the restatement's forward on the fetched record,
    and they are what the act used: from them and the agents' own normals come the record's actions and log-probabilities"""
    A = K + 1
    rng = np.random.default_rng(11 + K + two)
    pol = _policy(rng, K, hidden, two=two, log_std_clamp=(-1.5, 0.5) if two else None)
    e = _trainer(amd, pol, N, K, T, P.options())
    e.pg_kl_init(kl_coef=1.0)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch()
    e.pg_advantages()
    mean_old, ls_old = e.pg_kl_old_dist()
    rmean, rls = KR.snapshot(pol, P.flat_params(pol), rec)
    assert _same(mean_old, rmean)
    assert _same(ls_old, rls if two else rls[None, :])
    keys, ticks = e.mlp_agent_state()
    assert np.all(ticks == T)
    with np.errstate(all="ignore"):
        for t in range(T):
            z = R.normals([int(k) for k in keys], [t] * N, A)
            ls = ls_old[t] if two else np.broadcast_to(ls_old[0], (N, A))
            assert _same((mean_old[t] + R.exp32(ls) * z).astype(F), rec["action"][t]), t
            logp = (R.sum8(((-((z * z) * F(0.5))) - ls).T) - F(A) * R.HALF_LOG_2PI).astype(F)
            assert _same(logp, rec["logp"][t]), t
    assert np.abs(mean_old).max() > 0 and not _same(mean_old[0], mean_old[1])
    e.close()


# ---- 2. every minibatch of an update -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(act="tanh"), dict(act="relu", two=True, log_std_clamp=(-1.0, -0.2))], ids=["tanh-free", "relu-two-clamp"])
def test_one_update_equals_the_restatement(amd, case):
    """3 epochs x 2 minibatches of 4 envs driven through pg_minibatch with kl_coef = 1 and the value clip on: after every
    minibatch theta / m / v, adc_pg_stats and adc_pg_kl_stats are the restatement's.  The first minibatch sees the collecting
    distribution itself (kl == 0 exactly); the second starts at env 4 (a snapshot row indexed without n0 would show)."""
    N, K, T, mb = 8, 9, 4, 4
    rng = np.random.default_rng(21)
    pol = _policy(rng, K, **case)
    opts = P.options(lr=3e-3, vf_coef=1.0, ent_coef=0.01, minibatch_envs=mb)
    e = _trainer(amd, pol, N, K, T, opts)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch(bootstrap=True)
    kl_opts = KR.kl_options(kl_coef=1.0, adaptive=False, vf_clip=_median_sq(pol, rec, opts))
    e.pg_kl_init(**kl_opts)
    with pytest.raises(Exception, match="pg_advantages"):               # (the add-on's snapshot is taken with the advantages)
        e.pg_minibatch(0, mb)
    adv, ret = e.pg_advantages(fetch=True)
    state = _fresh_state(pol)
    snap = KR.snapshot(pol, state["theta"], rec)
    fractions = []
    for ep in range(3):
        for n0 in (0, mb):
            stats, kst = e.pg_minibatch(n0, mb), e.pg_kl_stats()
            state, rstats, rkst = KR.minibatch(pol, state, rec, adv, ret, snap, n0, mb, opts, kl_opts, 1.0)
            _assert_state(e.pg_state(), state, (ep, n0))
            _assert_stats(stats, rstats, (ep, n0))
            _assert_kl_stats(kst, rkst, (ep, n0))
            if (ep, n0) == (0, 0):
                assert kst["kl"] == 0.0 and not np.signbit(kst["kl"])
            else:
                assert kst["kl"] > 0.0
            fractions.append(kst["vf_clip_fraction"])
    assert any(0.0 < f < 1.0 for f in fractions)
    assert _same(F(e.pg_kl_coef()), F(1.0)), "pg_minibatch never adapts"
    e.close()


# ---- 3. the adaptive coefficient through the trainer ---------------------------------------------------------------------------------
# (at lr = 0.03 Adam's first steps are its largest: the last epoch's mean KL is about 1.08, 0.25 and 0.06 in the three
#  iterations - above 2 x the target, within its band, below 0.5 x - so the coefficient rises, stays and falls;
#  profiles/pr_pg_kl.txt has the restatement's figures)
ADAPTIVE = dict(kl_coef=0.5, kl_target=0.25, adaptive=True, factor_up=40.0, factor_down=0.25)


def _adaptive_run(amd, kl_penalty, iterations=3, resume_at=None, saved=None):
    """`iterations` iterations of PGTrainer on 8 envs; returns the trainer's states after each, the statistics and the records"""
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    N, K, T = 8, 9, 4
    rng = np.random.default_rng(31)
    pol = _policy(rng, K, (12, 12))
    e = _engine(amd, _planes(N, K))
    tr = PGTrainer(e, pol, T, epochs=3, minibatches=2, lr=3e-2, vf_coef=1.0, kl_penalty=kl_penalty)
    out = []
    for it in range(iterations):
        if resume_at is not None and it == resume_at:
            tr.state(saved)
        e.rollout_reset()
        e.run_days("mlp", T, BUDGET)
        rec = e.rollout_fetch(bootstrap=True)
        if resume_at is not None and it < resume_at:        # (only the envs' and agents' position: the state comes from `saved`)
            out.append(None)
            continue
        stats = e.pg_update(tr.epochs)
        out.append((tr.state(), stats, e.pg_kl_stats() if kl_penalty is not None else None, rec))
    e.close()
    return pol, tr.config, out


def test_three_iterations_with_an_adaptive_coefficient(amd):
    """PGTrainer(kl_penalty=...).iteration() three times, the restatement fed from the records it leaves: the statistics, the
    coefficient sequence and theta after every iteration are the restatement's, and the coefficient both rises and falls"""
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    N, K, T = 8, 9, 4
    rng = np.random.default_rng(31)
    pol = _policy(rng, K, (12, 12))
    e = _engine(amd, _planes(N, K))
    tr = PGTrainer(e, pol, T, epochs=3, minibatches=2, lr=3e-2, vf_coef=1.0, kl_penalty=ADAPTIVE)
    opts, kl_opts = P.options(**tr.config), KR.kl_options(**ADAPTIVE)
    state, coef, coefs = _fresh_state(pol), F(ADAPTIVE["kl_coef"]), []
    records, update = [], e.pg_update

    def recording_update(epochs):           # (the record and its bootstrap value as the update is about to see them)
        records.append(e.rollout_fetch(bootstrap=True))
        return update(epochs)
    e.pg_update = recording_update
    for it in range(3):
        stats = tr.iteration(T, BUDGET)
        rec = records[it]
        state, rstats, rkst = KR.update(pol, state, rec, rec["bootstrap_value"], 3, opts, kl_opts, coef)
        print(f"iteration {it}: kl {rkst['kl']:.6e}  coefficient {float(coef):.6g} -> {float(rkst['kl_coef_next']):.6g}")
        _assert_stats(stats, rstats, it)
        assert _same(np.float64(stats["kl"]), np.float64(rkst["kl"])) and _same(F(stats["kl_coef"]), coef), it
        _assert_kl_stats(e.pg_kl_stats(), rkst, it)
        coef = rkst["kl_coef_next"]
        coefs.append(float(coef))
        assert _same(F(e.pg_kl_coef()), coef), it
        got = tr.state()
        _assert_state(got, state, it)
        assert _same(F(got["kl_coef"]), coef)
    # the restatement's coefficient both rose and fell within the three iterations
    steps = np.sign(np.diff([ADAPTIVE["kl_coef"]] + coefs))
    assert (steps > 0).any() and (steps < 0).any(), coefs
    e.close()


# ---- 4. a learner population ---------------------------------------------------------------------------------------------------------
POP_KL = (dict(kl_coef=1.0, kl_target=0.02, adaptive=True, vf_clip=0.0), dict(kl_coef=0.3, kl_target=1e-4, adaptive=True, factor_up=3.0),
          dict(kl_coef=0.0, kl_target=0.01, adaptive=True, vf_clip=0.0))
POP_CFG = (dict(lr=3e-3), dict(lr=1e-2, eps_clip=0.1, vf_coef=1.0), dict(lr=5e-3, normalize_advantages=False, reward_scale=0.05))


def _population(amd, kl, M=3, n=4, K=5, T=4, seed=201, vf_clip1=None):
    """M learners of n envs with different weights and configurations under PGPopulationTrainer"""
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer
    rng = np.random.default_rng(seed)
    pols = [_policy(rng, K, (12,)) for _ in range(M)]
    e = _engine(amd, _planes(M * n, K))
    configs = [dict(c, epochs=2, minibatches=2) for c in POP_CFG[:M]]
    if kl is not None and vf_clip1 is not None:
        kl = [dict(k) for k in kl]
        kl[1]["vf_clip"] = vf_clip1
    return e, PGPopulationTrainer(e, pols, T, configs, kl_penalty=kl), pols, kl


def test_a_population_equals_solo_engines(amd):
    """M = 3 learners x 4 envs with three different (kl_coef, kl_target, vf_clip), one of them kl_coef = 0: after each of two
    updates every member is bit for bit a single engine of 4 envs at env_id_base + 4 m under that member's settings (the
    population law), and the kl_coef = 0, vf_clip = 0 member also a member of a population without the add-on"""
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    M, n, K, T = 3, 4, 5, 4
    # a value clip for member 1 from its own first record
    e, tr, pols, _ = _population(amd, None)
    e.run_days("mlp", T, BUDGET)
    rec = PP.member_record(e.rollout_fetch(bootstrap=True), 1, n)
    cap = _median_sq(pols[1], rec, P.options(**tr.configs[1]))
    e.close()
    e, tr, pols, kl = _population(amd, list(POP_KL), vf_clip1=cap)
    plain, plain_tr, _, _ = _population(amd, None)
    solos = []
    for m in range(M):
        s = _engine(amd, _planes(M * n, K)[:, PP.member_slice(m, n)], env_id_base=m * n)
        cfg = {k: v for k, v in tr.configs[m].items() if k != "minibatch_envs"}
        solos.append(PGTrainer(s, pols[m], T, epochs=2, minibatches=2, kl_penalty=kl[m], **cfg))
    seen_up, fractions = False, []
    for it in range(2):
        stats, pstats = tr.iteration(T, BUDGET), plain_tr.iteration(T, BUDGET)
        kst = e.pg_kl_stats()
        for m in range(M):
            sstats = solos[m].iteration(T, BUDGET)
            _assert_state(tr.state(m), solos[m].state(), (it, m))
            _assert_stats(stats[m], sstats, (it, m))
            _assert_kl_stats(kst[m], solos[m].engine.pg_kl_stats(), (it, m))
            assert _same(F(tr.state(m)["kl_coef"]), F(solos[m].state()["kl_coef"])), (it, m)
            assert _same(np.float64(stats[m]["kl"]), np.float64(sstats["kl"])) and stats[m]["kl"] > 0, (it, m)
            seen_up = seen_up or kst[m]["kl_coef_next"] > kst[m]["kl_coef"]
        fractions.append(kst[1]["vf_clip_fraction"])
        _assert_state(e.pg_pop_state(2), plain.pg_pop_state(2), ("without the add-on", it))
        _assert_stats(stats[2], pstats[2], ("without the add-on", it))
        assert not _same(e.pg_pop_state(0)["theta"], plain.pg_pop_state(0)["theta"]), "the penalty moves member 0"
    assert seen_up and any(0.0 < f < 1.0 for f in fractions), fractions
    assert e.pg_kl_coef(2) == 0.0 and len({float(e.pg_kl_coef(m)) for m in range(M)}) == M
    for s in solos:
        s.engine.close()
    plain.close()
    e.close()


# ---- 5. copies -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["pg_pop_copy", "pbt_step"])
def test_a_copy_gives_the_donors_coefficient(amd, how):
    """member 2 is replaced - by pg_pop_copy(0, 2), or by a PBT round in which it ranks last: its coefficient is the donor's
    afterwards, and its next update is the donor's continuation on member 2's envs under member 2's own settings"""
    M, n, K, T = 3, 4, 5, 4
    kl = [dict(kl_coef=1.0, kl_target=1e-4, adaptive=True, factor_up=3.0), dict(kl_coef=0.5, kl_target=10.0, adaptive=True),
          dict(kl_coef=0.125, kl_target=0.02, adaptive=False, vf_clip=0.0)]
    e, tr, pols, _ = _population(amd, kl)
    tr.iteration(T, BUDGET)
    before = [tr.state(m) for m in range(M)]
    assert len({float(b["kl_coef"]) for b in before}) == M and float(before[0]["kl_coef"]) == 3.0
    if how == "pg_pop_copy":
        donor = 0
        e.pg_pop_copy(0, 2)
    else:
        donor = 1
        e.pbt_init("pg", replace_count=1)
        res = e.pbt_step(np.array([1.0, 2.0, 0.0]))
        assert list(res["src"]) == [-1, -1, 1]
    assert _same(F(e.pg_kl_coef(2)), F(before[donor]["kl_coef"])) and not _same(F(before[2]["kl_coef"]), F(before[donor]["kl_coef"]))
    for m in (0, 1):
        assert _same(F(e.pg_kl_coef(m)), F(before[m]["kl_coef"])), m
    _assert_state(e.pg_pop_state(2), before[donor])
    e.rollout_reset()
    e.run_days("mlp", T, BUDGET)
    rec = PP.member_record(e.rollout_fetch(bootstrap=True), 2, n)
    stats = e.pg_pop_update(2)
    state = {k: before[donor][k] for k in ("theta", "m", "v", "steps")}
    opts = P.options(**tr.configs[2])
    state, rstats, rkst = KR.update(pols[donor], state, rec, rec["bootstrap_value"], 2, opts, KR.kl_options(**kl[2]), before[donor]["kl_coef"])
    _assert_state(e.pg_pop_state(2), state)
    _assert_stats(stats[2], rstats)
    _assert_kl_stats(e.pg_kl_stats()[2], rkst)
    e.close()


# ---- 6. a resumed run ------------------------------------------------------------------------------------------------------------------
def test_a_resumed_state_continues_to_the_same_theta(amd):
    """state() - theta, moments, steps and the coefficient - carried into a fresh engine stepped to the same env position reaches
    the straight run's theta and coefficient"""
    _, _, full = _adaptive_run(amd, ADAPTIVE, 2)
    saved = full[0][0]
    assert not _same(F(saved["kl_coef"]), F(ADAPTIVE["kl_coef"])), "the coefficient adapted in the first iteration"
    _, _, resumed = _adaptive_run(amd, ADAPTIVE, 2, resume_at=1, saved=saved)
    _assert_state(resumed[1][0], full[1][0])
    assert _same(F(resumed[1][0]["kl_coef"]), F(full[1][0]["kl_coef"]))
    _assert_kl_stats(resumed[1][2], full[1][2])
    # (without the coefficient the second iteration is another one)
    _, _, wrong = _adaptive_run(amd, ADAPTIVE, 2, resume_at=1, saved={k: v for k, v in saved.items() if k != "kl_coef"})
    assert not _same(wrong[1][0]["theta"], full[1][0]["theta"])


# ---- 7. nothing else moved -------------------------------------------------------------------------------------------------------------
def test_nothing_else_moved(amd):
    """the add-on live with kl_coef = 0 and vf_clip = 0: three iterations give the theta of a trainer without it, bit for bit,
    and the KL is measured.  Training under the add-on takes no draws: the envs' and the agents' streams are where they are
    without the updates."""
    _, _, without = _adaptive_run(amd, None)
    _, _, zero = _adaptive_run(amd, dict(kl_coef=0.0, kl_target=0.01, adaptive=True, vf_clip=0.0))
    for it in range(3):
        _assert_state({k: zero[it][0][k] for k in ("theta", "m", "v", "steps")}, without[it][0], it)
        _assert_stats(zero[it][1], without[it][1], it)
        assert zero[it][2]["kl"] > 0 and zero[it][2]["kl_coef_next"] == 0.0 and zero[it][2]["vf_clip_fraction"] == 0.0
        for k in zero[it][3]:
            assert _same(zero[it][3][k], without[it][3][k]), (k, it)
    N, K, T = 12, 10, 4
    rng = np.random.default_rng(61)
    pol = _policy(rng, K)
    ends = []
    for updates in (False, True):
        e = _trainer(amd, pol, N, K, T, P.options(lr=3e-3))
        e.pg_kl_init(kl_coef=1.0, kl_target=0.01, vf_clip=1.0)
        for _ in range(2):
            e.rollout_reset()
            e.run_days("mlp", T, BUDGET)
            if updates:
                e.pg_update(2)
        ends.append((e.get_rng_state(), e.mlp_agent_state()))
        e.close()
    (sa, aa), (sb, ab) = ends
    assert _same(sa[0], sb[0]) and _same(sa[1], sb[1])
    assert _same(aa[0], ab[0]) and _same(aa[1], ab[1]) and np.all(aa[1] == 2 * T)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd import _ffi
    N, K, T = 8, 6, 3
    rng = np.random.default_rng(71)
    pol = _policy(rng, K, (8,))
    opts = P.options(minibatch_envs=N // 2)
    e = _engine(amd, _planes(N, K))
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    not_ready = (lambda: e.pg_kl_stats(), lambda: e.pg_kl_coef(), lambda: e.pg_kl_coef(0, 0.5), lambda: e.pg_kl_old_dist())
    # without a live PPO / A2C trainer; while a TD3 trainer lives
    with pytest.raises(_ffi.EngineStateError, match="adc_engine_pg_init"):
        e.pg_kl_init()
    for call in not_ready:
        with pytest.raises(_ffi.EngineStateError, match="pg_kl_init"):
            call()
    e.td3_init(critic_widths=(8, 1), batch_size=8, capacity=40)
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.pg_kl_init()
    e.rollout_enable(T, obs=True)                                       # (ends the TD3 trainer)
    e.pg_init(**opts)
    # count neither 1 nor the members; a bad configuration; a bad coefficient or member
    two = (_ffi.PGKLConfig * 2)(amd.StepEngine.pg_kl_config(), amd.StepEngine.pg_kl_config())
    assert e._lib.adc_engine_pg_kl_init(e._h, two, 2) == _ffi.ADC_EINVAL
    assert e._lib.adc_engine_pg_kl_init(e._h, two, 0) == _ffi.ADC_EINVAL
    bad = amd.StepEngine.pg_kl_config()
    bad.kl_target = 0.0
    assert e._lib.adc_engine_pg_kl_init(e._h, C.byref(bad), 1) == _ffi.ADC_EINVAL
    with pytest.raises(ValueError):
        e.pg_kl_init(per_member=[dict(), dict()])
    with pytest.raises(_ffi.EngineStateError, match="pg_kl_init"):
        e.pg_kl_stats()                                                 # (the refused inits left no add-on)
    e.run_days("mlp", 2, BUDGET)
    e.pg_advantages()
    e.pg_kl_init(kl_coef=0.5, vf_clip=1.0)
    for member in (-1, 1):
        with pytest.raises(ValueError, match="no such member"):
            e.pg_kl_coef(member)
    for value in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="coef"):
            e.pg_kl_coef(0, value)
    # a minibatch without a snapshot since the add-on began / since the last recorded day
    with pytest.raises(_ffi.EngineStateError, match="pg_advantages"):
        e.pg_minibatch(0, 4)
    with pytest.raises(_ffi.EngineStateError, match="advantages"):
        e.pg_kl_old_dist()
    e.pg_advantages()
    assert e.pg_minibatch(0, 4)["steps"] == 1 and e.pg_kl_stats()["kl"] == 0.0
    e.run_days("mlp", 1, BUDGET)
    with pytest.raises(_ffi.EngineStateError, match="pg_advantages"):
        e.pg_minibatch(0, 4)
    assert e.pg_update(1)["steps"] == 3 and e.pg_kl_stats()["kl"] > 0
    e.pg_kl_coef(0, 0.125)
    assert e.pg_kl_coef() == F(0.125) and e.pg_kl_stats()["kl_coef_next"] == F(0.125)
    # a second init starts over from its configuration
    e.pg_kl_init(kl_coef=2.0, adaptive=False, kl_target=0.0)
    assert e.pg_kl_coef() == F(2.0)
    # the add-on does not survive pg_init, mlp_init, rollout_enable, mlp_learners, pg_pop_init
    for end in (lambda: e.pg_init(**opts), lambda: e.mlp_init(pol, deterministic=False), lambda: e.rollout_enable(T, obs=True), lambda: e.mlp_learners(2)):
        e.mlp_learners(0)
        e.rollout_enable(T, obs=True)
        e.pg_init(**opts)
        e.pg_kl_init()
        end()
        for call in not_ready:
            with pytest.raises(_ffi.EngineStateError, match="pg_kl_init"):
                call()
    e.mlp_learners(2)
    e.rollout_enable(T, obs=True)
    pop = P.options(minibatch_envs=2)
    e.pg_pop_init(pop)
    three = (_ffi.PGKLConfig * 3)(*[amd.StepEngine.pg_kl_config() for _ in range(3)])
    assert e._lib.adc_engine_pg_kl_init(e._h, three, 3) == _ffi.ADC_EINVAL
    e.pg_kl_init(per_member=[dict(kl_coef=0.5), dict(kl_coef=0.7)])
    assert [float(e.pg_kl_coef(m)) for m in range(2)] == [0.5, float(F(0.7))]
    with pytest.raises(ValueError, match="no such member"):
        e.pg_kl_coef(2)
    e.pg_pop_init(pop)
    with pytest.raises(_ffi.EngineStateError, match="pg_kl_init"):
        e.pg_kl_stats()
    # the engine still works: a shared configuration, recorded days, an update, every member's own coefficient
    e.pg_kl_init(kl_coef=0.5, kl_target=1e-6)
    e.run_days("mlp", 2, BUDGET)
    with pytest.raises(_ffi.EngineStateError, match="pg_pop_advantages"):
        e.pg_pop_minibatch(0)
    stats = e.pg_pop_update(2)
    kst = e.pg_kl_stats()
    assert [s["steps"] for s in stats] == [4, 4] and all(k["kl"] > 0 and k["kl_coef_next"] == F(0.75) for k in kst)
    e.close()
    s = amd.ShardedStepEngine(N, K, shards=2, seed=5)
    with pytest.raises(NotImplementedError, match="engine_shards=1"):
        s.pg_kl_init()
    s.close()
