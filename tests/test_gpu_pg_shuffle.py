"""GPU tests of the PPO learners' shuffled sample-level minibatches and target-KL early stop (parts/kernel_pg_shuffle.inc,
parts/pg_shuffle_api.inc) against the numpy restatement tests/pg_shuffle_ref.py, bit for bit: the order and the record rows on the
device, every minibatch of two epochs (also under the KL add-on), the chunk and slab edges of a gathered minibatch, a whole update
and the early stop, a learner population against solo engines, a resumed run, that nothing else moved, and every refusal."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import pg_kl_ref as KR
from tests import pg_pop_ref as PP
from tests import pg_ref as P
from tests import pg_shuffle_ref as S

pytestmark = pytest.mark.gpu
F = np.float32
BUDGET = 1000.0
SEED = 41
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


def _planes(N, K, seed=SEED):
    return H.implicit_params(N, K, seed + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, seed=SEED, env_id_base=0, **kw):
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


def _median_sq(rec, opts):
    adv, ret = P.gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], rec["bootstrap_value"], **opts)
    dv = (rec["value"] - ret).astype(F)
    return float(F(np.median((dv * dv).astype(np.float64))))


# ---- 1. the order and the rows on the device -------------------------------------------------------------------------------------------
def test_the_order_and_rows_of_a_single_learner(amd):
    """N = 8, T = 5: 40 samples, b = 6 (the cycle is walked); the engine's seed (shuffle seed 0) and the step count as the tick"""
    N, K, T = 8, 3, 5
    pol = _policy(np.random.default_rng(3), K, (8,))
    e = _trainer(amd, pol, N, K, T, P.options())
    e.pg_shuffle_init(minibatch_samples=16)
    e.run_days("mlp", T, BUDGET)
    e.pg_advantages()
    for steps in (0, 7):
        st = e.pg_state()
        st["steps"] = steps
        e.pg_state(st)
        e.pg_shuffle_epoch()
        order, rows = e.pg_shuffle_order()
        ref = S.order(SEED, T * N, steps)
        assert order.shape == (1, T * N) and _same(order[0], ref) and _same(rows[0], S.rows(ref, N, N))
        assert np.array_equal(np.sort(order[0]), np.arange(T * N, dtype=np.uint32))
    assert not _same(ref, S.order(SEED, T * N, 0))
    e.close()


def test_the_order_and_rows_of_a_population(amd):
    """3 members x 8 envs with three seeds: every member's own order, its rows inside its own env block"""
    M, n, K, T = 3, 8, 3, 5
    N = M * n
    pol = _policy(np.random.default_rng(4), K, (8,))
    e = _engine(amd, _planes(N, K))
    e.mlp_init(pol, deterministic=False)
    e.mlp_learners(M)
    e.rollout_enable(T, obs=True)
    e.pg_pop_init(P.options())
    seeds = (5, 6, 0)
    e.pg_shuffle_init(per_member=[dict(minibatch_samples=16, seed=s) for s in seeds])
    e.run_days("mlp", T, BUDGET)
    e.pg_pop_advantages()
    e.pg_shuffle_epoch()
    order, rows = e.pg_shuffle_order()
    assert order.shape == (M, T * n)
    for m in range(M):
        ref = S.order(seeds[m] or SEED, T * n, 0)
        assert _same(order[m], ref) and _same(rows[m], S.rows(ref, n, N, m)), m
        assert np.all((rows[m] % N) // n == m) and np.array_equal(np.sort(rows[m] // N), np.repeat(np.arange(T), n)), m
    assert not _same(order[0], order[1]) and not _same(order[0], order[2])
    e.close()


# ---- 2. every minibatch of two epochs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(act="tanh"), dict(act="relu", two=True, log_std_clamp=(-1.0, -0.2)), dict(act="tanh", kl=True)],
                         ids=["tanh-free", "relu-two-clamp", "tanh-kl-vfclip"])
def test_every_minibatch_of_two_epochs(amd, case):
    """N = 8, K = 9, T = 5, minibatch_samples = 16: minibatches of 16, 16 and 8 samples - the last short and below the 16-row
    tile - driven through pg_shuffle_epoch / pg_shuffle_minibatch; after each, theta / m / v and adc_pg_stats (and adc_pg_kl_stats
    with the KL add-on at kl_coef = 1 and the value clip on) are the restatement's; the second epoch's order differs"""
    N, K, T, mb = 8, 9, 5, 16
    case = dict(case)
    with_kl = case.pop("kl", False)
    pol = _policy(np.random.default_rng(21), K, **case)
    opts = P.options(lr=3e-3, vf_coef=1.0, ent_coef=0.01)
    sh = S.shuffle_options(minibatch_samples=mb)
    e = _trainer(amd, pol, N, K, T, opts)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch(bootstrap=True)
    kl_opts = snap = coef = None
    e.pg_shuffle_init(**sh)
    if with_kl:                                                         # (attached after the shuffle add-on: either order)
        kl_opts, coef = KR.kl_options(kl_coef=1.0, adaptive=False, vf_clip=_median_sq(rec, opts)), 1.0
        e.pg_kl_init(**kl_opts)
    adv, ret = e.pg_advantages(fetch=True)
    state = _fresh_state(pol)
    if with_kl:
        snap = KR.snapshot(pol, state["theta"], rec)
    orders = []
    for ep in range(2):
        e.pg_shuffle_epoch()
        order = e.pg_shuffle_order()[0][0]
        ref = S.order(SEED, T * N, state["steps"])
        assert _same(order, ref), ep
        orders.append(ref)
        for j, (i0, i1) in enumerate(S.minibatches(T * N, mb)):
            stats = e.pg_shuffle_minibatch(j)
            state, rstats, rkst, stopped = S.minibatch(pol, state, rec, adv, ret, ref[i0:i1].astype(np.int64), opts, sh, False, snap, kl_opts, coef)
            assert not stopped
            _assert_state(e.pg_state(), state, (ep, j))
            _assert_stats(stats, rstats, (ep, j))
            assert stats["samples"] == i1 - i0 and stats["steps"] == state["steps"]
            if with_kl:
                _assert_kl_stats(e.pg_kl_stats(), rkst, (ep, j))
    assert [i1 - i0 for i0, i1 in S.minibatches(T * N, mb)] == [16, 16, 8] and not _same(orders[0], orders[1])
    assert e.pg_shuffle_stats() == dict(epochs_begun=2, minibatches_evaluated=6, steps_taken=6, stopped=0)
    e.close()


# ---- 3. chunk and slab edges -------------------------------------------------------------------------------------------------------------
def test_chunk_and_slab_edges(amd):
    """N = 344, K = 3, T = 6, hidden (8,), minibatch_samples = 1030: minibatches of 1030, 1030 and 4 samples - a full one crosses
    the 1024-sample chunk and ends inside a 64-sample slab; n_s = 2064 walks the cycle and the rows span all days.  The scratch
    was sized for one env's days by pg_init and grown by pg_shuffle_init."""
    N, K, T, mb = 344, 3, 6, 1030
    pol = _policy(np.random.default_rng(33), K, (8,))
    opts = P.options(lr=3e-3, minibatch_envs=1)
    sh = S.shuffle_options(minibatch_samples=mb)
    e = _trainer(amd, pol, N, K, T, opts)
    e.pg_shuffle_init(**sh)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch(bootstrap=True)
    adv, ret = e.pg_advantages(fetch=True)
    e.pg_shuffle_epoch()
    order, rows = e.pg_shuffle_order()
    ref = S.order(SEED, T * N, 0)
    assert _same(order[0], ref) and _same(rows[0], S.rows(ref, N, N))
    state = _fresh_state(pol)
    for j, (i0, i1) in enumerate(S.minibatches(T * N, mb)):
        stats = e.pg_shuffle_minibatch(j)
        if i1 - i0 == mb:
            assert len(set((ref[i0:i1] // N).tolist())) == T, "a full minibatch holds samples of every day"
        state, rstats, _, _ = S.minibatch(pol, state, rec, adv, ret, ref[i0:i1].astype(np.int64), opts, sh)
        _assert_state(e.pg_state(), state, j)
        _assert_stats(stats, rstats, j)
        assert stats["samples"] == i1 - i0
    assert [i1 - i0 for i0, i1 in S.minibatches(T * N, mb)] == [1030, 1030, 4]
    # env ranges keep working next to it (one env: what pg_init's scratch was sized for)
    assert e.pg_minibatch(5, 1)["samples"] == T
    e.close()


# ---- 4. a whole update and the early stop ------------------------------------------------------------------------------------------------
def test_a_whole_update_and_the_early_stop(amd):
    """pg_update(3) at N = 8, T = 5, minibatch_samples = 16, lr 3e-2 without target_kl equals the restatement's update, statistics
    included.  Then 1.5 target_kl is put strictly between the largest approx_kl of epoch 0 and the largest later one: the device
    stops at the restatement's minibatch with its theta, adc_pg_shuffle_stats reports it and the step count is the steps taken"""
    N, K, T, mb = 8, 9, 5, 16
    pol = _policy(np.random.default_rng(41), K, (12, 12))
    opts = P.options(lr=3e-2, vf_coef=1.0)
    e = _trainer(amd, pol, N, K, T, opts)
    e.pg_shuffle_init(minibatch_samples=mb)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch(bootstrap=True)
    stats = e.pg_update(3)
    trace = []
    state, rstats, _, rsst = S.update(pol, _fresh_state(pol), rec, rec["bootstrap_value"], 3, opts, S.shuffle_options(minibatch_samples=mb), SEED, trace=trace)
    _assert_state(e.pg_state(), state)
    _assert_stats(stats, rstats)
    assert (stats["samples"], stats["steps"]) == (8, 9) and e.pg_shuffle_stats() == rsst == dict(epochs_begun=3, minibatches_evaluated=9, steps_taken=9, stopped=0)
    kls = [(ep, j, kl) for ep, j, kl, _ in trace]
    print("approx_kl per minibatch:", " ".join(f"{ep}.{j}:{kl:.4e}" for ep, j, kl in kls))
    first, later = max(kl for ep, _, kl in kls if ep == 0), max(kl for ep, _, kl in kls if ep > 0)
    assert later > first > 0, "the restatement's approx_kl grows beyond epoch 0's at this learning rate"
    target = float(F(0.5 * (first + later) / 1.5))
    assert first < 1.5 * np.float64(F(target)) < later
    # the same record, the state back at its start
    e.pg_state(_fresh_state(pol))
    e.pg_shuffle_init(minibatch_samples=mb, target_kl=target)
    stats = e.pg_update(3)
    trace = []
    sh = S.shuffle_options(minibatch_samples=mb, target_kl=target)
    state, rstats, _, rsst = S.update(pol, _fresh_state(pol), rec, rec["bootstrap_value"], 3, opts, sh, SEED, trace=trace)
    ep, j = trace[-1][:2]
    print(f"stopped at epoch {ep} minibatch {j} after {state['steps']} steps")
    assert rsst["stopped"] == 1 and ep >= 1 and 0 < state["steps"] < 9, "the stop is neither at the first minibatch nor absent"
    got = e.pg_state()
    _assert_state(got, state)
    _assert_stats(stats, rstats)
    assert e.pg_shuffle_stats() == rsst and rsst["steps_taken"] == got["steps"] == stats["steps"] and rsst["minibatches_evaluated"] == got["steps"] + 1
    assert stats["samples"] == rstats["samples"]
    # from the moved state a bound below the first minibatch's approx_kl ends the next update before its first step: nothing
    # moves, and the next order is drawn with the same tick - the same order
    rec2 = e.rollout_fetch(bootstrap=True)
    trace = []
    S.update(pol, state, rec2, rec2["bootstrap_value"], 1, opts, S.shuffle_options(minibatch_samples=mb), SEED, trace=trace)
    kl0 = trace[0][2]
    print(f"approx_kl of the first minibatch from the moved state: {kl0:.4e}")
    assert kl0 > 0
    sh = S.shuffle_options(minibatch_samples=mb, target_kl=float(F(kl0 / 3.0)))
    e.pg_shuffle_init(**sh)
    stats = e.pg_update(2)
    state2, rstats, _, rsst = S.update(pol, state, rec2, rec2["bootstrap_value"], 2, opts, sh, SEED)
    assert e.pg_shuffle_stats() == rsst == dict(epochs_begun=1, minibatches_evaluated=1, steps_taken=0, stopped=1)
    _assert_state(e.pg_state(), state)
    _assert_stats(stats, rstats)
    e.pg_advantages()
    e.pg_shuffle_epoch()
    assert _same(e.pg_shuffle_order()[0][0], S.order(SEED, T * N, state["steps"]))
    e.close()


# ---- 5. a population equals solo engines ---------------------------------------------------------------------------------------------------
POP_CFG = (dict(lr=3e-2, vf_coef=1.0), dict(lr=2e-2, eps_clip=0.1), dict(lr=3e-2, normalize_advantages=False, reward_scale=0.05))
POP_SEEDS = (5, 6, 7)
# (member 0's coefficient is 0 and stays 0: its approx_kl keeps growing into the second epoch as without the add-on, while the
#  penalised members' peaks right after the first step - which is what lets the members stop at different minibatches)
POP_KL = (dict(kl_coef=0.0, kl_target=0.02, adaptive=True), dict(kl_coef=0.3, kl_target=1e-4, adaptive=True, factor_up=3.0),
          dict(kl_coef=0.5, kl_target=10.0, adaptive=True))


@pytest.mark.parametrize("with_kl", [False, True], ids=["plain", "kl-adaptive"])
def test_a_population_equals_solo_engines(amd, with_kl):
    """3 members x 8 envs with different seeds and target_kl, the bounds from the restatement over each member's own first record:
    members 0 and 2 stop at two different minibatches, member 1 never stops.  After each of two updates every member
    is bit for bit a solo engine of its env block (state, statistics, shuffle statistics; with the KL add-on adaptive also its
    coefficient), so a stopped member no longer moves while the others go on"""
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer, PGTrainer
    M, n, K, T, mb, epochs = 3, 8, 5, 5, 16, 2
    rng = np.random.default_rng(201)
    pols = [_policy(rng, K, (12,)) for _ in range(M)]
    planes = _planes(M * n, K)
    kl = [dict(k) for k in POP_KL] if with_kl else None

    def solo(m, target):
        s = _engine(amd, planes[:, PP.member_slice(m, n)], env_id_base=m * n)
        return PGTrainer(s, pols[m], T, epochs=epochs, minibatch_size=mb, target_kl=target, shuffle_seed=POP_SEEDS[m],
                         kl_penalty=kl[m] if with_kl else None, **POP_CFG[m])
    # the restatement's approx_kl per minibatch of members 0 and 2 over their own first records, without a stop
    def probe_kls(m):
        probe = solo(m, None)
        probe.engine.run_days("mlp", T, BUDGET)
        rec = probe.engine.rollout_fetch(bootstrap=True)
        probe.engine.close()
        trace = []
        S.update(pols[m], _fresh_state(pols[m]), rec, rec["bootstrap_value"], epochs, P.options(**probe.config), S.shuffle_options(minibatch_samples=mb),
                 POP_SEEDS[m], KR.kl_options(**kl[m]) if with_kl else None, kl[m]["kl_coef"] if with_kl else None, trace=trace)
        return [(ep, k) for ep, _, k, _ in trace]
    # (until it stops a member goes the way it goes without a stop.  A bound between a minibatch's approx_kl and the largest
    #  before it stops the member there, if that minibatch is a new maximum: member 0 takes its last such minibatch, member 2
    #  its first after the first step, or the next where the two would coincide)
    def records(kls):
        out, top = [], 0.0
        for i, (_, k) in enumerate(kls):
            if k > top:
                if i > 0 and float(F(0.5 * (top + k) / 1.5)) > 0 and top < 1.5 * np.float64(F(0.5 * (top + k) / 1.5)) < k:
                    out.append((i, float(F(0.5 * (top + k) / 1.5))))
                top = k
        return out
    rec0, rec2 = records(probe_kls(0)), records(probe_kls(2))
    assert rec0 and rec2, "approx_kl rises above zero after the first step"
    at0, target0 = rec0[-1]
    at2, target2 = next(((i, t) for i, t in rec2 if i != at0), (None, None))
    assert at2 is not None, (rec0, rec2)
    targets = (target0, None, target2)
    evaluated = [at0 + 1, at2 + 1]
    per_epoch = len(S.minibatches(T * n, mb))
    e = _engine(amd, planes)
    configs = [dict(c, epochs=epochs, minibatch_size=mb, target_kl=t, shuffle_seed=s) for c, t, s in zip(POP_CFG, targets, POP_SEEDS)]
    tr = PGPopulationTrainer(e, pols, T, configs, kl_penalty=kl)
    solos = [solo(m, targets[m]) for m in range(M)]
    for it in range(2):
        stats = tr.iteration(T, BUDGET)
        sst = e.pg_shuffle_stats()
        kst = e.pg_kl_stats() if with_kl else None
        for m in range(M):
            sstats = solos[m].iteration(T, BUDGET)
            _assert_state(tr.state(m), solos[m].state(), (it, m))
            _assert_stats(stats[m], sstats, (it, m))
            assert stats[m]["samples"] == sstats["samples"] and sst[m] == solos[m].engine.pg_shuffle_stats(), (it, m, sst[m])
            if with_kl:
                _assert_kl_stats(kst[m], solos[m].engine.pg_kl_stats(), (it, m))
                assert _same(F(tr.state(m)["kl_coef"]), F(solos[m].state()["kl_coef"])), (it, m)
        print(f"iteration {it}:", sst)
        if it == 0:
            for m, ev in ((0, evaluated[0]), (2, evaluated[1])):
                assert sst[m] == dict(epochs_begun=(ev - 1) // per_epoch + 1, minibatches_evaluated=ev, steps_taken=ev - 1, stopped=1), (m, ev)
            assert sst[1] == dict(epochs_begun=2, minibatches_evaluated=6, steps_taken=6, stopped=0)
            assert len({s["steps_taken"] for s in sst}) == M, "the members stop at different minibatches"
            assert [tr.state(m)["steps"] for m in range(M)] == [s["steps_taken"] for s in sst]
    if with_kl:
        assert len({float(e.pg_kl_coef(m)) for m in range(M)}) > 1
    for s in solos:
        s.engine.close()
    e.close()


# ---- 6. a resumed run ----------------------------------------------------------------------------------------------------------------------
def _run(amd, iterations=2, resume_at=None, saved=None, shuffle_seed=0):
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    N, K, T = 8, 9, 5
    pol = _policy(np.random.default_rng(31), K, (12, 12))
    e = _engine(amd, _planes(N, K))
    tr = PGTrainer(e, pol, T, epochs=2, minibatch_size=16, lr=3e-3, vf_coef=1.0, shuffle_seed=shuffle_seed)
    out = []
    for it in range(iterations):
        if resume_at is not None and it == resume_at:
            tr.state(saved)
        if resume_at is not None and it < resume_at:        # (only the envs' and agents' position: the state comes from `saved`)
            e.rollout_reset()
            e.run_days("mlp", T, BUDGET)
            out.append(None)
            continue
        tr.iteration(T, BUDGET)
        out.append(tr.state())
    e.close()
    return out


def test_a_resumed_state_continues_to_the_same_theta(amd):
    """two updates in one go; one update, pg_state out and into a fresh engine stepped to the same env position, a second update:
    the same theta - the tick comes from the step count.  (With the step count left at 0 the second update draws other orders.)"""
    full = _run(amd)
    resumed = _run(amd, resume_at=1, saved=full[0])
    _assert_state(resumed[1], full[1])
    assert full[0]["steps"] == 6 and full[1]["steps"] == 12
    wrong = _run(amd, resume_at=1, saved=dict(full[0], steps=0))
    assert not _same(wrong[1]["theta"], full[1]["theta"])
    assert not _same(_run(amd, 1, shuffle_seed=9)[0]["theta"], full[0]["theta"]), "the seed enters the order"


# ---- 7. nothing else moved ---------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moved(amd):
    """an update with the add-on takes no draws and writes no record: the envs' and agents' stream positions and the rollout record
    are the same before and after; pg_minibatch over an env range gives, with the add-on live, what it gives without it"""
    N, K, T = 8, 9, 4
    pol = _policy(np.random.default_rng(61), K)
    opts = P.options(lr=3e-3, minibatch_envs=4)
    a, b = _trainer(amd, pol, N, K, T, opts), _trainer(amd, pol, N, K, T, opts)
    a.pg_shuffle_init(minibatch_samples=16, target_kl=10.0)
    for e in (a, b):
        e.run_days("mlp", T, BUDGET)
        e.pg_advantages()
    a.pg_shuffle_epoch()
    for n0 in (0, 4):
        sa, sb = a.pg_minibatch(n0, 4), b.pg_minibatch(n0, 4)
        _assert_stats(sa, sb, n0)
        assert sa["samples"] == sb["samples"] == 4 * T
        _assert_state(a.pg_state(), b.pg_state(), n0)
    before = (a.get_rng_state(), a.mlp_agent_state(), a.rollout_fetch())
    stats = a.pg_update(2)
    assert stats["steps"] > 2
    after = (a.get_rng_state(), a.mlp_agent_state(), a.rollout_fetch())
    assert _same(before[0][0], after[0][0]) and _same(before[0][1], after[0][1])
    assert _same(before[1][0], after[1][0]) and _same(before[1][1], after[1][1])
    for k in before[2]:
        assert _same(before[2][k], after[2][k]), k
    a.close()
    b.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd import _ffi
    N, K, T = 8, 6, 3
    pol = _policy(np.random.default_rng(71), K, (8,))
    opts = P.options(minibatch_envs=N // 2)
    e = _engine(amd, _planes(N, K))
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    not_ready = (lambda: e.pg_shuffle_stats(), lambda: e.pg_shuffle_epoch(), lambda: e.pg_shuffle_minibatch(0), lambda: e.pg_shuffle_order())
    # without a live PPO / A2C trainer; while a TD3 trainer lives
    with pytest.raises(_ffi.EngineStateError, match="adc_engine_pg_init"):
        e.pg_shuffle_init(minibatch_samples=8)
    for call in not_ready:
        with pytest.raises(_ffi.EngineStateError, match="pg_shuffle_init"):
            call()
    e.td3_init(critic_widths=(8, 1), batch_size=8, capacity=40)
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.pg_shuffle_init(minibatch_samples=8)
    e.rollout_enable(T, obs=True)                                       # (ends the TD3 trainer)
    e.pg_init(**opts)
    # count neither 1 nor the members; a bad configuration; more samples than a member records
    cfg = amd.StepEngine.pg_shuffle_config
    two = (_ffi.PGShuffleConfig * 2)(cfg(minibatch_samples=8), cfg(minibatch_samples=8))
    assert e._lib.adc_engine_pg_shuffle_init(e._h, two, 2) == _ffi.ADC_EINVAL
    assert e._lib.adc_engine_pg_shuffle_init(e._h, two, 0) == _ffi.ADC_EINVAL
    assert e._lib.adc_engine_pg_shuffle_init(e._h, None, 1) == _ffi.ADC_EINVAL
    bad = cfg(minibatch_samples=8)
    bad.target_kl = -1.0
    assert e._lib.adc_engine_pg_shuffle_init(e._h, C.byref(bad), 1) == _ffi.ADC_EINVAL
    with pytest.raises(ValueError, match="horizon"):
        e.pg_shuffle_init(minibatch_samples=T * N + 1)
    with pytest.raises(ValueError):
        e.pg_shuffle_init(per_member=[dict(), dict()])
    with pytest.raises(_ffi.EngineStateError, match="pg_shuffle_init"):
        e.pg_shuffle_stats()                                            # (the refused inits left no add-on)
    e.run_days("mlp", 2, BUDGET)
    e.pg_shuffle_init(minibatch_samples=T * N)                          # (the most it may be: grows the scratch)
    # a minibatch before the advantages, before the epoch, outside the epoch
    with pytest.raises(_ffi.EngineStateError, match="advantages"):
        e.pg_shuffle_minibatch(0)
    with pytest.raises(_ffi.EngineStateError, match="advantages"):
        e.pg_shuffle_epoch()
    e.pg_advantages()
    with pytest.raises(_ffi.EngineStateError, match="pg_shuffle_epoch"):
        e.pg_shuffle_minibatch(0)
    with pytest.raises(_ffi.EngineStateError, match="pg_shuffle_epoch"):
        e.pg_shuffle_order()
    e.pg_shuffle_epoch()
    for index in (-1, 1):                                               # (2 recorded days x 8 envs = 16 samples: one short minibatch)
        with pytest.raises(ValueError, match="no such minibatch"):
            e.pg_shuffle_minibatch(index)
    st = e.pg_shuffle_minibatch(0)
    assert st["steps"] == 1 and st["samples"] == 2 * N
    e.run_days("mlp", 1, BUDGET)                                        # (a new recorded day: the advantages and the order are stale)
    with pytest.raises(_ffi.EngineStateError, match="advantages"):
        e.pg_shuffle_minibatch(0)
    e.pg_advantages()
    with pytest.raises(_ffi.EngineStateError, match="pg_shuffle_epoch"):
        e.pg_shuffle_minibatch(0)
    assert e.pg_update(2)["steps"] == 3 and e.pg_shuffle_stats()["steps_taken"] == 2
    # a second init starts over from its configuration; the env ranges keep working
    e.pg_shuffle_init(minibatch_samples=5, target_kl=0.5)
    stats = e.pg_update(1)
    assert stats["steps"] == 3 + 5 and stats["samples"] == 4
    assert e.pg_minibatch(0, 4)["steps"] == 9
    # the add-on does not survive pg_init, mlp_init, rollout_enable, mlp_learners
    for end in (lambda: e.pg_init(**opts), lambda: e.mlp_init(pol, deterministic=False), lambda: e.rollout_enable(T, obs=True), lambda: e.mlp_learners(2)):
        e.mlp_learners(0)
        e.rollout_enable(T, obs=True)
        e.pg_init(**opts)
        e.pg_shuffle_init(minibatch_samples=8)
        end()
        for call in not_ready:
            with pytest.raises(_ffi.EngineStateError, match="pg_shuffle_init"):
                call()
    e.mlp_learners(2)
    e.rollout_enable(T, obs=True)
    pop = P.options(minibatch_envs=2)
    e.pg_pop_init(pop)
    three = (_ffi.PGShuffleConfig * 3)(*[cfg(minibatch_samples=4) for _ in range(3)])
    assert e._lib.adc_engine_pg_shuffle_init(e._h, three, 3) == _ffi.ADC_EINVAL
    with pytest.raises(ValueError, match="equal in all"):
        e.pg_shuffle_init(per_member=[dict(minibatch_samples=4), dict(minibatch_samples=6)])
    with pytest.raises(ValueError, match="horizon"):
        e.pg_shuffle_init(minibatch_samples=T * (N // 2) + 1)
    with pytest.raises(_ffi.EngineStateError, match="pg_shuffle_init"):
        e.pg_shuffle_stats()
    e.pg_pop_init(pop)
    # the engine still works: per-member configurations, recorded days, an update
    e.pg_shuffle_init(per_member=[dict(minibatch_samples=5, seed=3), dict(minibatch_samples=5, target_kl=1e3)])
    e.run_days("mlp", T, BUDGET)
    with pytest.raises(_ffi.EngineStateError, match="advantages"):
        e.pg_shuffle_minibatch(0)
    stats = e.pg_pop_update(2)
    sst = e.pg_shuffle_stats()
    assert [s["steps"] for s in stats] == [6, 6] and [s["samples"] for s in stats] == [2, 2]
    assert sst == [dict(epochs_begun=2, minibatches_evaluated=6, steps_taken=6, stopped=0)] * 2
    assert e.pg_pop_minibatch(0)[1]["steps"] == 7                       # (the env ranges keep working)
    e.close()
    s = amd.ShardedStepEngine(N, K, shards=2, seed=5)
    with pytest.raises(NotImplementedError, match="engine_shards=1"):
        s.pg_shuffle_init()
    s.close()


def test_the_order_is_gone_once_the_record_moves(amd):
    """the order is [members][n_s] of the days recorded when it was drawn: after rollout_reset - with no day, fewer days or more
    days recorded since - pg_shuffle_order is refused, not copied into arrays sized by the record as it is now; the next update
    draws an order of the new size"""
    from adcraft_amd import _ffi
    N, K, T = 8, 3, 4
    pol = _policy(np.random.default_rng(81), K, (8,))
    e = _trainer(amd, pol, N, K, T, P.options(lr=3e-3))
    e.pg_shuffle_init(minibatch_samples=16)
    e.run_days("mlp", 3, BUDGET)
    e.pg_update(1)
    assert e.pg_shuffle_order()[0].shape == (1, 3 * N)
    e.rollout_reset()
    for days in (0, 1, 3):                                              # (none, fewer, and 4 > 3 recorded days in all)
        if days:
            e.run_days("mlp", days, BUDGET)
        with pytest.raises(_ffi.EngineStateError, match="order drawn under them is gone"):
            e.pg_shuffle_order()
    e.pg_advantages()
    with pytest.raises(_ffi.EngineStateError, match="pg_shuffle_epoch"):
        e.pg_shuffle_order()
    tick = e.pg_state()["steps"]
    e.pg_update(1)
    order, rows = e.pg_shuffle_order()
    assert order.shape == rows.shape == (1, 4 * N) and _same(order[0], S.order(SEED, 4 * N, tick))
    assert sorted(rows[0].tolist()) == list(range(4 * N))
    e.close()


def test_a_minibatch_driven_after_the_stop_changes_nothing(amd):
    """a single learner driven by hand: the first minibatch's approx_kl (rounding noise above zero, or zero) against a target_kl of
    1e-30 or an unreachable one; once the update has stopped a further pg_shuffle_minibatch leaves the state, the step count and
    the shuffle statistics as they are and returns zero statistics, and the next advantages begin a new update"""
    N, K, T = 8, 3, 4
    pol = _policy(np.random.default_rng(91), K, (8,))
    e = _trainer(amd, pol, N, K, T, P.options(lr=3e-2))
    e.pg_shuffle_init(minibatch_samples=16, target_kl=1e-30)
    e.run_days("mlp", T, BUDGET)
    e.pg_advantages()
    e.pg_shuffle_epoch()
    first = e.pg_shuffle_minibatch(0)
    print("approx_kl of the first minibatch:", first["approx_kl"])
    stopped_at_once = first["approx_kl"] > 1.5 * np.float64(F(1e-30))
    second = e.pg_shuffle_minibatch(1)
    sst = e.pg_shuffle_stats()
    assert sst["stopped"] == 1 and sst["minibatches_evaluated"] == (1 if stopped_at_once else 2), sst
    state, steps = e.pg_state(), sst["steps_taken"]
    assert state["steps"] == steps == sst["minibatches_evaluated"] - 1
    after = e.pg_shuffle_minibatch(0)
    assert all(after[k] == 0.0 for k in P.STAT_KEYS) and after["steps"] == steps and after["samples"] == 16
    _assert_state(e.pg_state(), state)
    assert e.pg_shuffle_stats() == sst
    e.pg_advantages()
    assert e.pg_shuffle_stats() == dict(epochs_begun=0, minibatches_evaluated=0, steps_taken=0, stopped=0)
    e.close()
