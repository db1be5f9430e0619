"""GPU tests of the running reward normaliser (adc_engine_rew_norm_*; the law is csrc/adc_rew_norm.h): after an update the
device's count, mean, M2, multiplier and the envs' carry equal, bit for bit, the host twin adc_rew_norm_host run on the fetched
record - per member for a learner population, where a member's result also equals a single engine's of its envs - the
advantages under a live normaliser equal the host twin adc_pg_gae_norm_host, a trainer's iteration equals the host restatement
of the same sequence, a resumed run continues bit for bit, a copied member carries its donor's normaliser, a reset zeroes the
reset envs' carry, every refusal leaves the engine usable, and nothing changes unless it is asked for.  None of these symbols
exists before this feature: every test here fails on the parent commit.

The shapes: 2 keywords; (N, T) = (3, 5) (S = 15) and (70, 16) (S = 1120: the smallest of these that crosses a 1024-sample
chunk); per member 132 envs x 16 days x 2 learners (S = 1056 each: a chunk boundary inside a member) and 6 x 5 x 3.  Episodes
last 4 days, so days end episodes inside every record and - at 5 days - a running return is handed from rollout to rollout."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import pg_pop_ref as PP
from tests import pg_ref as P
from tests import rew_norm_ref as RR

pytestmark = pytest.mark.gpu
F, D64 = np.float32, np.float64


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


SEED, BUDGET, K = 43, 1000.0, 2
RESETS = dict(max_days=4, auto_reset=True)          # (episodes of 4 days: days end episodes inside every record)
SHAPES = [(3, 5), (70, 16)]


def _planes(N, seed=SEED):
    return H.implicit_params(N, K, seed + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, seed=SEED, env_id_base=0, **kw):
    _, N, k = planes.shape
    e = amd.StepEngine(N, k, seed=seed, env_id_base=env_id_base, **dict(RESETS, **kw))
    e.set_all_params(planes)
    e.reset()
    return e


def _policy(rng, hidden=(8,)):
    pol = R.random_policy(rng, K, hidden, "tanh", value=True, normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _solo(amd, pol, N, T, planes=None, env_id_base=0, **pg):
    e = _engine(amd, _planes(N) if planes is None else planes, env_id_base=env_id_base)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.pg_init(**pg)
    return e


def _state(e, member=0, envs=None):
    """the device's normaliser `member` with its envs' carry (all envs, or the member's `envs`)"""
    sl = slice(None) if envs is None else slice(member * envs, (member + 1) * envs)
    return dict(e.rew_norm_state(member), returns=e.rew_norm_returns()[sl].copy())


def _days(rec, t0=0, t1=None, sl=slice(None)):
    return tuple(np.ascontiguousarray(rec[k][t0:t1, sl]) for k in ("reward", "terminated", "truncated"))


# ---- 1. the device against the host twin, the shared normaliser -----------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0.0, 0.9, 1.0])
@pytest.mark.parametrize("N,T", SHAPES)
def test_three_rollouts_equal_the_host_twin(amd, lib, N, T, gamma):
    """count == 0, the merge, the cap hit by the third update, the carry across rollouts, dones inside every record"""
    cap = 5 * N * T // 2
    e = _solo(amd, _policy(np.random.default_rng(N)), N, T, gamma=gamma)
    e.rew_norm_init(count_cap=cap)
    st0 = _state(e)
    assert RR.same(st0, RR.fresh(N)) and st0["scale"] == F(1.0)
    ref, handed_on = RR.fresh(N), False
    for it in range(3):
        e.rollout_reset()
        e.run_days("mlp", T, BUDGET)
        e.rew_norm_update()
        rec = e.rollout_fetch()
        done = rec["terminated"] | rec["truncated"]
        assert done.any() and not done.all(), "the record was meant to cross episode ends"
        ref = RR.twin(lib, ref, *_days(rec), F(gamma), count_cap=cap)
        got = _state(e)
        assert RR.same(got, ref), it
        handed_on = handed_on or bool(np.any(got["returns"] != 0))
    assert ref["count"] == cap and ref["scale"] != F(1.0) and ref["M2"] > 0
    assert handed_on or gamma == 0.0 or T % 4 == 0, "a running return was meant to be handed from rollout to rollout"
    if N == 3:
        st = RR.fresh(N)
        assert RR.same(RR.update(st, *_days(rec), F(gamma)), RR.twin(lib, st, *_days(rec), F(gamma))), "the numpy restatement"
    e.close()


def test_two_updates_consume_the_days_once_each(amd, lib):
    from adcraft_amd import _ffi
    N, T = 70, 16
    e = _solo(amd, _policy(np.random.default_rng(1)), N, T, gamma=0.9)
    e.rew_norm_init()
    ref = RR.fresh(N)
    for t0, t1 in ((0, 10), (10, 16)):
        e.run_days("mlp", t1 - t0, BUDGET)
        e.rew_norm_update()
        rec = e.rollout_fetch()
        assert rec["reward"].shape[0] == t1
        ref = RR.twin(lib, ref, *_days(rec, t0, t1), F(0.9))
        assert RR.same(_state(e), ref), t0
        if t1 == 10:
            assert np.any(ref["returns"] != 0), "day 10 is inside an episode: its running return is carried into the next update"
    assert ref["count"] == N * T
    with pytest.raises(_ffi.EngineStateError, match="no day has been recorded"):
        e.rew_norm_update()
    assert RR.same(_state(e), ref)
    e.rollout_reset()
    with pytest.raises(_ffi.EngineStateError, match="no day has been recorded"):
        e.rew_norm_update()
    e.close()


@pytest.mark.parametrize("N,T", SHAPES)
def test_rewards_that_are_all_zero_end_at_the_floor(amd, lib, N, T):
    """keywords nobody clicks on earn and cost nothing: M2 stays 0 and the multiplier is float32(1 / min_std)"""
    planes = _planes(N)
    planes[4] = 0.0                                             # (the buy-side click-through rate)
    e = _solo(amd, _policy(np.random.default_rng(2)), N, T, planes=planes, gamma=0.9)
    e.rew_norm_init(min_std=0.3)
    e.run_days("mlp", T, BUDGET)
    e.rew_norm_update()
    rec = e.rollout_fetch()
    assert not rec["reward"].any(), "the record was meant to hold no reward"
    got = _state(e)
    assert RR.same(got, RR.twin(lib, RR.fresh(N), *_days(rec), F(0.9), min_std=0.3))
    assert got["count"] == N * T and got["M2"] == 0.0 and got["scale"] == F(D64(1.0) / D64(0.3))
    e.close()


# ---- 2. the advantages under a live normaliser ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T", SHAPES)
def test_advantages_equal_the_host_twin_with_clip_off_and_on(amd, lib, N, T):
    opts = dict(gamma=0.9, lam=0.8, reward_scale=0.5, normalize_advantages=(N == 3))
    e = _solo(amd, _policy(np.random.default_rng(3)), N, T, **opts)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch(bootstrap=True)
    plain = e.pg_advantages(fetch=True)
    args = (rec["reward"], rec["terminated"], rec["truncated"], rec["value"], rec["bootstrap_value"])
    e.rew_norm_init(clip=0.0)
    unit = e.pg_advantages(fetch=True)
    assert _same(unit[0], plain[0]) and _same(unit[1], plain[1]), "a fresh normaliser multiplies by 1 and clips nothing"
    e.rew_norm_update()
    scale = e.rew_norm_state()["scale"]
    off = e.pg_advantages(fetch=True)
    ref = RR.twin_gae(lib, *args, scale, 0.0, **opts)
    assert _same(off[0], ref[0]) and _same(off[1], ref[1])
    assert not _same(off[1], plain[1])
    # a clip that binds on about half of the rewards (a second init starts over and consumes the record from its first day)
    r = np.abs((rec["reward"] * F(0.5)) * scale)
    clip = float(np.median(r[r > 0]))
    e.rew_norm_init(clip=clip)
    e.rew_norm_update()
    assert e.rew_norm_state()["scale"] == scale
    on = e.pg_advantages(fetch=True)
    ref = RR.twin_gae(lib, *args, scale, clip, **opts)
    assert _same(on[0], ref[0]) and _same(on[1], ref[1])
    assert not _same(on[1], off[1]), "the clip was meant to bind"
    if N == 3:
        num = RR.gae(*args, scale, clip, **opts)
        assert _same(on[0], num[0]) and _same(on[1], num[1]), "the numpy restatement"
    e.close()


# ---- 3. per-member normalisers ---------------------------------------------------------------------------------------------------
def _population(amd, pols, N, T, configs, planes=None):
    e = _engine(amd, _planes(N) if planes is None else planes)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(len(pols))
    for m, pol in enumerate(pols):
        e.mlp_set_learner(m, pol)
    e.rollout_enable(T, obs=True)
    e.pg_pop_init(configs)
    return e


@pytest.mark.parametrize("M,N,T", [(2, 132, 16), (3, 6, 5)])
def test_members_equal_the_host_twin_and_solo_engines(amd, lib, M, N, T):
    n = N // M
    rng = np.random.default_rng(10 * M)
    pols = [_policy(rng) for _ in range(M)]
    configs = [dict(gamma=float(F(g)), lam=0.9, normalize_advantages=bool(m % 2)) for m, g in enumerate(np.linspace(0.8, 0.99, M))]
    planes = _planes(N)
    e = _population(amd, pols, N, T, configs, planes)
    e.rew_norm_init(per_member=True, clip=2.0)
    refs = [RR.fresh(n) for _ in range(M)]
    solos = []
    for m in range(M):
        s = _solo(amd, pols[m], n, T, planes=planes[:, m * n:(m + 1) * n], env_id_base=m * n, **configs[m])
        s.rew_norm_init(clip=2.0)
        solos.append(s)
    for it in range(2):                                         # (the second rollout merges into count > 0)
        e.rollout_reset()
        e.run_days("mlp", T, BUDGET)
        e.rew_norm_update()
        rec = e.rollout_fetch(bootstrap=True)
        adv, ret = e.pg_pop_advantages(fetch=True)
        for m in range(M):
            sl = PP.member_slice(m, n)
            refs[m] = RR.twin(lib, refs[m], *_days(rec, sl=sl), F(configs[m]["gamma"]))
            got = _state(e, m, n)
            assert RR.same(got, refs[m]), (m, it)
            r = PP.member_record(rec, m, n)
            radv, rret = RR.twin_gae(lib, r["reward"], r["terminated"], r["truncated"], r["value"], r["bootstrap_value"], got["scale"], 2.0,
                                     **configs[m])
            assert _same(adv[:, sl], radv) and _same(ret[:, sl], rret), (m, it)
            # a single engine of the member's envs
            s = solos[m]
            s.rollout_reset()
            s.run_days("mlp", T, BUDGET)
            s.rew_norm_update()
            assert _same(s.rollout_fetch()["reward"], r["reward"]), (m, it)
            assert RR.same(_state(s), got), (m, it)
            sadv, sret = s.pg_advantages(fetch=True)
            assert _same(sadv, adv[:, sl]) and _same(sret, ret[:, sl]), (m, it)
    assert not RR.same(refs[0], refs[1], returns=False)
    assert all(r["count"] == 2 * T * n for r in refs)
    # a changed gamma is the one the next update uses
    e.pg_pop_set_config(0, **dict(configs[0], gamma=0.5))
    e.rollout_reset()
    e.run_days("mlp", T, BUDGET)
    e.rew_norm_update()
    rec = e.rollout_fetch()
    assert RR.same(_state(e, 0, n), RR.twin(lib, refs[0], *_days(rec, sl=PP.member_slice(0, n)), F(0.5)))
    assert RR.same(_state(e, 1, n), RR.twin(lib, refs[1], *_days(rec, sl=PP.member_slice(1, n)), F(configs[1]["gamma"])))
    for s in solos:
        s.close()
    e.close()


def test_a_shared_normaliser_over_a_population_discounts_every_env_by_its_member(amd, lib):
    M, N, T = 3, 6, 5
    n = N // M
    rng = np.random.default_rng(31)
    pols = [_policy(rng) for _ in range(M)]
    gammas = [float(F(g)) for g in (0.5, 0.9, 1.0)]
    e = _population(amd, pols, N, T, [dict(gamma=g) for g in gammas])
    e.rew_norm_init(clip=0.0)
    e.run_days("mlp", T, BUDGET)
    e.rew_norm_update()
    rec = e.rollout_fetch(bootstrap=True)
    got = _state(e)
    assert RR.same(got, RR.twin(lib, RR.fresh(N), *_days(rec), np.repeat(np.array(gammas, F), n)))
    adv, ret = e.pg_pop_advantages(fetch=True)
    for m in range(M):
        r = PP.member_record(rec, m, n)
        radv, rret = RR.twin_gae(lib, r["reward"], r["terminated"], r["truncated"], r["value"], r["bootstrap_value"], got["scale"], 0.0, gamma=gammas[m])
        assert _same(adv[:, PP.member_slice(m, n)], radv) and _same(ret[:, PP.member_slice(m, n)], rret), m
    e.close()


# ---- 4. the trainers: an iteration against the host restatement, resume, off means off ------------------------------------------
CFG = dict(epochs=2, minibatches=3, lr=3e-3, gamma=0.9)


def test_an_iteration_equals_the_host_restatement(amd, lib):
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    N, T = 3, 5
    rng = np.random.default_rng(404)
    pol = _policy(rng)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    planes = _planes(N)

    def trainer():
        return PGTrainer(_engine(amd, planes), pol, T, agent_seeds=seeds, normalize_rewards=True, rew_norm=dict(clip=1.5), **CFG)
    # the sequence by hand on a second engine, for the record and the bootstrap value before the weights move
    by_hand = trainer()
    h = by_hand.engine
    h.rollout_reset()
    h.run_days("mlp", T, BUDGET)
    h.rew_norm_update()
    rec = h.rollout_fetch(bootstrap=True)
    h.close()
    tr = trainer()
    assert tr.normalize_rewards
    tr.iteration(budget=BUDGET)
    assert _same(tr.engine.rollout_fetch()["reward"], rec["reward"])
    st = RR.twin(lib, RR.fresh(N), *_days(rec), F(0.9))
    assert RR.same(tr.rew_norm_state(), st)
    opts = P.options(**tr.config)
    ref = RR.pg_update(pol, PP.fresh_state(pol), rec, rec["bootstrap_value"], st["scale"], 1.5, tr.epochs, opts)
    got = tr.state()
    for k in ("theta", "m", "v"):
        assert _same(got[k], ref[k]), k
    assert got["steps"] == ref["steps"] == 6
    assert not _same(got["theta"], RR.pg_update(pol, PP.fresh_state(pol), rec, rec["bootstrap_value"], F(1.0), 0.0, tr.epochs, opts)["theta"])
    tr.engine.close()


def test_a_population_iteration_equals_the_host_restatement(amd, lib):
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer
    M, N, T = 3, 6, 5
    n = N // M
    rng = np.random.default_rng(505)
    pols = [_policy(rng) for _ in range(M)]
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    configs = [dict(epochs=2, minibatches=2, lr=3e-3, gamma=float(F(g))) for g in (0.8, 0.9, 0.99)]
    planes = _planes(N)

    def trainer():
        return PGPopulationTrainer(_engine(amd, planes), pols, T, configs, agent_seeds=seeds, normalize_rewards=True, rew_norm=dict(clip=1.5))
    by_hand = trainer()
    h = by_hand.engine
    h.rollout_reset()
    h.run_days("mlp", T, BUDGET)
    h.rew_norm_update()
    rec = h.rollout_fetch(bootstrap=True)
    h.close()
    tr = trainer()
    tr.iteration(budget=BUDGET)
    assert _same(tr.engine.rollout_fetch()["reward"], rec["reward"])
    for m in range(M):
        st = RR.twin(lib, RR.fresh(n), *_days(rec, sl=PP.member_slice(m, n)), F(configs[m]["gamma"]))
        assert RR.same(tr.rew_norm_state(m), st), m
        r = PP.member_record(rec, m, n)
        ref = RR.pg_update(pols[m], PP.fresh_state(pols[m]), r, r["bootstrap_value"], st["scale"], 1.5, tr.epochs, P.options(**tr.configs[m]))
        got = tr.state(m)
        for k in ("theta", "m", "v"):
            assert _same(got[k], ref[k]), (k, m)
    tr.engine.close()


def test_a_resumed_trainer_continues_bit_for_bit(amd):
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    N, T = 6, 5
    rng = np.random.default_rng(606)
    pol = _policy(rng)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    planes = _planes(N)

    def trainer():
        return PGTrainer(_engine(amd, planes), pol, T, agent_seeds=seeds, normalize_rewards=True, **CFG)
    tr = trainer()
    full = []
    for _ in range(3):
        tr.iteration(budget=BUDGET)
        full.append((tr.state(), tr.rew_norm_state()))
    assert full[0][1]["count"] == T * N and full[2][1]["count"] == 3 * T * N
    assert np.any(full[0][1]["returns"] != 0), "the carry is part of what a resumed run needs"
    tr.engine.close()
    # iteration 1's state alone, carried into a fresh engine stepped to the same env position
    tr = trainer()
    tr.engine.run_days("mlp", T, BUDGET)
    assert tr.rew_norm_state()["count"] == 0
    tr.state(full[0][0])
    tr.rew_norm_state(full[0][1])
    assert RR.same(tr.rew_norm_state(), full[0][1])
    for it in (1, 2):
        tr.iteration(budget=BUDGET)
        for k in ("theta", "m", "v"):
            assert _same(tr.state()[k], full[it][0][k]), (k, it)
        assert RR.same(tr.rew_norm_state(), full[it][1]), it
    tr.engine.close()


def test_off_means_off(amd):
    """an engine that never had a normaliser, and one whose normaliser was dropped by a fresh pg_init: the same theta"""
    from adcraft_amd import _ffi
    N, T = 6, 5
    rng = np.random.default_rng(707)
    pol = _policy(rng)
    opts = dict(gamma=0.9, lr=3e-3, minibatch_envs=2)
    thetas = []
    for tried in (False, True):
        e = _solo(amd, pol, N, T, **opts)
        if tried:
            e.rew_norm_init()
            assert e.rew_norm_state()["count"] == 0
            e.pg_init(**opts)
            with pytest.raises(_ffi.EngineStateError, match="rew_norm_init"):
                e.rew_norm_state()
        e.run_days("mlp", T, BUDGET)
        e.pg_update(2)
        for call in (lambda: e.rew_norm_update(), lambda: e.rew_norm_returns(), lambda: e.rew_norm_copy([-1])):
            with pytest.raises(_ffi.EngineStateError, match="rew_norm_init"):
                call()
        thetas.append(e.pg_state()["theta"])
        e.close()
    assert _same(thetas[0], thetas[1])


# ---- 5. copy, the scheduler, reset ------------------------------------------------------------------------------------------------
def test_copy_and_the_scheduler_carry_the_donors_normaliser(amd):
    from adcraft_amd.baselines.pbt import PBTScheduler
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer
    N, T, M = 12, 5, 4
    rng = np.random.default_rng(808)
    pols = [_policy(rng) for _ in range(M)]
    e = _engine(amd, _planes(N))
    tr = PGPopulationTrainer(e, pols, T, [dict(epochs=1, minibatches=1, lr=float(F(lr)), gamma=0.9) for lr in np.logspace(-4, -2, M)],
                             normalize_rewards=True)
    tr.iteration(budget=BUDGET)
    before = [e.rew_norm_state(m) for m in range(M)]
    carry = e.rew_norm_returns()
    assert all(b["count"] == T * N // M for b in before) and before[0]["M2"] != before[2]["M2"] and np.any(carry != 0)
    with pytest.raises(ValueError, match="also a source"):
        e.rew_norm_copy([1, 2, -1, -1])
    with pytest.raises(ValueError, match="src_of_m"):
        e.rew_norm_copy([4, -1, -1, -1])
    e.rew_norm_copy([-1, 0, 2, 0])
    for m, src in enumerate((0, 0, 2, 0)):
        assert e.rew_norm_state(m) == before[src], m
    assert _same(e.rew_norm_returns(), carry), "the carry is the envs': a copy leaves it"
    # a scheduler's round: every replaced member has its donor's normaliser, the kept ones their own
    sch = PBTScheduler(tr, replace_fraction=0.25, tuned=("lr",), bounds={"lr": (1e-4, 1e-2)}, seed=9)
    tr.iteration(budget=BUDGET)
    before = [e.rew_norm_state(m) for m in range(M)]
    carry = e.rew_norm_returns()
    raw = tr.returns()
    res = sch.step()
    assert (res["src"] >= 0).sum() == 1
    assert np.allclose(res["fitness"], raw, rtol=1e-12), "the fitness is the raw recorded reward's, whatever the normaliser holds"
    for m in range(M):
        src = int(res["src"][m])
        assert e.rew_norm_state(m) == before[m if src < 0 else src], m
    assert _same(e.rew_norm_returns(), carry)
    tr.iteration(budget=BUDGET)
    e.close()


def test_a_masked_reset_zeroes_exactly_the_masked_envs_carry(amd):
    N, T = 6, 5
    e = _solo(amd, _policy(np.random.default_rng(909)), N, T, gamma=0.9)
    e.rew_norm_init()
    e.run_days("mlp", T, BUDGET)
    e.rew_norm_update()
    assert np.any(e.rew_norm_returns() != 0), "day 5 is the first of an episode: its reward is carried"
    carry = e.rew_norm_returns() + np.arange(1, N + 1) * 0.5                  # (every env's nonzero, whatever it earned)
    e.rew_norm_returns(carry)
    mask = np.array([1, 0, 0, 1, 1, 0], np.uint8)
    e.reset(env_mask=mask)
    now = e.rew_norm_returns()
    assert np.all(now[mask == 1] == 0) and _same(now[mask == 0], carry[mask == 0])
    st = e.rew_norm_state()
    e.reset()
    assert not e.rew_norm_returns().any() and e.rew_norm_state() == st, "a reset ends the envs' returns and leaves the moments"
    # the getter / setter of the carry
    e.rew_norm_returns(carry)
    assert _same(e.rew_norm_returns(), carry)
    with pytest.raises(ValueError, match="one value per env"):
        e.rew_norm_returns(carry[:3])
    e.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(amd):
    from adcraft_amd import _ffi
    N, T = 6, 5
    rng = np.random.default_rng(1010)
    pol = R.random_policy(rng, K, (8,), normalize=True)                 # (no value network: TD3 takes it too)
    pol.shift, pol.scale = R.realistic_norm(K)
    opts = dict(gamma=0.9, lr=3e-3)
    e = _engine(amd, _planes(N))
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    # init: no trainer; per_member without a population; a TD3 trainer, either way round
    with pytest.raises(_ffi.EngineStateError, match="pg_init"):
        e.rew_norm_init()
    e.pg_init(**opts)
    with pytest.raises(_ffi.EngineStateError, match="population"):
        e.rew_norm_init(per_member=True)
    with pytest.raises(ValueError, match="min_std"):
        e.rew_norm_init(min_std=0.0)
    # after the refused inits the update is that of an engine that never tried
    e.run_days("mlp", T, BUDGET)
    e.pg_update(1)
    other = _engine(amd, _planes(N))
    other.mlp_init(pol, deterministic=False)
    other.rollout_enable(T, obs=True)
    other.pg_init(**opts)
    other.run_days("mlp", T, BUDGET)
    other.pg_update(1)
    assert _same(e.pg_state()["theta"], other.pg_state()["theta"])
    other.close()
    base = dict(critic_widths=(8, 1), batch_size=8, capacity=40)
    e.rew_norm_init()
    e.rollout_reset()
    with pytest.raises(_ffi.EngineStateError, match="no day has been recorded"):
        e.rew_norm_update()
    with pytest.raises(_ffi.EngineStateError, match="reward normaliser"):
        e.td3_init(**base)
    for member in (-1, 1):
        with pytest.raises(ValueError, match="no such normaliser"):
            e.rew_norm_state(member)
    with pytest.raises(_ffi.EngineStateError, match="shared"):
        e.rew_norm_copy([-1])
    bad = dict(e.rew_norm_state(), scale=F(0.0))
    with pytest.raises(ValueError, match="scale"):
        e.rew_norm_state(0, bad)
    e.rollout_enable(T, obs=True)                                       # (ends the trainer and the normaliser)
    with pytest.raises(_ffi.EngineStateError, match="rew_norm_init"):
        e.rew_norm_state()
    e.td3_init(**base)
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.rew_norm_init()
    # lifetime: pg_init, mlp_init, mlp_learners, pg_pop_init end it
    for end in (lambda: e.pg_init(**opts), lambda: e.mlp_learners(2), lambda: e.mlp_init(pol, deterministic=False)):
        e.rollout_enable(T, obs=True)
        e.mlp_learners(0)
        e.pg_init(**opts)
        e.rew_norm_init()
        end()
        with pytest.raises(_ffi.EngineStateError, match="rew_norm_init"):
            e.rew_norm_state()
    e.mlp_learners(2)
    e.rollout_enable(T, obs=True)
    e.pg_pop_init(opts)
    e.rew_norm_init(per_member=True)
    with pytest.raises(ValueError, match="no such normaliser"):
        e.rew_norm_state(2)
    with pytest.raises(_ffi.EngineStateError, match="reward normaliser"):
        e.td3_pop_init(base)
    e.pg_pop_init(opts)
    with pytest.raises(_ffi.EngineStateError, match="rew_norm_init"):
        e.rew_norm_state()
    # the engine still works: recorded days, an update of both, a state
    e.rew_norm_init(per_member=True)
    e.run_days("mlp", 2, BUDGET)
    e.rew_norm_update()
    e.pg_pop_update(1)
    st = e.rew_norm_state(1)
    assert st["count"] == 2 * N // 2 and np.isfinite(st["M2"]) and st["scale"] > 0
    e.close()
