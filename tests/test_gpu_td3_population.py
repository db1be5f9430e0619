"""GPU tests of TD3 learner populations (parts/kernel_td3_pop.inc, parts/td3_pop_api.inc): M off-policy learners in lock-step on one
engine.  Everything a member computes - its ring, its batch indices, theta, psi, both targets, the four moment vectors, the
counters, its statistics - is held, bit for bit, against the numpy restatement tests/td3_ref.py on the member's slice
(tests/td3_pop_ref.py) and against a solo engine of the member's envs at env_id_base = m n.  No tolerances anywhere.  None of
these symbols exists before this feature: every test here fails on the parent commit."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import td3_pop_ref as TP
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


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


SEED, BUDGET = 41, 1000.0
RESETS = dict(max_days=4, auto_reset=True)
N, K, M, T = 12, 5, 3, 6
n, D, A = N // M, 5 * K + 2, K + 1
HIDDEN, WIDTHS, B0 = (20, 9), (11, 7, 1), 7
SIGMAS = (0.2, 0.05, 0.4)
# what all members share, then what is each member's own: two take the engine's seed, one its own; one clips, two do not
SHARED = dict(critic_widths=WIDTHS, batch_size=B0, policy_delay=2)
OWN = (dict(gamma=0.9, tau=0.05, actor_lr=1e-3, critic_lr=3e-3, target_noise=0.3, target_noise_clip=0.25, reward_scale=0.5, seed=0),
       dict(gamma=0.99, tau=0.01, actor_lr=3e-3, critic_lr=1e-3, target_noise=0.1, target_noise_clip=0.2, seed=77, max_grad_norm=0.5),
       dict(gamma=0.8, tau=0.2, actor_lr=2e-3, critic_lr=2e-3, beta1=0.8, beta2=0.99, action_lo=0.05, action_hi=0.9, reward_scale=0.1, seed=0))


def _options(capacity, members=M, **shared):
    return [T3.options(**dict(SHARED, capacity=capacity, **dict(OWN[m], **shared))) for m in range(members)]


def _planes(envs=N):
    return H.implicit_params(envs, K, SEED + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, env_id_base=0, **kw):
    e = amd.StepEngine(planes.shape[1], planes.shape[2], seed=SEED, env_id_base=env_id_base, **kw)
    e.set_all_params(planes)
    e.reset()
    return e


def _action_norm():
    return np.full(A, 0.25, F), np.full(A, 1.5, F)


def _members(seed, members=M, widths=WIDTHS):
    """per member: a policy (its log_std the member's exploration sigma) and two critics, all different; the normalisation is shared"""
    rng = np.random.default_rng(seed)
    pols, crits = [], []
    for m in range(members):
        pol = R.random_policy(rng, K, HIDDEN, "tanh", normalize=True, scale=0.6)
        pol.shift, pol.scale = R.realistic_norm(K)
        pol.log_std = np.full(A, np.log(SIGMAS[m]), F)
        pols.append(pol)
        crits.append(T3.random_critics_for_tests(rng, K, widths))
    return pols, crits


def _population(amd, pols, crits, opts, planes=None, horizon=T, **engine_kw):
    e = _engine(amd, _planes() if planes is None else planes, **dict(RESETS, **engine_kw))
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(len(pols))
    for m in range(1, len(pols)):
        e.mlp_set_learner(m, pols[m])
    e.rollout_enable(horizon, obs=True)
    e.td3_pop_init(opts)
    for m in range(len(pols)):
        e.td3_pop_set_critics(m, crits[m], action_norm=_action_norm() if m == 0 else None)
    return e


def _solo(amd, pol, crit, opts, m, envs=n, horizon=T):
    """the solo twin of member m: an engine of the member's envs at env_id_base = m envs, the same planes and seeds"""
    e = _engine(amd, _planes()[:, TP.member_slice(m, envs)], env_id_base=m * envs, **RESETS)
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(horizon, obs=True)
    e.td3_init(**opts)
    e.td3_set_critics(crit, action_norm=_action_norm())
    return e


def _random_buffer(rng, size):
    return dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * 0.5 + 0.4).astype(F),
                r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))


def _assert_state(got, ref, what=""):
    for k in T3.STATE_KEYS:
        assert _same(got[k], ref[k]), (k, what)
    assert (got["updates"], got["actor_steps"]) == (ref["updates"], ref["actor_steps"]), what


def _assert_stats(got, ref, what="", keys=T3.STAT_KEYS):
    for k in keys:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


def _assert_buffer(got, ref, what=""):
    for k in ("x", "a", "r", "done", "x2"):
        assert _same(got[k], ref[k]), (k, what)
    assert (got["size"], got["written"], got["capacity"]) == (ref["size"], ref["written"], ref["capacity"]), what


def _current_input(e, pol):
    return T3.current_input(pol, e.fetch(), e.get_episode_state()[0] == 0)


CRITIC_STATS = ("critic_loss", "q1_mean", "q2_mean", "y_mean", "critic_grad_norm")
ACTOR_STATS = ("actor_loss", "actor_grad_norm")


# ---- 1. the store ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [10, 40])
def test_store_fills_every_members_ring_as_the_restatement_and_a_solo_engine(amd, capacity):
    """two collections of T = 6 days through auto-resets, 24 transitions per member each: longer than a ring of 10 (the skip rule),
    and a ring of 40 wraps in the second store"""
    from adcraft_amd import _ffi
    pols, crits = _members(301)
    opts = _options(capacity)
    e = _population(amd, pols, crits, opts)
    solos = [_solo(amd, pols[m], crits[m], opts[m], m) for m in range(M)]
    rings = [TP.MemberRing(capacity, D, A, m, n) for m in range(M)]
    assert e.td3_pop_buffer(fetch=False) == dict(size=0, written=0, capacity=capacity, batch_size=B0)
    for rnd in range(2):
        e.rollout_reset()
        e.run_days("mlp", T, BUDGET)
        assert e.td3_pop_store() == T * n
        rec, now = e.rollout_fetch(), _current_input(e, pols[0])
        done = rec["terminated"] | rec["truncated"]
        assert done.any() and not done.all(), "the record was meant to cross an episode end"
        for m in range(M):
            rings[m].store(rec, now)
            got = e.td3_pop_buffer(m)
            _assert_buffer(got, rings[m].buffer(), (rnd, m))
            s = solos[m]
            s.rollout_reset()
            s.run_days("mlp", T, BUDGET)
            assert s.td3_store() == T * n
            _assert_buffer(got, s.td3_buffer(), ("solo", rnd, m))
    assert e.td3_pop_buffer(fetch=False)["written"] == 2 * T * n
    assert not _same(e.td3_pop_buffer(0)["x"], e.td3_pop_buffer(1)["x"]), "members differ, or the test would show nothing"
    # the envs stepped outside the record since an unstored recorded day
    e.rollout_reset()
    e.run_days("mlp", 1, BUDGET)
    e.run_days("fixed", 1, BUDGET)
    with pytest.raises(_ffi.EngineStateError, match="outside the record"):
        e.td3_pop_store()
    with pytest.raises(_ffi.EngineStateError, match="outside the record"):
        e.td3_pop_store()
    e.rollout_reset()
    with pytest.raises(_ffi.EngineStateError, match="no unstored day"):
        e.td3_pop_store()
    for s in solos:
        s.close()
    e.close()


# ---- 2. batch indices ------------------------------------------------------------------------------------------------------------
def test_batch_indices_are_the_restatements_under_the_members_key(amd):
    pols, crits = _members(302)
    opts = _options(40)
    e = _population(amd, pols, crits, opts)
    rng = np.random.default_rng(3)
    for m in range(M):
        e.td3_pop_buffer_load(m, _random_buffer(rng, 33))
    for u in (0, 3):
        idx = [e.td3_pop_batch_indices(m, u) for m in range(M)]
        for m in range(M):
            assert _same(idx[m], T3.batch_indices(TP.member_seed(opts[m], SEED), u, 33, B0)), (m, u)
            assert idx[m].min() >= 0 and idx[m].max() < 33
        assert _same(idx[0], idx[2]), "two members that take the engine's seed share their indices"
        assert not _same(idx[0], idx[1]), "a member with its own seed does not"
    e.close()


# ---- 3. updates against the restatement ------------------------------------------------------------------------------------------
def test_five_updates_equal_the_restatement_on_every_members_ring(amd):
    """one collection stored (24 transitions per member), then U = 5 updates one at a time with policy_delay 2 and B = 7: updates 2
    and 4 step the actors and move the targets.  One member clips its gradients, two do not."""
    pols, crits = _members(303)
    opts = _options(40)
    e = _population(amd, pols, crits, opts)
    states = [T3.fresh_state(pols[m], crits[m]) for m in range(M)]
    assert e.td3_pop_param_counts() == (states[0]["theta"].size, states[0]["psi"].size)
    for m in range(M):
        _assert_state(e.td3_pop_state(m), states[m], "theta starts as the member's device policy, the targets as copies")
    e.run_days("mlp", T, BUDGET)
    assert e.td3_pop_store() == T * n
    bufs = [e.td3_pop_buffer(m) for m in range(M)]
    for u in range(5):
        stats = e.td3_pop_update(1)
        assert len(stats) == M
        for m in range(M):
            states[m], rstats = TP.member_update(pols[m], states[m], bufs[m], _action_norm(), opts[m], SEED)
            _assert_state(e.td3_pop_state(m), states[m], (u, m))
            _assert_stats(stats[m], rstats, (u, m))
            assert (stats[m]["updates"], stats[m]["actor_steps"], stats[m]["buffer_size"], stats[m]["samples"]) == (u + 1, (u + 1) // 2, T * n, B0)
    assert not _same(states[0]["theta"], T3.flat_of(pols[0].layers)) and not _same(states[0]["psi_target"], states[0]["psi"])
    e.close()


# ---- 4. updates against solo twins -----------------------------------------------------------------------------------------------
def test_two_iterations_equal_three_solo_trainers(amd):
    """collect -> store -> three updates, twice, through TD3PopulationTrainer against three TD3Trainer engines of 4 envs at
    env_id_base = 4 m: states, statistics, rings, and the third collection's recorded actions - the updated actors reach the
    policy kernel"""
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer, TD3Trainer
    pols, crits = _members(304)
    opts = _options(40)
    keys = lambda o: {k: v for k, v in o.items() if k != "critic_widths"}
    common = dict(critic_hidden=WIDTHS[:-1], learning_starts=T * n, updates_per_iteration=3)
    e = _engine(amd, _planes(), **RESETS)
    tr = TD3PopulationTrainer(e, pols, SIGMAS, [dict(keys(opts[m]), critics=crits[m], action_norm=_action_norm(), **common) for m in range(M)], horizon=T)
    solos = []
    for m in range(M):
        s = _engine(amd, _planes()[:, TP.member_slice(m, n)], env_id_base=m * n, **RESETS)
        solos.append((s, TD3Trainer(s, pols[m], horizon=T, exploration_sigma=SIGMAS[m], critics=crits[m], action_norm=_action_norm(), **common,
                                    **keys(opts[m]))))
    for it in range(2):
        stats = tr.iteration(T, BUDGET)
        for m, (s, st) in enumerate(solos):
            sstats = st.iteration(T, BUDGET)
            _assert_state(tr.state(m), st.state(), (it, m))
            _assert_stats(stats[m], sstats, (it, m))
            _assert_buffer(e.td3_pop_buffer(m), s.td3_buffer(), (it, m))
            assert _same(e.mlp_learner_params(m)[:st.state()["theta"].size], st.state()["theta"])
            assert _same(T3.flat_of(tr.policy(m).layers), st.state()["theta"])
    assert tr.state(0)["updates"] == 6 and tr.state(0)["actor_steps"] == 3
    assert not _same(tr.state(0)["theta"], T3.flat_of(pols[0].layers))
    # a member's exploration from the next day on, through the trainer, as the solo trainer's
    tr.set_exploration(0.3, member=1)
    solos[1][1].set_exploration(0.3)
    e.rollout_reset()
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch()
    for m, (s, _) in enumerate(solos):
        s.rollout_reset()
        s.run_days("mlp", T, BUDGET)
        srec = s.rollout_fetch()
        for k in ("action", "obs", "reward"):
            assert _same(TP.member_record(rec, m, n)[k], srec[k]), (k, m)
        s.close()
    e.close()


# ---- 5. one call of U updates equals U calls of one ------------------------------------------------------------------------------
def test_one_call_of_five_updates_equals_five_calls_of_one(amd):
    pols, crits = _members(305)
    opts = _options(40)
    rng = np.random.default_rng(5)
    bufs = [_random_buffer(rng, 37) for _ in range(M)]
    engines = [_population(amd, pols, crits, opts) for _ in range(3)]
    for e in engines:
        for m in range(M):
            e.td3_pop_buffer_load(m, bufs[m])
    at_once = engines[0].td3_pop_update(5)
    singles = [engines[1].td3_pop_update(1) for _ in range(5)]
    assert engines[2].td3_pop_update(5, stats=False) is None
    for m in range(M):
        ref = engines[0].td3_pop_state(m)
        assert ref["updates"] == 5 and ref["actor_steps"] == 2
        _assert_state(engines[1].td3_pop_state(m), ref, ("one at a time", m))
        _assert_state(engines[2].td3_pop_state(m), ref, ("without statistics", m))
        _assert_stats(at_once[m], singles[4][m], m, CRITIC_STATS)                 # the call's last update
        _assert_stats(at_once[m], singles[3][m], m, ACTOR_STATS)                  # the call's last actor step (update 4)
        assert singles[4][m]["actor_grad_norm"] == 0.0 and at_once[m]["actor_grad_norm"] > 0.0
    for e in engines:
        e.close()


# ---- 6. a second chunk -----------------------------------------------------------------------------------------------------------
def test_a_batch_of_1100_is_two_chunks_per_member(amd):
    """B = 1100 > 1024: the chunked float64 sums of a member run over two chunks of its own batch elements.  Critics (9,), a ring
    of 64, policy_delay 1: one update with the actor step.  State and statistics equal the solo twin's."""
    pols, crits = _members(306, widths=(9, 1))
    opts = _options(64, critic_widths=(9, 1), batch_size=1100, policy_delay=1)
    rng = np.random.default_rng(6)
    bufs = [_random_buffer(rng, 50) for _ in range(M)]
    e = _population(amd, pols, crits, opts)
    for m in range(M):
        e.td3_pop_buffer_load(m, bufs[m])
    stats = e.td3_pop_update(1)
    for m in range(M):
        s = _solo(amd, pols[m], crits[m], opts[m], m)
        s.td3_buffer_load(bufs[m])
        sstats = s.td3_update(1)
        got = e.td3_pop_state(m)
        assert got["actor_steps"] == 1
        _assert_state(got, s.td3_state(), m)
        _assert_stats(stats[m], sstats, m)
        s.close()
    e.close()


# ---- 7. M = 1 --------------------------------------------------------------------------------------------------------------------
def test_a_population_of_one_is_the_solo_engine(amd):
    pols, crits = _members(307, members=1)
    opts = _options(40, members=1)
    planes = _planes()[:, :n]
    e = _population(amd, pols, crits, opts, planes=planes)
    s = _solo(amd, pols[0], crits[0], opts[0], 0)
    for rnd in range(2):
        for x in (e, s):
            x.rollout_reset()
            x.run_days("mlp", T, BUDGET)
        assert e.td3_pop_store() == s.td3_store() == T * n
        stats, sstats = e.td3_pop_update(3), s.td3_update(3)
        _assert_buffer(e.td3_pop_buffer(0), s.td3_buffer(), rnd)
        _assert_state(e.td3_pop_state(0), s.td3_state(), rnd)
        _assert_stats(stats[0], sstats, rnd)
    for x in (e, s):
        x.close()


# ---- 8. resume and the population-based-training primitives ----------------------------------------------------------------------
def test_resume_copy_and_set_config(amd):
    pols, crits = _members(308)
    opts = _options(40)
    rng = np.random.default_rng(8)
    bufs = [_random_buffer(rng, 29) for _ in range(M)]
    a = _population(amd, pols, crits, opts)
    for m in range(M):
        a.td3_pop_buffer_load(m, bufs[m])
    a.td3_pop_update(3)
    saved = [(a.td3_pop_state(m), a.td3_pop_buffer(m)) for m in range(M)]
    a.td3_pop_update(2)
    final = [a.td3_pop_state(m) for m in range(M)]
    # a fresh engine (other critics at first) resumed from the saved states and rings continues to the same bits
    b = _population(amd, pols, _members(999)[1], opts)
    for m in range(M):
        b.td3_pop_state(m, saved[m][0])
        b.td3_pop_buffer_load(m, saved[m][1])
    for m in range(M):
        _assert_state(b.td3_pop_state(m), saved[m][0], m)
        _assert_buffer(b.td3_pop_buffer(m), dict(saved[m][1]), m)
        assert _same(b.mlp_learner_params(m)[:saved[m][0]["theta"].size], saved[m][0]["theta"]), "the member's policy layers follow its theta"
    b.td3_pop_update(2)
    for m in range(M):
        _assert_state(b.td3_pop_state(m), final[m], ("resumed", m))
    # copy 0 -> 2 with the ring: member 2 goes on as member 0 would under member 2's configuration (and envs)
    a.td3_pop_copy(0, 2, with_ring=True)
    _assert_state(a.td3_pop_state(2), final[0], "the copy")
    _assert_buffer(a.td3_pop_buffer(2), a.td3_pop_buffer(0), "the copied ring")
    _assert_state(a.td3_pop_state(1), final[1], "the copy touched member 1")
    assert _same(a.mlp_learner_params(2)[:final[0]["theta"].size], final[0]["theta"])
    twin = _solo(amd, pols[2], crits[2], opts[2], 2)
    twin.td3_state(final[0])
    twin.td3_buffer_load(a.td3_pop_buffer(0))
    a.td3_pop_update(2)
    twin.td3_update(2)
    _assert_state(a.td3_pop_state(2), twin.td3_state(), "member 2 after the copy against a solo twin built from the copied state")
    assert not _same(a.td3_pop_state(2)["psi"], a.td3_pop_state(0)["psi"]), "member 2 kept its own configuration"
    twin.close()
    # without the ring, dst keeps its own
    ring1 = a.td3_pop_buffer(1)
    a.td3_pop_copy(0, 1)
    _assert_state(a.td3_pop_state(1), a.td3_pop_state(0), "the copy without the ring")
    _assert_buffer(a.td3_pop_buffer(1), ring1, "the ring stayed")
    # a learning rate changed for one member from the next update on; a shared field may not change
    before = [b.td3_pop_state(m) for m in range(M)]
    changed = dict(opts[1], critic_lr=0.02)
    b.td3_pop_set_config(1, **changed)
    with pytest.raises(ValueError):
        b.td3_pop_set_config(1, **dict(changed, batch_size=B0 + 1))
    with pytest.raises(ValueError):
        b.td3_pop_set_config(3, **changed)
    b.td3_pop_update(1)
    for m in range(M):
        ref, _ = TP.member_update(pols[m], before[m], saved[m][1], _action_norm(), changed if m == 1 else opts[m], SEED)
        _assert_state(b.td3_pop_state(m), ref, ("set_config", m))
    old, _ = TP.member_update(pols[1], before[1], saved[1][1], _action_norm(), opts[1], SEED)
    assert not _same(old["psi"], b.td3_pop_state(1)["psi"])
    a.close()
    b.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(amd):
    from adcraft_amd import _ffi
    pols, crits = _members(309)
    opts = _options(40)
    rng = np.random.default_rng(9)
    e = _engine(amd, _planes(), **RESETS)
    e.mlp_init(pols[0], deterministic=False)
    e.rollout_enable(T, obs=True)
    # without learners
    with pytest.raises(_ffi.EngineStateError, match="learners"):
        e.td3_pop_init(opts[0])
    cfg = amd.StepEngine.td3_config(**opts[0])
    assert e._lib.adc_engine_td3_pop_init(e._h, C.byref(cfg), 1) == _ffi.ADC_ESTATE
    with pytest.raises(_ffi.EngineStateError, match="td3_pop_init"):
        e.td3_pop_update(1)
    # a two-headed policy
    e.mlp_init(R.random_policy(rng, K, HIDDEN, two_heads=True), deterministic=False)
    e.mlp_learners(M)
    with pytest.raises(_ffi.EngineStateError, match="two-headed"):
        e.td3_pop_init(opts)
    # without the recorded input
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    e.rollout_enable(T)
    with pytest.raises(_ffi.EngineStateError, match="ADC_ROLLOUT_OBS"):
        e.td3_pop_init(opts)
    e.rollout_enable(T, obs=True)
    # a policy-gradient population alive, and the reverse
    e.pg_pop_init(dict())
    with pytest.raises(_ffi.EngineStateError, match="policy-gradient"):
        e.td3_pop_init(opts)
    e.rollout_enable(T, obs=True)                                  # (ends the policy-gradient trainer)
    # the solo trainer keeps refusing an engine with learners
    with pytest.raises(_ffi.EngineStateError, match="learners active"):
        e.td3_init(**opts[0])
    # configurations that do not fit the members
    with pytest.raises(ValueError, match="count"):
        e.td3_pop_init(opts[:2])
    with pytest.raises(ValueError, match="equal"):
        e.td3_pop_init([opts[0], dict(opts[1], capacity=41), opts[2]])
    e.td3_pop_init(opts)
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.pg_pop_init(dict())
    with pytest.raises(_ffi.EngineStateError, match="td3_init"):
        e.td3_update(1)                                             # (the solo calls do not see the population)
    # an update before every member's critics are uploaded; on an empty ring
    for m in range(M - 1):
        e.td3_pop_set_critics(m, crits[m], action_norm=_action_norm())
    with pytest.raises(_ffi.EngineStateError, match="critic layer"):
        e.td3_pop_update(1)
    e.td3_pop_set_critics(M - 1, crits[M - 1])
    for call in (lambda: e.td3_pop_update(1), lambda: e.td3_pop_batch_indices(0, 0)):
        with pytest.raises(_ffi.EngineStateError, match="empty"):
            call()
    # members and counts out of range
    for call in (lambda: e.td3_pop_state(M), lambda: e.td3_pop_buffer_load(-1, _random_buffer(rng, 4)), lambda: e.td3_pop_copy(0, M),
                 lambda: e.td3_pop_sync_targets(M), lambda: e.td3_pop_set_critics(M, crits[0]), lambda: e.td3_pop_update(0)):
        with pytest.raises(ValueError):
            call()
    e.run_days("mlp", 2, BUDGET)
    assert e.td3_pop_store() == 2 * n
    assert e.td3_pop_update(2)[0]["updates"] == 2
    # the trainer goes with the learners it trains
    e.mlp_learners(M)
    with pytest.raises(_ffi.EngineStateError, match="td3_pop_init"):
        e.td3_pop_update(1)
    e.close()


def test_wrapped_member_rings_reloaded_at_a_slot_continue_bit_for_bit_and_the_shared_refusals_say_why(amd):
    """the smallest population whose store wraps the rings (2 members x 2 envs x 3 days into 5 slots): every member's state and
    ring - the ring loaded in two pieces, the second at slot 2 - carry a fresh engine through two more updates to the bits of the
    uninterrupted run; then every refusal the off-policy front ends share, by its words, and the engine goes on"""
    from adcraft_amd import _ffi
    members, envs, days = 2, 4, 3
    pols, crits = _members(7, members, widths=(8, 1))
    opts = _options(5, members, critic_widths=(8, 1), batch_size=4)
    fresh = lambda: _population(amd, pols, crits, opts, planes=_planes(envs), horizon=days)
    a = fresh()
    a.run_days("mlp", days, BUDGET)
    assert a.td3_pop_store() == 6
    a.td3_pop_update(1)
    states, rings = [a.td3_pop_state(m) for m in range(members)], [a.td3_pop_buffer(m) for m in range(members)]
    assert all((g["size"], g["written"], g["capacity"], g["batch_size"]) == (5, 6, 5, 4) for g in rings)
    assert not _same(rings[0]["x"], rings[1]["x"])
    b = fresh()
    part = lambda g, lo, hi: {k: g[k][lo:hi] for k in ("x", "a", "r", "done", "x2")}
    for m in range(members):
        b.td3_pop_buffer_load(m, part(rings[m], 0, 2))
        b.td3_pop_buffer_load(m, part(rings[m], 2, 5), slot=2, written=6)
        b.td3_pop_state(m, states[m])
    assert b.td3_pop_param_counts() == a.td3_pop_param_counts()
    for m in range(members):
        _assert_buffer(b.td3_pop_buffer(m), rings[m], m)
        _assert_state(b.td3_pop_state(m), states[m], m)
        assert _same(a.td3_pop_batch_indices(m, 1), b.td3_pop_batch_indices(m, 1)) and a.td3_pop_batch_indices(m, 1).shape == (4,)
    for sa, sb in zip(a.td3_pop_update(2), b.td3_pop_update(2)):
        _assert_stats(sb, sa)
    for m in range(members):
        _assert_state(b.td3_pop_state(m), a.td3_pop_state(m), m)
    assert b.td3_pop_state(0)["updates"] == 3
    a.close()
    lib, h, p = b._lib, b._h, lambda v: v.ctypes.data
    x, ac, r, dn = np.zeros((4, D), F), np.zeros((4, A), F), np.zeros(4, F), np.zeros(4, np.uint8)
    (w, bias), idx = crits[0][0][0], np.zeros(4, np.int32)
    last = [b.td3_pop_state(m) for m in range(members)]
    vec = [p(last[1][k]) for k in amd.StepEngine.TD3_STATE]
    refused = (
        (r"no such member", lambda: lib.adc_engine_td3_pop_buffer_fetch(h, 2, 0, 1, p(x), p(ac), p(r), p(dn), p(x))),
        (r"no such member", lambda: lib.adc_engine_td3_pop_batch_indices(h, -1, 0, p(idx))),
        (r"no such member", lambda: lib.adc_engine_td3_pop_copy(h, 0, 2, 1)),
        (r"slot range is not inside \[0, size\)", lambda: lib.adc_engine_td3_pop_buffer_fetch(h, 1, 4, 2, p(x), p(ac), p(r), p(dn), p(x))),
        (r"x, a, r, done or x2 is NULL", lambda: lib.adc_engine_td3_pop_buffer_load(h, 1, 0, 4, p(x), None, p(r), p(dn), p(x), 4)),
        (r"slot range is not inside \[0, capacity\)", lambda: lib.adc_engine_td3_pop_buffer_load(h, 1, 3, 4, p(x), p(ac), p(r), p(dn), p(x), 12)),
        (r"written: at least slot \+ count", lambda: lib.adc_engine_td3_pop_buffer_load(h, 1, 0, 4, p(x), p(ac), p(r), p(dn), p(x), 3)),
        (r"critic: 0 or 1", lambda: lib.adc_engine_td3_pop_set_critic_layer(h, 1, 2, 0, p(w), p(bias))),
        (r"no such critic layer", lambda: lib.adc_engine_td3_pop_set_critic_layer(h, 1, 0, 2, p(w), p(bias))),
        (r"weights or bias is NULL", lambda: lib.adc_engine_td3_pop_set_critic_layer(h, 1, 0, 0, p(w), None)),
        (r"idx_b is NULL", lambda: lib.adc_engine_td3_pop_batch_indices(h, 1, 0, None)),
        (r"update: 0 to 2\^32 - 2", lambda: lib.adc_engine_td3_pop_batch_indices(h, 1, -1, p(idx))),
        (r"updates: 1 to 65536", lambda: lib.adc_engine_td3_pop_update(h, 0, None)),
        (r"a state vector is NULL", lambda: lib.adc_engine_td3_pop_state_set(h, 1, *vec[:-1], None, 0, 0)),
        (r"updates: 0 to 2\^31 - 2", lambda: lib.adc_engine_td3_pop_state_set(h, 1, *vec, 2 ** 31 - 1, 0)),
    )
    for words, call in refused:
        with pytest.raises(ValueError, match=words):
            _ffi.check(call())
    for m in range(members):
        _assert_buffer(b.td3_pop_buffer(m), rings[m], m)
        _assert_state(b.td3_pop_state(m), last[m], m)
    assert b.td3_pop_update(1)[0]["updates"] == 4
    # one member's targets become copies; the other's stay
    b.td3_pop_sync_targets(1)
    synced, other = b.td3_pop_state(1), b.td3_pop_state(0)
    assert _same(synced["psi_target"], synced["psi"]) and not _same(other["psi_target"], other["psi"])
    assert _same(synced["theta_target"], synced["theta"]) and not _same(other["theta_target"], other["theta"])
    b.replay_prio_init()
    with pytest.raises(_ffi.EngineStateError, match="prioritised replay is alive"):
        b.td3_pop_batch_indices(0, 0)
    b.close()
