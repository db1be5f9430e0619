"""GPU tests of SAC learner populations (parts/kernel_sac_pop.inc, parts/sac_pop_api.inc) and of the learners' squashed act
(k_mlp_policy<2, true>): M soft actor-critic learners in lock-step on one engine.  Everything a member computes - its act, its
ring, its batch indices, theta, psi, target psi, the four moment vectors, its temperature cell, the counter, its statistics - is
held, bit for bit, against the numpy restatement tests/sac_ref.py on the member's slice (tests/sac_pop_ref.py) and against a solo
engine of the member's envs at env_id_base = m n.  No tolerances anywhere.  None of these symbols exists before this feature:
every test here fails on the parent commit."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import sac_pop_ref as SP
from tests import sac_ref as S
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
CLAMP = (-1.0, -0.5)
# what all members share, then what is each member's own: two take the engine's seed, one its own; one clips, two do not; one
# keeps its temperature (alpha_lr 0).  Five updates at target_update_interval 2 cross the Polyak gate both ways
SHARED = dict(critic_widths=WIDTHS, batch_size=B0, target_update_interval=2)
OWN = (dict(gamma=0.9, tau=0.05, actor_lr=1e-3, critic_lr=3e-3, alpha_lr=3e-3, target_entropy=-3.0, init_alpha=0.3, reward_scale=0.5, seed=0),
       dict(gamma=0.99, tau=0.01, actor_lr=3e-3, critic_lr=1e-3, alpha_lr=1e-3, target_entropy=-6.0, init_alpha=0.7, reward_scale=1.0, seed=77,
            max_grad_norm=0.5),
       dict(gamma=0.8, tau=0.2, actor_lr=2e-3, critic_lr=2e-3, alpha_lr=0.0, target_entropy=-1.0, init_alpha=1.5, reward_scale=0.1, beta1=0.8,
            beta2=0.99, seed=0))


def _options(capacity, members=M, **shared):
    return [S.options(K, **dict(SHARED, capacity=capacity, **dict(OWN[m], **shared))) for m in range(members)]


def _planes(envs=N):
    return H.implicit_params(envs, K, SEED + 1, mean_volume=24, cvr=0.5)


def _bounds():
    """budget in [50, 1500], bids in [0.02, 3 + k / 10]: shared by all members"""
    return np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], 3.0 + np.arange(K) / 10.0]).astype(F)


def _engine(amd, planes, env_id_base=0, **kw):
    e = amd.StepEngine(planes.shape[1], planes.shape[2], seed=SEED, env_id_base=env_id_base, **kw)
    e.set_all_params(planes)
    e.reset()
    return e


def _members(seed, members=M, widths=WIDTHS, value=False):
    """per member: a two-headed policy under the tight clamp (its log-std head's biases on both sides of it) and two critics, all
    different; the normalisation is shared"""
    rng = np.random.default_rng(seed)
    pols, crits = [], []
    for m in range(members):
        pol = S.sac_policy(rng, K, HIDDEN, "tanh", clamp=CLAMP, normalize=True, scale=0.6, value=value)
        pol.shift, pol.scale = R.realistic_norm(K)
        pol.layers[-1][1][A:] = np.linspace(CLAMP[0] - 0.6, CLAMP[1] + 0.6, A).astype(F)
        pols.append(pol)
        crits.append(T3.random_critics_for_tests(rng, K, widths))
    return pols, crits


def _learners(amd, pols, planes=None, squash=True, **engine_kw):
    e = _engine(amd, _planes() if planes is None else planes, **dict(RESETS, **engine_kw))
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(len(pols))
    for m in range(1, len(pols)):
        e.mlp_set_learner(m, pols[m])
    if squash:
        e.mlp_learners_set_squash(*_bounds())
    return e


def _population(amd, pols, crits, opts, planes=None, horizon=T, **engine_kw):
    e = _learners(amd, pols, planes, **engine_kw)
    e.rollout_enable(horizon, obs=True)
    e.sac_pop_init(opts)
    for m in range(len(pols)):
        e.sac_pop_set_critics(m, crits[m])
    return e


def _solo_engine(amd, pol, m, envs=n):
    """the solo twin of member m's envs: an engine of the member's envs at env_id_base = m envs, the same planes and seeds"""
    e = _engine(amd, _planes()[:, SP.member_slice(m, envs)], env_id_base=m * envs, **RESETS)
    e.mlp_init(pol, deterministic=False)
    e.mlp_set_squash(*_bounds())
    return e


def _solo(amd, pol, crit, opts, m, envs=n, horizon=T):
    e = _solo_engine(amd, pol, m, envs)
    e.rollout_enable(horizon, obs=True)
    e.sac_init(**opts)
    e.sac_set_critics(crit)
    return e


def _random_buffer(rng, size):
    return dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * 1.5).astype(F),
                r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))


def _assert_state(got, ref, what=""):
    for k in S.STATE_KEYS:
        assert _same(got[k], ref[k]), (k, what, got[k][:4], ref[k][:4])
    assert got["updates"] == ref["updates"], what


def _assert_stats(got, ref, what="", keys=S.STAT_KEYS):
    for k in keys:
        assert _same(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k], what)


def _assert_buffer(got, ref, what=""):
    for k in ("x", "a", "r", "done", "x2"):
        assert _same(got[k], ref[k]), (k, what)
    assert (got["size"], got["written"], got["capacity"]) == (ref["size"], ref["written"], ref["capacity"]), what


def _current_input(e, pol):
    return T3.current_input(pol, e.fetch(), e.get_episode_state()[0] == 0)


def _last_act(e):
    st = e.mlp_last()
    st["bids"], st["budget"] = e.get_actions()
    return st


ACT_KEYS = ("mean", "log_std", "action", "logp", "value", "bids", "budget")


# ---- 1. the learners' squashed act -----------------------------------------------------------------------------------------------
def test_a_day_of_learners_under_their_squash_equals_three_solo_engines(amd):
    """two recorded days (the reset observation, then a real one) of M learners under the learners' squash: bids, budgets, the
    last act and the record equal three solo engines' under mlp_set_squash; the record and mlp_last keep u; turned off, and dropped
    by mlp_learners, the act is the learners' act without it"""
    from adcraft_amd import _ffi
    pols, _ = _members(300, value=True)
    lo, hi = _bounds()
    e, plain = _learners(amd, pols), _learners(amd, pols, squash=False)
    solos = [_solo_engine(amd, pols[m], m) for m in range(M)]
    for x in [e, plain] + solos:
        x.rollout_enable(2, obs=True)
    for day in range(2):
        e.mlp_step()
        plain.mlp_step()
        got = _last_act(e)
        for m, s in enumerate(solos):
            s.mlp_step()
            ref = _last_act(s)
            for k in ACT_KEYS:
                assert _same(got[k][SP.member_slice(m, n)], ref[k]), (day, m, k)
        assert not _same(got["bids"], _last_act(plain)["bids"]), "the squash changes what the envs are given"
        assert (got["budget"] >= lo[0]).all() and (got["budget"] <= hi[0]).all() and (got["bids"] <= hi[1:] + 0.005).all()
    rec = e.rollout_fetch()
    for m, s in enumerate(solos):
        srec = s.rollout_fetch()
        for k in ("action", "logp", "value", "obs", "reward", "terminated", "truncated"):
            assert _same(SP.member_record(rec, m, n)[k], srec[k]), (k, m)
    assert np.abs(rec["action"]).max() > 1.0, "the record keeps u, not the squashed action"
    assert not _same(rec["action"][:, :n], rec["action"][:, n:2 * n]), "members differ, or the test would show nothing"
    # off again: the learners' act without it, on the observation these envs now hold
    z = (np.random.default_rng(1).standard_normal((N, A)) * 2).astype(F)
    e.mlp_act(0.0, z)
    on = _last_act(e)
    e.mlp_learners_set_squash(None, None)
    e.mlp_act(0.0, z)
    off = _last_act(e)
    assert _same(on["action"], off["action"]) and not _same(on["bids"], off["bids"])
    for m in range(M):
        want = R.act(pols[m], R.flat_obs(e.fetch())[SP.member_slice(m, n)], z[SP.member_slice(m, n)])
        for k in ACT_KEYS:
            assert _same(off[k][SP.member_slice(m, n)], want[k]), ("turned off", m, k)
    # dropped by mlp_learners (any argument), and refused without learners; the single policy's entry point stays refused with them
    e.mlp_learners_set_squash(lo, hi)
    with pytest.raises(_ffi.EngineStateError, match="learners active"):
        e.mlp_set_squash(lo, hi)
    e.mlp_learners(M)
    for m in range(M):
        e.mlp_set_learner(m, pols[m])
    e.mlp_act(0.0, z)
    for k in ACT_KEYS:
        assert _same(_last_act(e)[k], off[k]), ("after mlp_learners", k)
    want = R.act(pols[0], R.flat_obs(e.fetch()), z)                     # (the centre policy, without a squash)
    e.mlp_learners_set_squash(lo, hi)
    e.mlp_learners(0)
    with pytest.raises(_ffi.EngineStateError, match="needs learners"):
        e.mlp_learners_set_squash(lo, hi)
    e.mlp_act(0.0, z)
    assert _same(_last_act(e)["bids"], want["bids"]), "the learners' squash went with the learners"
    # ... and by a population, which ends the learners (it is not the single policy's squash, which a population refuses)
    e.mlp_learners(M)
    e.mlp_learners_set_squash(lo, hi)
    e.mlp_population(M)
    with pytest.raises(_ffi.EngineStateError, match="needs learners"):
        e.mlp_learners_set_squash(lo, hi)
    e.mlp_act(0.0, z)                                                   # (every member of a fresh population is the centre)
    assert _same(_last_act(e)["bids"], want["bids"]), "the learners' squash went with the learners a population ended"
    e.mlp_population(0)
    e.mlp_set_squash(lo, hi)                                            # (the single policy's own is accepted again)
    with pytest.raises(_ffi.EngineStateError, match="squashed action"):
        e.mlp_learners(M)
    for x in [e, plain] + solos:
        x.close()


# ---- 2. the store ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [10, 40])
def test_store_fills_every_members_ring_as_the_restatement_and_a_solo_engine(amd, capacity):
    """two collections of T = 6 days through auto-resets, 24 transitions per member each: longer than a ring of 10 (the skip rule),
    and a ring of 40 wraps in the second store"""
    from adcraft_amd import _ffi
    pols, crits = _members(301)
    opts = _options(capacity)
    e = _population(amd, pols, crits, opts)
    solos = [_solo(amd, pols[m], crits[m], opts[m], m) for m in range(M)]
    rings = [SP.MemberRing(capacity, D, A, m, n) for m in range(M)]
    assert e.sac_pop_buffer(fetch=False) == dict(size=0, written=0, capacity=capacity, batch_size=B0)
    for rnd in range(2):
        e.rollout_reset()
        e.run_days("mlp", T, BUDGET)
        assert e.sac_pop_store() == T * n
        rec, now = e.rollout_fetch(), _current_input(e, pols[0])
        done = rec["terminated"] | rec["truncated"]
        assert done.any() and not done.all(), "the record was meant to cross an episode end"
        for m in range(M):
            rings[m].store(rec, now)
            got = e.sac_pop_buffer(m)
            _assert_buffer(got, rings[m].buffer(), (rnd, m))
            s = solos[m]
            s.rollout_reset()
            s.run_days("mlp", T, BUDGET)
            assert s.sac_store() == T * n
            _assert_buffer(got, s.sac_buffer(), ("solo", rnd, m))
    assert e.sac_pop_buffer(fetch=False)["written"] == 2 * T * n
    assert not _same(e.sac_pop_buffer(0)["x"], e.sac_pop_buffer(1)["x"]), "members differ, or the test would show nothing"
    assert np.abs(e.sac_pop_buffer(0)["a"]).max() > 1.0, "the ring holds u, not the squashed action"
    # the envs stepped outside the record since an unstored recorded day
    e.rollout_reset()
    e.run_days("mlp", 1, BUDGET)
    e.run_days("fixed", 1, BUDGET)
    with pytest.raises(_ffi.EngineStateError, match="outside the record"):
        e.sac_pop_store()
    e.rollout_reset()
    with pytest.raises(_ffi.EngineStateError, match="no unstored day"):
        e.sac_pop_store()
    for s in solos:
        s.close()
    e.close()


# ---- 3. batch indices ------------------------------------------------------------------------------------------------------------
def test_batch_indices_are_the_restatements_under_the_members_key(amd):
    pols, crits = _members(302)
    opts = _options(40)
    e = _population(amd, pols, crits, opts)
    rng = np.random.default_rng(3)
    for m in range(M):
        e.sac_pop_buffer_load(m, _random_buffer(rng, 33))
    for u in (0, 3):
        idx = [e.sac_pop_batch_indices(m, u) for m in range(M)]
        for m in range(M):
            assert _same(idx[m], T3.batch_indices(SP.member_seed(opts[m], SEED), u, 33, B0)), (m, u)
            assert idx[m].min() >= 0 and idx[m].max() < 33
        assert _same(idx[0], idx[2]), "two members that take the engine's seed share their indices"
        assert not _same(idx[0], idx[1]), "a member with its own seed does not"
    e.close()


# ---- 4. updates against the restatement and against solo twins -------------------------------------------------------------------
def test_five_updates_equal_the_restatement_and_three_solo_engines(amd):
    """one collection stored (24 transitions per member), then U = 5 updates one at a time with B = 7: updates 2 and 4 move the
    target critics.  One member clips its gradients, two do not; one keeps its temperature.  After every update every member's state
    (log_alpha and its moments included) and statistics equal sac_ref.update's on its ring under its key, and its solo twin's"""
    pols, crits = _members(303)
    opts = _options(40)
    e = _population(amd, pols, crits, opts)
    solos = [_solo(amd, pols[m], crits[m], opts[m], m) for m in range(M)]
    states = [SP.member_fresh_state(pols[m], crits[m], opts[m]) for m in range(M)]
    assert e.sac_pop_param_counts() == (states[0]["theta"].size, states[0]["psi"].size)
    for m in range(M):
        _assert_state(e.sac_pop_state(m), states[m], "theta starts as the member's device policy, the target critics as copies, alpha as init_alpha")
    e.run_days("mlp", T, BUDGET)
    assert e.sac_pop_store() == T * n
    bufs = [e.sac_pop_buffer(m) for m in range(M)]
    for m, s in enumerate(solos):
        s.run_days("mlp", T, BUDGET)
        assert s.sac_store() == T * n
        _assert_buffer(bufs[m], s.sac_buffer(), m)
    cell2 = states[2]["log_alpha"].copy()
    clipped = False
    for u in range(5):
        before = [e.sac_pop_state(m)["psi_target"] for m in range(M)]
        stats = e.sac_pop_update(1)
        assert len(stats) == M
        for m in range(M):
            states[m], rstats = SP.member_update(pols[m], states[m], bufs[m], opts[m], SEED)
            got = e.sac_pop_state(m)
            _assert_state(got, states[m], (u, m))
            _assert_stats(stats[m], rstats, (u, m))
            sstats = solos[m].sac_update(1)
            _assert_state(got, solos[m].sac_state(), ("solo", u, m))
            _assert_stats(stats[m], sstats, ("solo", u, m))
            assert (stats[m]["updates"], stats[m]["buffer_size"], stats[m]["samples"]) == (u + 1, T * n, B0)
            assert (not _same(before[m], got["psi_target"])) == (u % 2 == 1), "the Polyak gate"
        clipped = clipped or min(stats[1]["critic_grad_norm"], stats[1]["actor_grad_norm"]) > OWN[1]["max_grad_norm"]
        assert _same(e.sac_pop_state(2)["log_alpha"], cell2) and stats[2]["alpha"] == float(S.alpha_of(cell2[0])), "alpha_lr 0: the cell stays"
    assert clipped, "member 1's clip was meant to engage"
    assert not _same(states[0]["log_alpha"], SP.member_fresh_state(pols[0], crits[0], opts[0])["log_alpha"])
    assert not _same(states[0]["theta"], T3.flat_of(pols[0].layers)) and not _same(states[0]["psi_target"], states[0]["psi"])
    for m in range(M):
        assert _same(e.mlp_learner_params(m)[:states[m]["theta"].size], states[m]["theta"]), "the member's policy layers follow its theta"
    for s in solos:
        s.close()
    e.close()


def test_two_iterations_through_the_trainer_equal_three_solo_trainers(amd):
    """collect -> store -> three updates, twice, through SACPopulationTrainer against three SACTrainer engines of 4 envs at
    env_id_base = 4 m: states, statistics and rings - the second collection runs under the updated actors, so they reach the policy
    kernel; then copy and set_config through the trainer"""
    from adcraft_amd.baselines.sac_trainer import SACPopulationTrainer, SACTrainer
    pols, crits = _members(304)
    opts = _options(40)
    lo, hi = _bounds()
    keys = lambda o: {k: v for k, v in o.items() if k != "critic_widths"}
    common = dict(critic_hidden=WIDTHS[:-1], learning_starts=T * n, updates_per_iteration=3)
    e = _engine(amd, _planes(), **RESETS)
    tr = SACPopulationTrainer(e, pols, [dict(keys(opts[m]), critics=crits[m], **common) for m in range(M)], lo, hi, horizon=T)
    solos = []
    for m in range(M):
        s = _engine(amd, _planes()[:, SP.member_slice(m, n)], env_id_base=m * n, **RESETS)
        solos.append((s, SACTrainer(s, pols[m], lo, hi, horizon=T, critics=crits[m], **common, **keys(opts[m]))))
    for it in range(2):
        stats = tr.iteration(T, BUDGET)
        for m, (s, st) in enumerate(solos):
            sstats = st.iteration(T, BUDGET)
            _assert_state(tr.state(m), st.state(), (it, m))
            _assert_stats(stats[m], sstats, (it, m))
            _assert_buffer(e.sac_pop_buffer(m), s.sac_buffer(), (it, m))
            out = tr.policy(m)
            assert _same(T3.flat_of(out.policy.layers), st.state()["theta"]) and _same(out.action_lo, lo) and _same(out.action_hi, hi)
    assert tr.state(0)["updates"] == 6 and tr.returns().shape == (M,)
    tr.copy(0, 1)
    got, src = tr.state(1), tr.state(0)
    _assert_state(got, src, "the trainer's copy")
    tr.set_config(1, critic_lr=0.02)
    assert tr.configs[1]["critic_lr"] == 0.02 and tr.configs[1]["seed"] == 77
    with pytest.raises(ValueError):
        tr.set_config(1, batch_size=B0 + 1)
    for s, _ in solos:
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
            e.sac_pop_buffer_load(m, bufs[m])
    at_once = engines[0].sac_pop_update(5)
    singles = [engines[1].sac_pop_update(1) for _ in range(5)]
    assert engines[2].sac_pop_update(5, stats=False) is None
    for m in range(M):
        ref = engines[0].sac_pop_state(m)
        assert ref["updates"] == 5
        _assert_state(engines[1].sac_pop_state(m), ref, ("one at a time", m))
        _assert_state(engines[2].sac_pop_state(m), ref, ("without statistics", m))
        _assert_stats(at_once[m], singles[4][m], m)                              # the call's last update
    # ... and no member clipping (the chain that only enqueues) gives every member what it gets beside a member that clips
    free = _options(40, max_grad_norm=0.0)
    f = _population(amd, pols, crits, free)
    for m in range(M):
        f.sac_pop_buffer_load(m, bufs[m])
    f.sac_pop_update(5)
    for m in (0, 2):
        _assert_state(f.sac_pop_state(m), engines[0].sac_pop_state(m), ("beside a clipping member", m))
    assert not _same(f.sac_pop_state(1)["psi"], engines[0].sac_pop_state(1)["psi"]), "member 1's clip was meant to engage"
    for e in engines + [f]:
        e.close()


# ---- 6. a second chunk -----------------------------------------------------------------------------------------------------------
def test_a_batch_of_1100_is_two_chunks_per_member(amd):
    """B = 1100 > 1024: the chunked float64 sums of a member - its gradients', its pieces', the lp sum its temperature steps on - run
    over two chunks of its own batch elements.  Critics (9,), a ring of 64: two updates.  State and statistics equal the solo twin's."""
    pols, crits = _members(306, widths=(9, 1))
    opts = _options(64, critic_widths=(9, 1), batch_size=1100, target_update_interval=1)
    rng = np.random.default_rng(6)
    bufs = [_random_buffer(rng, 50) for _ in range(M)]
    e = _population(amd, pols, crits, opts)
    for m in range(M):
        e.sac_pop_buffer_load(m, bufs[m])
    stats = e.sac_pop_update(2)
    for m in range(M):
        s = _solo(amd, pols[m], crits[m], opts[m], m)
        s.sac_buffer_load(bufs[m])
        sstats = s.sac_update(2)
        got = e.sac_pop_state(m)
        assert got["updates"] == 2
        _assert_state(got, s.sac_state(), m)
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
        assert e.sac_pop_store() == s.sac_store() == T * n
        stats, sstats = e.sac_pop_update(3), s.sac_update(3)
        _assert_buffer(e.sac_pop_buffer(0), s.sac_buffer(), rnd)
        _assert_state(e.sac_pop_state(0), s.sac_state(), rnd)
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
        a.sac_pop_buffer_load(m, bufs[m])
    a.sac_pop_update(3)
    saved = [(a.sac_pop_state(m), a.sac_pop_buffer(m)) for m in range(M)]
    a.sac_pop_update(2)
    final = [a.sac_pop_state(m) for m in range(M)]
    # a fresh engine (other critics at first) resumed from the saved states and rings continues to the same bits
    b = _population(amd, pols, _members(999)[1], opts)
    for m in range(M):
        b.sac_pop_state(m, saved[m][0])
        b.sac_pop_buffer_load(m, saved[m][1])
    for m in range(M):
        _assert_state(b.sac_pop_state(m), saved[m][0], m)
        _assert_buffer(b.sac_pop_buffer(m), dict(saved[m][1]), m)
        assert _same(b.mlp_learner_params(m)[:saved[m][0]["theta"].size], saved[m][0]["theta"]), "the member's policy layers follow its theta"
    b.sac_pop_update(2)
    for m in range(M):
        _assert_state(b.sac_pop_state(m), final[m], ("resumed", m))
    # copy 0 -> 2 with the ring: member 2 goes on as member 0 would under member 2's configuration (its alpha_lr 0 among it)
    assert not _same(final[0]["log_alpha"], final[2]["log_alpha"])
    a.sac_pop_copy(0, 2, with_ring=True)
    _assert_state(a.sac_pop_state(2), final[0], "the copy, the temperature cell included")
    _assert_buffer(a.sac_pop_buffer(2), a.sac_pop_buffer(0), "the copied ring")
    _assert_state(a.sac_pop_state(1), final[1], "the copy touched member 1")
    assert _same(a.mlp_learner_params(2)[:final[0]["theta"].size], final[0]["theta"])
    twin = _solo(amd, pols[2], crits[2], opts[2], 2)
    twin.sac_state(final[0])
    twin.sac_buffer_load(a.sac_pop_buffer(0))
    st_a, st_t = a.sac_pop_update(2), twin.sac_update(2)
    _assert_state(a.sac_pop_state(2), twin.sac_state(), "member 2 after the copy against a solo twin built from the copied state")
    _assert_stats(st_a[2], st_t, "member 2 after the copy")
    assert not _same(a.sac_pop_state(2)["psi"], a.sac_pop_state(0)["psi"]), "member 2 kept its own configuration"
    assert _same(a.sac_pop_state(2)["log_alpha"], final[0]["log_alpha"]), "... its alpha_lr 0: the copied cell stays"
    twin.close()
    # without the ring, dst keeps its own
    ring1 = a.sac_pop_buffer(1)
    a.sac_pop_copy(0, 1)
    _assert_state(a.sac_pop_state(1), a.sac_pop_state(0), "the copy without the ring")
    _assert_buffer(a.sac_pop_buffer(1), ring1, "the ring stayed")
    # learning rates, the target entropy and the discount changed for one member from the next update on; init_alpha is not read
    # again; a shared field may not change
    before = [b.sac_pop_state(m) for m in range(M)]
    changed = dict(opts[1], critic_lr=0.02, alpha_lr=0.01, target_entropy=-2.5, gamma=0.7, init_alpha=9.0)
    b.sac_pop_set_config(1, **changed)
    for field, value in (("batch_size", B0 + 1), ("capacity", 41), ("target_update_interval", 3), ("critic_widths", (11, 1))):
        with pytest.raises(ValueError):
            b.sac_pop_set_config(1, **dict(changed, **{field: value}))
    with pytest.raises(ValueError):
        b.sac_pop_set_config(3, **changed)
    _assert_state(b.sac_pop_state(1), before[1], "set_config moved no state")
    b.sac_pop_update(1)
    for m in range(M):
        ref, _ = SP.member_update(pols[m], before[m], saved[m][1], changed if m == 1 else opts[m], SEED)
        _assert_state(b.sac_pop_state(m), ref, ("set_config", m))
    old, _ = SP.member_update(pols[1], before[1], saved[1][1], opts[1], SEED)
    assert not _same(old["psi"], b.sac_pop_state(1)["psi"]) and not _same(old["log_alpha"], b.sac_pop_state(1)["log_alpha"])
    a.close()
    b.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_working(amd):
    from adcraft_amd import _ffi
    pols, crits = _members(309)
    opts = _options(40)
    lo, hi = _bounds()
    rng = np.random.default_rng(9)
    e = _engine(amd, _planes(), **RESETS)
    with pytest.raises(_ffi.EngineStateError, match="mlp_init"):
        e.mlp_learners_set_squash(lo, hi)
    e.mlp_init(pols[0], deterministic=False)
    e.rollout_enable(T, obs=True)
    # the learners' squash without learners; SAC population without learners
    with pytest.raises(_ffi.EngineStateError, match="needs learners"):
        e.mlp_learners_set_squash(lo, hi)
    with pytest.raises(_ffi.EngineStateError, match="learners"):
        e.sac_pop_init(opts[0])
    cfg = amd.StepEngine.sac_config(**opts[0])
    assert e._lib.adc_engine_sac_pop_init(e._h, C.byref(cfg), 1) == _ffi.ADC_ESTATE
    with pytest.raises(_ffi.EngineStateError, match="sac_pop_init"):
        e.sac_pop_update(1)
    # bad bounds
    e.mlp_learners(M)
    for bad_lo, bad_hi in ((lo, lo), (lo, np.where(np.arange(A) == 1, np.inf, hi)), (np.full(A, np.nan, F), hi)):
        with pytest.raises(ValueError, match="squash bounds"):
            e.mlp_learners_set_squash(bad_lo, bad_hi)
    # the free head; the clamp off; the learners' squash not set; no record; no recorded input
    e.mlp_init(R.random_policy(rng, K, HIDDEN), deterministic=False)
    e.mlp_learners(M)
    e.mlp_learners_set_squash(lo, hi)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="two-headed"):
        e.sac_pop_init(opts)
    e.mlp_init(R.random_policy(rng, K, HIDDEN, two_heads=True), deterministic=False)
    e.mlp_learners(M)
    e.mlp_learners_set_squash(lo, hi)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="clamp_log_std"):
        e.sac_pop_init(opts)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="mlp_learners_set_squash"):
        e.sac_pop_init(opts)
    e.mlp_learners_set_squash(lo, hi)
    e.mlp_init(pols[0], deterministic=False)                            # (the record, the learners and their squash went with it)
    e.mlp_learners(M)
    e.mlp_learners_set_squash(lo, hi)
    with pytest.raises(_ffi.EngineStateError, match="rollout record"):
        e.sac_pop_init(opts)
    e.rollout_enable(T)
    with pytest.raises(_ffi.EngineStateError, match="ADC_ROLLOUT_OBS"):
        e.sac_pop_init(opts)
    e.rollout_enable(T, obs=True)
    # a policy-gradient population alive
    e.pg_pop_init(dict())
    with pytest.raises(_ffi.EngineStateError, match="policy-gradient"):
        e.sac_pop_init(opts)
    e.rollout_enable(T, obs=True)                                       # (ends the policy-gradient trainer)
    # the solo trainer keeps refusing an engine with learners
    with pytest.raises(_ffi.EngineStateError, match="learners active"):
        e.sac_init(**opts[0])
    # configurations that do not fit the members
    with pytest.raises(ValueError, match="count"):
        e.sac_pop_init(opts[:2])
    with pytest.raises(ValueError, match="equal"):
        e.sac_pop_init([opts[0], dict(opts[1], capacity=41), opts[2]])
    with pytest.raises(ValueError, match="tau"):
        e.sac_pop_init([opts[0], dict(opts[1], tau=0.0), opts[2]])
    e.sac_pop_init(opts)
    # the other trainers, the normalisers and the scheduler over a SAC population
    with pytest.raises(_ffi.EngineStateError, match="soft actor-critic"):
        e.pg_pop_init(dict())
    with pytest.raises(_ffi.EngineStateError):
        e.td3_pop_init(dict(critic_widths=WIDTHS, batch_size=B0, capacity=40))
    with pytest.raises(_ffi.EngineStateError, match="soft actor-critic"):
        e.obs_norm_init()
    with pytest.raises(_ffi.EngineStateError):
        e.rew_norm_init()
    with pytest.raises(_ffi.EngineStateError):
        e.td3_norm_init(observations=True)
    for kind in ("td3", "pg"):
        with pytest.raises(_ffi.EngineStateError):
            e.pbt_init(kind, replace_count=1)
    for call in (lambda: e.sac_update(1), lambda: e.td3_pop_update(1)):
        with pytest.raises(_ffi.EngineStateError, match="has not been called"):
            call()                                                      # (the solo and the TD3 calls do not see the population)
    # an update before every member's critics are uploaded; on an empty ring
    for m in range(M - 1):
        e.sac_pop_set_critics(m, crits[m])
    with pytest.raises(_ffi.EngineStateError, match="critic layer"):
        e.sac_pop_update(1)
    e.sac_pop_set_critics(M - 1, crits[M - 1])
    for call in (lambda: e.sac_pop_update(1), lambda: e.sac_pop_batch_indices(0, 0)):
        with pytest.raises(_ffi.EngineStateError, match="empty"):
            call()
    with pytest.raises(_ffi.EngineStateError, match="no unstored day"):
        e.sac_pop_store()
    # members and counts out of range
    for call in (lambda: e.sac_pop_state(M), lambda: e.sac_pop_buffer_load(-1, _random_buffer(rng, 4)), lambda: e.sac_pop_copy(0, M),
                 lambda: e.sac_pop_sync_targets(M), lambda: e.sac_pop_set_critics(M, crits[0]), lambda: e.sac_pop_update(0)):
        with pytest.raises(ValueError):
            call()
    # the learners' squash turned off under the trainer
    e.mlp_learners_set_squash(None, None)
    with pytest.raises(_ffi.EngineStateError, match="mlp_learners_set_squash"):
        e.sac_pop_update(1)
    e.mlp_learners_set_squash(lo, hi)
    # the engine is usable: collect, store, update
    e.run_days("mlp", 2, BUDGET)
    assert e.sac_pop_store() == 2 * n
    st = e.sac_pop_update(2)
    assert st[0]["updates"] == 2 and all(np.isfinite(s["critic_loss"]) and np.isfinite(s["actor_loss"]) and s["alpha"] > 0 for s in st)
    # the trainer goes with the learners it trains, and with the record
    e.mlp_learners(M)
    with pytest.raises(_ffi.EngineStateError, match="sac_pop_init"):
        e.sac_pop_update(1)
    e.mlp_learners_set_squash(lo, hi)
    e.sac_pop_init(opts)
    e.rollout_enable(T, obs=True)
    with pytest.raises(_ffi.EngineStateError, match="sac_pop_init"):
        e.sac_pop_state(0)
    e.close()


def test_lds_overflow_is_refused(amd):
    """K = 720 with the widest networks: the batch kernels' row, activations, deltas and head vectors do not fit 64 KB"""
    Kb = 720
    rng = np.random.default_rng(5)
    pol = S.sac_policy(rng, Kb, (256, 256, 256), "tanh", clamp=(-5.0, 2.0))
    e = amd.StepEngine(1, Kb, seed=7, max_days=1 << 20, loss_threshold=1e12)
    e.set_all_params(H.implicit_params(1, Kb, 8, mean_volume=8, cvr=0.5))
    e.reset()
    e.mlp_init(pol, deterministic=False)
    e.mlp_learners(1)
    e.mlp_learners_set_squash(np.full(Kb + 1, 0.02, F), np.full(Kb + 1, 3.0, F))
    e.rollout_enable(2, obs=True)
    Db, Ab, maxw = 5 * Kb + 2, Kb + 1, 2 * (Kb + 1)
    floats = (Db + Ab) + (3 * 256 + 2 * Ab) + 2 * (3 * 256 + 1) + 3 * maxw + 6 * Ab + 8
    assert floats * 4 > 64 * 1024
    with pytest.raises(ValueError, match="LDS"):
        e.sac_pop_init(dict(critic_widths=(256, 256, 256, 1), batch_size=8, capacity=16))
    e.mlp_act(10.0)                                                    # the engine stays usable
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
    assert a.sac_pop_store() == 6
    a.sac_pop_update(1)
    states, rings = [a.sac_pop_state(m) for m in range(members)], [a.sac_pop_buffer(m) for m in range(members)]
    assert all((g["size"], g["written"], g["capacity"], g["batch_size"]) == (5, 6, 5, 4) for g in rings)
    assert not _same(rings[0]["x"], rings[1]["x"])
    b = fresh()
    part = lambda g, lo, hi: {k: g[k][lo:hi] for k in ("x", "a", "r", "done", "x2")}
    for m in range(members):
        b.sac_pop_buffer_load(m, part(rings[m], 0, 2))
        b.sac_pop_buffer_load(m, part(rings[m], 2, 5), slot=2, written=6)
        b.sac_pop_state(m, states[m])
    assert b.sac_pop_param_counts() == a.sac_pop_param_counts()
    for m in range(members):
        _assert_buffer(b.sac_pop_buffer(m), rings[m], m)
        _assert_state(b.sac_pop_state(m), states[m], m)
        assert _same(a.sac_pop_batch_indices(m, 1), b.sac_pop_batch_indices(m, 1)) and a.sac_pop_batch_indices(m, 1).shape == (4,)
    for sa, sb in zip(a.sac_pop_update(2), b.sac_pop_update(2)):
        _assert_stats(sb, sa)
    for m in range(members):
        _assert_state(b.sac_pop_state(m), a.sac_pop_state(m), m)
    assert b.sac_pop_state(0)["updates"] == 3
    a.close()
    lib, h, p = b._lib, b._h, lambda v: v.ctypes.data
    x, ac, r, dn = np.zeros((4, D), F), np.zeros((4, A), F), np.zeros(4, F), np.zeros(4, np.uint8)
    (w, bias), idx = crits[0][0][0], np.zeros(4, np.int32)
    last = [b.sac_pop_state(m) for m in range(members)]
    vec = [p(last[1][k]) for k in amd.StepEngine.SAC_STATE]
    refused = (
        (r"no such member", lambda: lib.adc_engine_sac_pop_buffer_fetch(h, 2, 0, 1, p(x), p(ac), p(r), p(dn), p(x))),
        (r"no such member", lambda: lib.adc_engine_sac_pop_batch_indices(h, -1, 0, p(idx))),
        (r"no such member", lambda: lib.adc_engine_sac_pop_copy(h, 0, 2, 1)),
        (r"slot range is not inside \[0, size\)", lambda: lib.adc_engine_sac_pop_buffer_fetch(h, 1, 4, 2, p(x), p(ac), p(r), p(dn), p(x))),
        (r"x, a, r, done or x2 is NULL", lambda: lib.adc_engine_sac_pop_buffer_load(h, 1, 0, 4, p(x), None, p(r), p(dn), p(x), 4)),
        (r"slot range is not inside \[0, capacity\)", lambda: lib.adc_engine_sac_pop_buffer_load(h, 1, 3, 4, p(x), p(ac), p(r), p(dn), p(x), 12)),
        (r"written: at least slot \+ count", lambda: lib.adc_engine_sac_pop_buffer_load(h, 1, 0, 4, p(x), p(ac), p(r), p(dn), p(x), 3)),
        (r"critic: 0 or 1", lambda: lib.adc_engine_sac_pop_set_critic_layer(h, 1, 2, 0, p(w), p(bias))),
        (r"no such critic layer", lambda: lib.adc_engine_sac_pop_set_critic_layer(h, 1, 0, 2, p(w), p(bias))),
        (r"weights or bias is NULL", lambda: lib.adc_engine_sac_pop_set_critic_layer(h, 1, 0, 0, p(w), None)),
        (r"idx_b is NULL", lambda: lib.adc_engine_sac_pop_batch_indices(h, 1, 0, None)),
        (r"update: 0 to 2\^32 - 2", lambda: lib.adc_engine_sac_pop_batch_indices(h, 1, -1, p(idx))),
        (r"updates: 1 to 65536", lambda: lib.adc_engine_sac_pop_update(h, 0, None)),
        (r"a state vector is NULL", lambda: lib.adc_engine_sac_pop_state_set(h, 1, *vec[:-1], None, 0)),
        (r"updates: 0 to 2\^31 - 2", lambda: lib.adc_engine_sac_pop_state_set(h, 1, *vec, 2 ** 31 - 1)),
    )
    for words, call in refused:
        with pytest.raises(ValueError, match=words):
            _ffi.check(call())
    # (SAC's update counter ends at 2^31 - 1: the state's largest count leaves no update)
    b.sac_pop_state(1, dict(last[1], updates=2 ** 31 - 2))
    with pytest.raises(_ffi.EngineStateError, match="the update counter is exhausted"):
        b.sac_pop_update(1)
    b.sac_pop_state(1, last[1])
    for m in range(members):
        _assert_buffer(b.sac_pop_buffer(m), rings[m], m)
        _assert_state(b.sac_pop_state(m), last[m], m)
    assert b.sac_pop_update(1)[0]["updates"] == 4
    # one member's targets become copies; the other's stay
    b.sac_pop_sync_targets(1)
    synced, other = b.sac_pop_state(1), b.sac_pop_state(0)
    assert _same(synced["psi_target"], synced["psi"]) and not _same(other["psi_target"], other["psi"])
    b.replay_prio_init()
    with pytest.raises(_ffi.EngineStateError, match="prioritised replay is alive"):
        b.sac_pop_batch_indices(0, 0)
    b.close()
