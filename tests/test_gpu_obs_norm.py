"""GPU tests of the running observation normaliser (adc_engine_obs_norm_*; the law is csrc/adc_norm.h): after an update the
device's count, mean, M2, shift and scale equal, bit for bit, the host twin adc_obs_norm_host run on the fetched record - per
member for a learner population, where a member's result also equals a single engine's of its envs - the next act reads the
new vectors, a resumed run continues bit for bit, a copied member carries its donor's normaliser, every refusal leaves the
engine usable, and nothing exists unless it is asked for.  None of these symbols exists before this feature: every test here
fails on the parent commit.

The shapes are the smallest that cross a chunk of 1024 samples, a tile of 256 columns and a member boundary:
64 envs x 5 keywords (D = 27) x 20 days (S = 1280: a full chunk and one of 256); 8 envs x 60 keywords (D = 302) x 130 days
(S = 1040: columns past one tile, a tail chunk of 16); 48 envs x 25 keywords (D = 127) x 23 days x 4 learners (n = 12,
S = 276 per member, whose rows are not contiguous).  Members, chunks and column tiles at once - 3 learners x 7 envs x 52 keywords
x 150 days, where a member's second chunk starts inside a day - live in tests/test_gpu_replay_shapes.py, for this normaliser, the
reward normaliser beside it and the TD3 / SAC learners' own."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import norm_ref as NR

pytestmark = pytest.mark.gpu
F = np.float32


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


SEED, BUDGET = 43, 1000.0
RESETS = dict(max_days=7, auto_reset=True)          # (first-day rows (0 - shift) * scale are among the samples)


def _planes(N, K, seed=SEED):
    return H.implicit_params(N, K, seed + 1, mean_volume=24, cvr=0.5)


def _engine(amd, planes, seed=SEED, env_id_base=0, **kw):
    _, N, K = planes.shape
    e = amd.StepEngine(N, K, seed=seed, env_id_base=env_id_base, **dict(RESETS, **kw))
    e.set_all_params(planes)
    e.reset()
    return e


def _policy(rng, K, hidden=(12,), vary=0.0, **kw):
    pol = R.random_policy(rng, K, hidden, "tanh", value=True, normalize=True, scale=0.6, **kw)
    shift, scale = R.realistic_norm(K)
    if vary:
        shift = (shift + rng.standard_normal(shift.size).astype(F) * F(vary)).astype(F)
        scale = (scale * np.exp(rng.standard_normal(scale.size) * vary).astype(F)).astype(F)
    pol.shift, pol.scale = shift, scale
    return pol


def _with_vectors(pol, st):
    import copy
    out = copy.copy(pol)
    out.shift, out.scale = st["shift"], st["scale"]
    return out


def _assert_next_act(e, lib, policies_of_env):
    """the next act's means equal adc_mlp_act_host under the given policies' (updated) vectors, env by env"""
    out = e.fetch()
    obs = R.flat_obs(out)
    obs[np.asarray(out["terminated"], bool) | np.asarray(out["truncated"], bool)] = 0.0       # (auto-reset: the reset observation)
    e.mlp_set_deterministic(True)
    e.mlp_act(BUDGET)
    last = e.mlp_last()
    e.mlp_set_deterministic(False)
    for env, pol in enumerate(policies_of_env):
        ref = R.twin_act(lib, pol, obs[env], deterministic=True)
        assert _same(last["mean"][env], ref["mean"][0]), env
        assert _same(last["value"][env], ref["value"][0]), env


# ---- 1. the device against the host twin, the shared normaliser ------------------------------------------------------------------
@pytest.mark.parametrize("N,K,T", [(64, 5, 20), (8, 60, 130)])
def test_update_equals_the_host_twin_and_the_next_act_uses_the_new_vectors(amd, lib, N, K, T):
    D = 5 * K + 2
    rng = np.random.default_rng(N + K)
    pol = _policy(rng, K)
    e = _engine(amd, _planes(N, K))
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.obs_norm_init()
    st0 = e.obs_norm_state()
    assert st0["count"] == 0 and _same(st0["shift"], pol.shift) and _same(st0["scale"], pol.scale)
    e.run_days("mlp", T, BUDGET)
    e.obs_norm_update()
    got = e.obs_norm_state()
    rec = e.rollout_fetch()
    x = rec["obs"].reshape(T * N, D)
    done = rec["terminated"] | rec["truncated"]
    assert done.any() and not done.all(), "the record was meant to cross auto-resets"
    ref = NR.twin(lib, NR.fresh(D, pol.shift, pol.scale), x)
    assert NR.same(got, ref)
    if D < 64:
        assert NR.same(got, NR.update(NR.fresh(D, pol.shift, pol.scale), x)), "the numpy restatement"
    assert got["count"] == T * N and not _same(got["scale"], pol.scale)
    # the raw moments are those of the raw observations (float64 numpy on the de-normalised rows, loosely: the rows are rounded)
    raw = x.astype(np.float64) / pol.scale + pol.shift
    assert np.allclose(got["mean"], raw.mean(axis=0), rtol=1e-5, atol=1e-5 * (1 + np.abs(raw).max()))
    _assert_next_act(e, lib, [_with_vectors(pol, got)] * N)
    e.close()


# ---- 2. per-member normalisers ---------------------------------------------------------------------------------------------------
def test_members_equal_the_host_twin_and_solo_engines(amd, lib):
    N, K, T, M = 48, 25, 23, 4
    n, D = N // M, 5 * K + 2
    rng = np.random.default_rng(202)
    pols = [_policy(rng, K, vary=0.2 * (m > 0)) for m in range(M)]
    planes = _planes(N, K)
    e = _engine(amd, planes)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    for m in range(M):
        e.mlp_set_learner(m, pols[m])
    e.rollout_enable(T, obs=True)
    e.obs_norm_init(per_member=True)
    for m in range(M):
        st = e.obs_norm_state(m)
        assert st["count"] == 0 and _same(st["shift"], pols[0].shift), "every member starts from the shared vectors"
        st["shift"], st["scale"] = pols[m].shift, pols[m].scale
        e.obs_norm_state(m, st)
    e.run_days("mlp", T, BUDGET)
    e.obs_norm_update()
    rec = e.rollout_fetch()
    states = [e.obs_norm_state(m) for m in range(M)]
    for m in range(M):
        x = NR.member_rows(rec["obs"], m, n)
        assert x.shape == (T * n, D)
        assert NR.same(states[m], NR.twin(lib, NR.fresh(D, pols[m].shift, pols[m].scale), x)), m
        # a single engine of the member's envs
        s = _engine(amd, planes[:, m * n:(m + 1) * n], env_id_base=m * n)
        s.mlp_init(pols[m], deterministic=False)
        s.rollout_enable(T, obs=True)
        s.obs_norm_init()
        s.run_days("mlp", T, BUDGET)
        s.obs_norm_update()
        assert _same(s.rollout_fetch()["obs"], rec["obs"][:, m * n:(m + 1) * n]), m
        assert NR.same(s.obs_norm_state(), states[m]), m
        s.close()
    assert not NR.same(states[0], states[1])
    _assert_next_act(e, lib, [_with_vectors(pols[env // n], states[env // n]) for env in range(N)])
    # mlp_set_norm writes every member's vectors and leaves the moments alone
    e._lib.adc_engine_mlp_set_norm(e._h, pols[0].shift.ctypes.data, pols[0].scale.ctypes.data)
    for m in range(M):
        st = e.obs_norm_state(m)
        assert _same(st["shift"], pols[0].shift) and _same(st["scale"], pols[0].scale)
        assert st["count"] == states[m]["count"] and _same(st["mean"], states[m]["mean"]) and _same(st["M2"], states[m]["M2"])
    e.close()


# ---- 3. two updates without a reset ---------------------------------------------------------------------------------------------
def test_two_updates_consume_the_days_once_each(amd, lib):
    from adcraft_amd import _ffi
    N, K, T = 64, 5, 21
    D = 5 * K + 2
    rng = np.random.default_rng(303)
    pol = _policy(rng, K)
    e = _engine(amd, _planes(N, K))
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.obs_norm_init(count_cap=1000)
    ref = NR.fresh(D, pol.shift, pol.scale)
    for t0 in (0, 10):
        e.run_days("mlp", 10, BUDGET)
        e.obs_norm_update()
        obs = e.rollout_fetch()["obs"]
        assert obs.shape[0] == t0 + 10
        ref = NR.twin(lib, ref, obs[t0:].reshape(-1, D), count_cap=1000)       # (the days [t0, t0 + 10), collected under ref's vectors)
        assert NR.same(e.obs_norm_state(), ref), t0
    assert ref["count"] == 1000
    with pytest.raises(_ffi.EngineStateError, match="no day has been recorded"):
        e.obs_norm_update()
    assert NR.same(e.obs_norm_state(), ref)
    e.run_days("mlp", 1, BUDGET)                                            # (the engine still steps, and the day is a batch)
    e.obs_norm_update()
    ref = NR.twin(lib, ref, e.rollout_fetch()["obs"][20:].reshape(-1, D), count_cap=1000)
    assert NR.same(e.obs_norm_state(), ref)
    e.rollout_reset()
    with pytest.raises(_ffi.EngineStateError, match="no day has been recorded"):
        e.obs_norm_update()
    e.close()


# ---- 4. the trainers: resume, export, off by default -----------------------------------------------------------------------------
def test_a_resumed_trainer_continues_bit_for_bit(amd):
    from adcraft_amd.baselines.pg_trainer import PGTrainer
    N, K, T = 16, 5, 6
    rng = np.random.default_rng(404)
    pol = _policy(rng, K)
    pol.shift, pol.scale = np.zeros_like(pol.shift), np.ones_like(pol.scale)       # (identity vectors, as the example starts)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    cfg = dict(epochs=2, minibatches=2, lr=3e-3)
    planes = _planes(N, K)

    def trainer():
        return PGTrainer(_engine(amd, planes), pol, T, agent_seeds=seeds, normalize_observations=True, obs_norm=dict(min_std=0.05), **cfg)
    tr = trainer()
    assert tr.normalize_observations
    full = []
    for _ in range(3):
        tr.iteration(budget=BUDGET)
        full.append((tr.state(), tr.obs_norm_state()))
    exported = tr.policy()
    assert _same(exported.shift, full[2][1]["shift"]) and _same(exported.scale, full[2][1]["scale"]) and not _same(exported.scale, pol.scale)
    assert full[0][1]["count"] == T * N and full[2][1]["count"] == 3 * T * N
    tr.engine.close()
    # iteration 1's state alone, carried into a fresh engine stepped to the same env position
    tr = trainer()
    tr.engine.run_days("mlp", T, BUDGET)
    fresh = tr.obs_norm_state()
    assert fresh["count"] == 0
    tr.state(full[0][0])
    tr.obs_norm_state(full[0][1])
    assert NR.same(tr.obs_norm_state(), full[0][1])
    for it in (1, 2):
        tr.iteration(budget=BUDGET)
        for k in ("theta", "m", "v"):
            assert _same(tr.state()[k], full[it][0][k]), (k, it)
        assert NR.same(tr.obs_norm_state(), full[it][1]), it
    tr.engine.close()


def test_off_by_default(amd):
    from adcraft_amd import _ffi
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer, PGTrainer
    N, K, T = 8, 5, 3
    rng = np.random.default_rng(505)
    pol = _policy(rng, K)
    tr = PGTrainer(_engine(amd, _planes(N, K)), pol, T, epochs=1, minibatches=1)
    assert tr.normalize_observations is False
    tr.iteration(budget=BUDGET)
    for call in (lambda: tr.engine.obs_norm_state(), lambda: tr.engine.obs_norm_update(), lambda: tr.engine.obs_norm_copy([-1])):
        with pytest.raises(_ffi.EngineStateError, match="obs_norm_init"):
            call()
    assert _same(tr.policy().shift, pol.shift) and _same(tr.policy().scale, pol.scale)
    tr.engine.close()
    other = _policy(rng, K, vary=0.1)
    e = _engine(amd, _planes(N, K))
    with pytest.raises(ValueError, match="normalisation vectors are shared"):
        PGPopulationTrainer(e, [pol, other], T, dict(epochs=1, minibatches=1))
    e.close()


# ---- 5. copy ---------------------------------------------------------------------------------------------------------------------
def test_copy_and_the_scheduler_carry_the_donors_normaliser(amd):
    from adcraft_amd.baselines.pbt import PBTScheduler
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer
    N, K, T, M = 24, 5, 4, 4
    rng = np.random.default_rng(606)
    pols = [_policy(rng, K, vary=0.2 * (m > 0)) for m in range(M)]
    e = _engine(amd, _planes(N, K))
    tr = PGPopulationTrainer(e, pols, T, [dict(epochs=1, minibatches=1, lr=float(F(lr))) for lr in np.logspace(-4, -2, M)], normalize_observations=True)
    for m in range(M):
        st = tr.obs_norm_state(m)
        assert st["count"] == 0 and _same(st["shift"], pols[m].shift) and _same(st["scale"], pols[m].scale), "each member starts from its own policy's vectors"
    tr.iteration(budget=BUDGET)
    before = [tr.obs_norm_state(m) for m in range(M)]
    assert all(b["count"] == T * N // M for b in before) and not NR.same(before[0], before[2])
    assert _same(tr.policy(1).scale, before[1]["scale"])
    with pytest.raises(ValueError, match="also a source"):
        e.obs_norm_copy([1, 2, -1, -1])
    with pytest.raises(ValueError, match="src_of_m"):
        e.obs_norm_copy([4, -1, -1, -1])
    e.obs_norm_copy([-1, 0, 2, 0])
    after = [tr.obs_norm_state(m) for m in range(M)]
    for m, src in enumerate((0, 0, 2, 0)):
        assert NR.same(after[m], before[src]), m
    # a scheduler's round: every replaced member has its donor's normaliser, the kept ones their own
    sch = PBTScheduler(tr, replace_fraction=0.25, tuned=("lr",), bounds={"lr": (1e-4, 1e-2)}, seed=9)
    tr.iteration(budget=BUDGET)
    before = [tr.obs_norm_state(m) for m in range(M)]
    res = sch.step()
    assert (res["src"] >= 0).sum() == 1
    for m in range(M):
        src = int(res["src"][m])
        assert NR.same(tr.obs_norm_state(m), before[m if src < 0 else src]), m
    tr.iteration(budget=BUDGET)
    e.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(amd):
    from adcraft_amd import _ffi
    N, K, T = 8, 5, 3
    D = 5 * K + 2
    rng = np.random.default_rng(707)
    pol = R.random_policy(rng, K, (8,), normalize=True)                 # (no value network: TD3 takes it too)
    pol.shift, pol.scale = R.realistic_norm(K)
    e = _engine(amd, _planes(N, K))
    # init: before mlp_init; a policy without normalisation; a scale that cannot be divided by; per_member without learners
    with pytest.raises(_ffi.EngineStateError, match="mlp_init"):
        e.obs_norm_init()
    e.mlp_init(R.random_policy(rng, K, (8,)), deterministic=False)
    with pytest.raises(ValueError, match="without normalisation"):
        e.obs_norm_init()
    for bad in (0.0, -1.0, np.inf, np.nan):
        broken = _with_vectors(pol, dict(shift=pol.shift, scale=pol.scale.copy()))
        broken.scale[3] = bad
        e.mlp_init(broken, deterministic=False)
        with pytest.raises(ValueError, match="not finite or not > 0"):
            e.obs_norm_init()
    e.mlp_init(pol, deterministic=False)
    with pytest.raises(_ffi.EngineStateError, match="learners"):
        e.obs_norm_init(per_member=True)
    with pytest.raises(ValueError, match="min_std"):
        e.obs_norm_init(min_std=-1.0)
    cfg = amd.StepEngine.obs_norm_config()
    cfg.count_cap = -1
    import ctypes as C
    assert e._lib.adc_engine_obs_norm_init(e._h, C.byref(cfg)) == _ffi.ADC_EINVAL
    # update: no record; a record without the network input; no recorded day
    e.obs_norm_init()
    with pytest.raises(_ffi.EngineStateError, match="rollout record"):
        e.obs_norm_update()
    e.rollout_enable(T)
    with pytest.raises(_ffi.EngineStateError, match="obs_norm_init"):
        e.obs_norm_update()                                             # (the normaliser does not survive rollout_enable)
    e.obs_norm_init()
    with pytest.raises(_ffi.EngineStateError, match="ADC_ROLLOUT_OBS"):
        e.obs_norm_update()
    e.rollout_enable(T, obs=True)
    e.obs_norm_init()
    with pytest.raises(_ffi.EngineStateError, match="no day has been recorded"):
        e.obs_norm_update()
    # state and copy: members of a shared normaliser
    for member in (-1, 1):
        with pytest.raises(ValueError, match="no such normaliser"):
            e.obs_norm_state(member)
    with pytest.raises(_ffi.EngineStateError, match="shared"):
        e.obs_norm_copy([-1])
    st = e.obs_norm_state()
    st["scale"] = st["scale"].copy()
    st["scale"][0] = 0.0
    with pytest.raises(ValueError, match="scale"):
        e.obs_norm_state(0, st)
    # TD3, single and population, either way round
    base = dict(critic_widths=(8, 1), batch_size=8, capacity=40)
    with pytest.raises(_ffi.EngineStateError, match="observation normaliser"):
        e.td3_init(**base)
    e.rollout_enable(T, obs=True)                                       # (ends the normaliser)
    e.td3_init(**base)
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.obs_norm_init()
    e.mlp_init(pol, deterministic=False)
    e.mlp_learners(2)
    e.rollout_enable(T, obs=True)
    e.td3_pop_init(base)
    with pytest.raises(_ffi.EngineStateError, match="TD3"):
        e.obs_norm_init(per_member=True)
    e.rollout_enable(T, obs=True)                                       # (ends the TD3 population)
    e.obs_norm_init(per_member=True)
    with pytest.raises(_ffi.EngineStateError, match="observation normaliser"):
        e.td3_pop_init(base)
    with pytest.raises(ValueError, match="no such normaliser"):
        e.obs_norm_state(2)
    # lifetime: mlp_learners and mlp_init end it
    e.mlp_learners(0)
    with pytest.raises(_ffi.EngineStateError, match="obs_norm_init"):
        e.obs_norm_state()
    e.obs_norm_init()
    e.mlp_init(pol, deterministic=False)
    with pytest.raises(_ffi.EngineStateError, match="obs_norm_init"):
        e.obs_norm_state()
    # the engine still works: a recorded day, an update, a state
    e.rollout_enable(T, obs=True)
    e.obs_norm_init()
    e.run_days("mlp", 2, BUDGET)
    e.obs_norm_update()
    st = e.obs_norm_state()
    assert st["count"] == 2 * N and np.isfinite(st["mean"]).all() and st["mean"].shape == (D,)
    e.close()
