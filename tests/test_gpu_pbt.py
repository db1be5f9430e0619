"""GPU tests of the population-based training scheduler (adc_engine_pbt_*; parts/kernel_pbt.inc, parts/pbt_api.inc) over a PPO
population and over a TD3 population: the device's fitness against the numpy restatement tests/pbt_ref.py, the batched exploit
against the pair-by-pair primitives (adc_engine_pg_pop_copy, adc_engine_td3_pop_copy), a whole round against a twin engine
driven by hand with the primitives, resumption, refusals.  Byte equality everywhere.  N = 12, K = 5, M = 6 (n = 2), T = 6 across
an auto-reset, hidden (20, 9): nothing is a multiple of 4 or of a block.  None of these symbols exists before this feature:
every test here fails on the parent commit."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import pbt_ref as B
from tests import pg_ref as P
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
N, K, M, T = 12, 5, 6, 6
D, A = 5 * K + 2, K + 1
HIDDEN = (20, 9)


def _engine(amd, envs=N):
    planes = H.implicit_params(envs, K, SEED + 1, mean_volume=24, cvr=0.5)
    e = amd.StepEngine(envs, K, seed=SEED, **RESETS)
    e.set_all_params(planes)
    e.reset()
    return e


# ---- the PPO population ------------------------------------------------------------------------------------------------------------
def _pg_options(members=M, envs=N):
    lrs = np.logspace(-4, -2, members)
    return [P.options(lr=float(F(lrs[m])), ent_coef=float(F(0.001 * (m + 1))), eps_clip=float(F(0.1 + 0.03 * m)), vf_coef=float(F(0.3 + 0.1 * m)),
                      minibatch_envs=envs // members) for m in range(members)]


def _pg_population(amd, members=M, envs=N, seed=501):
    rng = np.random.default_rng(seed)
    pols = []
    for _ in range(members):
        pol = R.random_policy(rng, K, HIDDEN, "tanh", value=True, normalize=True, scale=0.6)
        pol.shift, pol.scale = R.realistic_norm(K)
        pols.append(pol)
    e = _engine(amd, envs)
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(members)
    for m in range(1, members):
        e.mlp_set_learner(m, pols[m])
    e.rollout_enable(T, obs=True)
    e.pg_pop_init(_pg_options(members, envs))
    return e


def _pg_iteration(e):
    e.rollout_reset()
    e.run_days("mlp", T, BUDGET)
    return e.pg_pop_update(1)


def _pg_snapshot(e, members=M):
    return [dict(e.pg_pop_state(m), params=e.mlp_learner_params(m)) for m in range(members)]


def _assert_pg_equal(a, b, what=""):
    for m, (x, y) in enumerate(zip(a, b)):
        for k in ("theta", "m", "v", "params"):
            assert _same(x[k], y[k]), (k, m, what)
        assert x["steps"] == y["steps"], (m, what)


def _assert_pg_stats(a, b, what=""):
    for m, (x, y) in enumerate(zip(a, b)):
        for k in P.STAT_KEYS + ("steps",):
            assert _same(np.float64(x[k]), np.float64(y[k])), (k, m, what)


def _pg_hp(opts):
    hp = np.zeros((len(opts), 8), F)
    for m, o in enumerate(opts):
        hp[m, :4] = [o[k] for k in B.PG_IDS]
    return hp


PG_PBT = dict(replace_count=2, tuned=("lr", "eps_clip", "vf_coef"), bounds={"lr": (2e-4, 5e-3), "eps_clip": (0.05, 0.2), "vf_coef": (0.1, 2.0)},
              factors=(0.8, 1.25), fitness_ema=0.5)


# ---- 1. the device's fitness -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [M, N])
def test_device_fitness_equals_the_restatement_on_the_fetched_record(amd, members):
    e = _pg_population(amd, members)
    e.pbt_init("pg", replace_count=1)
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch()
    done = rec["terminated"] | rec["truncated"]
    assert done.any() and not done.all(), "the record was meant to cross an auto-reset"
    got = e.pbt_fitness()
    assert _same(got, B.fitness(rec["reward"], members))
    assert len(set(got.tolist())) > 1, "members differ, or the test would show nothing"
    # fewer days than the record holds room for: only the recorded days count
    e.rollout_reset()
    e.run_days("mlp", 1, BUDGET)
    assert _same(e.pbt_fitness(), B.fitness(e.rollout_fetch()["reward"], members))
    e.close()


def test_device_fitness_with_more_envs_a_member_than_the_block_has_lanes(amd):
    """2 learners over 600 envs: n = 300 envs a member, so lanes 0 to 43 of k_pbt_fitness take a second pass of its env loop and
    lane 0 chains over 300 returns.  K = 3, a hidden layer of 4, T = 3 with max_days = 2: an auto-reset inside the record"""
    members, envs, k, t = 2, 600, 3, 3
    n = envs // members
    rng = np.random.default_rng(777)
    pols = [R.random_policy(rng, k, (4,), "tanh", value=True, scale=0.6) for _ in range(members)]
    pols[1].layers[-1][1][1:] += F(0.4)                           # (the second member bids higher: the members' returns differ)
    e = amd.StepEngine(envs, k, seed=SEED, max_days=2, auto_reset=True)
    e.set_all_params(H.implicit_params(envs, k, SEED + 1, mean_volume=24, cvr=0.5))
    e.reset()
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(members)
    e.mlp_set_learner(1, pols[1])
    e.rollout_enable(t, obs=True)
    e.pg_pop_init([P.options(minibatch_envs=n) for _ in range(members)])
    e.pbt_init("pg", replace_count=1)
    e.run_days("mlp", t, BUDGET)
    rec = e.rollout_fetch()
    done = rec["terminated"] | rec["truncated"]
    assert done.any() and not done.all(), "the record was meant to cross an auto-reset"
    want = B.fitness(rec["reward"], members)
    first = [float(np.sum(rec["reward"][:, m * n:m * n + 256].astype(np.float64))) / n for m in range(members)]
    assert all(abs(first[m] - want[m]) > 1e-6 * abs(want[m]) for m in range(members)), "the envs of the second pass matter to both members"
    got = e.pbt_fitness()
    assert _same(got, want), (got, want)
    assert got[0] != got[1]
    e.close()


# ---- 2. the batched exploit equals the primitives (PPO) ----------------------------------------------------------------------------
def test_batched_exploit_equals_pair_by_pair_copies(amd):
    e1, e2 = _pg_population(amd), _pg_population(amd)
    e1.pbt_init("pg", replace_count=1)
    for _ in range(2):
        s1, s2 = _pg_iteration(e1), _pg_iteration(e2)
    _assert_pg_stats(s1, s2, "the twins before any copy")
    before = _pg_snapshot(e1)
    assert not _same(before[1]["theta"], before[4]["theta"])
    # a keep-all plan changes nothing
    e1.pbt_exploit([-1, 1, -1, 3, -1, 5])
    _assert_pg_equal(_pg_snapshot(e1), before, "keep all")
    # donor 4 serves 1 and 3; 5 serves 0; 2 is kept
    e1.pbt_exploit([5, 4, 2, 4, -1, -1])
    for src, dst in ((4, 1), (4, 3), (5, 0)):
        e2.pg_pop_copy(src, dst)
    after = _pg_snapshot(e1)
    _assert_pg_equal(after, _pg_snapshot(e2), "after the copies")
    for src, dst in ((4, 1), (4, 3), (5, 0)):
        _assert_pg_equal([after[dst]], [before[src]], (src, dst))
    _assert_pg_equal([after[m] for m in (2, 4, 5)], [before[m] for m in (2, 4, 5)], "untouched members")
    # the layers were rebuilt: one more iteration acts and trains on them
    _assert_pg_stats(_pg_iteration(e1), _pg_iteration(e2), "the iteration after")
    _assert_pg_equal(_pg_snapshot(e1), _pg_snapshot(e2), "the iteration after")
    assert _same(e1.rollout_fetch()["action"], e2.rollout_fetch()["action"])
    e1.close()
    e2.close()


# ---- the TD3 population ------------------------------------------------------------------------------------------------------------
WIDTHS, B0, CAPACITY = (11, 7, 1), 7, 37
SIGMAS = (0.2, 0.05, 0.4, 0.1, 0.3, 0.15)


def _td3_options():
    return [T3.options(critic_widths=WIDTHS, batch_size=B0, policy_delay=2, capacity=CAPACITY, gamma=0.9, tau=float(F(0.01 * (m + 1))),
                       actor_lr=float(F(1e-3 * (m + 1))), critic_lr=float(F(3e-3 / (m + 1))), target_noise=float(F(0.1 + 0.05 * m)), target_noise_clip=0.25,
                       reward_scale=0.5, seed=(0, 77)[m % 2], max_grad_norm=(0.0, 0.5)[m == 2]) for m in range(M)]


def _td3_population(amd, seed=601):
    rng = np.random.default_rng(seed)
    e = _engine(amd)
    pols, crits = [], []
    for m in range(M):
        pol = R.random_policy(rng, K, HIDDEN, "tanh", normalize=True, scale=0.6)
        pol.shift, pol.scale = R.realistic_norm(K)
        pol.log_std = (np.full(A, np.log(SIGMAS[m])) + 0.01 * np.arange(A)).astype(F)
        pols.append(pol)
        crits.append(T3.random_critics_for_tests(rng, K, WIDTHS))
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    for m in range(1, M):
        e.mlp_set_learner(m, pols[m])
    e.rollout_enable(T, obs=True)
    e.td3_pop_init(_td3_options())
    for m in range(M):
        e.td3_pop_set_critics(m, crits[m], action_norm=(np.full(A, 0.25, F), np.full(A, 1.5, F)) if m == 0 else None)
    return e


def _td3_iteration(e, updates=2):
    e.rollout_reset()
    e.run_days("mlp", T, BUDGET)
    e.td3_pop_store()
    return e.td3_pop_update(updates)


def _td3_snapshot(e):
    return [dict(e.td3_pop_state(m), params=e.mlp_learner_params(m), ring=e.td3_pop_buffer(m)) for m in range(M)]


def _assert_ring(a, b, what=""):
    for k in ("x", "a", "r", "done", "x2"):
        assert _same(a[k], b[k]), (k, what)
    assert (a["size"], a["written"]) == (b["size"], b["written"]), what


def _assert_td3_member(x, y, what="", ring=True, log_std=True):
    for k in T3.STATE_KEYS:
        assert _same(x[k], y[k]), (k, what)
    assert (x["updates"], x["actor_steps"]) == (y["updates"], y["actor_steps"]), what
    assert _same(x["params"][:-A], y["params"][:-A]), ("the learner's policy layers", what)
    if log_std:
        assert _same(x["params"][-A:], y["params"][-A:]), ("log_std", what)
    if ring:
        _assert_ring(x["ring"], y["ring"], what)


def _assert_td3_equal(a, b, what=""):
    for m, (x, y) in enumerate(zip(a, b)):
        _assert_td3_member(x, y, (m, what))


def _assert_td3_stats(a, b, what=""):
    for m, (x, y) in enumerate(zip(a, b)):
        for k in T3.STAT_KEYS:
            assert _same(np.float64(x[k]), np.float64(y[k])), (k, m, what)


# ---- 3. the batched exploit equals the primitives (TD3), without and with the ring --------------------------------------------------
@pytest.mark.parametrize("with_ring", [False, True])
def test_td3_batched_exploit_equals_pair_by_pair_copies(amd, with_ring):
    e1, e2 = _td3_population(amd), _td3_population(amd)
    e1.pbt_init("td3", replace_count=1, with_ring=with_ring)
    for _ in range(4):                      # 4 x 12 transitions per member: the ring of 37 has wrapped
        s1, s2 = _td3_iteration(e1), _td3_iteration(e2)
    _assert_td3_stats(s1, s2, "the twins before any copy")
    before = _td3_snapshot(e1)
    assert before[0]["ring"]["size"] == CAPACITY and not _same(before[1]["ring"]["x"], before[4]["ring"]["x"])
    e1.pbt_exploit([-1, 1, 2, -1, 4, -1])
    _assert_td3_equal(_td3_snapshot(e1), before, "keep all")
    pairs = ((4, 1), (4, 3), (5, 0))
    e1.pbt_exploit([5, 4, 2, 4, -1, -1])
    for src, dst in pairs:
        e2.td3_pop_copy(src, dst, with_ring=with_ring)
    after = _td3_snapshot(e1)
    _assert_td3_equal(after, _td3_snapshot(e2), "after the copies")
    for src, dst in pairs:
        _assert_td3_member(after[dst], before[src], (src, dst), ring=with_ring, log_std=False)
        assert _same(after[dst]["params"][-A:], before[dst]["params"][-A:]), "the copy alone leaves the destination's log_std"
        if not with_ring:
            _assert_ring(after[dst]["ring"], before[dst]["ring"], "without the ring the destination keeps its own")
    for m in (2, 4, 5):
        _assert_td3_member(after[m], before[m], ("untouched", m))
    for it in range(2):
        _assert_td3_stats(_td3_iteration(e1, 1), _td3_iteration(e2, 1), ("a further update", it))
    _assert_td3_equal(_td3_snapshot(e1), _td3_snapshot(e2), "two further updates")
    e1.close()
    e2.close()


# ---- 4. the whole round ------------------------------------------------------------------------------------------------------------
def _assert_result(res, ref, what=""):
    for k in ("fitness", "smoothed", "rank", "src", "hp"):
        assert _same(res[k], ref[k]), (k, res[k], ref[k], what)


def test_whole_round_of_a_ppo_population(amd):
    """(no smoothing here, so that the handed-in ties are ties of what is ranked; the TD3 round and the resumed run smooth)"""
    e1, e2 = _pg_population(amd), _pg_population(amd)
    options = dict(PG_PBT, fitness_ema=0.0)
    e1.pbt_init("pg", **options)
    cfg = B.config_dict(amd.StepEngine.pbt_config("pg", M, **options))
    opts = _pg_options()
    state, hp = dict(round=0, smoothed=np.zeros(M)), _pg_hp(opts)
    nan_and_tie = np.array([1.0, np.nan, 3.0, 1.0, 3.0, -2.0])
    for rnd, handed in enumerate((None, nan_and_tie)):
        for _ in range(2 if rnd == 0 else 1):
            s1, s2 = _pg_iteration(e1), _pg_iteration(e2)
        _assert_pg_stats(s1, s2, ("the twins before the round", rnd))
        fit = e1.pbt_fitness() if handed is None else handed
        if handed is None:
            assert _same(fit, B.fitness(e1.rollout_fetch()["reward"], M))
        res = e1.pbt_step(handed)
        state, ref = B.round_(cfg, B.PG, SEED, state, fit, hp)
        _assert_result(res, ref, rnd)
        assert e1.pbt_state()["round"] == rnd + 1 and _same(e1.pbt_state()["smoothed"], state["smoothed"])
        replaced = [m for m in range(M) if res["src"][m] >= 0]
        assert len(replaced) == 2 and not set(replaced) & {int(res["src"][m]) for m in replaced}
        if handed is not None:
            assert res["rank"].tolist() == [2, 0, 4, 3, 5, 1], "the NaN ranks below every number, ties rank by index"
            assert sorted(replaced) == [1, 5] and {int(res["src"][m]) for m in replaced} <= {2, 4}
        # the twin by hand, with the primitives
        hp = ref["hp"]
        for m in replaced:
            e2.pg_pop_copy(int(res["src"][m]), m)
            opts[m] = dict(opts[m], **{k: float(hp[m, h]) for h, k in enumerate(B.PG_IDS)})
            e2.pg_pop_set_config(m, **opts[m])
        _assert_pg_equal(_pg_snapshot(e1), _pg_snapshot(e2), ("after the round", rnd))
    _assert_pg_stats(_pg_iteration(e1), _pg_iteration(e2), "the iteration after the rounds")
    _assert_pg_equal(_pg_snapshot(e1), _pg_snapshot(e2), "the iteration after the rounds")
    assert any(not _same(hp[m], _pg_hp(_pg_options())[m]) for m in range(M)), "some hyperparameter moved"
    e1.close()
    e2.close()


TD3_PBT = dict(replace_count=2, tuned=("actor_lr", "target_noise", "tau", "sigma"), with_ring=True, fitness_ema=0.25, factors=(0.5, 2.0),
               bounds={"actor_lr": (1e-4, 4e-3), "target_noise": (0.05, 0.3), "tau": (0.005, 0.05), "sigma": (0.08, 0.35)})


def _td3_hp(opts):
    hp = np.zeros((M, 8), F)
    for m, o in enumerate(opts):
        hp[m, :4] = [o[k] for k in B.TD3_IDS[:4]]
    return hp


def test_whole_round_of_a_td3_population(amd):
    e1, e2 = _td3_population(amd), _td3_population(amd)
    e1.pbt_init("td3", **TD3_PBT)
    cfg = B.config_dict(amd.StepEngine.pbt_config("td3", M, **TD3_PBT))
    opts = _td3_options()
    state, hp = dict(round=0, smoothed=np.zeros(M)), _td3_hp(opts)
    nan_and_tie = np.array([2.0, 2.0, np.nan, -1.0, 5.0, 2.0])
    moved = False
    for rnd, handed in enumerate((None, nan_and_tie)):
        for _ in range(2 if rnd == 0 else 1):
            s1, s2 = _td3_iteration(e1), _td3_iteration(e2)
        _assert_td3_stats(s1, s2, ("the twins before the round", rnd))
        fit = e1.pbt_fitness() if handed is None else handed
        res = e1.pbt_step(handed)
        state, ref = B.round_(cfg, B.TD3, SEED, state, fit, hp)
        _assert_result(res, ref, rnd)
        replaced = [m for m in range(M) if res["src"][m] >= 0]
        assert len(replaced) == 2
        hp = ref["hp"]
        log_std = [e2.mlp_learner_params(m)[-A:] for m in range(M)]
        for m in replaced:
            src = int(res["src"][m])
            e2.td3_pop_copy(src, m, with_ring=True)
            opts[m] = dict(opts[m], **{k: float(hp[m, h]) for h, k in enumerate(B.TD3_IDS[:4])})
            e2.td3_pop_set_config(m, **opts[m])
            new = B.log_std_after(cfg, ref["bits"][m], log_std[src])
            moved = moved or not _same(new, log_std[src])
            assert np.all(new >= cfg["lo"][B.SIGMA]) and np.all(new <= cfg["hi"][B.SIGMA])
            e2.mlp_set_learner_log_std(m, new)
        _assert_td3_equal(_td3_snapshot(e1), _td3_snapshot(e2), ("after the round", rnd))
    assert moved, "sigma was meant to move"
    _assert_td3_stats(_td3_iteration(e1), _td3_iteration(e2), "the iteration after the rounds")
    _assert_td3_equal(_td3_snapshot(e1), _td3_snapshot(e2), "the iteration after the rounds")
    e1.close()
    e2.close()


# ---- 5. resume ---------------------------------------------------------------------------------------------------------------------
def test_a_resumed_scheduler_continues_bit_for_bit(amd):
    e1, e2 = _pg_population(amd), _pg_population(amd)
    e1.pbt_init("pg", **PG_PBT)
    for _ in range(2):
        _pg_iteration(e1), _pg_iteration(e2)
    first = e1.pbt_step()
    # the fresh engine has seen the same days; it is handed the trainer's state, the configurations and the scheduler's state
    opts = _pg_options()
    for m in range(M):
        e2.pg_pop_state(m, e1.pg_pop_state(m))
        e2.pg_pop_set_config(m, **dict(opts[m], **{k: float(first["hp"][m, h]) for h, k in enumerate(B.PG_IDS)}))
    with pytest.raises(AssertionError):
        e2.pbt_state()
    e2.pbt_init("pg", **PG_PBT)
    saved = e1.pbt_state()
    assert saved["round"] == 1
    e2.pbt_state(saved)
    assert e2.pbt_state()["round"] == 1 and _same(e2.pbt_state()["smoothed"], saved["smoothed"])
    for rnd in range(2):
        _assert_pg_stats(_pg_iteration(e1), _pg_iteration(e2), rnd)
        r1, r2 = e1.pbt_step(), e2.pbt_step()
        _assert_result(r1, r2, rnd)
        _assert_pg_equal(_pg_snapshot(e1), _pg_snapshot(e2), rnd)
    assert e1.pbt_state()["round"] == 3
    e1.close()
    e2.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(amd):
    from adcraft_amd import _ffi
    # no population trainer
    e = _engine(amd)
    with pytest.raises(_ffi.EngineStateError, match="population trainer"):
        e.pbt_init("pg", replace_count=1)
    with pytest.raises(_ffi.EngineStateError, match="adc_engine_pbt_init"):
        e.pbt_step()
    e.close()
    e = _pg_population(amd)
    # q out of range (through the C entry point: Python's own check would refuse first)
    import ctypes as C
    cfg = amd.StepEngine.pbt_config("pg", M, 1)
    for q in (0, M // 2 + 1):
        cfg.replace_count = q
        assert e._lib.adc_engine_pbt_init(e._h, C.byref(cfg)) == _ffi.ADC_EINVAL
    with pytest.raises(ValueError, match="replace_count"):
        e.pbt_init("pg", replace_count=M // 2 + 1)
    with pytest.raises(_ffi.EngineStateError):
        e.pbt_fitness()
    e.pbt_init("pg", replace_count=3)
    # no day recorded
    with pytest.raises(_ffi.EngineStateError, match="no recorded day"):
        e.pbt_fitness()
    with pytest.raises(_ffi.EngineStateError, match="no recorded day"):
        e.pbt_step()
    _pg_iteration(e)
    before = _pg_snapshot(e)
    # a destination that is a source; a member that does not exist
    with pytest.raises(ValueError, match="also a source"):
        e.pbt_exploit([1, 2, -1, -1, -1, -1])
    with pytest.raises(ValueError, match="src_of_m"):
        e.pbt_exploit([M, -1, -1, -1, -1, -1])
    with pytest.raises(ValueError):
        e.pbt_exploit([-1] * (M - 1))
    with pytest.raises(ValueError):
        e.pbt_step(np.zeros(M + 1))
    _assert_pg_equal(_pg_snapshot(e), before, "a refused call changes nothing")
    assert e.pbt_state()["round"] == 0
    res = e.pbt_step()
    assert (res["src"] >= 0).sum() == 3 and e.pbt_state()["round"] == 1
    _pg_iteration(e)
    # the scheduler goes with the learners (and the trainer over them)
    e.mlp_learners(M)
    for call in (e.pbt_step, e.pbt_fitness, e.pbt_state, lambda: e.pbt_exploit([-1] * M)):
        with pytest.raises(_ffi.EngineStateError, match="adc_engine_pbt_init"):
            call()
    with pytest.raises(_ffi.EngineStateError, match="population trainer"):
        e.pbt_init("pg", replace_count=1)
    # ... and a new trainer takes a new scheduler, from round 0
    e.rollout_enable(T, obs=True)
    e.pg_pop_init(_pg_options())
    with pytest.raises(_ffi.EngineStateError, match="adc_engine_pbt_init"):
        e.pbt_step()
    e.pbt_init("pg", replace_count=1)
    _pg_iteration(e)
    assert (e.pbt_step()["src"] >= 0).sum() == 1 and e.pbt_state()["round"] == 1
    e.close()


# ---- 7. the Python scheduler over both trainers ------------------------------------------------------------------------------------
def test_scheduler_keeps_the_trainers_configurations_in_step(amd):
    from adcraft_amd.baselines.pbt import PBTScheduler
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer
    rng = np.random.default_rng(701)
    # PPO: a round every second call
    pols = []
    for _ in range(M):
        pol = R.random_policy(rng, K, HIDDEN, "tanh", value=True, normalize=True, scale=0.6)
        pol.shift, pol.scale = R.realistic_norm(K)
        pols.append(pol)
    e = _engine(amd)
    tr = PGPopulationTrainer(e, pols, T, [dict(epochs=1, minibatches=1, lr=float(F(lr))) for lr in np.logspace(-4, -2, M)])
    sch = PBTScheduler(tr, replace_fraction=0.34, tuned=("lr",), bounds={"lr": (2e-4, 5e-3)}, every=2, seed=9)
    assert sch.replace_count == 2
    start = [c["lr"] for c in tr.configs]
    tr.iteration(budget=BUDGET)
    assert sch.step() is None and e.pbt_state()["round"] == 0
    tr.iteration(budget=BUDGET)
    res = sch.step()
    assert res is not None and e.pbt_state()["round"] == 1 and len(sch.history) == 1
    for m in range(M):
        src = int(res["src"][m])
        assert _same(F(tr.configs[m]["lr"]), res["hp"][m, 0])
        if src < 0:
            assert tr.configs[m]["lr"] == start[m] and sch.origin[m] == m
        else:
            assert sch.origin[m] == src and tr.configs[m]["lr"] in (float(np.clip(F(F(start[src]) * F(f)), F(2e-4), F(5e-3))) for f in (0.8, 1.25))
    # the engine's table is what the dicts say: setting the dicts again changes nothing in the next update
    twin_stats = tr.iteration(budget=BUDGET)
    assert len(twin_stats) == M
    e.close()
    # TD3 with sigma
    pols = []
    for _ in range(M):
        pol = R.random_policy(rng, K, HIDDEN, "tanh", normalize=True, scale=0.6)
        pol.shift, pol.scale = R.realistic_norm(K)
        pol.log_std = np.zeros(A, F)
        pols.append(pol)
    e = _engine(amd)
    tr = TD3PopulationTrainer(e, pols, list(SIGMAS), dict(critic_hidden=WIDTHS[:-1], batch_size=B0, capacity=CAPACITY, learning_starts=0, updates_per_iteration=2),
                              horizon=T)
    sch = PBTScheduler(tr, replace_fraction=0.5, tuned=("sigma", "tau"), bounds={"sigma": (0.08, 0.35), "tau": (0.001, 0.01)}, factors=(0.5, 2.0),
                       with_ring=True)
    assert sch.replace_count == 3
    tr.iteration(budget=BUDGET)
    res = sch.step()
    assert (res["src"] >= 0).sum() == 3
    for m in range(M):
        assert _same(tr._templates[m].log_std, e.mlp_learner_params(m)[-A:]), ("the templates' log_std follows the device's", m)
        if res["src"][m] >= 0:
            assert _same(F(tr.configs[m]["tau"]), res["hp"][m, 3])
            _assert_ring(e.td3_pop_buffer(m), e.td3_pop_buffer(int(res["src"][m])), "the donor's ring came along")
    tr.iteration(budget=BUDGET)
    with pytest.raises(TypeError):
        PBTScheduler(object())
    e.close()
