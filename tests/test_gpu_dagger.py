"""GPU tests of DAgger days (parts/kernel_imitation.inc: k_dagger_mix; parts/imitation_api.inc: adc_engine_dagger_days; the law is
csrc/adc_dagger.h): beta = 1 against a twin under teach_days, beta = 0 against a twin under run_days("mlp"), beta = 0.5 against
both twins env by env and against tests/dagger_ref.py, the aggregated record through im_update against tests/im_ref.py bit for
bit, every refusal, DAggerTrainer's rounds and state, and chained days in env groups.  None of these symbols exists before this feature: every test here fails on
the parent commit.  The shape is tests/test_gpu_imitation.py's: 6 envs x 5 keywords, 4 days, max_days = 3 with auto_reset."""
import signal

import numpy as np
import pytest

from tests import dagger_ref as DR
from tests import im_ref as I
from tests import mlp_ref as R
from tests import pg_ref as P
from tests import stack_ref as S
from tests import td3_bounded_ref as TB
from tests import td3_ref as T3
from tests.test_dagger_host import MIX_BETA, MIX_DAYS, MIX_SEEDS
from tests.test_gpu_imitation import (BUDGET, K0, N0, RESETS, STEP_FIELDS, T0, _assert_state, _assert_stats, _engine, _fresh_state, _now, _policy,
                                      _refused, _same, _teacher_ready)

pytestmark = pytest.mark.gpu
F = np.float32
SEEDS = MIX_SEEDS
assert len(SEEDS) == N0 and MIX_DAYS == T0
# (N, K) of the record kernels' tests - k_teach_record, k_dagger_mix and their bounded forms run one lane per (env, component): the
# module's shape, 36 lanes of one block; and 5 x 257 = 1285 lanes, six blocks with the last one partial, where the split i / A, i % A
# runs across blocks, a = 256 reads the last bound, and an env group's pointer offsets fall inside a block's worth of lanes
RECORD_SHAPES = [(N0, K0), (5, 256)]


def _record_policy(rng, K, frames):
    """the module's policy at its own shape; one head over hidden (31,) at the wide one"""
    return _policy(rng, K, frames) if K == K0 else _policy(rng, K, frames, hidden=(31,))


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


def _learner(amd, pol, teacher, T=T0, N=N0, K=K0, record=True, mlp=True, bounds=None):
    """an engine ready for `teacher` whose learned agent is `pol` under the test's agent seeds"""
    e = _engine(amd, N, K, **RESETS)
    _teacher_ready(e, teacher, np.arange(N, dtype=np.uint64) + 11)
    if mlp:
        e.mlp_init(pol, np.arange(N, dtype=np.uint64) + 11, deterministic=False)
        if bounds is not None:
            e.mlp_set_bounds(*bounds)
        if record:
            e.rollout_enable(T, obs=True)
    return e


def _same_env(a, b, what=""):
    oa, ob = a.fetch(), b.fetch()
    for k in STEP_FIELDS:
        assert _same(oa[k], ob[k]), (what, k)
    assert all(np.array_equal(x, y) for x, y in zip(a.get_rng_state(), b.get_rng_state())), what


def _label(e):
    """[N, K + 1]: {budget, bids} in the engine's action buffers"""
    bids, budget = e.get_actions()
    N = len(np.asarray(budget).reshape(-1))
    return np.concatenate([np.asarray(budget, F).reshape(N, 1), np.asarray(bids, F).reshape(N, -1)], axis=1)


# ---- 1. beta = 1 is a teacher day -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("teacher", ["fixed", "zero_margin", "oracle"])
def test_beta_one_is_a_teacher_day(amd, teacher, frames):
    N, T = N0, T0
    pol = _policy(np.random.default_rng(7 + frames), K0, frames)
    a, b = _learner(amd, pol, teacher), _learner(amd, pol, teacher)
    for t in range(T):
        a.dagger_days(teacher, 1, 1.0, BUDGET)
        b.teach_days(teacher, 1, BUDGET)
        _same_env(a, b, t)
        assert _same(_label(a), _label(b)), t
    ra, rb = a.rollout_fetch(bootstrap=True), b.rollout_fetch(bootstrap=True)
    assert ra["reward"].shape == (T, N)
    done = ra["terminated"] | ra["truncated"]
    assert done[:-1].any() and not done.all(), "an auto-reset was meant to fall inside the record"
    for k in rb:
        assert _same(ra[k], rb[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(a.mlp_agent_state(), b.mlp_agent_state()))
    assert np.array_equal(a.mlp_agent_state()[1], np.full(N, T, np.uint32))
    if frames > 1:
        ha, hb = a.mlp_history_state(), b.mlp_history_state()
        assert all(_same(ha[k], hb[k]) for k in ha)
    assert _same(a.dagger_mask(), np.ones((T, N), np.uint8))
    assert _same(b.dagger_mask(), np.ones((T, N), np.uint8)), "rows of plain teacher days read 1"
    with pytest.raises(ValueError, match="overflow"):
        a.dagger_days(teacher, 1, 1.0, BUDGET)
    a.close()
    b.close()


# ---- 2. beta = 0 is the learner's day with the teacher's label -----------------------------------------------------------------------------
@pytest.mark.parametrize("teacher,frames", [("fixed", 1), ("fixed", 3), ("zero_margin", 1), ("oracle", 1)])
def test_beta_zero_is_the_learners_day_with_the_teachers_label(amd, teacher, frames):
    N, T = N0, T0
    pol = _policy(np.random.default_rng(17 + frames), K0, frames)
    a, b = _learner(amd, pol, teacher), _learner(amd, pol, teacher)
    fixed = _label(a)
    labels = []
    for t in range(T):
        a.dagger_days(teacher, 1, 0.0, BUDGET)
        b.run_days("mlp", 1, BUDGET)
        _same_env(a, b, t)
        labels.append(_label(a))
        if teacher == "fixed":
            assert _same(labels[-1], fixed), "the fixed teacher's action stays in the action buffers"
        else:
            assert not _same(labels[-1], _label(b)), "the label was meant to differ from what the learner played"
    ra, rb = a.rollout_fetch(bootstrap=True), b.rollout_fetch(bootstrap=True)
    for k in ("obs", "value", "reward", "terminated", "truncated", "bootstrap_value"):
        assert _same(ra[k], rb[k]), k
    assert _same(ra["action"], np.stack(labels))
    assert not _same(ra["action"], rb["action"])
    assert _same(ra["logp"], np.zeros((T, N), F)), "logp is +0"
    assert all(np.array_equal(x, y) for x, y in zip(a.mlp_agent_state(), b.mlp_agent_state()))
    if frames > 1:
        ha, hb = a.mlp_history_state(), b.mlp_history_state()
        assert all(_same(ha[k], hb[k]) for k in ha)
    assert _same(a.dagger_mask(), np.zeros((T, N), np.uint8))
    a.close()
    b.close()


# ---- 3. beta = 0.5 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RECORD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bounded", [False, True])
def test_a_mixed_day_follows_the_coin_env_by_env(amd, bounded, shape):
    (N, K), T, frames, teacher = shape, T0, 3, "fixed"
    pol = _record_policy(np.random.default_rng(27), K, frames)
    bounds = TB.box(K) if bounded else None
    m, tt, lt = (_learner(amd, pol, teacher, N=N, K=K, bounds=bounds) for _ in range(3))
    fixed = _label(m)
    assert len(set(fixed[:, K].tolist())) > 1, "component a = K of the label was meant to differ between envs"
    keys, ticks = m.mlp_agent_state()
    assert np.array_equal(keys, np.array([R.agent_key(s) for s in SEEDS[:N]], np.uint64)) and not ticks.any()
    want_mask = DR.mask(keys, ticks, T, MIX_BETA)
    assert want_mask[0].tolist() == [0, 1, 1, 1, 0, 1][:N]
    hist = S.History(N, K, frames)
    rows, values = [], []
    # the first day from identical states: an env follows the twin its coin names (envs are independent)
    row = hist.row(*_now(m))
    rows.append(S.normalized(pol, row))
    values.append(R.act(pol, row, None, deterministic=True)["value"])
    m.dagger_days(teacher, 1, MIX_BETA, BUDGET)
    tt.teach_days(teacher, 1, BUDGET)
    lt.run_days("mlp", 1, BUDGET)
    om, ot, ol = m.fetch(), tt.fetch(), lt.fetch()
    pick = want_mask[0].astype(bool)
    assert pick.any() and not pick.all(), "the coin was meant to pick the teacher in some envs and the learner in others"
    differ = False
    for k in STEP_FIELDS:
        gm, gt, gl = np.asarray(om[k]), np.asarray(ot[k]), np.asarray(ol[k])
        assert _same(gm[pick], gt[pick]), ("teacher-driven envs", k)
        assert _same(gm[~pick], gl[~pick]), ("learner-driven envs", k)
        differ = differ or not _same(gt, gl)
    assert differ, "the two twins were meant to end the day in different states"
    rm, rl = m.rollout_fetch(), lt.rollout_fetch()
    # (the played action of a learner-driven env is the learner's: under the bounds the box image its own day steps the env by)
    assert _same(rm["reward"][0][~pick], rl["reward"][0][~pick]) and _same(rm["reward"][0][pick], tt.rollout_fetch()["reward"][0][pick])
    assert _same(_label(m), fixed), "get_actions after a DAgger day returns the label"
    for t in range(1, T):
        row = hist.row(*_now(m))
        rows.append(S.normalized(pol, row))
        values.append(R.act(pol, row, None, deterministic=True)["value"])
        m.dagger_days(teacher, 1, MIX_BETA, BUDGET)
        assert _same(_label(m), fixed), t
    rec = m.rollout_fetch()
    assert _same(m.dagger_mask(), want_mask)
    assert np.array_equal(m.mlp_agent_state()[1], np.full(N, T, np.uint32))
    label = TB.unbox(fixed, *bounds) if bounded else fixed
    assert np.isfinite(label).all() and (not bounded or (np.abs(label) < 1).all()), "the fixed action was meant to lie inside the box"
    assert _same(rec["action"], np.stack([label] * T)), "every day's label is the fixed action (in box units under the bounds)"
    assert len(set(label[:, K].tolist())) > 1, "component a = K of the recorded label was meant to differ between envs"
    assert _same(rec["logp"], np.zeros((T, N), F))
    assert _same(rec["obs"], np.stack(rows))
    assert _same(rec["value"], np.stack(values))
    assert np.abs(rec["obs"][:, :, 5 * K + 2:]).sum() > 0
    st, ref = m.mlp_history_state(), hist.state()
    assert all(_same(st[k], ref[k]) for k in ("hist", "last", "from"))
    for e in (m, tt, lt):
        e.close()


# ---- 4. the update over an aggregated record ---------------------------------------------------------------------------------------------------
def test_two_aggregated_rounds_update_as_the_restatement_and_hand_over_to_pg(amd):
    N, K, T, mb = N0, K0, T0, 2
    pol = _policy(np.random.default_rng(37), K)
    opts = P.options(lr=3e-3, max_grad_norm=0.5, minibatch_envs=mb, gamma=0.9, reward_scale=0.05)
    im = I.im_options(beta=0.0, vf_coef=0.5)
    e = _learner(amd, pol, "fixed")
    e.pg_init(**opts)
    e.im_init(**im)
    state, ma = _fresh_state(pol), im["ma_start"]
    for rnd, beta in enumerate((1.0, 0.5)):
        e.dagger_days("fixed", 2, beta, BUDGET)                      # (no rollout_reset: the record aggregates)
        rec = e.rollout_fetch(bootstrap=True)
        assert rec["reward"].shape == (2 * (rnd + 1), N)
        adv, ret = e.im_advantages(fetch=True)
        radv, rret = I.returns(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], rec["bootstrap_value"], **opts)
        assert _same(adv, radv) and _same(ret, rret)
        ma, c = I.scale(ma, radv, **im)
        stats = e.im_update(2)
        state, rstats = I.update(pol, state, rec, radv, rret, c, 2, opts, im)
        _assert_state(e.pg_state(), state, rnd)
        _assert_stats(stats, rstats, rnd)
        assert stats["steps"] == state["steps"] == 2 * (N // mb) * (rnd + 1) and stats["samples"] == 2 * (rnd + 1) * mb
        assert _same(np.float64(e.im_state()["ma"]), np.float64(ma))
    keys, _ = e.mlp_agent_state()
    mask = e.dagger_mask()
    assert _same(mask[:2], np.ones((2, N), np.uint8)) and _same(mask[2:], DR.mask(keys, np.full(N, 2), 2, 0.5))
    assert mask[2:].any() and not mask[2:].all()
    # the hand-over: the learner's own days and pg_update continue from the clone's state by the policy-gradient law
    start = e.pg_state()
    e.rollout_reset()
    e.run_days("mlp", T, BUDGET)
    rec = e.rollout_fetch(bootstrap=True)
    stats = e.pg_update(2)
    ref, rstats = P.update(pol, start, rec, rec["bootstrap_value"], 2, opts)
    _assert_state(e.pg_state(), ref, "hand-over")
    for k in P.STAT_KEYS:
        assert _same(np.float64(stats[k]), np.float64(rstats[k])), k
    e.close()


# ---- 5. refusals and bookkeeping ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_bookkeeping(amd):
    from adcraft_amd._ffi import EngineStateError as State
    N, K, T = N0, K0, T0
    rng = np.random.default_rng(3)
    pol = _policy(rng, K)
    e, twin = _learner(amd, pol, "fixed", mlp=False), _learner(amd, pol, "fixed", mlp=False)
    day = lambda *a: e.dagger_days(*a)
    # --- everything adc_engine_teach_days refuses
    _refused(State, "mlp_init", day, "fixed", 1, 0.5)
    e.mlp_init(pol, SEEDS, deterministic=False)
    _refused(State, "rollout record", day, "fixed", 1, 0.5)
    e.rollout_enable(T, obs=False)
    _refused(State, "ADC_ROLLOUT_OBS", day, "fixed", 1, 0.5)
    e.rollout_enable(T, obs=True)
    _refused(ValueError, "own teacher", day, "mlp", 1, 0.5)
    _refused(ValueError, "overflow", day, "fixed", T + 1, 0.5)
    _refused(ValueError, "days < 0", day, "fixed", -1, 0.5)
    _refused(State, "agent_init", day, "zero_margin", 1, 0.5)
    _refused(State, "bid_curves_build", day, "oracle", 1, 0.5)
    e.mlp_population(2)
    _refused(State, "population", day, "fixed", 1, 0.5)
    e.mlp_population(0)
    e.mlp_learners(2)
    _refused(State, "learners", day, "fixed", 1, 0.5)
    e.mlp_learners(0)
    e.mlp_set_squash(np.zeros(K + 1, F), np.ones(K + 1, F))
    _refused(State, "squash", day, "fixed", 1, 0.5)
    e.mlp_set_squash(None, None)
    # --- its own
    for beta in (-0.25, 1.5, float("nan"), float("inf")):
        _refused(ValueError, r"beta: .* in \[0, 1\]", day, "fixed", 1, beta)
    _refused(ValueError, "keys its points by the bid it returned", day, "interpolation", 1, 0.5)
    _refused(ValueError, "unknown teacher", day, "nobody", 1, 0.5)
    assert e.rollout_fetch()["reward"].shape[0] == 0, "a refused call records nothing"
    # --- the engine still works: two plain teacher days, then two learner-driven DAgger days; the mask's rows
    e.teach_days("fixed", 2)
    twin.run_days("fixed", 2)
    _same_env(e, twin, "teacher days after the refusals")
    assert _same(e.dagger_mask(), np.ones((2, N), np.uint8))
    e.dagger_days("fixed", 2, 0.0)
    assert _same(e.dagger_mask(), np.repeat(np.array([1, 1, 0, 0], np.uint8), N).reshape(T, N))
    # --- the policy-gradient calls see a labelled record; MARWIL's weight is refused over DAgger days, cloning is not
    opts = P.options(minibatch_envs=2)
    e.pg_init(**opts)
    for call in (e.pg_advantages, lambda: e.pg_minibatch(0, 2), e.pg_update):
        _refused(State, "the record holds teacher days", call)
    e.im_init(beta=0.5)
    for call in (e.im_advantages, lambda: e.im_minibatch(0, 2), lambda: e.im_update(1)):
        _refused(State, "the record holds DAgger days: MARWIL", call)
    e.im_init(beta=0.0, vf_coef=1.0)
    e.im_advantages()
    assert np.isfinite(e.im_update(1)["logp"])
    # --- rollout_reset clears the DAgger count: plain teacher days under MARWIL again, and their rows read 1 again
    e.im_init(beta=0.5)
    e.rollout_reset()
    e.teach_days("fixed", 2)
    e.im_advantages()
    assert np.isfinite(e.im_update(1)["weight"])
    assert _same(e.dagger_mask(), np.ones((2, N), np.uint8))
    # --- the mask over a record the learner collected
    e.run_days("mlp", 1, BUDGET)
    _refused(State, "days the learner collected", e.dagger_mask)
    e.rollout_reset()
    e.run_days("mlp", 2, BUDGET)
    _refused(State, "days the learner collected", e.dagger_mask)
    assert np.isfinite(e.pg_update(1)["policy_loss"])
    e.close()
    twin.close()


def test_the_td3_store_takes_teacher_days_and_refuses_dagger_days(amd):
    from adcraft_amd._ffi import EngineStateError as State
    N, K, T = N0, K0, T0
    rng = np.random.default_rng(47)
    pol = _policy(rng, K, value=False)
    crit = T3.random_critics_for_tests(rng, K, (12, 1))
    e = _learner(amd, pol, "fixed")
    e.td3_init(**T3.options(critic_widths=(12, 1), batch_size=8, capacity=100, seed=123))
    e.td3_set_critics(crit)
    e.teach_days("fixed", 1)
    e.dagger_days("fixed", 1, 1.0)
    _refused(State, "the record holds DAgger days: their recorded action is the teacher's label", e.td3_store)
    e.rollout_reset()
    e.teach_days("fixed", 2)
    assert e.td3_store() == 2 * N, "plain teacher days are demonstrations still"
    e.close()


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------------
def test_the_trainer_aggregates_rounds_and_carries_its_state(amd):
    from adcraft_amd.baselines.imitation import DAggerTrainer
    N, K = N0, K0
    pol = _policy(np.random.default_rng(67), K)

    def make(aggregate, **kw):
        e = _engine(amd, N, K, **RESETS)
        e.sample_actions(0.3, 1.0, 40.0)
        return e, DAggerTrainer(e, pol, teacher="fixed", rounds=2, days=2, epochs=1, aggregate=aggregate, budget=BUDGET, minibatches=3,
                                agent_seeds=SEEDS, lr=3e-3, vf_coef=0.5, **kw)
    e, tr = make(True)
    assert tr.im_config["beta"] == 0.0 and (tr.beta(0), tr.beta(1), tr.beta(3)) == (1.0, 0.5, 0.125)
    s0, s1 = tr.iteration(), tr.iteration()
    assert (s0["round"], s0["beta"], s0["teacher_share"], s0["recorded"], s0["steps"]) == (0, 1.0, 1.0, 2, 3)
    assert (s1["round"], s1["beta"], s1["recorded"], s1["steps"], s1["samples"]) == (1, 0.5, 4, 6, 4 * (N // 3))
    mask = e.dagger_mask()
    assert mask.shape == (4, N) and mask[:2].all() and s1["teacher_share"] == float(mask[2:].mean()) and 0 < s1["teacher_share"] < 1
    with pytest.raises(ValueError, match="record is full"):
        tr.iteration()
    st = tr.state()
    assert st["round"] == 2 and st["recorded"] == 4 and st["steps"] == 6 and st["calls"] == 2
    assert _same(P.flat_params(tr.policy()), st["theta"])
    # round by round: the first round is the aggregated trainer's first, the second trains on its own two days alone
    f, tf = make(False)
    t0, t1 = tf.iteration(), tf.iteration()
    _assert_stats(t0, s0, "round 0")
    assert (t1["round"], t1["beta"], t1["recorded"], t1["samples"]) == (1, 0.5, 2, 2 * (N // 3))
    assert _same(f.dagger_mask(), mask[2:]), "the coins follow the agents' ticks, not the record"
    assert not _same(f.pg_state()["theta"], st["theta"])
    tf.load_state(st)
    assert tf.round == 2
    _assert_state(f.pg_state(), st, "loaded")
    assert f.im_state() == dict(ma=st["ma"], calls=2)
    assert np.isfinite(tf.iteration()["logp"]), "a trainer without aggregation goes on past `rounds`"
    with pytest.raises(ValueError, match="DAgger clones"):
        DAggerTrainer(f, pol, teacher="fixed", rounds=1, days=1, beta=0.5)
    e.close()
    f.close()


# ---- 6. chained days in env groups ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, K0), RECORD_SHAPES[1]], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("teacher", ["zero_margin", "oracle"])
def test_chained_days_in_env_groups_equal_days_one_call_at_a_time(amd, teacher, shape):
    """8 envs in 4 forced groups (the count tests/test_gpu_obs_history.py groups at): the chain forks once and every kernel of a
    DAgger day - both acts, k_dagger_mix, the step on the scratch, the outcome - runs group by group on the groups' streams.  At
    5 x 256 the groups are the envs [0], [1], [2], [3, 4]: every group's pointers start inside a block's worth of lanes"""
    (N, K), T, groups = shape, T0, 4
    pol = _record_policy(np.random.default_rng(57), K, 3)
    out = []
    for chained in (True, False):
        e = _engine(amd, N, K, **RESETS)
        e.set_env_groups(groups)
        _teacher_ready(e, teacher, np.arange(N, dtype=np.uint64) + 11)
        e.mlp_init(pol, np.arange(N, dtype=np.uint64) + 11, deterministic=False)
        e.rollout_enable(T, obs=True)
        if chained:
            e.dagger_days(teacher, T, MIX_BETA, BUDGET)
            assert e.env_groups() == groups, "the forced env groups did not engage"
        else:
            for _ in range(T):
                e.dagger_days(teacher, 1, MIX_BETA, BUDGET)
                e.fetch()
        out.append((e.rollout_fetch(bootstrap=True), e.dagger_mask(), e.fetch(), e.get_rng_state(), _label(e), e.mlp_history_state()))
        e.close()
    (ra, ma, oa, sa, la, ha), (rb, mb, ob, sb, lb, hb) = out
    for k in ra:
        assert _same(ra[k], rb[k]), k
    keys = np.array([R.agent_key(s) for s in np.arange(N) + 11], np.uint64)
    assert _same(ma, mb) and _same(ma, DR.mask(keys, np.zeros(N, np.int64), T, MIX_BETA))
    cut = [N * g // groups for g in range(groups + 1)]               # (a group's envs: [N g / G, N (g + 1) / G), 2 each at N = 8)
    assert all(ma[:, cut[g]:cut[g + 1]].any() and not ma[:, cut[g]:cut[g + 1]].all() for g in range(groups)), "both branches in every group"
    assert any(0 < row.sum() < N for row in ma), "the coin was meant to pick the teacher in some envs and the learner in others"
    assert len(set(la[:, K].tolist())) > 1, "component a = K of the label was meant to differ between envs"
    for k in STEP_FIELDS:
        assert _same(oa[k], ob[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(sa, sb)) and _same(la, lb)
    assert all(_same(ha[k], hb[k]) for k in ha)
