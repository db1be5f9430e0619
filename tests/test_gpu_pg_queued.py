"""GPU tests of the queued PPO / A2C update (parts/kernel_pg_queued.inc; adc_engine_pg_update_queued / _pg_pop_update_queued)
against the host-driven update, bit for bit.  Every case builds engines from the same seeds, collects the same record, runs the
host-driven update on one and the queued one on the other and requires the same learner state (theta, m, v, steps), the same device
layers, returned statistics, shuffle statistics, KL statistics and coefficients, and the same next act.  Where a case needs the
host-driven update to clip some steps and not others, or to stop at a given minibatch, a third engine is driven by hand through the
same minibatches (pg_minibatch / pg_shuffle_minibatch: the host-driven update's own steps) to choose the bound and to show that
it does; that engine's end state is the host-driven update's too.

Shapes: 4 envs per learner, 3 keywords, 5 recorded days (20 samples), one hidden layer of 8 and a value network, 3 epochs."""
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import pg_ref as P

pytestmark = pytest.mark.gpu
F = np.float32
BUDGET = 1000.0
SEED = 41
NO_RESETS = dict(max_days=1 << 20, loss_threshold=1e12)
N, K, T, EPOCHS = 4, 3, 5, 3
MB = 7                                  # 20 samples: minibatches of 7, 7 and 6
PER_EPOCH = 3


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


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _assert_same(got, ref, path="result"):
    """dicts, lists, arrays and scalars, bit for bit (a NaN equals the same NaN)"""
    if isinstance(ref, dict):
        assert isinstance(got, dict) and set(got) == set(ref), path
        for k in ref:
            _assert_same(got[k], ref[k], f"{path}[{k!r}]")
    elif isinstance(ref, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(ref), path
        for i, (g, r) in enumerate(zip(got, ref)):
            _assert_same(g, r, f"{path}[{i}]")
    elif isinstance(ref, np.ndarray):
        assert isinstance(got, np.ndarray) and got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(_bits(got), _bits(ref)), path
    elif isinstance(ref, float):
        assert np.array_equal(_bits(np.float64(got)), _bits(np.float64(ref))), (path, got, ref)
    else:
        assert got == ref and type(got) is type(ref), (path, got, ref)


def _planes(n_envs, seed=SEED):
    return H.implicit_params(n_envs, K, seed + 1, mean_volume=24, cvr=0.5)


def _policy(seed, two=False):
    pol = R.random_policy(np.random.default_rng(seed), K, (8,), "tanh", two_heads=two, value=True, normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _solo(amd, pol, opts, shuffle=None, kl=None, planes=None, env_id_base=0, collect=True):
    """a single learner over the record of T days collected by `pol`"""
    planes = _planes(N) if planes is None else planes
    e = amd.StepEngine(planes.shape[1], K, seed=SEED, env_id_base=env_id_base, **NO_RESETS)
    e.set_all_params(planes)
    e.reset()
    e.mlp_init(pol, deterministic=False)
    e.rollout_enable(T, obs=True)
    e.pg_init(**opts)
    if kl is not None:
        e.pg_kl_init(**kl)
    if shuffle is not None:
        e.pg_shuffle_init(**shuffle)
    if collect:
        e.run_days("mlp", T, BUDGET)
    return e


def _population(amd, pols, opts_m, shuffle_m, kl_m=None):
    M = len(pols)
    planes = _planes(M * N)
    e = amd.StepEngine(M * N, K, seed=SEED, **NO_RESETS)
    e.set_all_params(planes)
    e.reset()
    e.mlp_init(pols[0], deterministic=False)
    e.mlp_learners(M)
    for m, pol in enumerate(pols):
        e.mlp_set_learner(m, pol)
    e.rollout_enable(T, obs=True)
    e.pg_pop_init(list(opts_m))
    if kl_m is not None:
        e.pg_kl_init(per_member=list(kl_m))
    e.pg_shuffle_init(per_member=list(shuffle_m))
    e.run_days("mlp", T, BUDGET)
    return e


def _snapshot(e, stats, members=0, shuffle=False, kl=False, act=True):
    """everything the two updates must agree on; members = 0: a single learner"""
    out = dict(stats=stats)
    if members:
        out["state"] = [e.pg_pop_state(m) for m in range(members)]
        out["layers"] = [e.mlp_learner_params(m) for m in range(members)]
    else:
        out["state"] = e.pg_state()
        out["layers"] = e.mlp_params()
    if shuffle:
        out["shuffle"] = e.pg_shuffle_stats()
    if kl:
        out["kl"] = e.pg_kl_stats()
        out["kl_coef"] = [float(e.pg_kl_coef(m)) for m in range(max(members, 1))]
    if act:
        e.mlp_act()
        out["act"] = e.mlp_last()
    return out


def _drive_shuffled(e, epochs, population=False):
    """the host-driven update by hand: the advantages, then per epoch a new order and its minibatches.  Returns approx_kl of every
    minibatch in order (a population: one list per member)"""
    (e.pg_pop_advantages if population else e.pg_advantages)()
    kls = []
    for _ in range(epochs):
        e.pg_shuffle_epoch()
        for j in range(PER_EPOCH):
            st = e.pg_shuffle_minibatch(j)
            kls.append([s["approx_kl"] for s in (st if population else [st])])
    return [list(col) for col in zip(*kls)] if population else [k[0] for k in kls]


def _target_stopping_at(kls, serial):
    """target_kl whose bound 1.5 target lies strictly between approx_kl of minibatch `serial` and the largest before it"""
    before, at = max(kls[:serial]), kls[serial]
    assert at > before and at > 0, f"approx_kl of minibatch {serial} is no new maximum: {kls} (change the learning rate)"
    target = float(F(0.5 * (max(before, 0.0) + at) / 1.5))
    assert target > 0 and before < 1.5 * np.float64(F(target)) < at, (kls, target)
    return target


def _pair(amd, build, epochs=EPOCHS, members=0, **snap):
    """the host-driven update on one engine, the queued one on another; the two snapshots"""
    out = []
    for queued in (False, True):
        e = build()
        update = e.pg_pop_update if members else e.pg_update
        out.append(_snapshot(e, update(epochs, queued=queued), members, **snap))
        e.close()
    return out


# ---- 1. env-block minibatches, the norm clip on some steps -------------------------------------------------------------------------
def test_env_block_minibatches_with_a_clip_that_engages_on_some_steps(amd):
    """minibatch_envs = 2: two minibatches of 10 samples per epoch, six steps.  max_grad_norm is the geometric mean of the
    smallest and the largest gradient norm of the six unclipped steps; the host-driven steps taken by hand under it show norms on
    both sides of it, and end where the host-driven update ends"""
    pol = _policy(11)
    base = P.options(lr=3e-2, vf_coef=1.0, minibatch_envs=2)

    def by_hand(opts):
        e = _solo(amd, pol, opts)
        e.pg_advantages()
        norms = [e.pg_minibatch(n0, 2)["grad_norm"] for _ in range(EPOCHS) for n0 in (0, 2)]
        state = e.pg_state()
        e.close()
        return norms, state
    free, _ = by_hand(dict(base, max_grad_norm=0.0))
    assert min(free) < max(free)
    bound = float(F(np.sqrt(min(free) * max(free))))
    opts = dict(base, max_grad_norm=bound)
    norms, state = by_hand(opts)
    print("max_grad_norm", bound, "grad_norm per step:", " ".join(f"{g:.4e}" for g in norms))
    assert any(g > bound for g in norms) and any(g <= bound for g in norms), "the clip engages on some steps and not on others"
    host, queued = _pair(amd, lambda: _solo(amd, pol, opts))
    _assert_same(host["state"], state, "the host-driven update against its steps by hand")
    assert host["state"]["steps"] == 6 and host["stats"]["samples"] == 10
    _assert_same(queued, host)


# ---- 2. shuffled minibatches, the short tail, no stop ------------------------------------------------------------------------------
def test_shuffled_minibatches_with_a_short_tail(amd):
    """minibatch_samples = 7 over 20 samples: 7 + 7 + 6"""
    pol = _policy(12)
    opts, sh = P.options(lr=3e-2, vf_coef=1.0), dict(minibatch_samples=MB)
    host, queued = _pair(amd, lambda: _solo(amd, pol, opts, sh), shuffle=True)
    assert host["shuffle"] == dict(epochs_begun=3, minibatches_evaluated=9, steps_taken=9, stopped=0)
    assert host["state"]["steps"] == 9 and host["stats"]["samples"] == 6
    _assert_same(queued, host)


# ---- 3., 4. the early stop in the second epoch, plain and under the KL penalty and the value clip -------------------------------------
def _rllib():
    from adcraft_amd.baselines import pg_trainer
    cfg = pg_trainer.rllib_ppo()
    kl = cfg.pop("kl_penalty")
    for k in ("epochs", "minibatches"):
        cfg.pop(k)
    return P.options(**cfg), dict(kl)


STOP_CASES = {
    "plain": lambda: (_policy(13), P.options(vf_coef=1.0), None),
    "rllib-free-log-std": lambda: (_policy(14),) + _rllib(),
    "rllib-two-heads": lambda: (_policy(15, two=True),) + _rllib(),
}
STOP_LRS = (3e-3, 1e-3, 1e-2, 2e-3, 5e-3, 3e-4)


def _stop_case(amd, case):
    """(policy, options, KL options, shuffle options whose target_kl stops the host-driven update at the second minibatch of the
    second epoch).  approx_kl is a seven-sample estimate and need not grow from one minibatch to the next: the learning rate is the
    first of STOP_LRS under which that minibatch's approx_kl is a new maximum, so that a bound below it stops nothing earlier"""
    pol, opts, kl = STOP_CASES[case]()
    at = PER_EPOCH + 1
    for lr in STOP_LRS:
        opts = dict(opts, lr=lr)
        probe = _solo(amd, pol, opts, dict(minibatch_samples=MB), kl)
        kls = _drive_shuffled(probe, 2)
        probe.close()
        print(f"lr {lr}: approx_kl per minibatch:", " ".join(f"{k:.4e}" for k in kls))
        if kls[at] > max(kls[:at]) and kls[at] > 0:
            return pol, opts, kl, dict(minibatch_samples=MB, target_kl=_target_stopping_at(kls, at))
    raise AssertionError("under no learning rate of STOP_LRS is approx_kl of the second epoch's second minibatch a new maximum: change the inputs")


@pytest.mark.parametrize("case", list(STOP_CASES))
def test_the_early_stop_in_the_second_epoch(amd, case):
    """the host-driven update stops in the second epoch after one step of it and before its last minibatch; the queued one stops
    there too: steps_taken, minibatches_evaluated and epochs_begun are the same, and so is everything else.  Under the rllib_ppo
    preset's loss (KL penalty 1.0 adaptive to 0.01, value clip 10, clip range 0.5, vf_coef 2) with the free log_std and with two
    heads: the KL statistics and the adapted coefficient too"""
    pol, opts, kl, sh = _stop_case(amd, case)
    host, queued = _pair(amd, lambda: _solo(amd, pol, opts, sh, kl), shuffle=True, kl=kl is not None)
    assert host["shuffle"] == dict(epochs_begun=2, minibatches_evaluated=PER_EPOCH + 2, steps_taken=PER_EPOCH + 1, stopped=1), host["shuffle"]
    assert host["state"]["steps"] == PER_EPOCH + 1 and host["stats"]["samples"] == MB
    for k in ("steps_taken", "minibatches_evaluated", "epochs_begun"):
        assert queued["shuffle"][k] == host["shuffle"][k], k
    _assert_same(queued, host)


# ---- 5. a population: one member never stops, two stop at different minibatches ------------------------------------------------------
POP_CFG = (dict(lr=2e-3, vf_coef=1.0), dict(lr=3e-3, eps_clip=0.1), dict(lr=4e-3, normalize_advantages=False, reward_scale=0.05))
POP_SEEDS = (5, 6, 7)


def test_a_population_whose_members_stop_at_different_minibatches(amd):
    """M = 3 with per-member seeds, learning rates and target_kl: member 0 never stops, members 1 and 2 stop at two different
    minibatches (asserted on the host-driven population).  All three members equal the host-driven population's, and member 0
    also a solo engine of its env block under the host-driven update"""
    M = 3
    pols = [_policy(20 + m) for m in range(M)]
    opts_m = [P.options(**c) for c in POP_CFG]
    free = [dict(minibatch_samples=MB, seed=s) for s in POP_SEEDS]
    probe = _population(amd, pols, opts_m, free)
    kls = _drive_shuffled(probe, EPOCHS, population=True)
    probe.close()
    for m in range(M):
        print(f"member {m} approx_kl per minibatch:", " ".join(f"{k:.4e}" for k in kls[m]))

    def new_maxima(k):
        return [i for i in range(1, len(k)) if k[i] > max(k[:i]) and k[i] > 0]
    assert new_maxima(kls[1]) and set(new_maxima(kls[2])) - {new_maxima(kls[1])[-1]}, "approx_kl rises to new maxima in members 1 and 2"
    at1 = new_maxima(kls[1])[-1]
    at2 = next(i for i in new_maxima(kls[2]) if i != at1)
    shuffle_m = [free[0], dict(free[1], target_kl=_target_stopping_at(kls[1], at1)), dict(free[2], target_kl=_target_stopping_at(kls[2], at2))]
    host, queued = _pair(amd, lambda: _population(amd, pols, opts_m, shuffle_m), members=M, shuffle=True)
    sst = host["shuffle"]
    print("host-driven:", sst)
    assert sst[0] == dict(epochs_begun=EPOCHS, minibatches_evaluated=EPOCHS * PER_EPOCH, steps_taken=EPOCHS * PER_EPOCH, stopped=0)
    for m, at in ((1, at1), (2, at2)):
        assert sst[m] == dict(epochs_begun=at // PER_EPOCH + 1, minibatches_evaluated=at + 1, steps_taken=at, stopped=1), (m, at)
    assert sst[1]["minibatches_evaluated"] != sst[2]["minibatches_evaluated"]
    assert [s["steps"] for s in host["state"]] == [s["steps_taken"] for s in sst]
    _assert_same(queued, host)
    # member 0 alone: its env block, its configuration, its shuffle seed
    solo = _solo(amd, pols[0], opts_m[0], shuffle_m[0], planes=_planes(M * N)[:, :N])
    alone = _snapshot(solo, solo.pg_update(EPOCHS), shuffle=True, act=False)
    solo.close()
    _assert_same(queued["state"][0], alone["state"], "member 0 against a solo engine")
    _assert_same(queued["shuffle"][0], alone["shuffle"])
    _assert_same({k: queued["stats"][0][k] for k in P.STAT_KEYS}, {k: alone["stats"][k] for k in P.STAT_KEYS})


# ---- 6. A2C ----------------------------------------------------------------------------------------------------------------------------
def test_a2c(amd):
    """one epoch, no surrogate clip, one minibatch of all 20 samples, un-normalised advantages"""
    from adcraft_amd.baselines import pg_trainer
    cfg = pg_trainer.a2c(lr=3e-2)
    epochs, minibatches = cfg.pop("epochs"), cfg.pop("minibatches")
    assert (epochs, minibatches, cfg["eps_clip"]) == (1, 1, 0.0)
    pol = _policy(16)
    host, queued = _pair(amd, lambda: _solo(amd, pol, P.options(**cfg)), epochs=epochs)
    assert host["state"]["steps"] == 1 and host["stats"]["samples"] == T * N
    _assert_same(queued, host)


# ---- 7. resume -------------------------------------------------------------------------------------------------------------------------
def test_a_saved_state_resumes_a_queued_run(amd):
    """a queued update, pg_state out and into a fresh engine over the same record, a second queued update: two consecutive
    host-driven updates (the second epoch's ticks continue from the restored step count)"""
    pol = _policy(17)
    opts, sh = P.options(lr=3e-3, vf_coef=1.0), dict(minibatch_samples=MB)
    a = _solo(amd, pol, opts, sh)
    a.pg_update(2)
    ref = _snapshot(a, a.pg_update(2), shuffle=True)
    a.close()
    b = _solo(amd, pol, opts, sh)
    b.pg_update(2, queued=True)
    saved = b.pg_state()
    b.close()
    assert saved["steps"] == 2 * PER_EPOCH
    c = _solo(amd, pol, opts, sh)
    c.pg_state(saved)
    got = _snapshot(c, c.pg_update(2, queued=True), shuffle=True)
    c.close()
    assert ref["state"]["steps"] == 4 * PER_EPOCH
    _assert_same(got, ref)


# ---- 8. alternation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["env-blocks", "stop"])
def test_host_driven_and_queued_updates_alternate(amd, case):
    """a host-driven update then a queued one on the same engine, and the reverse, each equal to two host-driven updates: the
    device's control blocks (stopped, the steps taken) start anew with every call.  With env blocks all twelve steps are taken;
    under the stop the first update stops in its second epoch and the second one - the policy has moved from the record's - at
    a minibatch of its own"""
    if case == "stop":
        pol, opts, kl, sh = _stop_case(amd, "plain")
    else:
        pol, opts, kl, sh = _policy(18), P.options(lr=3e-2, vf_coef=1.0, minibatch_envs=2, max_grad_norm=0.05), None, None
    out = []
    for order in ((False, False), (False, True), (True, False), (True, True)):
        e = _solo(amd, pol, opts, sh, kl)
        first = e.pg_update(EPOCHS, queued=order[0])
        first_sh = e.pg_shuffle_stats() if sh else None
        snap = _snapshot(e, e.pg_update(EPOCHS, queued=order[1]), shuffle=sh is not None)
        snap["first"], snap["first_shuffle"] = first, first_sh
        out.append(snap)
        e.close()
    if case == "stop":
        assert out[0]["first_shuffle"]["stopped"] == 1 and out[0]["first_shuffle"]["steps_taken"] == PER_EPOCH + 1
    else:
        assert out[0]["state"]["steps"] == 12
    for got in out[1:]:
        _assert_same(got, out[0])


# ---- 9. a PBT round between two updates --------------------------------------------------------------------------------------------------
def test_a_pbt_round_after_a_queued_update_copies_what_it_copies_after_a_host_driven_one(amd):
    """three learners, an update, a PBT round with given fitness (the worst member becomes a copy of the best: weights, moments,
    step count, a perturbed learning rate), a second update: host-driven and queued end alike, the round's plan and
    hyperparameters included - the copied member's ticks and step constants continue from the donor's step count"""
    M = 3
    pols = [_policy(30 + m) for m in range(M)]
    opts_m = [P.options(**c) for c in POP_CFG]
    shuffle_m = [dict(minibatch_samples=MB, seed=s) for s in POP_SEEDS]
    out = []
    for queued in (False, True):
        e = _population(amd, pols, opts_m, shuffle_m)
        e.pbt_init("pg", replace_count=1, tuned=("lr",), bounds=dict(lr=(1e-5, 1e-1)), seed=3)
        e.pg_pop_update(1, queued=queued)
        plan = e.pbt_step(fitness=[1.0, 3.0, 2.0])
        snap = _snapshot(e, e.pg_pop_update(2, queued=queued), M, shuffle=True)
        snap["plan"] = plan
        out.append(snap)
        e.close()
    assert list(out[0]["plan"]["src"]) == [1, -1, -1]
    assert [s["steps"] for s in out[0]["state"]] == [3 * PER_EPOCH] * M
    _assert_same(out[1], out[0])
