"""GPU parity of the recurrent policy (MLPPolicy(gru=...); csrc/adc_gru.h, parts/kernel_mlp_gru.inc) with the host twin
adc_mlp_act_recurrent_host under the state rule restated in tests/gru_ref.py: the act and the state through auto-resets, a repeated
day, days without the agent, explicit resets, a resumed state, a population against single-policy engines, one generation of the
evolution strategy over the longer flat vector, the feed-forward policy through the new entry point, and the refusals.  Every
comparison is bitwise.  None of the entry points exists before this feature."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests import es_ref as E
from tests import gru_ref as G
from tests import helpers as H
from tests import mlp_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
SEED, BUDGET = 47, 1000.0
RESETS = dict(max_days=3, auto_reset=True)
LAST = ("mean", "log_std", "action", "logp", "value")


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


def _policy(rng, K, hidden, width, act="tanh", two=False, value=True, normalize=True):
    pol = G.random_policy(rng, K, hidden, width, act, two_heads=two, value=value, normalize=normalize, scale=0.6 if normalize else 0.05)
    if normalize:
        pol.shift, pol.scale = R.realistic_norm(K)
    pol.layers[-1][1][1:K + 1] += F(0.3)                           # bids around 80 cents: auctions are won
    return pol


class Twin:
    """the host twin under the restated state rule, env by env, alongside an engine"""

    def __init__(self, lib, e, seeds):
        self.lib, self.e = lib, e
        self.state = [G.State(e.mlp_gru_width()) for _ in range(e.num_envs)]
        self.keys = [R.agent_key(s) for s in seeds]
        self.tick = 0

    def act(self, pols, z=None, deterministic=False, commit=True):
        """what an act of the engine must give now (pols: one policy, or one per env); commit: the state rule moves, the tick too"""
        e = self.e
        day = e.get_episode_state()[0].astype(np.int64)
        x = R.flat_obs(e.fetch()).astype(F)
        out = {k: [] for k in LAST + ("h",)}
        self.zeros = []
        for n in range(e.num_envs):
            pol = pols[n] if isinstance(pols, (list, tuple)) else pols
            d = int(day[n])
            frm, h_in = self.state[n].begin(d)
            self.zeros.append(frm == d)
            t = G.twin_act(self.lib, pol, None if d == 0 else x[n], h_in, None if z is None else z[n], self.keys[n], self.tick, deterministic, BUDGET)
            if commit:
                self.state[n].commit(d, frm, t["h"][0])
            for k in out:
                out[k].append(t[k][0])
        if commit:
            self.tick += 1
        return {k: np.stack(v) for k, v in out.items()}

    def hidden(self):
        return {"h": np.stack([s.h for s in self.state]), "last": np.array([s.last for s in self.state], np.int32),
                "from": np.array([s.frm for s in self.state], np.int32)}


def _assert_hidden(e, twin, what=""):
    st, ref = e.mlp_hidden_state(), twin.hidden()
    for k in ("h", "last", "from"):
        assert _same(st[k], ref[k]), (k, what, st[k], ref[k])


def _assert_last(e, ref, what=""):
    st = e.mlp_last()
    for k in LAST:
        assert _same(st[k], ref[k]), (k, what, st[k], ref[k])


# (N, K, trunk, G): D = 17 with a trunk; D = 37 without one, Wh a block of 32 and a tail, 3G = 99 gate rows; the LDS maximum; the
# deepest trunk there is (the flat order's six terms), the cell's input in the second activation buffer; A = 257 > 256, where the
# head loop makes a second pass: two heads (514 outputs) with a value network next to them, and no trunk with a free log_std, where
# Wi reads the input row of 1282 floats (40 blocks of 32 and a tail of 2)
SHAPES = [(8, 3, (5,), 3), (4, 7, (), 33), (2, 2, (256,), 256), (4, 3, (6, 7, 5), 4), (2, 256, (31,), 33), (2, 256, (), 5)]
VALUE_TOO = (4,)                                                       # (the shapes whose two-headed variants have a value network too)
# activation, deterministic, two-headed log-std
VARIANTS = [(a, d, t) for a in ("tanh", "relu") for d in (False, True) for t in (False, True)]
CASES = [(0, v) for v in range(len(VARIANTS))] + [(1, 0), (2, 5), (3, 0), (4, 5), (5, 0)]


# ---- 1. the act and the state, day by day ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", CASES)
def test_act_and_state_equal_the_twin_over_auto_resets(amd, lib, shape, variant):
    """7 days of mlp_step with max_days = 3: two auto-resets fall inside.  After every day the last act's means, log-stds, actions,
    log-probability and value, the state h[N][2][G] and the words last / from are the twin's, bit for bit"""
    from adcraft_amd.baselines.es_trainer import flat_params
    N, K, hidden, width = SHAPES[shape]
    act, det, two = VARIANTS[variant]
    rng = np.random.default_rng(100 * shape + variant)
    pol = _policy(rng, K, hidden, width, act, two, value=variant % 2 == 0 or shape in VALUE_TOO, normalize=variant % 3 != 1)
    assert shape < 4 or (K + 1 > 256 and (shape == 4) == (two and bool(pol.value_layers)) and (shape == 5) == (pol.log_std is not None))
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    e = _engine(amd, _planes(N, K), **RESETS)
    e.mlp_init(pol, seeds, deterministic=det)
    assert e.mlp_gru_width() == width and e.mlp_frames() == 1
    assert _same(e.mlp_params(), flat_params(pol))
    twin = Twin(lib, e, seeds)
    _assert_hidden(e, twin, "before any act")
    e.rollout_enable(7)
    started = 0
    for t in range(7):
        ref = twin.act(pol, deterministic=det)
        started += int(np.sum(twin.zeros))
        e.mlp_step(BUDGET)
        _assert_last(e, ref, (shape, variant, t))
        _assert_hidden(e, twin, (shape, variant, t))
    assert started == 3 * N, "every env starts from zeros on days 0, 3 and 6"
    assert np.abs(twin.hidden()["h"]).sum() > 0
    rec = e.rollout_fetch()
    st = e.mlp_last()
    assert _same(rec["action"][6], st["action"]) and _same(rec["logp"][6], st["logp"]) and _same(rec["value"][6], st["value"])
    e.close()


# ---- 2. a second act on the same day ----------------------------------------------------------------------------------------------------
def test_a_repeated_act_reads_the_same_state_and_writes_the_same_bits(amd, lib):
    N, K, hidden, width = SHAPES[0]
    rng = np.random.default_rng(2)
    pol = _policy(rng, K, hidden, width)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    e = _engine(amd, _planes(N, K), **RESETS)
    e.mlp_init(pol, seeds, deterministic=False)
    twin = Twin(lib, e, seeds)
    for t in range(2):                                             # day 0 (from zeros) and day 1 (from a state)
        z = R.normals(twin.keys, [twin.tick] * N, K + 1)
        ref = twin.act(pol)
        e.mlp_act(BUDGET)
        first, hidden = e.mlp_last(), e.mlp_hidden_state()
        _assert_last(e, ref, t)
        e.mlp_act(BUDGET, replay_normals=z)
        _assert_last(e, first, (t, "again"))
        again = e.mlp_hidden_state()
        assert all(_same(hidden[k], again[k]) for k in hidden)
        _assert_hidden(e, twin, t)
        twin.tick += 1                                             # (the second act moved the agents' streams on as any act does)
        e.step_device()
    e.close()


# ---- 3. days without the agent, explicit resets ---------------------------------------------------------------------------------------
def test_days_without_the_agent_and_explicit_resets_start_from_zeros(amd, lib):
    N, K, hidden, width = SHAPES[0]
    rng = np.random.default_rng(3)
    pol = _policy(rng, K, hidden, width)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    e = _engine(amd, _planes(N, K), max_days=1 << 20, loss_threshold=1e12)
    e.mlp_init(pol, seeds, deterministic=True)
    twin = Twin(lib, e, seeds)

    def day(expect_zeros, what):
        ref = twin.act(pol, deterministic=True)
        assert list(twin.zeros) == list(expect_zeros), (what, twin.zeros)
        e.mlp_step(BUDGET)
        _assert_last(e, ref, what)
        _assert_hidden(e, twin, what)

    day([True] * N, "day 0")
    day([False] * N, "day 1")
    e.run_days("fixed", 2, BUDGET)                                 # days 2 and 3 pass without the agent
    day([True] * N, "day 4, after the gap")
    day([False] * N, "day 5")
    mask = np.arange(N) % 2 == 0
    before = e.mlp_hidden_state()
    e.reset(env_mask=mask)
    after = e.mlp_hidden_state()
    assert (after["last"][mask] == G.NONE).all() and _same(after["last"][~mask], before["last"][~mask]) and _same(after["h"], before["h"])
    for n in np.flatnonzero(mask):
        twin.state[n].forget()
    day(list(mask), "after the reset of every other env")
    day([False] * N, "the day after")
    e.mlp_hidden_forget()
    for s in twin.state:
        s.forget()
    day([True] * N, "after the forget")
    e.close()


# ---- 4. the state to the host and back --------------------------------------------------------------------------------------------------
def test_a_run_resumed_from_the_fetched_state_continues_bit_for_bit(amd):
    N, K, hidden, width = SHAPES[0]
    rng = np.random.default_rng(4)
    pol = _policy(rng, K, hidden, width)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    runs = []
    for resumed in (False, True, None):
        e = _engine(amd, _planes(N, K), max_days=1 << 20, loss_threshold=1e12)
        e.mlp_init(pol, seeds, deterministic=False)
        e.run_days("mlp", 3, BUDGET)
        if resumed is not False:
            # a new engine at the same env and agent state; its own hidden state is thrown away, then (resumed) the first run's put back
            assert all(_same(runs[0][0][k], v) for k, v in e.mlp_hidden_state().items())
            junk = {"h": np.full((N, 2, width), 0.25, F), "last": np.full(N, 2, np.int32), "from": np.zeros(N, np.int32)}
            e.mlp_set_hidden_state(junk)
            if resumed:
                e.mlp_set_hidden_state(runs[0][0])
        state = e.mlp_hidden_state()
        e.rollout_enable(3)
        e.run_days("mlp", 3, BUDGET)
        runs.append((state, e.rollout_fetch(), e.mlp_hidden_state()))
        e.close()
    (_, ra, ha), (_, rb, hb), (_, rc, _) = runs
    for k in ra:
        assert _same(ra[k], rb[k]), k
    assert all(_same(ha[k], hb[k]) for k in ha)
    assert not _same(ra["action"], rc["action"]), "the hidden state matters to the run"


# ---- 4b. env groups ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [0, 4])
def test_env_groups_give_the_same_record_and_state(amd, members):
    """the chained days run as env groups on their own streams: the state's pointers move with a group's first env"""
    N, K, hidden, width = SHAPES[0]
    T = 7
    rng = np.random.default_rng(40)
    pol = _policy(rng, K, hidden, width)
    seeds = np.arange(N, dtype=np.uint64) + 1
    out = []
    for groups in (1, 4):
        e = _engine(amd, _planes(N, K), **RESETS)
        e.set_env_groups(groups)
        e.mlp_init(pol, seeds, deterministic=False)
        if members:
            e.mlp_population(members)
            e.es_init(sigma=0.1, seed=5)
            e.es_perturb()
        e.rollout_enable(T, obs=True)
        e.run_days("mlp", T, BUDGET)
        assert e.env_groups() == groups
        out.append((e.rollout_fetch(bootstrap=True), e.mlp_hidden_state()))
        e.close()
    (ra, ha), (rb, hb) = out
    for k in ra:
        assert _same(ra[k], rb[k]), k
    for k in ha:
        assert _same(ha[k], hb[k]), k
    assert len({tuple(r) for r in ha["h"].reshape(N, -1)}) == N


# ---- 5. a population ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [(5,), (6, 7, 5)])
def test_a_members_envs_equal_a_single_policy_engine(amd, hidden):
    """4 members x 2 envs over 5 recorded days with auto-resets: each member's rows of the record and of the state are those of a
    single-policy engine of 2 envs at that env base under that member's parameters"""
    from adcraft_amd.baselines.es_trainer import flat_params, policy_from_flat
    M, n, K, width, T = 4, 2, 3, 3, 5
    N = M * n
    rng = np.random.default_rng(5)
    centre = _policy(rng, K, hidden, width)
    mem = [policy_from_flat(centre, flat_params(centre) + (rng.standard_normal(flat_params(centre).size) * 0.2).astype(F)) for _ in range(M)]
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    planes = _planes(N, K)
    e = _engine(amd, planes, **RESETS)
    e.mlp_init(centre, seeds, deterministic=False)
    e.mlp_population(M)
    for m in range(M):
        assert _same(e.mlp_member_params(m), flat_params(centre))
        e.mlp_set_member(m, mem[m])
        assert _same(e.mlp_member_params(m), flat_params(mem[m]))
    assert _same(e.mlp_params(), flat_params(centre))
    e.rollout_enable(T, obs=True)
    e.run_days("mlp", T, BUDGET)
    rec, hid = e.rollout_fetch(), e.mlp_hidden_state()
    e.close()
    for m in range(M):
        s = _engine(amd, planes[:, m * n:(m + 1) * n], env_id_base=m * n, **RESETS)
        s.mlp_init(mem[m], seeds[m * n:(m + 1) * n], deterministic=False)
        s.rollout_enable(T, obs=True)
        s.run_days("mlp", T, BUDGET)
        want, wh = s.rollout_fetch(), s.mlp_hidden_state()
        s.close()
        for k in ("obs", "action", "logp", "value", "reward"):
            assert _same(rec[k][:, m * n:(m + 1) * n], want[k]), (m, k)
        for k in wh:
            assert _same(hid[k][m * n:(m + 1) * n], wh[k]), (m, k)
    assert not _same(rec["action"][:, :n], rec["action"][:, n:2 * n])


# ---- 6. one generation of the evolution strategy ---------------------------------------------------------------------------------------
def test_one_es_generation_over_the_longer_flat_vector(amd, lib):
    """8 members x 2 envs: the members after the perturbation, every env's state forgotten by it, theta and both moments after the
    update (restatement and host twin), the centre rebuilt"""
    from adcraft_amd.baselines.es_trainer import flat_params, policy_from_flat
    M, n, K, hidden, width = 8, 2, 3, (5,), 3
    N = M * n
    kw = dict(sigma=0.05, lr=0.02, seed=99)
    rng = np.random.default_rng(6)
    pol = _policy(rng, K, hidden, width)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    e = _engine(amd, _planes(N, K), **RESETS)
    e.mlp_init(pol, seeds, deterministic=True)
    e.mlp_population(M)
    e.es_init(**kw)
    theta = flat_params(pol)
    P = theta.size
    assert P == e.mlp_param_count() == (5 * K + 2 + 1) * 5 + (5 + 1) * 9 + (3 + 1) * 9 + (3 + 1) * (K + 1)
    assert _same(e.es_state()["theta"], theta)
    e.mlp_step(BUDGET)                                             # every env has a state
    assert (e.mlp_hidden_state()["last"] == 0).all()
    e.es_perturb()
    assert (e.mlp_hidden_state()["last"] == G.NONE).all()
    ref_members = E.members(theta, kw["seed"], 0, M, kw["sigma"])
    for m in range(M):
        assert _same(e.mlp_member_params(m), ref_members[m]), m
    # a member acts on its own perturbed cell: env 0 against the twin under member 0's parameters, from zeros on day 1
    twin = Twin(lib, e, seeds)
    twin.tick = 1
    ref = twin.act([policy_from_flat(pol, ref_members[i // n]) for i in range(N)], deterministic=True)
    assert all(twin.zeros)
    e.mlp_step(BUDGET)
    _assert_last(e, ref, "members")
    st, want = e.mlp_hidden_state(), twin.hidden()                 # (slot 0 still holds what day 0 wrote: forgetting moves `last` alone)
    assert _same(st["h"][:, 1], want["h"][:, 1]) and _same(st["last"], want["last"]) and _same(st["from"], want["from"])
    e.run_days("mlp", 2, BUDGET)
    fit = e.es_fitness()
    e.es_update()
    zero = np.zeros(P, F)
    t1, m1, v1, _ = E.update(theta, zero, zero, fit, kw["seed"], 0, sigma=kw["sigma"], lr=kw["lr"])
    tt, mt, vt, _ = E.twin_update(lib, theta, zero, zero, fit, kw["seed"], 0, sigma=kw["sigma"], lr=kw["lr"])
    st = e.es_state()
    for got, a, b in ((st["theta"], t1, tt), (st["m"], m1, mt), (st["v"], v1, vt)):
        assert _same(got, a) and _same(got, b)
    assert st["generation"] == 1 and _same(e.mlp_params(), t1) and not _same(t1, theta)
    e.close()


# ---- 7. the feed-forward policy through the new entry point -------------------------------------------------------------------------
def test_width_zero_through_the_new_entry_point_is_mlp_init(amd):
    from adcraft_amd._ffi import check
    N, K, T = 5, 7, 6
    rng = np.random.default_rng(7)
    pol = R.random_policy(rng, K, (16, 8), "tanh", value=True, normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(K)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    out = []
    for new in (False, True):
        e = _engine(amd, _planes(N, K), **RESETS)
        if new:
            cfg = pol.config(K, False)
            check(e._lib.adc_engine_mlp_init_recurrent(e._h, C.byref(cfg), seeds.ctypes.data, 0))
            e._mlp, e._frames, e._members, e._learners = pol, 1, 0, 0
            e.mlp_set_weights(pol)
        else:
            e.mlp_init(pol, seeds, deterministic=False)
        assert e.mlp_gru_width() == 0 and e.mlp_hidden_state() is None
        e.rollout_enable(T, obs=True)
        e.run_days("mlp", T, BUDGET)
        out.append((e.rollout_fetch(bootstrap=True), e.mlp_last(), e.mlp_agent_state(), e.get_rng_state(), e.mlp_params()))
        e.close()
    (ra, la, aa, sa, pa), (rb, lb, ab, sb, pb) = out
    for k in ra:
        assert _same(ra[k], rb[k]), k
    for k in la:
        assert _same(la[k], lb[k]), k
    assert all(_same(x, y) for x, y in zip(aa + sa, ab + sb)) and _same(pa, pb)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_as_it_was(amd, lib):
    """what a recurrent policy does not go together with returns ADC_ESTATE with a sentence; widths and shapes that cannot be,
    ADC_EINVAL; the state calls on a feed-forward policy, ADC_ESTATE.  The engine's next days are the twin's as if nothing had
    been asked"""
    from adcraft_amd import _ffi
    N, K, hidden, width = SHAPES[0]
    A = K + 1
    rng = np.random.default_rng(8)
    pol = _policy(rng, K, hidden, width)
    seeds = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    e = _engine(amd, _planes(N, K), **RESETS)
    L, h = e._lib, e._h
    cfg = pol.config(K, True)
    for bad in (-1, 257):
        assert L.adc_engine_mlp_init_recurrent(h, C.byref(cfg), None, bad) == _ffi.ADC_EINVAL
    assert b"gru_width" in L.adc_last_error()
    g = C.c_int32(-1)
    assert L.adc_engine_mlp_gru_width(h, C.byref(g)) == _ffi.ADC_ESTATE           # (no policy yet)
    e.mlp_init(pol, seeds, deterministic=True)
    e.rollout_enable(4)
    twin = Twin(lib, e, seeds)
    ref = twin.act(pol, deterministic=True)
    e.mlp_step(BUDGET)
    _assert_last(e, ref, "day 0")
    lo, hi = np.full(A, 0.02, F), np.full(A, 3.0, F)
    refused = [("squash", lambda: L.adc_engine_mlp_set_squash(h, lo.ctypes.data, hi.ctypes.data)),
               ("bounded", lambda: L.adc_engine_mlp_set_bounds(h, lo.ctypes.data, hi.ctypes.data)),
               ("learners", lambda: L.adc_engine_mlp_learners(h, 2)),
               ("policy-gradient", lambda: L.adc_engine_pg_init(h, C.byref(e.pg_config()))),
               ("off-policy", lambda: L.adc_engine_td3_init(h, C.byref(e.td3_config()))),
               ("soft actor-critic", lambda: L.adc_engine_sac_init(h, C.byref(e.sac_config(num_keywords=K)))),
               ("imitation", lambda: L.adc_engine_im_init(h, C.byref(e.im_config()))),
               ("teacher", lambda: L.adc_engine_teach_days(h, 0, 1, BUDGET)),
               ("DAgger", lambda: L.adc_engine_dagger_days(h, 0, 1, BUDGET, 0.5))]
    for word, call in refused:
        assert call() == _ffi.ADC_ESTATE, word
        msg = L.adc_last_error()
        assert b"recurrent" in msg and word.encode() in msg, (word, msg)
    with pytest.raises(_ffi.EngineStateError):
        e.pg_advantages()                                          # (no trainer came to be)
    for t in range(2):
        ref = twin.act(pol, deterministic=True)
        e.mlp_step(BUDGET)
        _assert_last(e, ref, ("after the refusals", t))
        _assert_hidden(e, twin, ("after the refusals", t))
    # the state's words are checked on their way in
    bad_last = np.full(N, -3, np.int32)
    assert L.adc_engine_mlp_hidden_set(h, None, bad_last.ctypes.data, None) == _ffi.ADC_EINVAL
    _assert_hidden(e, twin, "after a refused set")
    # a feed-forward policy has no state to move and no cell to set
    ff = R.random_policy(rng, K, (4,), "tanh")
    e.mlp_init(ff, seeds)
    assert e.mlp_gru_width() == 0
    for call in (lambda: L.adc_engine_mlp_hidden_forget(h), lambda: L.adc_engine_mlp_hidden_get(h, None, None, None),
                 lambda: L.adc_engine_mlp_set_gru(h, *(a.ctypes.data for a in pol.gru))):
        assert call() == _ffi.ADC_ESTATE and b"not recurrent" in L.adc_last_error()
    e.mlp_set_squash(lo, hi)                                       # (and is refused nothing)
    e.mlp_step(BUDGET)
    e.close()
