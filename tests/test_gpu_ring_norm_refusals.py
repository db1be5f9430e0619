"""Every refusal the entry points of the two ring-normaliser families can return (parts/norm_api.inc: adc_engine_td3_norm_* and
adc_engine_sac_norm_* - init, update, state_get, state_set, returns_get, returns_set, copy), by return code and WHOLE sentence: the
sentences below are literals, copied from the source as it stood while each family had a front end of its own, so that giving the two
one body cannot reword one unseen.  tests/test_gpu_td3_norm.py and tests/test_gpu_sac_norm.py match fragments of some of them and
check what the normalisers compute; nothing is computed here.

The entry points are called through ctypes as they are (engine.py's wrappers refuse some arguments themselves).  Shapes: 4 envs x 2
keywords (D = 12, A = 3), a two-layer actor of width 8, critics (8, 1), 2 members, a 2-day record, ring capacity 8, batch 4."""
import ctypes as C
import signal

import numpy as np
import pytest

from tests import helpers as H
from tests import mlp_ref as R
from tests import sac_ref as S
from tests import td3_ref as T3

pytestmark = pytest.mark.gpu
F, D64 = np.float32, np.float64
N, K, T, B, CAP, M = 4, 2, 2, 4, 8, 2
D, A = 5 * K + 2, K + 1
HIDDEN, WIDTHS = (8,), (8, 1)
SEED, BUDGET = 43, 1000.0
OK, EINVAL, ESTATE = 0, -1, -4
FAMILIES = ("td3", "sac")

NOT_READY = {
    "td3": "adc_engine_td3_norm_init has not been called (or the TD3 trainer, the policy, the learners or the record were re-initialised since)",
    "sac": "adc_engine_sac_norm_init has not been called over a live adc_engine_sac_init / adc_engine_sac_pop_init trainer (or the trainer, the policy, the "
           "learners or the record were re-initialised since)",
}
NO_TRAINER = {
    "td3": "the TD3 normalisers belong to an off-policy trainer: adc_engine_td3_init or adc_engine_td3_pop_init first",
    "sac": "the SAC normalisers belong to a soft actor-critic trainer: adc_engine_sac_init or adc_engine_sac_pop_init first",
}
PER_MEMBER = {
    "td3": "per-member normalisers need a TD3 learner population (adc_engine_td3_pop_init)",
    "sac": "per-member normalisers need a SAC learner population (adc_engine_sac_pop_init)",
}
NOT_EMPTY = {
    "td3": "the record and the replay ring must be empty: their rows were written as network inputs (adc_engine_rollout_reset, and "
           "adc_engine_td3_norm_init before the first store)",
    "sac": "the record and the replay ring must be empty: their rows were written as network inputs (adc_engine_rollout_reset, and "
           "adc_engine_sac_norm_init before the first store)",
}
NULL_HANDLE = "engine handle is NULL"
NEITHER_PART = "observations or rewards: at least one must be nonzero"
NO_NORMALISATION = "the policy was initialised without normalisation"
NO_NEW_DAY = "no day has been recorded since the last update or adc_engine_rollout_reset"
NO_SUCH = "no such normaliser: 0 for the shared one, a member with per-member normalisers"
WITHOUT_OBS = "the normaliser was initialised without observations"
WITHOUT_REW = "the normaliser was initialised without rewards"
NULL_VECTOR = "mean, M2, shift or scale is NULL"
COUNT = "count >= 0"
SCALE = "scale must be finite and > 0"
FINITE = "shift and mean must be finite"
M2 = "M2 must be finite and >= 0"
SHARED = "the normaliser is shared by all envs: there are no members to copy between"
NULL_PLAN = "src_of_member_m is NULL"
BAD_PLAN = "src_of_member_m: a member, or the member itself / -1 to keep it"
CHAINED = "a destination is also a source: the copies of a round may not chain"
NULL_RETURNS = "g_n is NULL"


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


@pytest.fixture(autouse=True)
def time_limit(request):
    """every test under its own time limit (the handler runs when the interpreter next regains control)"""
    def expired(*_):
        raise TimeoutError(f"{request.node.name} ran longer than 60 s")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(60)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _policy(family, rng, normalize=True):
    if family == "sac":
        pol = S.sac_policy(rng, K, HIDDEN, "tanh", clamp=(-1.0, -0.5), normalize=normalize, scale=0.6)
    else:
        pol = R.random_policy(rng, K, HIDDEN, "tanh", normalize=normalize, scale=0.6)
        pol.log_std = np.full(A, np.log(0.2), F)
    if normalize:
        pol.shift, pol.scale = R.realistic_norm(K)
    return pol


def _options(family):
    if family == "sac":
        return S.options(K, critic_widths=WIDTHS, batch_size=B, capacity=CAP)
    return T3.options(critic_widths=WIDTHS, batch_size=B, capacity=CAP)


def _bounds():
    return np.concatenate([[50.0], np.full(K, 0.02)]).astype(F), np.concatenate([[1500.0], np.full(K, 3.0)]).astype(F)


def _engine(amd, family, rng, normalize=True, members=0):
    """an engine with its policy (and learners) and its record, no trainer yet"""
    planes = H.implicit_params(N, K, SEED + 1, mean_volume=24, cvr=0.5)
    e = amd.StepEngine(N, K, seed=SEED, max_days=4, auto_reset=True)
    e.set_all_params(planes)
    e.reset()
    pols = [_policy(family, rng, normalize) for _ in range(max(members, 1))]
    e.mlp_init(pols[0], deterministic=False)
    if members:
        e.mlp_learners(members)
        for m in range(1, members):
            e.mlp_set_learner(m, pols[m])
    if family == "sac":
        (e.mlp_learners_set_squash if members else e.mlp_set_squash)(*_bounds())
    e.rollout_enable(T, obs=True)
    return e


def _train(e, family, rng, members=0):
    """a fresh trainer of the family (an empty ring)"""
    crits = [T3.random_critics_for_tests(rng, K, WIDTHS) for _ in range(max(members, 1))]
    if members:
        getattr(e, f"{family}_pop_init")([_options(family)] * members)
        for m in range(members):
            getattr(e, f"{family}_pop_set_critics")(m, crits[m])
    else:
        getattr(e, f"{family}_init")(**_options(family))
        getattr(e, f"{family}_set_critics")(crits[0])


class Calls:
    """the family's entry points on an engine, as the C ABI has them; every call returns (code, adc_last_error's sentence)"""

    def __init__(self, e, family, handle="engine"):
        from adcraft_amd import _ffi
        self.lib, self.h, self.family = e._lib, (e._h if handle == "engine" else None), family
        self.config = _ffi.SACNormConfig if family == "sac" else _ffi.TD3NormConfig

    def _call(self, name, *args):
        rc = getattr(self.lib, f"adc_engine_{self.family}_norm_{name}")(self.h, *args)
        return rc, (self.lib.adc_last_error() or b"").decode() if rc != OK else None

    def init(self, observations=1, rewards=1, per_member=0, **fields):
        c = self.config()
        c.struct_size = C.sizeof(self.config)
        c.observations, c.rewards, c.per_member = observations, rewards, per_member
        c.obs_min_std, c.obs_count_cap, c.rew_min_std, c.rew_count_cap, c.rew_clip = 1e-2, 0, 1e-2, 0, 10.0
        for k, v in fields.items():
            setattr(c, k, v)
        return self._call("init", C.byref(c))

    def update(self):
        n = C.c_int64(-1)
        rc, msg = self._call("update", C.byref(n))
        return (rc, n.value) if rc == OK else (rc, msg)

    def state_get(self, member=0, obs=True, rew=True):
        n, rn, mean, m2, sc = C.c_int64(0), C.c_int64(0), C.c_double(0.0), C.c_double(0.0), C.c_float(0.0)
        vec = [np.zeros(D, t) for t in (D64, D64, F, F)]
        optr = [C.byref(n)] + [v.ctypes.data for v in vec] if obs else [None] * 5
        rptr = [C.byref(rn), C.byref(mean), C.byref(m2), C.byref(sc)] if rew else [None] * 4
        return self._call("state_get", member, *optr, *rptr)

    def state_set(self, member=0, obs_count=5, mean=0.0, m2=1.0, shift=0.0, scale=1.0, rew_count=5, rew_mean=0.0, rew_m2=1.0, rew_scale=1.0, null=None):
        vec = dict(mean=np.full(D, mean, D64), m2=np.full(D, m2, D64), shift=np.full(D, shift, F), scale=np.full(D, scale, F))
        ptr = [None if k == null else v.ctypes.data for k, v in vec.items()]
        return self._call("state_set", member, obs_count, *ptr, rew_count, rew_mean, rew_m2, rew_scale)

    def returns_get(self, null=False):
        g = np.zeros(N, D64)
        return self._call("returns_get", None if null else g.ctypes.data)

    def returns_set(self, null=False):
        g = np.zeros(N, D64)
        return self._call("returns_set", None if null else g.ctypes.data)

    def copy(self, src):
        a = None if src is None else np.ascontiguousarray(src, dtype=np.int32)
        return self._call("copy", None if a is None else a.ctypes.data)

    def all_but_init(self):
        return dict(update=self.update, state_get=self.state_get, state_set=self.state_set, returns_get=self.returns_get, returns_set=self.returns_set,
                    copy=lambda: self.copy([-1]))


# ---- 1. before an init, and what an init refuses ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_a_null_handle_and_a_family_not_initialised(amd, family):
    rng = np.random.default_rng(201)
    e = _engine(amd, family, rng)
    nul, c = Calls(e, family, handle=None), Calls(e, family)
    assert nul.init() == (EINVAL, NULL_HANDLE)
    for name, call in nul.all_but_init().items():
        assert call() == (EINVAL, NULL_HANDLE), name
    for name, call in c.all_but_init().items():                    # no trainer, no normaliser
        assert call() == (ESTATE, NOT_READY[family]), name
    _train(e, family, rng)
    for name, call in c.all_but_init().items():                    # a trainer, no normaliser
        assert call() == (ESTATE, NOT_READY[family]), name
    # the other family's normaliser is not this one's: its entry points still say not initialised
    other = "td3" if family == "sac" else "sac"
    assert c.init() == (OK, None)
    for name, call in Calls(e, other).all_but_init().items():
        assert call() == (ESTATE, NOT_READY[other]), name
    assert Calls(e, other).init() == (ESTATE, NO_TRAINER[other])
    e.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_what_an_init_refuses(amd, family):
    rng = np.random.default_rng(202)
    e = _engine(amd, family, rng)
    c = Calls(e, family)
    assert c.init(observations=0, rewards=0) == (EINVAL, NEITHER_PART)            # (the configuration's own check comes first)
    assert c.init() == (ESTATE, NO_TRAINER[family])
    _train(e, family, rng)
    assert c.init(observations=0, rewards=0) == (EINVAL, NEITHER_PART)
    assert c.init(obs_min_std=0.0) == (EINVAL, "obs_min_std must be finite and > 0")
    assert c.init(per_member=1) == (EINVAL, PER_MEMBER[family])
    e.run_days("mlp", 1, BUDGET)
    assert c.init() == (ESTATE, NOT_EMPTY[family])                                # a record begun
    getattr(e, f"{family}_store")()
    e.rollout_reset()
    assert c.init() == (ESTATE, NOT_EMPTY[family])                                # a ring begun
    assert c.init(per_member=1) == (EINVAL, PER_MEMBER[family])                   # (per_member is asked before the ring)
    for name, call in c.all_but_init().items():                                   # a refused init leaves no normaliser behind
        assert call() == (ESTATE, NOT_READY[family]), name
    _train(e, family, rng)
    assert c.init() == (OK, None)                                                 # the engine is usable after every refusal
    e.run_days("mlp", T, BUDGET)
    getattr(e, f"{family}_store")()
    assert c.update() == (OK, T * N)
    e.close()
    # a policy without normalisation: its observations cannot be normalised, its rewards can
    p = _engine(amd, family, rng, normalize=False)
    _train(p, family, rng)
    c = Calls(p, family)
    assert c.init() == (EINVAL, NO_NORMALISATION)
    assert c.init(rewards=0) == (EINVAL, NO_NORMALISATION)
    assert c.init(observations=0) == (OK, None)
    p.close()


# ---- 2. a live normaliser -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_what_a_live_shared_normaliser_refuses(amd, family):
    rng = np.random.default_rng(203)
    e = _engine(amd, family, rng)
    _train(e, family, rng)
    c = Calls(e, family)
    assert c.init() == (OK, None)
    assert c.update() == (ESTATE, NO_NEW_DAY)
    for member in (1, -1):
        assert c.state_get(member) == (EINVAL, NO_SUCH)
        assert c.state_set(member) == (EINVAL, NO_SUCH)
    # the strict checks of a set: the observation part first, vector by vector, then the reward part; nothing is written
    inf, nan = np.inf, np.nan
    for null in ("mean", "m2", "shift", "scale"):
        assert c.state_set(null=null) == (EINVAL, NULL_VECTOR), null
    assert c.state_set(obs_count=-1) == (EINVAL, COUNT)
    for bad in (0.0, -1.0, inf, nan):
        assert c.state_set(scale=bad) == (EINVAL, SCALE), bad
        assert c.state_set(rew_scale=bad) == (EINVAL, SCALE), bad
    for bad in (inf, -inf, nan):
        assert c.state_set(shift=bad) == (EINVAL, FINITE), bad
        assert c.state_set(mean=bad) == (EINVAL, FINITE), bad
        assert c.state_set(rew_mean=bad) == (EINVAL, FINITE), bad
    for bad in (-1.0, inf, nan):
        assert c.state_set(m2=bad) == (EINVAL, M2), bad
        assert c.state_set(rew_m2=bad) == (EINVAL, M2), bad
    assert c.state_set(rew_count=-1) == (EINVAL, COUNT)
    assert c.state_set(scale=0.0, mean=nan, m2=-1.0) == (EINVAL, SCALE)            # (a column's scale before its moments)
    assert c.state_set(m2=-1.0, rew_scale=0.0) == (EINVAL, M2)                     # (the observation part before the reward part)
    assert c.state_set(null="scale", obs_count=-1) == (EINVAL, NULL_VECTOR)
    assert c.copy([-1]) == (ESTATE, SHARED)
    assert c.copy(None) == (ESTATE, SHARED)                                        # (shared is asked before the plan)
    assert c.returns_get(null=True) == (EINVAL, NULL_RETURNS)
    assert c.returns_set(null=True) == (EINVAL, NULL_RETURNS)
    # usable after every refusal, and the refused sets wrote nothing
    assert c.state_get() == (OK, None) and c.state_set() == (OK, None) and c.returns_get() == (OK, None) and c.returns_set() == (OK, None)
    e.run_days("mlp", T, BUDGET)
    getattr(e, f"{family}_store")()
    assert c.update() == (OK, T * N)
    assert c.update() == (ESTATE, NO_NEW_DAY)
    e.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_what_a_normaliser_of_one_part_refuses(amd, family):
    rng = np.random.default_rng(204)
    e = _engine(amd, family, rng)
    _train(e, family, rng)
    c = Calls(e, family)
    assert c.init(observations=0) == (OK, None)                                    # rewards alone
    assert c.state_get() == (ESTATE, WITHOUT_OBS)
    assert c.state_get(obs=False) == (OK, None)
    assert c.state_set(scale=0.0, null="mean") == (OK, None)                       # (the part that is not there is not checked)
    assert c.state_set(rew_scale=0.0) == (EINVAL, SCALE)
    assert c.returns_get() == (OK, None)
    assert c.init(rewards=0) == (OK, None)                                         # observations alone (a second init starts over)
    assert c.state_get() == (ESTATE, WITHOUT_REW)
    assert c.state_get(rew=False) == (OK, None)
    assert c.state_set(rew_scale=0.0) == (OK, None)
    assert c.state_set(scale=0.0) == (EINVAL, SCALE)
    assert c.returns_get() == (ESTATE, WITHOUT_REW)
    assert c.returns_set() == (ESTATE, WITHOUT_REW)
    assert c.returns_get(null=True) == (ESTATE, WITHOUT_REW)                       # (the part is asked before the pointer)
    assert c.state_get(1) == (EINVAL, NO_SUCH)                                     # (the member before the parts)
    e.close()


# ---- 3. a population's normalisers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_what_a_population_refuses(amd, family):
    rng = np.random.default_rng(205)
    e = _engine(amd, family, rng, members=M)
    c = Calls(e, family)
    assert c.init(per_member=1) == (ESTATE, NO_TRAINER[family])
    _train(e, family, rng, members=M)
    assert c.init() == (OK, None)                                                  # one normaliser shared by the members
    assert c.copy([-1, -1]) == (ESTATE, SHARED)
    assert c.state_get(1) == (EINVAL, NO_SUCH)
    assert c.init(per_member=1) == (OK, None)
    assert c.state_get(1) == (OK, None)
    for member in (M, -1):
        assert c.state_get(member) == (EINVAL, NO_SUCH)
        assert c.state_set(member) == (EINVAL, NO_SUCH)
    assert c.state_set(1, m2=-1.0) == (EINVAL, M2)
    assert c.copy(None) == (EINVAL, NULL_PLAN)
    for plan in ([M, -1], [-1, -2], [0, M]):
        assert c.copy(plan) == (EINVAL, BAD_PLAN), plan
    assert c.copy([1, 0]) == (EINVAL, CHAINED)
    assert c.copy([M, 0]) == (EINVAL, BAD_PLAN)                                    # (every entry is checked before the chains)
    assert c.update() == (ESTATE, NO_NEW_DAY)
    for plan in ([-1, -1], [0, 1], [1, -1], [0, 0]):
        assert c.copy(plan) == (OK, None), plan
    e.run_days("mlp", T, BUDGET)
    getattr(e, f"{family}_pop_store")()
    assert c.update() == (OK, T * (N // M))
    # the normalisers end with the learners
    e.mlp_learners(M)
    for name, call in c.all_but_init().items():
        assert call() == (ESTATE, NOT_READY[family]), name
    e.close()
