"""The TD3 learners' running normalisers on the host: the twins adc_td3_norm_obs_host / adc_td3_norm_rew_host /
adc_td3_y_norm_host (the code the device kernels run, adc_td3_norm.h) against the numpy restatement tests/td3_norm_ref.py bit for
bit, the configuration check, the exported symbols and the trainers' argument validation.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from tests import td3_norm_ref as TN
from tests import td3_ref as T3

F, D64 = np.float32, np.float64
D = 17


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _rows(rng, S, constant_column=None):
    """raw observation rows: columns of very different size and offset, as counts, dollars and a running profit are"""
    x = (rng.standard_normal((S, D)) * (10.0 ** rng.integers(-2, 4, D)) + rng.standard_normal(D) * 100.0).astype(F)
    if constant_column is not None:
        x[:, constant_column] = F(3.25)
    return x


def _days(rng, N, T, episode=None, magnitude=50.0):
    reward = (rng.standard_normal((T, N)) * magnitude).astype(F)
    te, tr = np.zeros((T, N), bool), np.zeros((T, N), bool)
    if episode:
        ends = (np.arange(T) + 1) % episode == 0
        te[np.ix_(ends, np.arange(N) % 2 == 0)] = True
        tr[np.ix_(ends, np.arange(N) % 2 == 1)] = True
    return reward, te, tr


@pytest.mark.parametrize("S", [1, 1088])        # one sample; more than one 1024-sample chunk
def test_obs_twin_equals_the_restatement_over_three_merged_batches(lib, S):
    rng = np.random.default_rng(S)
    got = ref = TN.obs_fresh(D, shift=rng.standard_normal(D), scale=np.exp(rng.standard_normal(D)))
    for i in range(3):
        x = _rows(rng, S)
        got, ref = TN.twin_obs(lib, got, x), TN.obs_update(ref, x)
        assert TN.obs_same(got, ref), i
        assert got["count"] == (i + 1) * S
    # raw rows: the first batch's mean is the rows' own, whatever vectors were in force (no back-conversion)
    x = _rows(rng, S)
    one = TN.twin_obs(lib, TN.obs_fresh(D, shift=np.full(D, 7.0), scale=np.full(D, 0.125)), x)
    assert TN.obs_same(one, TN.twin_obs(lib, TN.obs_fresh(D), x))
    assert np.allclose(one["mean"], x.astype(D64).mean(axis=0), rtol=1e-12, atol=0)     # (float64 sums of at most 1088 float32 values)


def test_obs_count_cap_bites(lib):
    rng = np.random.default_rng(7)
    got = ref = TN.obs_fresh(D)
    for i in range(3):
        x = _rows(rng, 1088)
        got, ref = TN.twin_obs(lib, got, x, count_cap=1500), TN.obs_update(ref, x, count_cap=1500)
        assert TN.obs_same(got, ref), i
    assert got["count"] == 1500
    assert not TN.obs_same(got, TN.twin_obs(lib, TN.twin_obs(lib, TN.twin_obs(lib, TN.obs_fresh(D), x), x), x))


def test_obs_column_that_never_varies(lib):
    rng = np.random.default_rng(9)
    got = ref = TN.obs_fresh(D)
    for i in range(2):
        x = _rows(rng, 1088, constant_column=5)
        got, ref = TN.twin_obs(lib, got, x, min_std=0.05), TN.obs_update(ref, x, min_std=0.05)
        assert TN.obs_same(got, ref), i
    assert got["scale"][5] == F(D64(1.0) / D64(0.05)) and got["shift"][5] == F(3.25) and got["M2"][5] == 0.0


@pytest.mark.parametrize("N,T", [(1, 1), (64, 17)])       # S = 1; S = 1088
@pytest.mark.parametrize("gamma", [0.0, 0.9, 1.0])
def test_rew_twin_equals_the_restatement_over_three_merged_batches(lib, N, T, gamma):
    rng = np.random.default_rng(100 * N + T)
    got = ref = TN.rew_fresh(N)
    for i in range(3):
        days = _days(rng, N, T, magnitude=10.0 ** i)
        got, ref = TN.twin_rew(lib, got, *days, gamma), TN.rew_update(ref, *days, gamma)
        assert TN.rew_same(got, ref), i
    assert got["count"] == 3 * N * T


def test_rew_count_cap_all_zero_rewards_and_episode_ends(lib):
    rng = np.random.default_rng(3)
    N, T = 64, 17
    got = ref = TN.rew_fresh(N)
    for i in range(2):
        days = _days(rng, N, T)
        got, ref = TN.twin_rew(lib, got, *days, 0.9, count_cap=1500), TN.rew_update(ref, *days, 0.9, count_cap=1500)
        assert TN.rew_same(got, ref), i
    assert got["count"] == 1500
    z = np.zeros((T, N), F), np.zeros((T, N), bool), np.zeros((T, N), bool)
    got = TN.twin_rew(lib, TN.rew_fresh(N), *z, 0.9, min_std=0.3)
    assert TN.rew_same(got, TN.rew_update(TN.rew_fresh(N), *z, 0.9, min_std=0.3))
    assert got["scale"] == F(D64(1.0) / D64(0.3)) and got["M2"] == 0.0
    # an episode end resets the carry: the sample after it is that day's reward alone; per-env discounts (a population's members')
    reward, te, tr = _days(rng, N, T, episode=4)
    gammas = np.repeat(np.array([0.5, 0.9, 0.99, 1.0], F), N // 4)
    got, ref = TN.twin_rew(lib, TN.rew_fresh(N), reward, te, tr, gammas), TN.rew_update(TN.rew_fresh(N), reward, te, tr, gammas)
    assert TN.rew_same(got, ref)
    from tests import rew_norm_ref as RR
    g, carry = RR.scan(reward, te | tr, gammas, np.zeros(N))
    assert np.array_equal(g[4], reward[4].astype(D64)) and not np.array_equal(g[3], reward[3].astype(D64))
    assert np.array_equal(got["returns"], carry) and (T % 4 == 0 or np.any(carry != 0))


def _y_inputs(rng, n=4096):
    r = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 5, n)).astype(F)
    q = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 5, n)).astype(F)
    done = rng.integers(0, 2, n).astype(bool)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], F)
    r[:special.size], q[special.size:2 * special.size] = special, special
    r[2 * special.size:3 * special.size], q[2 * special.size:3 * special.size] = special, special[::-1]
    return r, done, q


def test_y_norm_with_unit_multiplier_and_no_clip_is_td3_y(lib):
    rng = np.random.default_rng(11)
    r, done, q = _y_inputs(rng)
    for gamma, rs in ((0.99, 1.0), (0.9, 0.01), (0.0, -2.5)):
        got = TN.twin_y(lib, r, done, q, gamma, rs, 1.0, 0.0)
        assert np.array_equal(got.view(np.uint32), TN.y_plain(r, done, q, gamma, rs).view(np.uint32))
        assert np.array_equal(got.view(np.uint32), TN.y_norm(r, done, q, gamma, rs, 1.0, 0.0).view(np.uint32))
    assert np.isnan(got).any() and (got == 0).any()


@pytest.mark.parametrize("clip", [0.0, 0.75])
def test_y_norm_twin_equals_the_restatement(lib, clip):
    rng = np.random.default_rng(12)
    r, done, q = _y_inputs(rng)
    for scale in (F(0.031), F(3.7)):
        got, ref = TN.twin_y(lib, r, done, q, 0.97, 0.5, scale, clip), TN.y_norm(r, done, q, 0.97, 0.5, scale, clip)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    if clip:
        rs = (r * F(0.5)) * F(0.031)
        assert (np.abs(rs) > clip).any() and (np.abs(rs) < clip).any(), "the clip was meant to bind on some rewards only"
        nan = np.isnan(r)
        assert nan.any() and np.isnan(got[nan]).all(), "a NaN reward passes the clip"


def test_config_check_messages():
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    c = StepEngine.td3_norm_config(observations=True)
    assert (c.observations, c.rewards, c.per_member, c.obs_min_std, c.obs_count_cap, c.rew_min_std, c.rew_count_cap, c.rew_clip) == (1, 0, 0, 1e-2, 0, 1e-2, 0, 10.0)
    assert c.struct_size == C.sizeof(_ffi.TD3NormConfig) == 56
    assert StepEngine.td3_norm_config(rewards=True, per_member=True, rew_clip=0.0).per_member == 1
    with pytest.raises(ValueError, match="observations or rewards"):
        StepEngine.td3_norm_config()
    for key in ("obs_min_std", "rew_min_std"):
        for bad in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(ValueError, match=key):
                StepEngine.td3_norm_config(observations=True, **{key: bad})
    for key in ("obs_count_cap", "rew_count_cap"):
        with pytest.raises(ValueError, match=key):
            StepEngine.td3_norm_config(rewards=True, **{key: -1})
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="rew_clip"):
            StepEngine.td3_norm_config(rewards=True, rew_clip=bad)
    msg = C.c_char_p()
    c.struct_size = 8
    assert _ffi.lib().adc_td3_norm_config_check(C.byref(c), C.byref(msg)) == _ffi.ADC_EINVAL and b"struct_size" in msg.value
    assert _ffi.lib().adc_td3_norm_config_check(None, None) == _ffi.ADC_EINVAL
    # the twins refuse a bad configuration and missing arrays
    good = TN.config()
    assert _ffi.lib().adc_td3_norm_obs_host(C.byref(c), 1, 1, None, None, None, None, None, None) == _ffi.ADC_EINVAL
    assert _ffi.lib().adc_td3_norm_obs_host(C.byref(good), 1, 1, None, None, None, None, None, None) == _ffi.ADC_EINVAL
    assert _ffi.lib().adc_td3_norm_rew_host(C.byref(good), 1, 1, None, None, None, None, None, None, None, None, None) == _ffi.ADC_EINVAL
    assert _ffi.lib().adc_td3_y_norm_host(None, 1, None, None, None, 1.0, 0.0, None) == _ffi.ADC_EINVAL


def test_new_symbols_are_exported(lib):
    for name in ("adc_td3_norm_config_check", "adc_engine_td3_norm_init", "adc_engine_td3_norm_update", "adc_engine_td3_norm_state_get",
                 "adc_engine_td3_norm_state_set", "adc_engine_td3_norm_returns_get", "adc_engine_td3_norm_returns_set", "adc_engine_td3_norm_copy",
                 "adc_td3_norm_obs_host", "adc_td3_norm_rew_host", "adc_td3_y_norm_host"):
        assert hasattr(lib, name), name
    from adcraft_amd.engine import StepEngine
    for name in ("td3_norm_config", "td3_norm_init", "td3_norm_update", "td3_norm_state", "td3_norm_returns", "td3_norm_copy"):
        assert callable(getattr(StepEngine, name)), name


def test_trainer_argument_validation():
    """the normalisers' options are checked before the engine is touched"""
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer, TD3Trainer

    class NoVectors:
        shift = scale = None
        log_std = np.zeros(4, F)

    for make in (lambda pol=None, **kw: TD3Trainer(None, pol, **kw), lambda pol=None, **kw: TD3PopulationTrainer(None, pol, 0.1, dict(), **kw)):
        with pytest.raises(ValueError, match="norm given without"):
            make(norm=dict(rew_clip=5.0))
        with pytest.raises(ValueError, match="unknown option"):
            make(normalize_rewards=True, norm=dict(per_member=True))
        with pytest.raises(TypeError, match="norm"):
            make(normalize_observations=True, norm=5.0)
        with pytest.raises(ValueError, match="normalisation vectors"):
            make(NoVectors(), normalize_observations=True)
