"""The running reward normaliser on the host: the twins adc_rew_norm_host and adc_pg_gae_norm_host (the code the device kernels
run, adc_rew_norm.h) against the numpy restatement tests/rew_norm_ref.py bit for bit, the law against float64 numpy's variance of
all returns taken in one go, the configuration check and the trainers' argument validation.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from tests import pg_ref as P
from tests import rew_norm_ref as RR

F, D64 = np.float32, np.float64
SHAPES = [(3, 5), (70, 16)]             # (N, T): S = 15; S = 1120, the smallest of these that crosses a 1024-sample chunk


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _days(rng, N, T, episode=None, magnitude=50.0, first_day=0):
    """rewards of mixed sign and size; with `episode`: day t ends an episode when (first_day + t + 1) % episode == 0, terminated
    in the even envs, truncated in the odd ones"""
    reward = (rng.standard_normal((T, N)) * magnitude).astype(F)
    te, tr = np.zeros((T, N), bool), np.zeros((T, N), bool)
    if episode:
        ends = (first_day + np.arange(T) + 1) % episode == 0
        te[np.ix_(ends, np.arange(N) % 2 == 0)] = True
        tr[np.ix_(ends, np.arange(N) % 2 == 1)] = True
    return reward, te, tr


@pytest.mark.parametrize("gamma", [0.0, 0.9, 1.0])
@pytest.mark.parametrize("N,T", SHAPES)
def test_twin_equals_the_restatement_over_consecutive_updates(lib, N, T, gamma):
    """three updates: the count == 0 branch, the merge, the carry across rollouts"""
    rng = np.random.default_rng(100 * N + T)
    got = ref = RR.fresh(N)
    for i in range(3):
        days = _days(rng, N, T, magnitude=10.0 ** i)
        got, ref = RR.twin(lib, got, *days, gamma), RR.update(ref, *days, gamma)
        assert RR.same(got, ref), i
        assert got["count"] == (i + 1) * N * T and got["scale"] > 0 and np.isfinite(got["M2"])
    assert got["M2"] > 0 and (gamma == 0.0 or np.any(got["returns"] != 0))
    assert got["scale"] != F(1.0)


@pytest.mark.parametrize("N", [3, 70])
def test_episodes_end_inside_the_record(lib, N):
    """episodes of 4 days inside 10-day records: the carry is zeroed after a terminated and after a truncated day's sample"""
    rng = np.random.default_rng(N)
    got = ref = RR.fresh(N)
    for i in range(2):
        reward, te, tr = _days(rng, N, 10, episode=4, first_day=10 * i)
        assert te.any() and tr.any() and (i == 1 or not (te | tr)[-1].any()), "the first record hands a running return on"
        got, ref = RR.twin(lib, got, reward, te, tr, 0.9), RR.update(ref, reward, te, tr, 0.9)
        assert RR.same(got, ref), i
    # day 7 of the first record ended an episode: the sample of day 8 is that day's reward alone
    reward, te, tr = _days(np.random.default_rng(N), N, 10, episode=4)
    g, _ = RR.scan(reward, te | tr, 0.9, np.zeros(N))
    assert np.array_equal(g[8], reward[8].astype(D64)) and not np.array_equal(g[7], reward[7].astype(D64))
    # per-env discounts
    gammas = np.linspace(0.5, 1.0, N).astype(F)
    assert RR.same(RR.twin(lib, RR.fresh(N), reward, te, tr, gammas), RR.update(RR.fresh(N), reward, te, tr, gammas))


@pytest.mark.parametrize("cap", [1000, 100000])
def test_count_cap_below_and_above_the_running_count(lib, cap):
    rng = np.random.default_rng(cap)
    N, T = 70, 16
    got = ref = RR.fresh(N)
    for i in range(2):
        days = _days(rng, N, T)
        got, ref = RR.twin(lib, got, *days, 0.9, count_cap=cap), RR.update(ref, *days, 0.9, count_cap=cap)
        assert RR.same(got, ref), i
    assert got["count"] == min(cap, 2 * N * T)


@pytest.mark.parametrize("N,T", SHAPES)
def test_all_zero_rewards_end_at_the_floor(lib, N, T):
    z = np.zeros((T, N), F), np.zeros((T, N), bool), np.zeros((T, N), bool)
    for min_std in (1e-2, 0.3):
        got = RR.twin(lib, RR.fresh(N), *z, 0.9, min_std=min_std)
        assert RR.same(got, RR.update(RR.fresh(N), *z, 0.9, min_std=min_std))
        assert got["scale"] == F(D64(1.0) / D64(min_std)) and got["M2"] == 0.0 and got["mean"] == 0.0


@pytest.mark.parametrize("clip", [0.0, 0.75])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("N,T", SHAPES)
def test_gae_twin_equals_the_restatement(lib, N, T, normalize, clip):
    rng = np.random.default_rng(N + T)
    reward, te, tr = _days(rng, N, T, episode=4, magnitude=30.0)
    value, boot = rng.standard_normal((T, N)).astype(F), rng.standard_normal(N).astype(F)
    opts = dict(gamma=0.97, lam=0.9, reward_scale=0.5, normalize_advantages=normalize)
    for scale in (F(0.031), np.exp(rng.standard_normal(N)).astype(F) * F(0.05)):
        got = RR.twin_gae(lib, reward, te, tr, value, boot, scale, clip, **opts)
        ref = RR.gae(reward, te, tr, value, boot, scale, clip, **opts)
        for a, b in zip(got, ref):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if clip:
        r = (reward * F(0.5)) * F(0.031)
        assert (np.abs(r) > clip).any() and (np.abs(r) < clip).any(), "the clip was meant to bind on some rewards only"
        off = RR.twin_gae(lib, reward, te, tr, value, boot, F(0.031), 0.0, **opts)
        assert not np.array_equal(off[1], RR.twin_gae(lib, reward, te, tr, value, boot, F(0.031), clip, **opts)[1])


@pytest.mark.parametrize("normalize", [False, True])
def test_gae_twin_with_unit_multiplier_is_the_plain_twin(lib, normalize):
    rng = np.random.default_rng(5)
    N, T = 70, 16
    reward, te, tr = _days(rng, N, T, episode=4)
    value, boot = rng.standard_normal((T, N)).astype(F), rng.standard_normal(N).astype(F)
    opts = dict(gamma=0.99, lam=0.95, reward_scale=0.01, normalize_advantages=normalize)
    got = RR.twin_gae(lib, reward, te, tr, value, boot, F(1.0), 0.0, **opts)
    ref = P.twin_gae(lib, reward, te, tr, value, boot, **opts)
    for a, b in zip(got, ref):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_law_is_the_variance_of_the_discounted_return(lib):
    """independent standard-normal rewards, gamma 0.9, no done, 8 envs, 5 updates of 200 days, no cap: M2 / count is numpy's
    population variance of all 8000 returns taken in one go.  Both sides are float64 over 8000 values of order 1 and the merge is
    algebraically exact: 1e-9 relative is several orders above their rounding and far below any real error."""
    rng = np.random.default_rng(2024)
    N, T = 8, 200
    reward = rng.standard_normal((5 * T, N)).astype(F)
    no = np.zeros((T, N), bool)
    st = RR.fresh(N)
    for i in range(5):
        st = RR.twin(lib, st, reward[i * T:(i + 1) * T], no, no, 0.9)
    g, _ = RR.scan(reward, np.zeros((5 * T, N), bool), 0.9, np.zeros(N))
    assert st["count"] == 8000
    var = np.var(g.reshape(-1))
    assert abs(st["M2"] / D64(st["count"]) - var) <= 1e-9 * var
    assert st["scale"] == F(1.0 / np.sqrt(st["M2"] / D64(st["count"])))


def test_config_check_refusals():
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    c = StepEngine.rew_norm_config()
    assert (c.per_member, c.min_std, c.clip, c.count_cap) == (0, 1e-2, 10.0, 0) and c.struct_size == C.sizeof(_ffi.RewNormConfig) == 32
    assert StepEngine.rew_norm_config(per_member=True, clip=0.0, count_cap=5).per_member == 1
    for bad in (dict(min_std=0.0), dict(min_std=-1.0), dict(min_std=np.inf), dict(min_std=np.nan)):
        with pytest.raises(ValueError, match="min_std"):
            StepEngine.rew_norm_config(**bad)
    for bad in (dict(clip=-1.0), dict(clip=np.inf), dict(clip=np.nan)):
        with pytest.raises(ValueError, match="clip"):
            StepEngine.rew_norm_config(**bad)
    with pytest.raises(ValueError, match="count_cap"):
        StepEngine.rew_norm_config(count_cap=-1)
    msg = C.c_char_p()
    c.struct_size = 8
    assert _ffi.lib().adc_rew_norm_config_check(C.byref(c), C.byref(msg)) == _ffi.ADC_EINVAL and b"struct_size" in msg.value
    assert _ffi.lib().adc_rew_norm_config_check(None, None) == _ffi.ADC_EINVAL
    # the twins refuse a bad configuration and missing arrays
    assert _ffi.lib().adc_rew_norm_host(C.byref(c), 1, 1, None, None, None, None, None, None, None, None, None) == _ffi.ADC_EINVAL
    good = RR.config()
    assert _ffi.lib().adc_rew_norm_host(C.byref(good), 1, 1, None, None, None, None, None, None, None, None, None) == _ffi.ADC_EINVAL


def test_trainer_argument_validation():
    """the reward normaliser's options are checked before the engine is touched"""
    from adcraft_amd.baselines.pg_trainer import PGPopulationTrainer, PGTrainer
    for make in (lambda **kw: PGTrainer(None, None, 4, **kw), lambda **kw: PGPopulationTrainer(None, None, 4, dict(), **kw)):
        with pytest.raises(ValueError, match="without normalize_rewards"):
            make(rew_norm=dict(clip=5.0))
        with pytest.raises(ValueError, match="unknown option"):
            make(normalize_rewards=True, rew_norm=dict(per_member=True))
        with pytest.raises(TypeError, match="rew_norm"):
            make(normalize_rewards=True, rew_norm=5.0)
