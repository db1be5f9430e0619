"""The SAC learners' running normalisers on the host: the twin adc_sac_y_norm_host (the code the device kernels run,
adc_sac_norm.h) against the numpy restatement tests/sac_norm_ref.py bit for bit, the plain SAC target's bits at scale 1 / clip 0
(against the restatement and against the existing twin adc_sac_target_host), the configuration check, the exported symbols and the
trainers' argument validation.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from tests import sac_norm_ref as SN
from tests import sac_ref as S
from tests import td3_ref as T3

F, D64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _y_inputs(rng, n=4096):
    r = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 5, n)).astype(F)
    q = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 5, n)).astype(F)
    lp = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)).astype(F)
    done = rng.integers(0, 2, n).astype(bool)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], F)
    r[:special.size], q[special.size:2 * special.size] = special, special
    r[2 * special.size:3 * special.size], q[2 * special.size:3 * special.size] = special, special[::-1]
    lp[3 * special.size:4 * special.size] = special
    return r, done, q, lp


def _same(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


def test_y_norm_with_unit_multiplier_and_no_clip_is_sac_y(lib):
    rng = np.random.default_rng(21)
    r, done, q, lp = _y_inputs(rng)
    assert done.any() and not done.all()
    for gamma, rs, alpha in ((0.99, 1.0, 1.0), (0.9, 0.01, 0.2), (0.0, 2.5, 0.0), (1.0, 1.0, 37.5)):
        got = SN.twin_y(lib, r, done, q, alpha, lp, gamma, rs, 1.0, 0.0)
        assert _same(got, SN.y_plain(r, done, q, alpha, lp, gamma, rs))
        assert _same(got, SN.y_norm(r, done, q, alpha, lp, gamma, rs, 1.0, 0.0))
    assert np.isnan(got).any() and np.isfinite(got).any()


def test_y_norm_with_unit_multiplier_is_the_sac_target_twin(lib):
    """through the networks: adc_sac_target_host's y equals sac_y_norm(scale 1, clip 0) of the q and lp the restatement computes"""
    rng = np.random.default_rng(22)
    K, B = 3, 16
    policy = S.sac_policy(rng, K, (8,))
    opts = S.options(K, critic_widths=(8, 8, 1), batch_size=B, capacity=64, gamma=0.97, reward_scale=0.5)
    critics = T3.random_critics_for_tests(rng, K, (8, 8, 1))
    st = S.fresh_state(policy, critics, opts)
    sh = T3.Shapes(policy, opts)
    x2 = rng.standard_normal((B, sh.D)).astype(F)
    r = (rng.standard_normal(B) * 30.0).astype(F)
    done = rng.integers(0, 2, B).astype(bool)
    alpha = F(0.37)
    y_twin, lp_twin = S.twin_target(lib, policy, st["theta"], st["psi_target"], alpha, 5, 3, x2, r, done, opts)
    y_ref, lp_ref, q_ref = SN.target(sh, policy.log_std_clamp, st["theta"], st["psi_target"], alpha, 5, 3, x2, r, done, opts, F(1.0), 0.0)
    assert _same(lp_twin, lp_ref) and _same(y_twin, y_ref)
    assert _same(SN.twin_y(lib, r, done, q_ref, alpha, lp_ref, 0.97, 0.5, 1.0, 0.0), y_twin)
    # ... and a multiplier and a clip move it
    assert not _same(SN.twin_y(lib, r, done, q_ref, alpha, lp_ref, 0.97, 0.5, 0.25, 1.0), y_twin)


@pytest.mark.parametrize("clip", [0.0, 0.75])
def test_y_norm_twin_equals_the_restatement(lib, clip):
    rng = np.random.default_rng(23)
    r, done, q, lp = _y_inputs(rng)
    for scale, alpha in ((F(0.031), F(0.2)), (F(3.7), F(1.5))):
        got, ref = SN.twin_y(lib, r, done, q, alpha, lp, 0.97, 0.5, scale, clip), SN.y_norm(r, done, q, alpha, lp, 0.97, 0.5, scale, clip)
        assert _same(got, ref)
    if clip:
        rs = (r * F(0.5)) * F(0.031)
        assert (np.abs(rs) > clip).any() and (np.abs(rs) < clip).any(), "the clip was meant to bind on some rewards only"
        nan = np.isnan(r)
        got = SN.twin_y(lib, r, done, q, 0.2, lp, 0.97, 0.5, 0.031, clip)
        assert nan.any() and np.isnan(got[nan]).all(), "a NaN reward passes the clip"


def test_entropy_term_is_not_scaled(lib):
    """y(scale) - y(1) is the reward's change alone: with r = 0 the multiplier moves nothing"""
    rng = np.random.default_rng(24)
    _, done, q, lp = _y_inputs(rng, 512)
    zero = np.zeros(512, F)
    assert _same(SN.twin_y(lib, zero, done, q, 0.7, lp, 0.99, 1.0, 0.01, 0.0), SN.twin_y(lib, zero, done, q, 0.7, lp, 0.99, 1.0, 1.0, 0.0))


def test_config_check_messages():
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    c = StepEngine.sac_norm_config(observations=True)
    assert (c.observations, c.rewards, c.per_member, c.obs_min_std, c.obs_count_cap, c.rew_min_std, c.rew_count_cap, c.rew_clip) == (1, 0, 0, 1e-2, 0, 1e-2, 0, 10.0)
    assert c.struct_size == C.sizeof(_ffi.SACNormConfig) == 56
    assert StepEngine.sac_norm_config(rewards=True, per_member=True, rew_clip=0.0).per_member == 1
    with pytest.raises(ValueError, match="observations or rewards"):
        StepEngine.sac_norm_config()
    for key in ("obs_min_std", "rew_min_std"):
        for bad in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(ValueError, match=key):
                StepEngine.sac_norm_config(observations=True, **{key: bad})
    for key in ("obs_count_cap", "rew_count_cap"):
        with pytest.raises(ValueError, match=key):
            StepEngine.sac_norm_config(rewards=True, **{key: -1})
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="rew_clip"):
            StepEngine.sac_norm_config(rewards=True, rew_clip=bad)
    msg = C.c_char_p()
    c.struct_size = 8
    assert _ffi.lib().adc_sac_norm_config_check(C.byref(c), C.byref(msg)) == _ffi.ADC_EINVAL and b"struct_size" in msg.value
    assert _ffi.lib().adc_sac_norm_config_check(None, None) == _ffi.ADC_EINVAL
    # the twin refuses a missing configuration, missing arrays and a negative clip
    L, one = _ffi.lib(), np.zeros(1, F)
    good = S.sac_config(3, **S.options(3))
    p = one.ctypes.data
    assert L.adc_sac_y_norm_host(None, 1, p, p, p, p, 1.0, 1.0, 0.0, p) == _ffi.ADC_EINVAL
    assert L.adc_sac_y_norm_host(C.byref(good), 1, None, None, None, None, 1.0, 1.0, 0.0, None) == _ffi.ADC_EINVAL
    assert L.adc_sac_y_norm_host(C.byref(good), 0, p, p, p, p, 1.0, 1.0, 0.0, p) == _ffi.ADC_EINVAL
    assert L.adc_sac_y_norm_host(C.byref(good), 1, p, p, p, p, 1.0, 1.0, -1.0, p) == _ffi.ADC_EINVAL


def test_new_symbols_are_exported(lib):
    for name in ("adc_sac_norm_config_check", "adc_engine_sac_norm_init", "adc_engine_sac_norm_update", "adc_engine_sac_norm_state_get",
                 "adc_engine_sac_norm_state_set", "adc_engine_sac_norm_returns_get", "adc_engine_sac_norm_returns_set", "adc_engine_sac_norm_copy",
                 "adc_sac_y_norm_host"):
        assert hasattr(lib, name), name
    from adcraft_amd.engine import StepEngine
    for name in ("sac_norm_config", "sac_norm_init", "sac_norm_update", "sac_norm_state", "sac_norm_returns", "sac_norm_copy"):
        assert callable(getattr(StepEngine, name)), name


def test_trainer_argument_validation():
    """the normalisers' options are checked before the engine is touched"""
    from adcraft_amd.baselines.sac_trainer import SACPopulationTrainer, SACTrainer

    class NoVectors:
        shift = scale = None
        num_keywords = 3

    for make in (lambda pol=None, **kw: SACTrainer(None, pol, 0.0, 1.0, **kw), lambda pol=None, **kw: SACPopulationTrainer(None, pol, dict(), 0.0, 1.0, **kw)):
        with pytest.raises(ValueError, match="norm given without"):
            make(norm=dict(rew_clip=5.0))
        with pytest.raises(ValueError, match="unknown option"):
            make(normalize_rewards=True, norm=dict(per_member=True))
        with pytest.raises(TypeError, match="norm"):
            make(normalize_observations=True, norm=5.0)
        with pytest.raises(ValueError, match="normalisation vectors"):
            make(NoVectors(), normalize_observations=True)
    # the solo trainer takes the options as keywords too, but not both ways at once
    with pytest.raises(ValueError, match="norm given without"):
        SACTrainer(None, None, 0.0, 1.0, rew_clip=5.0)
    with pytest.raises(ValueError, match="not both"):
        SACTrainer(None, None, 0.0, 1.0, normalize_rewards=True, rew_clip=5.0, norm=dict(rew_clip=5.0))
