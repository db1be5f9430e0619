"""Imitation learning on the host: the twins adc_im_weight_host / adc_im_grad_host (the code the device kernel runs,
adc_imitation.h) against the numpy restatement in tests/im_ref.py bit for bit - gradient, pieces' sums, ma, c, w - the exported
symbols, the configuration check, and that cloning a constant action raises its log-probability.  No device is needed."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import im_ref as I
from tests import mlp_ref as R
from tests import pg_ref as P

F = np.float32
NEW_SYMBOLS = ("adc_engine_teach_days", "adc_im_config_check", "adc_engine_im_init", "adc_engine_im_advantages", "adc_engine_im_minibatch",
               "adc_engine_im_update", "adc_engine_im_state_get", "adc_engine_im_state_set", "adc_im_weight_host", "adc_im_grad_host")


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_the_new_symbols_are_exported_and_the_abi_is_unchanged(lib):
    from adcraft_amd import _ffi
    header = (Path(__file__).resolve().parents[1] / "include" / "adcraft_engine.h").read_text()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
        assert re.search(rf"\bint {name}\(", header), name
    assert lib.adc_abi_version() == 5 and lib.adc_stream_revision() == 5
    assert (_ffi.ABI_VERSION, _ffi.STREAM_REVISION) == (5, 5)
    assert C.sizeof(_ffi.IMConfig) == 40 and C.sizeof(_ffi.IMStats) == 72


@pytest.mark.parametrize("kw", [dict(beta=-0.1), dict(beta=float("inf")), dict(vf_coef=-1.0), dict(w_max=-1.0), dict(ma_start=-1.0),
                                dict(ma_rate=1.5), dict(ma_rate=float("nan"))])
def test_the_configuration_check_refuses(kw):
    with pytest.raises(ValueError):
        I.im_config(**kw)


def _policy(rng, act, hidden, two, value, clamp, K):
    pol = R.random_policy(rng, K, hidden, activation=act, two_heads=two, value=value, log_std_clamp=clamp)
    if len(pol.value_layers) > 0 and len(hidden) > 1:        # (a value network of another depth than the policy's)
        pol.value_layers = R.random_policy(rng, K, hidden[:1], activation=act, value=True).value_layers
    if clamp is not None and not two:                        # (a free log_std inside the bounds, but for ONE component below them)
        ls = np.linspace(clamp[0] + 0.1, clamp[1] - 0.1, K + 1).astype(F)
        ls[1] = F(clamp[0] - 0.5)
        pol.log_std = ls
    return pol


def _batch(rng, policy, S, adv_scale):
    """S teacher samples: network inputs, the teacher's actions (near the policy's means, so that logp stays finite), advantages
    wide enough that exp(beta adv / c) is capped for some and not for others"""
    K = policy.num_keywords
    obs = (rng.standard_normal((S, 5 * K + 2)) * 0.7).astype(F)
    theta = P.flat_params(policy)
    action = (rng.standard_normal((S, K + 1)) * 1.5).astype(F)
    adv = (rng.standard_normal(S) * adv_scale).astype(F)
    ret = (rng.standard_normal(S) * 2).astype(F)
    value_old = (ret - adv).astype(F)
    return theta, obs, action, adv, ret, value_old


# activation, hidden, two heads, value network, clamp, K, samples, imitation options
CASES = [
    ("tanh", (13, 8), False, True, None, 2, 1040, dict(beta=0.7, ma_rate=0.01)),
    ("relu", (), True, True, (-1.5, 0.0), 10, 300, dict(beta=0.7, vf_coef=0.5, w_max=3.0)),
    ("tanh", (), False, False, (-1.2, -0.2), 2, 64, dict(beta=0.0, train_log_std=False)),
    ("relu", (13, 8), True, False, None, 10, 1040, dict(beta=0.0, vf_coef=0.0)),
    ("tanh", (13, 8), False, True, (-1.0, 0.5), 10, 257, dict(beta=0.7, train_log_std=False, w_max=1.5, ma_start=40.0)),
    ("relu", (13, 8), False, True, (-1.0, 0.5), 2, 130, dict(beta=0.7, w_max=0.0)),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_weight_and_grad_twins_equal_the_restatement_bit_for_bit(lib, case):
    act, hidden, two, value, clamp, K, S, kw = CASES[case]
    rng = np.random.default_rng(500 + case)
    pol = _policy(rng, act, hidden, two, value, clamp, K)
    im = I.im_options(**kw)
    theta, obs, action, adv, ret, value_old = _batch(rng, pol, S, adv_scale=30.0)
    # the moving scale and the weights, two calls in a row (the second starts from the first's ma)
    ma_t, ma_r = im["ma_start"], im["ma_start"]
    for _ in range(2):
        ma_t, c_t, w_t = I.twin_weight(lib, ma_t, adv, **im)
        ma_r, c_r = I.scale(ma_r, adv, **im)
        w_r = I.weight(adv, c_r, **im)
        assert _same(np.float64(ma_t), np.float64(ma_r)) and _same(F(c_t), F(c_r)) and _same(w_t, w_r)
    assert ma_t != im["ma_start"] or im["ma_rate"] == 0
    if im["beta"] == 0:
        assert np.all(w_t == 1)
    elif im["w_max"] > 0:
        assert (w_t == F(im["w_max"])).any() and (w_t < F(im["w_max"])).any(), "the case was meant to cap some weights and not others"
    else:
        assert w_t.max() > 20
    g, sums, st = I.twin_grad(lib, pol, theta, obs, action, adv, ret, value_old, c_t, **im)
    rg, rsums, rst = I.grad(pol, theta, obs, action, adv, ret, value_old, c_r, **im)
    assert _same(g, rg)
    assert _same(sums, rsums)
    for k in I.STAT_KEYS:
        assert _same(np.float64(st[k]), np.float64(rst[k])), k
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    assert _same(np.float64(st["weight"]), np.float64(P.csum(w_r.astype(np.float64)) / np.float64(S)))
    # what the cases claim to cover
    if not two:
        gls = g[-(K + 1):]
        if not im["train_log_std"]:
            assert np.all(gls == 0)
        elif clamp is not None:
            ls = P.unflatten(pol, theta)[2]
            moved = (ls < clamp[0]) | (ls > clamp[1])
            assert moved.sum() == 1 and np.all(gls[moved] == 0) and np.all(gls[~moved] != 0)
        else:
            assert np.all(gls != 0)
    if two and clamp is not None:
        raw = R.network(obs, P.unflatten(pol, theta)[0], pol.activation)[:, K + 1:]
        moved = (raw < F(clamp[0])) | (raw > F(clamp[1]))
        assert moved.any() and not moved.all()
    if not value or im["vf_coef"] == 0:
        nv = sum(w.size + b.size for w, b in pol.value_layers)
        npol = sum(w.size + b.size for w, b in pol.layers)
        assert np.all(g[npol:npol + nv] == 0)


def test_behaviour_cloning_with_unit_scale_is_a_squared_error(lib):
    """log_std = 0, beta = 0, train_log_std = 0: the policy loss is 0.5 |a - mean|^2 + A * 0.5 log(2 pi), the mean's delta mean - a"""
    rng = np.random.default_rng(9)
    K, S = 3, 50
    pol = R.random_policy(rng, K, (), activation="tanh", value=False)
    pol.log_std = np.zeros(K + 1, F)
    theta, obs, action, adv, ret, value_old = _batch(rng, pol, S, 1.0)
    g, sums, st = I.twin_grad(lib, pol, theta, obs, action, adv, ret, value_old, F(10.0), beta=0.0, vf_coef=0.0, train_log_std=False)
    w, b = P.unflatten(pol, theta)[0][0]
    mean = obs.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
    err = action.astype(np.float64) - mean
    loss = (0.5 * (err ** 2).sum(axis=1) + (K + 1) * 0.5 * np.log(2 * np.pi)).mean()
    assert abs(st["policy_loss"] - loss) <= 1e-5 * abs(loss)
    gb = (-err).mean(axis=0)
    assert np.allclose(g[w.size:w.size + b.size], gb, rtol=1e-4, atol=1e-6)


# the cloning run of tests/test_gpu_imitation.py, on the host: a constant teacher action, log_std = 0 left untrained, Adam; the
# learning rate and the seed are those of the GPU test
CLONE = dict(seed=77, lr=0.05, updates=30, budget=3.0, bid=1.25)


def clone_policy(K):
    rng = np.random.default_rng(CLONE["seed"])
    pol = R.random_policy(rng, K, (8,), "tanh", value=True, normalize=True, scale=0.6)
    pol.shift, pol.scale = R.realistic_norm(K)
    pol.log_std = np.zeros(K + 1, F)
    return pol


def test_cloning_a_constant_action_raises_its_log_probability(lib):
    K, S = 5, 24
    rng = np.random.default_rng(CLONE["seed"] + 1)
    pol = clone_policy(K)
    obs = (rng.standard_normal((S, 5 * K + 2)) * 0.7).astype(F)
    action = np.tile(np.concatenate([[CLONE["budget"]], np.full(K, CLONE["bid"])]).astype(F), (S, 1))
    zeros = np.zeros(S, F)
    opts = P.options(lr=CLONE["lr"])
    im = I.im_options(beta=0.0, vf_coef=0.0, train_log_std=False)
    theta = P.flat_params(pol)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    logps = []
    for step in range(CLONE["updates"] + 1):
        g, _, st = I.twin_grad(lib, pol, theta, obs, action, zeros, zeros, zeros, F(10.0), **im)
        rg, _, rst = I.grad(pol, theta, obs, action, zeros, zeros, zeros, F(10.0), **im)
        assert _same(g, rg)
        logps.append(rst["logp"])
        theta, m, v = P.step(theta, m, v, rg, step, **opts)
    assert logps[-1] > logps[0], logps
    assert np.array_equal(theta[-(K + 1):], np.zeros(K + 1, F)), "log_std was not to be trained"
