"""Imitation learning on the host: the twins adc_im_weight_host / adc_im_grad_host (the code the device kernel runs,
adc_imitation.h) against the numpy restatement in tests/im_ref.py bit for bit - gradient, pieces' sums, ma, c, w - the exported
symbols, the configuration check, and that cloning a constant action raises its log-probability; the gradient against PyTorch
float64 autograd of the loss written out on its own (the yardstick of tests/learner_shapes.py, at small shapes and at W1-W3), and
the returns against a plain discounted sum per sample.  No device is needed.  Measured figures: profiles/pr_imitation_shapes.txt."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import im_ref as I
from tests import learner_shapes as W
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


# ---- the gradient against PyTorch autograd --------------------------------------------------------------------------------------------
def _torch_im_grad(pol, theta, obs, action, adv, ret, c, dtype, im):
    """the imitation loss in PyTorch from the same arrays - per sample -(w.detach() * logp) + vf_coef * 0.5 (V - ret)^2, their mean -
    and its flat gradient by autograd in `dtype`.  The forward pass, the clamp, logp and the flat order are
    tests/test_pg_host.py::_torch_grad's; w = 1 under behaviour cloning, else min(exp(beta adv / c), w_max); no entropy term; with
    train_log_std off the log-stds are detached, a free vector's and a head's alike"""
    import torch
    layers, value_layers, log_std = P.unflatten(pol, theta)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    params = []

    def net(ls):
        out = []
        for w, b in ls:
            out.append((t(w).requires_grad_(), t(b).requires_grad_()))
            params.extend(out[-1])
        return out
    pl, vl = net(layers), net(value_layers)
    actf = torch.tanh if pol.activation == "tanh" else torch.relu

    def forward(ls, x):
        for i, (w, b) in enumerate(ls):
            x = x @ w + b
            if i + 1 < len(ls):
                x = actf(x)
        return x
    x, A = t(obs), pol.num_keywords + 1
    o = forward(pl, x)
    if log_std is not None:
        raw = t(log_std).requires_grad_()
        params.append(raw)
        mean, ls = o, raw.expand_as(o)
    else:
        mean, ls = o[:, :A], o[:, A:]
    if pol.log_std_clamp is not None:
        ls = torch.clamp(ls, float(F(pol.log_std_clamp[0])), float(F(pol.log_std_clamp[1])))
    if not im["train_log_std"]:
        ls = ls.detach()
    z = (t(action) - mean) / torch.exp(ls)
    logp = (-0.5 * z * z - ls).sum(dim=1) - A * 0.5 * np.log(2 * np.pi)
    if im["beta"] == 0:
        w = torch.ones_like(logp)
    else:
        w = torch.exp(float(F(im["beta"])) * t(adv) / float(F(c)))
        if im["w_max"] > 0:
            w = torch.clamp(w, max=float(F(im["w_max"])))
    loss = -(w.detach() * logp).mean()
    if vl:
        V = forward(vl, x)[:, 0]
        loss = loss + float(F(im["vf_coef"])) * (0.5 * (V - t(ret)) ** 2).mean()
    loss.backward()
    grads = [torch.zeros_like(p) if p.grad is None else p.grad for p in params]       # (a detached free log_std has no gradient)
    return np.concatenate([g.detach().numpy().astype(np.float64).reshape(-1) for g in grads])


def z64(pol, theta, obs, action):
    """z = (action - mean) / sd [S, A] of the float64 forward pass on the network's input rows"""
    layers, _, log_std = P.unflatten(pol, theta)
    h, A = np.asarray(obs, np.float64), pol.num_keywords + 1
    for i, (w, b) in enumerate(layers):
        h = h @ w.astype(np.float64) + b.astype(np.float64)
        if i + 1 < len(layers):
            h = np.tanh(h) if pol.activation == "tanh" else np.maximum(h, 0.0)
    mean = h[:, :A]
    ls = h[:, A:] if log_std is None else np.broadcast_to(log_std.astype(np.float64), mean.shape)
    if pol.log_std_clamp is not None:
        ls = np.clip(ls, float(F(pol.log_std_clamp[0])), float(F(pol.log_std_clamp[1])))
    return (np.asarray(action, np.float64) - mean) / np.exp(ls)


Z_MAX = 6.0


def conditioned(pol, obs, action):
    """the inputs' condition, in place: the mean head's biases moved to the teacher's mean action, then the output layer's weights
    (not its biases) halved until max |z| <= 6 over all samples and components in the float64 forward pass.  Without it a random
    policy sits tens of standard deviations from a teacher's budget of 40, log p is O(1e3 A) and float32 autograd's own error, the
    yardstick, is whatever that cancellation leaves.  Returns max |z|"""
    A = pol.num_keywords + 1
    w, b = pol.layers[-1]
    b[:A] = np.asarray(action, np.float64).mean(axis=0).astype(F)
    for _ in range(24):
        worst = float(np.abs(z64(pol, P.flat_params(pol), obs, action)).max())
        if worst <= Z_MAX:
            return worst
        w *= F(0.5)
    raise AssertionError(f"max |z| stays at {worst}: the biases and log-stds alone put the teacher's actions out of reach")


def fixed_teacher_actions(rng, envs, K):
    """a "fixed" teacher's: one action an env, budget 40, bids in [0.3, 1]"""
    return np.concatenate([np.full((envs, 1), 40.0), 0.3 + 0.7 * rng.random((envs, K))], axis=1).astype(F)


def _teacher_batch(rng, pol, S, adv_scale=30.0, envs=8):
    """S samples of `envs` envs (sample s = t * envs + env) under a fixed teacher, the policy conditioned on them"""
    K = pol.num_keywords
    obs = (rng.standard_normal((S, 5 * K + 2)) * 0.7).astype(F)
    action = fixed_teacher_actions(rng, envs, K)[np.arange(S) % envs]
    worst = conditioned(pol, obs, action)
    adv = (rng.standard_normal(S) * adv_scale).astype(F)
    ret = (rng.standard_normal(S) * 2).astype(F)
    return P.flat_params(pol), obs, action, adv, ret, (ret - adv).astype(F), worst


def alive_view(terms, dead, *vectors):
    """the terms that are not `dead` (exact zeros by design) moved together: (terms re-indexed, the vectors cut the same way)"""
    keep, out, pos = [], [], 0
    for name, a, b in terms:
        if name not in dead:
            keep.append(np.arange(a, b))
            out.append((name, pos, pos + b - a))
            pos += b - a
    keep = np.concatenate(keep)
    return out, [np.asarray(v)[keep] for v in vectors]


# the imitation options of the shapes W1-W3 (tests/learner_shapes.py), on the host and on the device; ma_rate = 1 makes the scale c the
# advantages' own root mean square, whatever their magnitude: exp(0.7 adv / c) then passes the cap 1.5 for some samples and not for others
W_IM = dict(W1=dict(beta=0.7, w_max=1.5, ma_rate=1.0), W2=dict(beta=0.0, vf_coef=0.5), W3=dict(beta=0.7, w_max=1.5, ma_rate=1.0, train_log_std=False))
W_SAMPLES = 40


def _small_case(name):
    """(policy, imitation options, samples, the terms that are zero by design)"""
    rng = np.random.default_rng({"bc": 611, "marwil-cap": 612, "frozen-log-std": 613, "two-heads-clamp": 614, "no-value-loss": 615}[name])
    if name == "bc":
        return rng, _policy(rng, "tanh", (13, 8), False, True, None, 2), dict(beta=0.0), 1040, ()
    if name == "marwil-cap":
        return rng, _policy(rng, "tanh", (13, 8), False, True, (-1.0, 0.5), 10), dict(beta=0.7, w_max=1.5, ma_rate=1.0), 257, ()
    if name == "frozen-log-std":
        return rng, _policy(rng, "tanh", (13, 8), False, True, (-1.2, -0.2), 2), dict(beta=0.0, train_log_std=False), 130, ("log_std",)
    if name == "two-heads-clamp":
        pol = _policy(rng, "relu", (13, 8), True, True, (-1.5, 0.0), 10)
        pol.layers[-1][1][11:] = np.linspace(-2.1, 0.6, 11).astype(F)          # (the log-std head's biases on both sides of the clamp)
        return rng, pol, dict(beta=0.7, vf_coef=0.5, w_max=3.0, ma_rate=1.0), 300, ()
    pol = _policy(rng, "relu", (13, 8), False, True, None, 10)
    return rng, pol, dict(beta=0.0, vf_coef=0.0), 300, tuple(n for n, _, _ in W.pg_terms(pol) if n.startswith("value"))


def _w_case(name):
    rng = np.random.default_rng(620 + ("W1", "W2", "W3").index(name))
    return rng, W.pg_policy(rng, name), dict(W_IM[name]), W_SAMPLES, ()


A1_CASES = ("bc", "marwil-cap", "frozen-log-std", "two-heads-clamp", "no-value-loss", "W1", "W2", "W3")


@pytest.mark.parametrize("name", A1_CASES)
def test_gradient_against_pytorch_autograd(lib, name):
    """The host twin adc_im_grad_host against float64 autograd of the loss written out in PyTorch (_torch_im_grad: not derived from
    the law header) under learner_shapes.yardstick - at most twice float32 autograd's own error over the whole vector and in
    every term, the per-term floor 2^-23 - on a fixed teacher's actions (budget 40, bids in [0.3, 1]) with the policy conditioned
    to max |z| <= 6.  A term that is zero by design (a free log_std that is not trained, the value network under vf_coef = 0) is
    asserted to be exactly zero in the twin and in autograd and left out of the yardstick, which divides by a term's largest entry."""
    import torch
    rng, pol, kw, S, dead = (_w_case if name in W.SHAPES else _small_case)(name)
    if pol.log_std is not None and pol.log_std_clamp is None:
        pol.log_std = np.clip(pol.log_std, -1.6, 0.0).astype(F)     # (sd >= 0.2: a bid 0.35 from the mean stays within 2 sd)
    im = I.im_options(**kw)
    theta, obs, action, adv, ret, value_old, worst = _teacher_batch(rng, pol, S)
    assert worst <= Z_MAX and np.abs(z64(pol, theta, obs, action)).max() <= Z_MAX
    layers, value_layers, _ = P.unflatten(pol, theta)
    if pol.activation == "relu":
        assert W.relu_margin(obs, layers, value_layers) > 1e-6, "a relu pre-activation sits on its kink: choose another seed"
    _, c = I.scale(im["ma_start"], adv, **im)
    w = I.weight(adv, c, **im)
    if im["beta"] == 0:
        assert np.all(w == 1)
    else:
        assert (w == F(im["w_max"])).any() and (w < F(im["w_max"])).any(), "the case was meant to cap some weights and not others"
    g, _, _ = I.twin_grad(lib, pol, theta, obs, action, adv, ret, value_old, c, **im)
    g64 = _torch_im_grad(pol, theta, obs, action, adv, ret, c, torch.float64, im)
    g32 = _torch_im_grad(pol, theta, obs, action, adv, ret, c, torch.float32, im)
    terms = W.pg_terms(pol)
    for tname, a, b in terms:
        if tname in dead:
            assert not g[a:b].any() and not g64[a:b].any() and not g32[a:b].any(), (name, tname)
    if pol.log_std_clamp is not None:
        A = pol.num_keywords + 1
        raw = R.network(obs, layers, pol.activation)[:, A:] if pol.log_std is None else np.broadcast_to(pol.log_std, (S, A))
        moved = (raw < F(pol.log_std_clamp[0])) | (raw > F(pol.log_std_clamp[1]))
        assert moved.any() and not moved.all(), "the clamp was meant to move some log-stds and not others"
    if name == "W3":
        # train_log_std = 0 on a two-headed policy: the log-std head's columns of the output layer, weights and biases, are +0
        A = pol.num_keywords + 1
        (_, wa, wb), (_, ba, bb) = terms[-2], terms[-1]
        gw, gb = g[wa:wb].reshape(-1, 2 * A), g[ba:bb]
        assert terms[-2][0] == "policy W1" and gb.size == 2 * A
        for part in (gw[:, A:], gb[A:]):
            assert not part.any() and not np.signbit(part).any(), "the log-std head was not to be trained"
        assert np.abs(gw[:, :A]).max() > 0 and np.abs(gb[:A]).max() > 0
    live, (gl, g64l, g32l) = alive_view(terms, dead, g, g64, g32)
    W.assert_terms_alive(gl, live, name)
    W.yardstick(f"{name} IM twin", gl, g64l, g32l, live)


# ---- the returns against a plain discounted sum ---------------------------------------------------------------------------------------
def test_returns_equal_the_plain_discounted_sum(lib):
    """ret[t] of a teacher record is the discounted sum of the scaled rewards up to the first episode end, or to the record's end
    and then gamma^m times the bootstrap value (adc_pg.h "GAE" under lambda = 1, adc_imitation.h "returns"): the recorded values
    telescope out.  Here it is summed forward per sample in float64, gamma and reward_scale at their float32 values, and compared
    with im_ref.returns and with the twin adc_pg_gae_host under lambda = 1.

    The tolerance, derived.  The device's path to ret[t] over a window of m days is, per day t + k, six rounded float32 operations
    (r = reward * s; gamma * next; r + .; . - value; (gamma nt) * adv; delta + .; the two products by nt = 0 or 1 are exact), then
    one more for ret = adv + value: 6 m + 1 roundings, each within 2^-24 of its result.  What day t + k rounds reaches ret[t]
    multiplied by gamma^k, and gamma^k times any of that day's results is at most
        M = sum_k gamma^k |s r[t + k]| + gamma^m |bootstrap| + 2 |value[t]|
    provided the later days' values are small against the rewards before them - which the inputs are drawn to satisfy and the
    test asserts on them in float64 before it compares.  So |ret - ret64| <= (6 m + 1) 2^-24 M to first order, and adv = ret - value
    (one rounding fewer) within the same bound.  The worst observed error as a fraction of the bound is printed."""
    rng = np.random.default_rng(21)
    T, N, gamma, scale = 12, 8, 0.97, 0.1
    sign = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    reward = (sign((T, N)) * (10 + 20 * rng.random((T, N)))).astype(F)               # |s r| in [1, 3]
    value = (sign((T, N)) * (0.05 + 0.2 * rng.random((T, N)))).astype(F)             # |value| <= 0.25: a quarter of the smallest |s r|
    boot = (sign(N) * (1 + 4 * rng.random(N))).astype(F)
    term, trunc = np.zeros((T, N), bool), np.zeros((T, N), bool)
    term[3, 1] = term[7, 2] = term[8, 2] = term[T - 1, 3] = term[5, 6] = True
    trunc[4, 4] = trunc[0, 5] = trunc[10, 5] = trunc[T - 1, 6] = trunc[6, 7] = term[6, 7] = True
    done = term | trunc
    assert term[1:-1].any() and trunc[1:-1].any() and not done[:, 0].any(), "an end of each kind inside the record, and env 0 uncut"
    g, s = float(F(gamma)), float(F(scale))
    ret64, bound, cond = np.zeros((T, N)), np.zeros((T, N)), np.zeros((T, N))
    for n in range(N):
        for t in range(T):
            total, mass, worst, k = 0.0, 0.0, 0.0, 0
            while True:
                r = s * float(reward[t + k, n])
                total += g ** k * r
                mass += g ** k * abs(r)
                k += 1
                if done[t + k - 1, n] or t + k == T:
                    break
            m = k
            if not done[t + m - 1, n]:
                total += g ** m * float(boot[n])
                mass += g ** m * abs(float(boot[n]))
            M = mass + 2 * abs(float(value[t, n]))
            # the condition: gamma^k times the largest result of day t + k's operations, from this window's float64 quantities
            tail = total
            for k in range(m):
                nxt = 0.0 if done[t + k, n] else (float(boot[n]) if t + k + 1 == T else float(value[t + k + 1, n]))
                r, v = s * float(reward[t + k, n]), abs(float(value[t + k, n]))
                worst = max(worst, g ** k * max(abs(r) + g * abs(nxt) + v, abs(tail) / g ** k + v))
                tail -= g ** k * r
            ret64[t, n], bound[t, n], cond[t, n] = total, (6 * m + 1) * 2.0 ** -24 * M, worst / M
    assert cond.max() <= 1.0, cond.max()
    opts = dict(gamma=gamma, reward_scale=scale)
    for what, (adv, ret) in (("restatement", I.returns(reward, term, trunc, value, boot, **opts)),
                             ("twin", P.twin_gae(lib, reward, term, trunc, value, boot, lam=1.0, normalize_advantages=False, **opts))):
        e_ret = np.abs(ret.astype(np.float64) - ret64) / bound
        e_adv = np.abs(adv.astype(np.float64) - (ret64 - value.astype(np.float64))) / bound
        print(f"returns, {what}: worst |ret - float64 sum| / bound {e_ret.max():.3f}, worst |adv - (sum - value)| / bound {e_adv.max():.3f}")
        assert e_ret.max() <= 1.0 and e_adv.max() <= 1.0, (what, e_ret.max(), e_adv.max())
    radv, rret = I.returns(reward, term, trunc, value, boot, **opts)
    assert _same(adv, radv) and _same(ret, rret)
    # a day that ends an episode takes nothing from the days after it, and an uncut env's first return carries gamma^T bootstrap
    assert ret64[3, 1] == s * float(reward[3, 1]) and abs(ret64[0, 0] - sum(g ** k * s * float(reward[k, 0]) for k in range(T)) - g ** T * float(boot[0])) < 1e-12
