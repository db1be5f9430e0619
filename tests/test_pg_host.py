"""Policy-gradient training on the host: the twins adc_pg_gae_host / adc_pg_grad_host / adc_pg_step_host (the code the device
kernels run, adc_pg.h) against the numpy restatement in tests/pg_ref.py bit for bit, the gradient against PyTorch autograd, GAE
against a plain float64 loop, the configuration checks and the Python surface.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

from tests import mlp_ref as R
from tests import pg_ref as P

F = np.float32


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _batch(rng, policy, S, drift=0.03):
    """S samples as a record would hold them, collected by `policy`; and a theta a few updates away from it, so that the
    ratios spread around 1"""
    K = policy.num_keywords
    obs = (rng.standard_normal((S, 5 * K + 2)) * 0.7).astype(F)
    saved = policy.shift, policy.scale
    policy.shift = policy.scale = None                       # (the record holds the network's input, already normalised)
    a = R.act(policy, obs, rng.standard_normal((S, K + 1)).astype(F), deterministic=False)
    policy.shift, policy.scale = saved
    theta = P.flat_params(policy)
    theta = (theta + rng.standard_normal(theta.size).astype(F) * F(drift)).astype(F)
    adv = rng.standard_normal(S).astype(F)
    ret = (rng.standard_normal(S) * 2).astype(F)
    value_old = (ret + rng.standard_normal(S)).astype(F)
    return theta, obs, a["action"], a["logp"], adv, ret, value_old


# activation, hidden, two heads, value network, clamp, K, samples, options
GRAD_CASES = [
    ("tanh", (16, 8), False, True, None, 3, 300, dict()),
    ("relu", (32,), True, True, (-1.5, 0.0), 4, 257, dict(ent_coef=0.01)),
    ("tanh", (), False, False, (-1.2, -0.8), 2, 64, dict(eps_clip=0.0)),
    ("relu", (7, 33, 5), False, True, None, 3, 1100, dict(eps_clip=0.05, vf_coef=1.0, ent_coef=0.02)),
    ("tanh", (24, 24), True, False, None, 5, 2100, dict(eps_clip=-1.0)),
    ("tanh", (8,), False, True, (-1.0, 0.5), 6, 1024, dict(eps_clip=0.3)),
]


def _policy(rng, act, hidden, two, value, clamp, K):
    pol = R.random_policy(rng, K, hidden, activation=act, two_heads=two, value=value, log_std_clamp=clamp)
    if len(pol.value_layers) > 0 and len(hidden) > 1:        # (a value network of another depth than the policy's)
        pol.value_layers = R.random_policy(rng, K, hidden[:1], activation=act, value=True).value_layers
    if clamp is not None and not two:                        # (a free log_std on both sides of both bounds)
        pol.log_std = np.linspace(clamp[0] - 0.5, clamp[1] + 0.5, K + 1).astype(F)
    return pol


@pytest.mark.parametrize("case", range(len(GRAD_CASES)))
def test_grad_twin_equals_the_restatement_bit_for_bit(lib, case):
    act, hidden, two, value, clamp, K, S, kw = GRAD_CASES[case]
    rng = np.random.default_rng(100 + case)
    pol = _policy(rng, act, hidden, two, value, clamp, K)
    batch = _batch(rng, pol, S)
    opts = P.options(**kw)
    g, sums, st = P.twin_grad(lib, pol, *batch, **opts)
    rg, rsums, rst = P.grad(pol, *batch, **opts)
    assert _same(g, rg)
    assert _same(sums, rsums)
    for k in P.STAT_KEYS:
        assert _same(np.float64(st[k]), np.float64(rst[k])), k
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    # the cases cover what they claim to: clipped and unclipped samples, a clamp that moves some components and not others
    if opts["eps_clip"] > 0:
        assert 0.0 < st["clip_fraction"] < 1.0
    else:
        assert st["clip_fraction"] == 0.0
    if clamp is not None and not two:
        ls = P.unflatten(pol, batch[0])[2]
        moved = (ls < clamp[0]) | (ls > clamp[1])
        assert moved.any() and not moved.all()
        assert np.all(g[-ls.size:][moved] == 0) and np.all(g[-ls.size:][~moved] != 0)
    if clamp is not None and two:                              # (the log-std head: per sample and component)
        raw = R.network(batch[1], P.unflatten(pol, batch[0])[0], pol.activation)[:, K + 1:]
        moved = (raw < F(clamp[0])) | (raw > F(clamp[1]))
        assert moved.any() and not moved.all() and moved.any(axis=0).all() and not moved.all(axis=0).any()


@pytest.mark.parametrize("kw", [dict(), dict(optimiser="sgd", lr=0.05), dict(max_grad_norm=0.0), dict(max_grad_norm=1e6, lr=1e-2),
                                dict(max_grad_norm=0.01, beta1=0.8, beta2=0.99, eps=1e-6), dict(optimiser="sgd", max_grad_norm=0.0, lr=1.0)])
def test_step_twin_equals_the_restatement_bit_for_bit(lib, kw):
    rng = np.random.default_rng(7)
    opts = P.options(**kw)
    for Q in (5, 1024, 2500):
        tw = [rng.standard_normal(Q).astype(F), np.zeros(Q, F), np.zeros(Q, F)]
        ref = [a.copy() for a in tw]
        for steps in range(4):
            g = (rng.standard_normal(Q) * 10.0 ** rng.integers(-3, 2)).astype(F)
            tw = list(P.twin_step(lib, *tw, g, steps, **opts))
            ref = list(P.step(*ref, g, steps, **opts))
            for a, b in zip(tw, ref):
                assert _same(a, b), (Q, steps)
        assert not np.array_equal(tw[0], ref[0] * 0)


def _record(rng, T, N):
    reward = (rng.standard_normal((T, N)) * 30).astype(F)
    value = (rng.standard_normal((T, N)) * 5).astype(F)
    term, trunc = rng.random((T, N)) < 0.1, rng.random((T, N)) < 0.1
    term[-1, : N // 3] = True                                     # episodes that end on the horizon's last day, both ways
    trunc[-1, N // 3: 2 * N // 3] = True
    boot = (rng.standard_normal(N) * 5).astype(F)
    return reward, term, trunc, value, boot


@pytest.mark.parametrize("kw", [dict(), dict(normalize_advantages=False), dict(gamma=1.0, lam=1.0, reward_scale=0.01),
                                dict(gamma=0.9, lam=0.0, normalize_advantages=False)])
def test_gae_twin_equals_the_restatement_bit_for_bit(lib, kw):
    rng = np.random.default_rng(3)
    opts = P.options(**kw)
    for T, N in ((1, 1), (10, 9), (60, 37), (7, 300)):            # (7 x 300: a sample count that is not a multiple of the chunk)
        rec = _record(rng, T, N)
        adv, ret = P.twin_gae(lib, *rec, **opts)
        radv, rret = P.gae(*rec, **opts)
        assert _same(adv, radv) and _same(ret, rret), (T, N)
        if opts["normalize_advantages"] and T * N > 1:
            assert abs(float(adv.mean())) < 1e-5 and abs(float(adv.std()) - 1.0) < 1e-4


def test_gae_against_a_plain_float64_loop(lib):
    """Every day of the float32 chain is eight rounded operations on magnitudes of at most |r| + |v| + |adv| <= 3 M, M the
    largest of them; what a day inherits from the next is multiplied by gamma * lambda <= 1.  So after d days the chain is
    within d * 8 * 3 M * 2^-24 of exact arithmetic, and at most T days are chained: the bound is 24 T M 2^-24."""
    rng = np.random.default_rng(5)
    T, N, gamma, lam, scale = 60, 50, 0.99, 0.95, 0.1
    reward, term, trunc, value, boot = _record(rng, T, N)
    adv, ret = P.twin_gae(lib, reward, term, trunc, value, boot, gamma=gamma, lam=lam, reward_scale=scale, normalize_advantages=False)
    g, l, sc = float(F(gamma)), float(F(lam)), float(F(scale))
    a64 = np.zeros((T, N))
    for n in range(N):
        nxt, a = float(boot[n]), 0.0
        for t in range(T - 1, -1, -1):
            nt = 0.0 if (term[t, n] or trunc[t, n]) else 1.0
            delta = float(reward[t, n]) * sc + g * nxt * nt - float(value[t, n])
            a = delta + g * l * nt * a
            a64[t, n] = a
            nxt = float(value[t, n])
    M = max(np.abs(a64).max(), np.abs(value).max(), np.abs(reward).max() * sc)
    bound = 24 * T * M * 2.0 ** -24
    err = np.abs(adv.astype(np.float64) - a64).max()
    err_ret = np.abs(ret.astype(np.float64) - (a64 + value)).max()
    print(f"GAE: max |adv - float64| {err:.3e}, max |ret - float64| {err_ret:.3e}, bound {bound:.3e}")
    assert err <= bound and err_ret <= bound + M * 2.0 ** -23
    # a day that ends an episode takes nothing from the days after it
    done = term | trunc
    t, n = np.argwhere(done)[0]
    assert adv[t, n] == F(F(reward[t, n] * F(scale)) - value[t, n])


def _torch_grad(pol, theta, obs, action, logp_old, adv, ret, value_old, dtype, opts):
    """the same loss in PyTorch from the same arrays; the flat gradient by autograd in `dtype`"""
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
    z = (t(action) - mean) / torch.exp(ls)
    logp = (-0.5 * z * z - ls).sum(dim=1) - A * 0.5 * np.log(2 * np.pi)
    entropy = ls.sum(dim=1) + A * (0.5 + 0.5 * np.log(2 * np.pi))
    ratio = torch.exp(logp - t(logp_old))
    s1 = ratio * t(adv)
    if opts["eps_clip"] > 0:
        eps = float(F(opts["eps_clip"]))
        s1 = torch.minimum(s1, torch.clamp(ratio, 1 - eps, 1 + eps) * t(adv))
    loss = -s1.mean() - float(F(opts["ent_coef"])) * entropy.mean()
    if vl:
        V = forward(vl, x)[:, 0]
        loss = loss + float(F(opts["vf_coef"])) * 0.5 * ((V - t(ret)) ** 2).mean()
    loss.backward()
    return np.concatenate([p.grad.detach().numpy().astype(np.float64).reshape(-1) for p in params])


@pytest.mark.parametrize("case", range(len(GRAD_CASES)))
def test_gradient_against_pytorch_autograd(lib, case):
    """The yardstick is float32 autograd's own error against float64 autograd on the same arrays; the twin's error against
    float64 autograd must be at most twice that.  An error is a largest absolute difference over the largest float64 entry
    (an entry-wise quotient is undefined where the exact gradient is zero, as under a clamp).  Asserted twice:
    over the whole flat gradient, as stated; and in every term on its own - each layer's weights, each layer's biases,
    log_std - so that a wrong entry in a term of small magnitude cannot hide behind a large one.  A term may have as few as
    one entry, and float32 autograd's error on so few can fall below what the format can hold at all (3.6e-08 on the eight
    first-layer biases of case 5): per term the yardstick is therefore not taken below 2^-23, one float32 ulp of the term's
    largest entry - every entry is a float32 that went through several float32 roundings per sample, for autograd and the
    twin alike.  Measured figures: profiles/pr_pg_trainer.txt."""
    import torch
    act, hidden, two, value, clamp, K, S, kw = GRAD_CASES[case]
    rng = np.random.default_rng(100 + case)
    pol = _policy(rng, act, hidden, two, value, clamp, K)
    batch = _batch(rng, pol, S)
    opts = P.options(**kw)
    g, _, _ = P.twin_grad(lib, pol, *batch, **opts)
    g64 = _torch_grad(pol, *batch, torch.float64, opts)
    g32 = _torch_grad(pol, *batch, torch.float32, opts)
    assert g64.shape == g.shape
    terms, pos = [], 0
    for name, net in (("policy", pol.layers), ("value", pol.value_layers)):
        for l, (w, b) in enumerate(net):
            terms += [(f"{name} W{l}", pos, pos + w.size), (f"{name} b{l}", pos + w.size, pos + w.size + b.size)]
            pos += w.size + b.size
    if pol.log_std is not None:
        terms.append(("log_std", pos, pos + pol.log_std.size))
        pos += pol.log_std.size
    assert pos == g.size
    scale = np.abs(g64).max()
    err_twin, err_f32 = np.abs(g.astype(np.float64) - g64).max() / scale, np.abs(g32 - g64).max() / scale
    print(f"case {case} whole     : twin {err_twin:.3e}  float32 autograd {err_f32:.3e}  ratio {err_twin / err_f32:.3f}")
    assert err_twin <= 2 * err_f32
    failed = []
    for name, a, b in terms:
        scale = np.abs(g64[a:b]).max()
        assert scale > 0, name
        err_twin = np.abs(g[a:b].astype(np.float64) - g64[a:b]).max() / scale
        err_f32 = np.abs(g32[a:b] - g64[a:b]).max() / scale
        print(f"case {case} {name:10s}: twin {err_twin:.3e}  float32 autograd {err_f32:.3e}  ratio {err_twin / err_f32 if err_f32 else float('nan'):.3f}")
        if not err_twin <= 2 * max(err_f32, 2.0 ** -23):
            failed.append((name, err_twin, err_f32))
    assert not failed, failed


BAD = [dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=float("nan")), dict(lam=2.0), dict(lam=-1.0), dict(eps_clip=1.0), dict(vf_coef=-1.0),
       dict(ent_coef=-0.1), dict(reward_scale=0.0), dict(reward_scale=float("inf")), dict(max_grad_norm=-1.0), dict(optimiser=7),
       dict(lr=-1e-3), dict(lr=float("nan")), dict(beta1=1.0), dict(beta2=-0.5), dict(eps=0.0), dict(minibatch_envs=-4)]


@pytest.mark.parametrize("bad", BAD, ids=[next(iter(b)) + "=" + str(next(iter(b.values()))) for b in BAD])
def test_config_check_rejects_each_bad_field(lib, bad):
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    good = StepEngine.pg_config()
    msg = C.c_char_p()
    assert lib.adc_pg_config_check(C.byref(good), C.byref(msg)) == 0 and msg.value is None
    for k, v in bad.items():
        setattr(good, "lambda_" if k == "lam" else k, v)
    assert lib.adc_pg_config_check(C.byref(good), C.byref(msg)) == _ffi.ADC_EINVAL
    assert msg.value
    good = StepEngine.pg_config()
    good.struct_size += 4
    assert lib.adc_pg_config_check(C.byref(good), C.byref(msg)) == _ffi.ADC_EINVAL and b"struct_size" in msg.value
    assert lib.adc_pg_config_check(None, C.byref(msg)) == _ffi.ADC_EINVAL
    if "optimiser" not in bad:
        with pytest.raises(ValueError):
            StepEngine.pg_config(**bad)
    # SGD does not look at Adam's fields
    if set(bad) & {"beta1", "beta2", "eps"}:
        StepEngine.pg_config(optimiser="sgd", **bad)


def test_python_surface():
    from adcraft_amd.baselines import pg_trainer as T
    from adcraft_amd.engine import ShardedStepEngine, StepEngine
    ppo, a2c = T.ppo(), T.a2c()
    assert (ppo["epochs"], ppo["minibatches"], ppo["eps_clip"], ppo["lam"], ppo["normalize_advantages"]) == (10, 4, 0.2, 0.95, True)
    assert (a2c["epochs"], a2c["minibatches"], a2c["eps_clip"], a2c["lam"], a2c["normalize_advantages"]) == (1, 1, 0.0, 1.0, False)
    assert T.ppo(lr=1e-3, epochs=3)["lr"] == 1e-3 and T.ppo(epochs=3)["epochs"] == 3
    for preset in (ppo, a2c):                                     # what is left after the loop's own keys is a valid adc_pg_config
        cfg = {k: v for k, v in preset.items() if k not in ("epochs", "minibatches")}
        c = StepEngine.pg_config(**cfg)
        assert abs(c.gamma - 0.99) < 1e-7 and c.struct_size == C.sizeof(type(c))
    with pytest.raises(ValueError, match="optimiser"):
        StepEngine.pg_config(optimiser="rmsprop")
    # policy() round-trips through the flat order, for every kind of head
    rng = np.random.default_rng(2)
    for two, value, hidden in ((False, True, (8, 4)), (True, False, (5,)), (False, False, ())):
        pol = R.random_policy(rng, 3, hidden, two_heads=two, value=value, normalize=True)
        theta = T.flat_params(pol)
        assert _same(theta, P.flat_params(pol))
        q = C.c_int64(0)
        from adcraft_amd import _ffi
        cfg = pol.config(3)
        assert _ffi.lib().adc_pg_param_count_host(C.byref(cfg), 3, C.byref(q)) == 0 and q.value == theta.size
        perm = rng.standard_normal(theta.size).astype(F)
        back = T.policy_from_flat(pol, perm)
        assert _same(T.flat_params(back), perm) and back.shapes() == pol.shapes()
        assert back.shift is pol.shift and back.activation == pol.activation
        for (w, b), (w2, b2) in zip(pol.layers + pol.value_layers, P.with_params(pol, perm).layers + P.with_params(pol, perm).value_layers):
            assert w.shape == w2.shape and b.shape == b2.shape
        with pytest.raises(ValueError):
            T.policy_from_flat(pol, perm[:-1])
    sharded = object.__new__(ShardedStepEngine)
    for name in ("pg_init", "pg_advantages", "pg_minibatch", "pg_update", "pg_state", "pg_param_count"):
        with pytest.raises(NotImplementedError, match="engine_shards=1"):
            getattr(sharded, name)
