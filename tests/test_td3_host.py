"""Off-policy (TD3) training on the host: the twins adc_td3_batch_indices_host / adc_td3_target_host / adc_td3_critic_grad_host /
adc_td3_actor_grad_host / adc_td3_polyak_host (the code the device kernels run, adc_td3.h) against the numpy restatement in
tests/td3_ref.py bit for bit, both gradients against PyTorch autograd, the batch indices' range and uniformity, the
configuration checks and the Python surface.  No device is needed.  None of these symbols exists before this feature."""
import ctypes as C

import numpy as np
import pytest

from tests import mlp_ref as R
from tests import td3_ref as T3

F = np.float32
K = 9                       # A = 10, D = 47, D + A = 57: no multiple of 4, 8 or 32


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _setup(rng, act, widths, norm, size, hidden=(16, 8), K=K):
    """a policy, a state whose targets and moments differ from the live networks, an action normalisation and a ring of `size` rows"""
    pol = R.random_policy(rng, K, hidden, activation=act)
    critics = T3.random_critics_for_tests(rng, K, widths)
    st = T3.fresh_state(pol, critics)
    for k in ("theta_target", "psi_target"):
        st[k] = (st[k] + rng.standard_normal(st[k].size).astype(F) * F(0.05)).astype(F)
    A, D = K + 1, 5 * K + 2
    nrm = ((rng.random(A) * 0.5).astype(F), (0.5 + rng.random(A)).astype(F)) if norm else None
    buf = dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * 0.8 + 0.3).astype(F),
               r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))
    buf["done"][0], buf["done"][1] = True, False
    return pol, st, nrm, buf


# activation, critic widths, action normalisation, action clamp, batch, ring size
CASES = [
    ("tanh", (12, 1), True, True, 5, 3),
    ("relu", (7, 33, 5, 1), False, True, 64, 37),
    ("tanh", (32, 32, 1), True, False, 257, 37),
    ("relu", (1,), True, False, 64, 37),
    ("tanh", (1,), False, True, 5, 3),
    ("relu", (12, 1), False, False, 1100, 84),
    ("tanh", (7, 33, 5, 1), True, True, 1100, 84),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_twins_equal_the_restatement(lib, case):
    act, widths, norm, clamp, B, size = CASES[case]
    rng = np.random.default_rng(300 + case)
    pol, st, nrm, buf = _setup(rng, act, widths, norm, size)
    opts = T3.options(critic_widths=widths, batch_size=B, capacity=size, seed=77 + case, reward_scale=0.5, gamma=0.9, target_noise=0.6,
                      target_noise_clip=0.5, **(dict(action_lo=-0.4, action_hi=0.9) if clamp else {}))
    sh, seed, u = T3.Shapes(pol, opts), opts["seed"], 3 + case
    p, q = C.c_int64(0), C.c_int64(0)
    cfg, mcfg = T3.td3_config(**opts), pol.config(K)
    assert lib.adc_td3_param_counts_host(C.byref(mcfg), K, C.byref(cfg), C.byref(p), C.byref(q)) == 0
    assert (p.value, q.value) == (sh.P, sh.Qc) == (st["theta"].size, st["psi"].size // 2)
    idx = T3.batch_indices(seed, u, size, B)
    assert _same(T3.twin_batch_indices(lib, seed, u, size, B), idx)
    assert idx.min() >= 0 and idx.max() < size and len(set(idx.tolist())) < B, "the batch was meant to hold duplicates"
    slots = np.unique(idx)
    buf["done"][slots[0]], buf["done"][slots[1]] = True, False           # (done samples present, whatever the batch drew)
    done = buf["done"][idx]
    assert done.any() and not done.all()
    # the target: noise on both sides of the clip, the action clamp engaged when on
    y = T3.target(sh, st["theta_target"], st["psi_target"], nrm, seed, u, buf["x2"][idx], buf["r"][idx], done, opts)
    assert _same(T3.twin_target(lib, pol, st["theta_target"], st["psi_target"], nrm, seed, u, buf["x2"][idx], buf["r"][idx], done, opts), y)
    e = F(opts["target_noise"]) * T3.noise(seed, u, B, K + 1)
    assert (np.abs(e) > 0.5).any() and (np.abs(e) < 0.5).any()
    assert np.isfinite(y).all() and _same(y[done], (buf["r"][idx][done] * F(0.5)).astype(F)), "a day that ends an episode bootstraps nothing"
    # the critics' gradient and sums
    g, sums = T3.critic_grad(sh, st["psi"], nrm, buf["x"][idx], buf["a"][idx], y)
    tg, tsums = T3.twin_critic_grad(lib, pol, st["psi"], nrm, buf["x"][idx], buf["a"][idx], y, opts)
    assert _same(tg, g) and _same(tsums, sums) and np.abs(g).max() > 0
    # the actor's gradient through critic 1's action inputs
    ga, sa = T3.actor_grad(sh, st["theta"], st["psi"], nrm, buf["x"][idx])
    tga, tsa = T3.twin_actor_grad(lib, pol, st["theta"], st["psi"], nrm, buf["x"][idx], opts)
    assert _same(tga, ga) and _same(tsa, sa) and np.abs(ga).max() > 0
    assert _same(T3.twin_polyak(lib, st["psi_target"], st["psi"], 0.005), T3.polyak(st["psi_target"], st["psi"], 0.005))
    assert not _same(T3.polyak(st["psi_target"], st["psi"], 0.005), st["psi_target"])


def _torch_nets(layer_lists, dtype):
    import torch
    params, nets = [], []
    for layers in layer_lists:
        net = [(torch.tensor(w.astype(np.float64), dtype=dtype).requires_grad_(), torch.tensor(b.astype(np.float64), dtype=dtype).requires_grad_())
               for w, b in layers]
        nets.append(net)
        for w, b in net:
            params += [w, b]
    return nets, params


def _torch_forward(net, x, act, pre=None):
    import torch
    f = torch.tanh if act == "tanh" else torch.relu
    for i, (w, b) in enumerate(net):
        x = x @ w + b
        if i + 1 < len(net):
            if pre is not None:
                pre.append(x.detach())
            x = f(x)
    return x


def _torch_grads(sh, st, nrm, x, a, y, dtype, pre=None):
    """(critic gradient [2 Qc], actor gradient [P]) by autograd in `dtype` from the same arrays"""
    import torch
    t = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype)
    an = (lambda v: (v - t(nrm[0])) * t(nrm[1])) if nrm is not None else (lambda v: v)
    critics, cp = _torch_nets(sh.critics(st["psi"]), dtype)
    row = torch.cat([t(x), an(t(a))], dim=1)
    loss = sum((0.5 * (_torch_forward(net, row, sh.act, pre)[:, 0] - t(y)) ** 2).mean() for net in critics)
    loss.backward()
    gc = np.concatenate([p.grad.detach().numpy().astype(np.float64).reshape(-1) for p in cp])
    (actor,), ap = _torch_nets([sh.actor(st["theta"])], dtype)
    (q1, _), _ = _torch_nets(sh.critics(st["psi"]), dtype)
    mu = _torch_forward(actor, t(x), sh.act, pre)
    (-_torch_forward(q1, torch.cat([t(x), an(mu)], dim=1), sh.act, pre)[:, 0].mean()).backward()
    ga = np.concatenate([p.grad.detach().numpy().astype(np.float64).reshape(-1) for p in ap])
    return gc, ga


def _terms(name, n_in, widths):
    out, pos = [], 0
    for l, n_out in enumerate(widths):
        out += [(f"{name} W{l}", pos, pos + n_in * n_out), (f"{name} b{l}", pos + n_in * n_out, pos + (n_in + 1) * n_out)]
        pos += (n_in + 1) * n_out
        n_in = n_out
    return out, pos


@pytest.mark.parametrize("case", [0, 1, 2, 3, 5])
def test_gradients_against_pytorch_autograd(lib, case):
    """Both gradients against float64 autograd with the yardstick of tests/test_pg_host.py: the twin's error (largest absolute
    difference over the largest float64 entry) is at most twice float32 autograd's own, over the whole gradient and in every
    term on its own, the per-term yardstick not taken below 2^-23.  The actor's gradient is the independent check of the
    critic's input-gradient path.  Before that, the float64 pre-activations of every relu are checked to be away from the kink
    (|pre| > 1e-6), so that float64 autograd alone is a fair reference; nothing else in either loss has a kink (the target y is
    a constant of both)."""
    import torch
    act, widths, norm, _, B, size = CASES[case]
    rng = np.random.default_rng(400 + case)
    pol, st, nrm, buf = _setup(rng, act, widths, norm, size)
    opts = T3.options(critic_widths=widths, batch_size=B, capacity=size, seed=5)
    sh = T3.Shapes(pol, opts)
    idx = T3.batch_indices(5, 0, size, B)
    x, a = buf["x"][idx], buf["a"][idx]
    y = (rng.standard_normal(B) * 2).astype(F)
    pre = []
    gc64, ga64 = _torch_grads(sh, st, nrm, x, a, y, torch.float64, pre)
    if act == "relu":
        assert min(float(p.abs().min()) for p in pre) > 1e-6, "a relu pre-activation sits on its kink: choose another seed"
    gc32, ga32 = _torch_grads(sh, st, nrm, x, a, y, torch.float32)
    gc, _ = T3.twin_critic_grad(lib, pol, st["psi"], nrm, x, a, y, opts)
    ga, _ = T3.twin_actor_grad(lib, pol, st["theta"], st["psi"], nrm, x, opts)
    c1, n1 = _terms("critic1", sh.D + sh.A, sh.q_widths)
    c2 = [(nm.replace("critic1", "critic2"), lo + n1, hi + n1) for nm, lo, hi in c1]
    at, _ = _terms("actor", sh.D, sh.pol_widths)
    failed = []
    for what, g, g64, g32, terms in (("critic", gc, gc64, gc32, c1 + c2), ("actor", ga, ga64, ga32, at)):
        assert g.shape == g64.shape
        scale = np.abs(g64).max()
        err_twin, err_f32 = np.abs(g.astype(np.float64) - g64).max() / scale, np.abs(g32 - g64).max() / scale
        print(f"case {case} {what} whole : twin {err_twin:.3e}  float32 autograd {err_f32:.3e}  ratio {err_twin / err_f32:.3f}")
        assert err_twin <= 2 * err_f32, what
        for name, lo, hi in terms:
            scale = np.abs(g64[lo:hi]).max()
            assert scale > 0, name
            err_twin = np.abs(g[lo:hi].astype(np.float64) - g64[lo:hi]).max() / scale
            err_f32 = np.abs(g32[lo:hi] - g64[lo:hi]).max() / scale
            print(f"case {case} {name:12s}: twin {err_twin:.3e}  float32 autograd {err_f32:.3e}")
            if not err_twin <= 2 * max(err_f32, 2.0 ** -23):
                failed.append((name, err_twin, err_f32))
    assert not failed, failed


def _chi2_quantile(k, z):
    """Wilson-Hilferty: the chi-square quantile at k degrees of freedom whose standard-normal quantile is z"""
    return k * (1.0 - 2.0 / (9.0 * k) + z * np.sqrt(2.0 / (9.0 * k))) ** 3


def test_batch_indices_are_uniform_and_inside(lib):
    """2^16 draws at size 1000: every slot is hit, and the chi-square statistic against uniform lies between the 1e-6 and the
    1 - 1e-6 quantiles of the chi-square distribution at 999 degrees of freedom (standard-normal quantile +-4.7534; by
    Wilson-Hilferty 800.7 and 1226.1; the distribution's mean is 999, its standard deviation 44.7)."""
    B, size = 1 << 16, 1000
    idx = T3.twin_batch_indices(lib, 9, 4, size, B)
    assert idx.min() >= 0 and idx.max() < size
    counts = np.bincount(idx, minlength=size)
    assert counts.min() > 0
    chi2 = float((((counts - B / size) ** 2) / (B / size)).sum())
    lo, hi = _chi2_quantile(999, -4.7534), _chi2_quantile(999, 4.7534)
    print(f"chi-square {chi2:.1f}, bound [{lo:.1f}, {hi:.1f}]")
    assert 800.0 < lo < 801.5 and 1225.0 < hi < 1227.0
    assert lo < chi2 < hi
    assert _same(idx[:4096], T3.batch_indices(9, 4, size, 4096))
    # the edges of the range: size 1 always reads slot 0; another update, another seed and another size read other slots
    assert not T3.twin_batch_indices(lib, 9, 4, 1, 64).any()
    for other in (T3.twin_batch_indices(lib, 9, 5, size, 256), T3.twin_batch_indices(lib, 10, 4, size, 256)):
        assert not _same(other, idx[:256])
    big = T3.twin_batch_indices(lib, 9, 4, 1 << 30, 4096)
    assert big.min() >= 0 and big.max() < (1 << 30) and big.max() > (1 << 29)
    for bad in ((9, -1, 10, 4), (9, 0, 0, 4), (9, 0, 10, 0)):
        out = np.zeros(4, np.int32)
        assert lib.adc_td3_batch_indices_host(*bad, out.ctypes.data) != 0


BAD = [dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=float("nan")), dict(tau=0.0), dict(tau=1.5), dict(tau=float("nan")), dict(policy_delay=0),
       dict(target_noise=-0.1), dict(target_noise_clip=-1.0), dict(action_lo=float("nan")), dict(reward_scale=0.0), dict(reward_scale=float("inf")),
       dict(batch_size=0), dict(batch_size=(1 << 20) + 1), dict(capacity=0), dict(n_critic_layers=0), dict(n_critic_layers=5),
       dict(critic_widths=(256, 256, 2, 0)), dict(critic_widths=(257, 256, 1, 0)), dict(critic_widths=(0, 256, 1, 0)), dict(actor_lr=-1e-3),
       dict(critic_lr=float("nan")), dict(beta1=1.0), dict(beta2=-0.5), dict(eps=0.0), dict(optimiser=7), dict(max_grad_norm=-1.0)]


@pytest.mark.parametrize("bad", BAD, ids=[next(iter(b)) + "=" + str(next(iter(b.values()))) for b in BAD])
def test_config_check_rejects_each_bad_field(lib, bad):
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    good = StepEngine.td3_config()
    msg = C.c_char_p()
    assert lib.adc_td3_config_check(C.byref(good), C.byref(msg)) == 0 and msg.value is None
    for k, v in bad.items():
        if k == "critic_widths":
            for i, w in enumerate(v):
                good.critic_widths[i] = w
        else:
            setattr(good, k, v)
    assert lib.adc_td3_config_check(C.byref(good), C.byref(msg)) == _ffi.ADC_EINVAL
    assert msg.value
    good = StepEngine.td3_config()
    good.struct_size += 4
    assert lib.adc_td3_config_check(C.byref(good), C.byref(msg)) == _ffi.ADC_EINVAL and b"struct_size" in msg.value
    assert lib.adc_td3_config_check(None, C.byref(msg)) == _ffi.ADC_EINVAL
    if not set(bad) & {"optimiser", "n_critic_layers", "critic_widths"}:
        with pytest.raises(ValueError):
            StepEngine.td3_config(**bad)
    if set(bad) & {"beta1", "beta2", "eps"}:                      # SGD does not look at Adam's fields
        StepEngine.td3_config(optimiser="sgd", **bad)


def test_python_surface(lib):
    from adcraft_amd.baselines import td3_trainer as T
    from adcraft_amd.engine import ShardedStepEngine, StepEngine
    d = T.td3()
    assert (d["gamma"], d["tau"], d["policy_delay"], d["target_noise"], d["target_noise_clip"], d["batch_size"], d["actor_lr"], d["critic_lr"],
            d["exploration_sigma"]) == (0.99, 0.005, 2, 0.2, 0.5, 256, 1e-3, 1e-3, 0.1)
    assert T.td3(tau=0.01)["tau"] == 0.01 and tuple(d["critic_hidden"]) == (256, 256)
    loop_keys = ("critic_hidden", "exploration_sigma", "learning_starts", "updates_per_iteration")
    c = StepEngine.td3_config(**{k: v for k, v in d.items() if k not in loop_keys})
    assert c.struct_size == C.sizeof(type(c)) and abs(c.tau - 0.005) < 1e-9 and c.policy_delay == 2 and c.batch_size == 256
    assert abs(c.target_noise - 0.2) < 1e-7 and abs(c.target_noise_clip - 0.5) < 1e-7 and list(c.critic_widths)[:3] == [256, 256, 1]
    c0 = StepEngine.td3_config()
    assert (c0.gamma, c0.tau, c0.policy_delay, c0.batch_size) == (c.gamma, c.tau, c.policy_delay, c.batch_size)
    with pytest.raises(ValueError, match="optimiser"):
        StepEngine.td3_config(optimiser="rmsprop")
    with pytest.raises(ValueError, match="critic_widths"):
        StepEngine.td3_config(critic_widths=())
    with pytest.raises(ValueError, match="one output"):
        StepEngine.td3_config(critic_widths=(8, 2))
    # random_critics: torch's default Linear initialisation on the D + A inputs, two different critics, seeded
    crit = T.random_critics(K, (12, 7), seed=3)
    assert len(crit) == 2 and [w.shape for w, _ in crit[0]] == [(6 * K + 3, 12), (12, 7), (7, 1)]
    for layers in crit:
        for w, b in layers:
            bound = 1.0 / np.sqrt(w.shape[0])
            assert w.dtype == F and b.dtype == F and np.abs(w).max() <= bound and np.abs(b).max() <= bound and np.abs(w).max() > 0.5 * bound
    assert not _same(crit[0][0][0], crit[1][0][0]) and _same(crit[0][0][0], T.random_critics(K, (12, 7), seed=3)[0][0][0])
    # the actor's flat order round-trips and is the restatement's
    rng = np.random.default_rng(2)
    pol = R.random_policy(rng, 3, (8, 4), value=True, normalize=True)
    theta = T.actor_params(pol)
    assert _same(theta, T3.flat_of(pol.layers))
    perm = rng.standard_normal(theta.size).astype(F)
    back = T.policy_from_actor(pol, perm)
    assert _same(T.actor_params(back), perm) and back.shapes() == pol.shapes() and back.shift is pol.shift
    with pytest.raises(ValueError):
        T.policy_from_actor(pol, perm[:-1])
    # a two-headed policy has no TD3 shape
    two = R.random_policy(rng, 3, (8,), two_heads=True)
    mcfg, cfg = two.config(3), StepEngine.td3_config(critic_widths=(4, 1))
    assert lib.adc_td3_param_counts_host(C.byref(mcfg), 3, C.byref(cfg), None, None) != 0
    sharded = object.__new__(ShardedStepEngine)
    for name in ("td3_init", "td3_set_critics", "td3_store", "td3_buffer", "td3_buffer_load", "td3_batch_indices", "td3_update", "td3_state"):
        with pytest.raises(NotImplementedError, match="engine_shards=1"):
            getattr(sharded, name)
