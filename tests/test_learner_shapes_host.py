"""The host twins at the wide, deep and ragged network shapes W1-W3 (tests/learner_shapes.py): adc_pg_grad_host, the TD3 twins
and the SAC twins against the numpy restatements bit for bit, and their gradients against PyTorch float64 autograd under the
yardstick of tests/test_pg_host.py - the reference not derived from the law, here with sum8 over 256 terms and gradients of up to
665 k parameters.  The restated LDS counts and the last K that fits them are pinned too.  No device is needed; the device's side
of the same shapes is tests/test_gpu_learner_shapes.py.  Measured figures: profiles/pr_learner_shapes.txt."""
import time

import numpy as np
import pytest

from tests import learner_shapes as W
from tests import pg_ref as P
from tests import sac_ref as S
from tests import td3_ref as T3
from tests.test_pg_host import _batch, _torch_grad
from tests.test_sac_host import _torch_grads as _sac_torch_grads
from tests.test_td3_host import _setup as _td3_setup
from tests.test_td3_host import _torch_grads as _td3_torch_grads

F = np.float32
NAMES = ("W1", "W2", "W3")
SAMPLES = 40                    # (the device tests' count: 5 days of 8 envs, below one 1024-sample chunk)
# the drift of theta from the collecting policy: 0.03 (tests/test_pg_host.py) moves a 256-wide layer's outputs by whole units and
# every ratio past the clip; these leave clipped and unclipped samples
DRIFT = dict(W1=3e-3, W2=3e-3, W3=3e-4)
PG_OPTS = dict(W1=dict(ent_coef=0.01), W2=dict(vf_coef=1.0), W3=dict(ent_coef=0.02))


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _pg_case(name):
    rng = np.random.default_rng(530 + NAMES.index(name))
    pol = W.pg_policy(rng, name)
    return pol, _batch(rng, pol, SAMPLES, drift=DRIFT[name]), P.options(**PG_OPTS[name])


@pytest.mark.parametrize("name", NAMES)
def test_pg_grad_twin_equals_the_restatement_bit_for_bit(lib, name):
    pol, batch, opts = _pg_case(name)
    t0 = time.perf_counter()
    rg, rsums, rst = P.grad(pol, *batch, **opts)
    t1 = time.perf_counter()
    g, sums, st = P.twin_grad(lib, pol, *batch, **opts)
    print(f"{name} PG: {g.size} parameters, restatement {t1 - t0:.2f} s, twin {time.perf_counter() - t1:.2f} s")
    assert _same(g, rg) and _same(sums, rsums)
    for k in P.STAT_KEYS:
        assert _same(np.float64(st[k]), np.float64(rst[k])), k
    W.assert_terms_alive(g, W.pg_terms(pol), name)
    assert 0.0 < st["clip_fraction"] < 1.0
    s = W.SHAPES[name]
    if s["clamp"] is not None and not s["two"]:
        ls = P.unflatten(pol, batch[0])[2]
        moved = (ls < s["clamp"][0]) | (ls > s["clamp"][1])
        assert moved.any() and not moved.all() and np.all(g[-ls.size:][moved] == 0) and np.all(g[-ls.size:][~moved] != 0)


@pytest.mark.parametrize("name", NAMES)
def test_pg_gradient_against_pytorch_autograd(lib, name):
    import torch
    pol, batch, opts = _pg_case(name)
    layers, value_layers, _ = P.unflatten(pol, batch[0])
    if pol.activation == "relu":
        assert W.relu_margin(batch[1], layers, value_layers) > 1e-6, "a relu pre-activation sits on its kink: choose another seed"
    g, _, _ = P.twin_grad(lib, pol, *batch, **opts)
    g64, g32 = _torch_grad(pol, *batch, torch.float64, opts), _torch_grad(pol, *batch, torch.float32, opts)
    W.yardstick(f"{name} PG twin", g, g64, g32, W.pg_terms(pol))


def _td3_case(name, seed):
    s = W.SHAPES[name]
    rng = np.random.default_rng(seed)
    pol, st, nrm, buf = _td3_setup(rng, s["act"], s["critics"], True, 37, hidden=s["hidden"], K=s["K"])
    return pol, st, nrm, buf, s


@pytest.mark.parametrize("name", NAMES)
def test_td3_twins_equal_the_restatement(lib, name):
    pol, st, nrm, buf, s = _td3_case(name, 600 + NAMES.index(name))
    B, size, seed, u = 8, 37, 91, 2
    opts = T3.options(critic_widths=s["critics"], batch_size=B, capacity=size, seed=seed, reward_scale=0.5, gamma=0.9, target_noise=0.6,
                      target_noise_clip=0.5, action_lo=-0.4, action_hi=0.9)
    sh = T3.Shapes(pol, opts)
    idx = T3.batch_indices(seed, u, size, B)
    done = buf["done"][idx]
    t0 = time.perf_counter()
    y = T3.target(sh, st["theta_target"], st["psi_target"], nrm, seed, u, buf["x2"][idx], buf["r"][idx], done, opts)
    g, sums = T3.critic_grad(sh, st["psi"], nrm, buf["x"][idx], buf["a"][idx], y)
    ga, sa = T3.actor_grad(sh, st["theta"], st["psi"], nrm, buf["x"][idx])
    print(f"{name} TD3: actor {ga.size}, critics {g.size} parameters, restatement {time.perf_counter() - t0:.2f} s")
    assert _same(T3.twin_target(lib, pol, st["theta_target"], st["psi_target"], nrm, seed, u, buf["x2"][idx], buf["r"][idx], done, opts), y)
    tg, tsums = T3.twin_critic_grad(lib, pol, st["psi"], nrm, buf["x"][idx], buf["a"][idx], y, opts)
    assert _same(tg, g) and _same(tsums, sums)
    tga, tsa = T3.twin_actor_grad(lib, pol, st["theta"], st["psi"], nrm, buf["x"][idx], opts)
    assert _same(tga, ga) and _same(tsa, sa)
    ct, at = W.offpolicy_terms(sh)
    W.assert_terms_alive(g, ct, name)
    W.assert_terms_alive(ga, at, name)


@pytest.mark.parametrize("name", NAMES)
def test_td3_gradients_against_pytorch_autograd(lib, name):
    import torch
    pol, st, nrm, buf, s = _td3_case(name, 700 + NAMES.index(name))
    B, size = 8, 37
    opts = T3.options(critic_widths=s["critics"], batch_size=B, capacity=size, seed=5)
    sh = T3.Shapes(pol, opts)
    idx = T3.batch_indices(5, 0, size, B)
    x, a = buf["x"][idx], buf["a"][idx]
    y = (np.random.default_rng(1).standard_normal(B) * 2).astype(F)
    pre = []
    gc64, ga64 = _td3_torch_grads(sh, st, nrm, x, a, y, torch.float64, pre)
    if s["act"] == "relu":
        assert min(float(p.abs().min()) for p in pre) > 1e-6, "a relu pre-activation sits on its kink: choose another seed"
    gc32, ga32 = _td3_torch_grads(sh, st, nrm, x, a, y, torch.float32)
    gc, _ = T3.twin_critic_grad(lib, pol, st["psi"], nrm, x, a, y, opts)
    ga, _ = T3.twin_actor_grad(lib, pol, st["theta"], st["psi"], nrm, x, opts)
    ct, at = W.offpolicy_terms(sh)
    W.yardstick(f"{name} TD3 critic twin", gc, gc64, gc32, ct)
    W.yardstick(f"{name} TD3 actor twin", ga, ga64, ga32, at)


def _sac_case(name, seed, size=37):
    s = W.SHAPES[name]
    rng = np.random.default_rng(seed)
    pol = W.sac_policy(rng, name, scale=0.5)
    crit = W.critics(rng, name)
    opts = S.options(s["K"], critic_widths=s["critics"], capacity=size)
    st = S.fresh_state(pol, crit, opts)
    st["psi_target"] = (st["psi_target"] + rng.standard_normal(st["psi_target"].size).astype(F) * F(0.05)).astype(F)
    A, D = s["K"] + 1, 5 * s["K"] + 2
    buf = dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * 1.5).astype(F),
               r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))
    buf["done"][0], buf["done"][1] = True, False
    return pol, st, buf, s


@pytest.mark.parametrize("name", NAMES)
def test_sac_twins_equal_the_restatement(lib, name):
    pol, st, buf, s = _sac_case(name, 800 + NAMES.index(name))
    K, B, size, seed, u, alpha = s["K"], 8, 37, 33, 3, F(0.37)
    opts = S.options(K, critic_widths=s["critics"], batch_size=B, capacity=size, seed=seed, reward_scale=0.5, gamma=0.9, eps_sq=1e-6)
    sh = T3.Shapes(pol, opts)
    idx = T3.batch_indices(seed, u, size, B)
    done = buf["done"][idx]
    t0 = time.perf_counter()
    y, lp2 = S.target(sh, pol.log_std_clamp, st["theta"], st["psi_target"], alpha, seed, u, buf["x2"][idx], buf["r"][idx], done, opts)
    g, sums = S.critic_grad(sh, st["psi"], buf["x"][idx], buf["a"][idx], y)
    ga, lpa, sa = S.actor_grad(sh, pol.log_std_clamp, st["theta"], st["psi"], alpha, seed, u, buf["x"][idx], opts)
    print(f"{name} SAC: actor {ga.size}, critics {g.size} parameters, restatement {time.perf_counter() - t0:.2f} s")
    ty, tlp2 = S.twin_target(lib, pol, st["theta"], st["psi_target"], alpha, seed, u, buf["x2"][idx], buf["r"][idx], done, opts)
    assert _same(ty, y) and _same(tlp2, lp2) and np.isfinite(y).all()
    tg, tsums = S.twin_critic_grad(lib, pol, st["psi"], buf["x"][idx], buf["a"][idx], y, opts)
    assert _same(tg, g) and _same(tsums, sums)
    tga, tlpa, tsa = S.twin_actor_grad(lib, pol, st["theta"], st["psi"], alpha, seed, u, buf["x"][idx], opts)
    assert _same(tga, ga) and _same(tlpa, lpa) and _same(tsa, sa)
    ct, at = W.offpolicy_terms(sh)
    W.assert_terms_alive(g, ct, name)
    W.assert_terms_alive(ga, at, name)
    raw = T3.forward(buf["x"][idx], sh.actor(st["theta"]), sh.act)[-1][:, K + 1:]
    moved = (raw < F(pol.log_std_clamp[0])) | (raw > F(pol.log_std_clamp[1]))
    assert moved.any() and not moved.all(), "the clamp was meant to move some log-stds and not others"


@pytest.mark.parametrize("name", NAMES)
def test_sac_gradients_against_pytorch_autograd(lib, name):
    import torch
    pol, st, buf, s = _sac_case(name, 900 + NAMES.index(name))
    K, B, size, alpha, upd, clamp = s["K"], 8, 37, F(0.3), 1, pol.log_std_clamp
    opts = S.options(K, critic_widths=s["critics"], batch_size=B, capacity=size, seed=5)
    sh = T3.Shapes(pol, opts)
    idx = T3.batch_indices(5, upd, size, B)
    x, u = buf["x"][idx], buf["a"][idx]
    y = (np.random.default_rng(1).standard_normal(B) * 2).astype(F)
    z = S.noise(5, S.ST_SAC_PI, upd, B, sh.A)
    checks = {}
    gc64, ga64 = _sac_torch_grads(sh, st, clamp, alpha, opts["eps_sq"], x, u, y, z, torch.float64, checks)
    if s["act"] == "relu":
        assert min(float(p.abs().min()) for p in checks["pre"]) > 1e-6, "a relu pre-activation sits on its kink: choose another seed"
    assert checks["dq"] > 1e-6, "two critic values tie: choose another seed"
    raw = checks["raw"]
    assert min(np.abs(raw - float(F(clamp[0]))).min(), np.abs(raw - float(F(clamp[1]))).min()) > 1e-6, "a raw log-std sits on the clamp"
    gc32, ga32 = _sac_torch_grads(sh, st, clamp, alpha, opts["eps_sq"], x, u, y, z, torch.float32)
    gc, _ = S.twin_critic_grad(lib, pol, st["psi"], x, u, y, opts)
    ga, _, _ = S.twin_actor_grad(lib, pol, st["theta"], st["psi"], alpha, 5, upd, x, opts)
    ct, at = W.offpolicy_terms(sh)
    W.yardstick(f"{name} SAC critic twin", gc, gc64, gc32, ct)
    W.yardstick(f"{name} SAC actor twin", ga, ga64, ga32, at)


def test_the_restated_lds_counts_and_the_last_keyword_count_that_fits():
    """the closed forms of the four counts under the widest networks, from the layouts written at the top of kernel_pg.inc,
    kernel_td3.inc and kernel_sac.inc, and the K they put one step from the refusal"""
    for K in (300, 700, 1059, 1483):
        assert W.widest_count("pg", K) == 14 * K + 1548
        assert W.widest_count("pg_kl", K) == 16 * K + 1550
        assert W.widest_count("td3", K) == 10 * K + 1548
        assert W.widest_count("sac", K) == 20 * K + 2331
    assert [W.boundary_K(f) for f in ("pg", "pg_kl", "td3", "sac")] == [1059, 927, 1483, 702]
    assert W.boundary_K("pg", frames=8) == 302 and W.widest_count("pg", 303, frames=1) <= W.LDS_FLOATS
    # the counts of tests/test_gpu_pg_trainer.py's refusals are the same functions at their narrow shape
    assert W.pg_lds_floats(1488, [8, 1489], [8, 1]) == 11 * 1488 + 25 and W.pg_lds_floats(1259, [8, 1260], [8, 1], kl=True) == 13 * 1259 + 27
