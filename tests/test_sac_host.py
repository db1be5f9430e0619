"""Soft actor-critic on the host: the twins adc_sac_logp_host / adc_sac_target_host / adc_sac_critic_grad_host /
adc_sac_actor_grad_host / adc_sac_alpha_step_host and adc_mlp_squash_host (the code the device kernels run, adc_sac.h and
adc_mlp.h) against the numpy restatement in tests/sac_ref.py bit for bit, both gradients against PyTorch float64 autograd, the
law's edge cases, the configuration checks and the trainer's preset.  No device is needed.  None of these symbols exists before this feature."""
import ctypes as C

import numpy as np
import pytest

from tests import mlp_ref as R
from tests import sac_ref as S
from tests import td3_ref as T3

F = np.float32


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _setup(rng, K, act, hidden, widths, size, clamp=(-1.0, -0.5), scale=0.5):
    """a two-headed policy, a state whose targets differ from the live critics, and a ring of `size` rows holding unsquashed actions"""
    pol = S.sac_policy(rng, K, hidden, act, clamp=clamp, scale=scale)
    critics = T3.random_critics_for_tests(rng, K, widths)
    opts = S.options(K, critic_widths=widths, capacity=size)
    st = S.fresh_state(pol, critics, opts)
    st["psi_target"] = (st["psi_target"] + rng.standard_normal(st["psi_target"].size).astype(F) * F(0.05)).astype(F)
    A, D = K + 1, 5 * K + 2
    buf = dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=(rng.standard_normal((size, A)) * 1.5).astype(F),
               r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))
    return pol, st, buf


# K, activation, hidden, critic widths, batch, ring size: A = 2, 3, 10 (the % 4 and % 8 tails); batch 1030 crosses a 1024-sample chunk
CASES = [
    (1, "tanh", (16, 8), (12, 1), 7, 5),
    (2, "relu", (12,), (1,), 7, 5),
    (9, "tanh", (), (12, 1), 7, 37),
    (9, "relu", (16, 8), (1,), 7, 37),
    (2, "tanh", (12,), (12, 1), 1030, 84),
    (9, "relu", (), (12, 1), 1030, 84),
    (1, "relu", (16, 8), (1,), 1030, 84),
    (9, "tanh", (16, 8), (12, 1), 1030, 84),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_twins_equal_the_restatement(lib, case):
    K, act, hidden, widths, B, size = CASES[case]
    rng = np.random.default_rng(900 + case)
    pol, st, buf = _setup(rng, K, act, hidden, widths, size)
    opts = S.options(K, critic_widths=widths, batch_size=B, capacity=size, seed=31 + case, reward_scale=0.5, gamma=0.9, eps_sq=1e-6)
    sh, seed, u, alpha, A = T3.Shapes(pol, opts), opts["seed"], 2 + case, F(0.37), K + 1
    p, q = C.c_int64(0), C.c_int64(0)
    cfg, mcfg = S.sac_config(K, **opts), pol.config(K)
    assert lib.adc_sac_param_counts_host(C.byref(mcfg), K, C.byref(cfg), C.byref(p), C.byref(q)) == 0
    assert (p.value, q.value) == (sh.P, sh.Qc) == (st["theta"].size, st["psi"].size // 2)
    idx = T3.batch_indices(seed, u, size, B)
    slots = np.unique(idx)
    buf["done"][slots[0]], buf["done"][slots[1]] = True, False
    done = buf["done"][idx]
    # lp and the squash
    mean, raw, z = (rng.standard_normal((B, A)).astype(F) for _ in range(3))
    raw = (raw * F(0.5) - F(0.75)).astype(F)                             # both sides of the clamp [-1, -0.5] and inside it
    h = S.head(np.concatenate([mean, raw], axis=1), z, pol.log_std_clamp, 1e-6)
    assert h["moved"].any() and not h["moved"].all()
    tu, tt, tlp = S.twin_logp(lib, pol, 1e-6, mean, raw, z)
    assert _same(tu, h["u"]) and _same(tt, h["t"]) and _same(tlp, h["lp"]) and np.isfinite(tlp).all()
    lo, hi = (rng.random(A) * 0.5).astype(F), (1.0 + rng.random(A) * 20).astype(F)
    assert _same(S.twin_squash(lib, h["u"][0], lo, hi), S.squash(h["u"][0], lo, hi))
    # the soft target under the live actor
    y, lp2 = S.target(sh, pol.log_std_clamp, st["theta"], st["psi_target"], alpha, seed, u, buf["x2"][idx], buf["r"][idx], done, opts)
    ty, tlp2 = S.twin_target(lib, pol, st["theta"], st["psi_target"], alpha, seed, u, buf["x2"][idx], buf["r"][idx], done, opts)
    assert _same(ty, y) and _same(tlp2, lp2)
    assert np.isfinite(y).all() and _same(y[done], (buf["r"][idx][done] * F(0.5)).astype(F)), "a day that ends an episode bootstraps nothing"
    # the critics' gradient on [x | tanh(u)]
    g, sums = S.critic_grad(sh, st["psi"], buf["x"][idx], buf["a"][idx], y)
    tg, tsums = S.twin_critic_grad(lib, pol, st["psi"], buf["x"][idx], buf["a"][idx], y, opts)
    assert _same(tg, g) and _same(tsums, sums) and np.abs(g).max() > 0
    # the actor's gradient through the smaller critic, and the temperature's step from its lp
    ga, lpa, sa = S.actor_grad(sh, pol.log_std_clamp, st["theta"], st["psi"], alpha, seed, u, buf["x"][idx], opts)
    tga, tlpa, tsa = S.twin_actor_grad(lib, pol, st["theta"], st["psi"], alpha, seed, u, buf["x"][idx], opts)
    assert _same(tga, ga) and _same(tlpa, lpa) and _same(tsa, sa) and np.abs(ga).max() > 0
    if B > 100:
        assert 0 < sa[3] < B, "both critics were meant to be picked"
    la3 = np.array([S.log_alpha_init(0.7), 0.01, 0.002], F)
    assert _same(np.array([lib.adc_sac_log_alpha_init_host(0.7)], F), la3[:1])
    new, a2 = S.twin_alpha_step(lib, K, la3, sa[1], B, u, opts)
    assert _same(new, S.alpha_step(la3, sa[1], B, u, opts)) and _same(np.array([a2], F), np.array([S.alpha_of(new[0])], F))
    assert not _same(new, la3)


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


def _torch_grads(sh, st, clamp, alpha, eps_sq, x, u, y, z, dtype, checks=None):
    """(critic gradient [2 Qc], actor gradient [P]) by autograd in `dtype`: the stated losses with z, alpha and y held constant"""
    import torch
    t = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype)
    pre = [] if checks is not None else None
    critics, cp = _torch_nets(sh.critics(st["psi"]), dtype)
    row = torch.cat([t(x), torch.tanh(t(u))], dim=1)
    loss = sum((0.5 * (_torch_forward(net, row, sh.act, pre)[:, 0] - t(y)) ** 2).mean() for net in critics)
    loss.backward()
    gc = np.concatenate([p.grad.detach().numpy().astype(np.float64).reshape(-1) for p in cp])
    (actor,), ap = _torch_nets([sh.actor(st["theta"])], dtype)
    (q1, q2), _ = _torch_nets(sh.critics(st["psi"]), dtype)
    o = _torch_forward(actor, t(x), sh.act, pre)
    A = sh.A
    mean, raw = o[:, :A], o[:, A:]
    ls = torch.clamp(raw, float(F(clamp[0])), float(F(clamp[1])))
    uu = mean + torch.exp(ls) * t(z)
    tt = torch.tanh(uu)
    lp = (-(t(z) ** 2) * 0.5 - ls).sum(dim=1) - A * float(R.HALF_LOG_2PI) - torch.log(1 - tt * tt + float(F(eps_sq))).sum(dim=1)
    rowp = torch.cat([t(x), tt], dim=1)
    qa, qb = _torch_forward(q1, rowp, sh.act, pre)[:, 0], _torch_forward(q2, rowp, sh.act, pre)[:, 0]
    (float(alpha) * lp - torch.minimum(qa, qb)).mean().backward()
    ga = np.concatenate([p.grad.detach().numpy().astype(np.float64).reshape(-1) for p in ap])
    if checks is not None:
        checks.update(pre=pre, dq=(qa - qb).detach().abs().min().item(), raw=raw.detach().numpy())
    return gc, ga


def _terms(name, n_in, widths):
    out, pos = [], 0
    for l, n_out in enumerate(widths):
        out += [(f"{name} W{l}", pos, pos + n_in * n_out), (f"{name} b{l}", pos + n_in * n_out, pos + (n_in + 1) * n_out)]
        pos += (n_in + 1) * n_out
        n_in = n_out
    return out, pos


@pytest.mark.parametrize("case", [0, 1, 2, 3, 4, 5])
def test_gradients_against_pytorch_autograd(lib, case):
    """Both gradients against float64 autograd with the yardstick of tests/test_td3_host.py: the twin's error (largest absolute
    difference over the largest float64 entry) is at most twice float32 autograd's own, over the whole gradient and in every term
    on its own, the per-term yardstick not taken below 2^-23.  The losses are the stated ones with the law's z, alpha and y held
    constant.  First the inputs are checked to lie away from the kinks: every relu pre-activation (|pre| > 1e-6), the two critics'
    values (|q1 - q2| > 1e-6), and the raw log-stds against the clamp's bounds (|raw - bound| > 1e-6): outside the clamp the law
    gives +0, as torch.clamp does."""
    import torch
    K, act, hidden, widths, B, size = CASES[case]
    B = min(B, 64)
    rng = np.random.default_rng(1200 + case)
    clamp = (-1.0, -0.5)
    pol, st, buf = _setup(rng, K, act, hidden, widths, size, clamp=clamp)
    opts = S.options(K, critic_widths=widths, batch_size=B, capacity=size, seed=5)
    sh, alpha, upd = T3.Shapes(pol, opts), F(0.3), 1
    idx = T3.batch_indices(5, upd, size, B)
    x, u = buf["x"][idx], buf["a"][idx]
    y = (rng.standard_normal(B) * 2).astype(F)
    z = S.noise(5, S.ST_SAC_PI, upd, B, sh.A)
    checks = {}
    gc64, ga64 = _torch_grads(sh, st, clamp, alpha, opts["eps_sq"], x, u, y, z, torch.float64, checks)
    if act == "relu" and checks["pre"]:
        assert min(float(p.abs().min()) for p in checks["pre"]) > 1e-6, "a relu pre-activation sits on its kink: choose another seed"
    assert checks["dq"] > 1e-6, "two critic values tie: choose another seed"
    raw = checks["raw"]
    assert min(np.abs(raw - float(F(clamp[0]))).min(), np.abs(raw - float(F(clamp[1]))).min()) > 1e-6, "a raw log-std sits on the clamp: choose another seed"
    assert (raw < clamp[0]).any() or (raw > clamp[1]).any(), "the clamp was meant to move some log-stds"
    gc32, ga32 = _torch_grads(sh, st, clamp, alpha, opts["eps_sq"], x, u, y, z, torch.float32)
    gc, _ = S.twin_critic_grad(lib, pol, st["psi"], x, u, y, opts)
    ga, _, _ = S.twin_actor_grad(lib, pol, st["theta"], st["psi"], alpha, 5, upd, x, opts)
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


def test_tie_takes_critic_one_and_a_smaller_critic_two_is_taken(lib):
    K, act, hidden, widths, B, size = CASES[3][0], "tanh", (16, 8), (12, 1), 7, 37
    rng = np.random.default_rng(77)
    pol, st, buf = _setup(rng, K, act, hidden, widths, size)
    opts = S.options(K, critic_widths=widths, batch_size=B, capacity=size, seed=3)
    sh = T3.Shapes(pol, opts)
    x = buf["x"][:B]
    psi = st["psi"].copy()
    psi[sh.Qc:] = psi[:sh.Qc]                                            # identical critics: q1 == q2 in every element
    g, _, s4 = S.twin_actor_grad(lib, pol, st["theta"], psi, 0.2, 3, 0, x, opts)
    rg, _, r4 = S.actor_grad(sh, pol.log_std_clamp, st["theta"], psi, 0.2, 3, 0, x, opts)
    assert s4[3] == 0 and _same(g, rg) and _same(s4, r4)
    psi2 = psi.copy()
    psi2[-1] = psi2[-1] - F(0.25)                                         # critic 2's last bias: q2 = q1 - 0.25
    g2, _, t4 = S.twin_actor_grad(lib, pol, st["theta"], psi2, 0.2, 3, 0, x, opts)
    rg2, _, u4 = S.actor_grad(sh, pol.log_std_clamp, st["theta"], psi2, 0.2, 3, 0, x, opts)
    assert t4[3] == B and _same(g2, rg2) and _same(t4, u4)
    assert _same(g2, g), "a bias shifts the value, not its input gradient"
    assert abs((t4[0] - s4[0]) / B - 0.25) < 1e-5


def test_saturated_actions_give_finite_lp_and_deltas(lib):
    """|u| >= 10: t = +-1, w = 0; lp and du stay finite (eps_sq inside the logarithm and the quotient)"""
    K = 2
    rng = np.random.default_rng(5)
    pol = S.sac_policy(rng, K, (12,), "tanh", clamp=(-1.0, 2.0))
    A = K + 1
    mean = np.array([[12.0, -15.0, 10.0], [0.1, 40.0, -10.0]], F)
    raw, z = np.zeros((2, A), F), np.zeros((2, A), F)
    u, t, lp = S.twin_logp(lib, pol, 1e-6, mean, raw, z)
    h = S.head(np.concatenate([mean, raw], axis=1), z, pol.log_std_clamp, 1e-6)
    assert _same(lp, h["lp"]) and np.isfinite(lp).all()
    assert (np.abs(t[0]) == 1).all() and (h["w"][0] == 0).all()
    # a policy whose last bias saturates every action: the actor's gradient stays finite
    pol.layers[-1] = (pol.layers[-1][0], np.concatenate([np.full(A, 20.0, F), np.zeros(A, F)]))
    critics = T3.random_critics_for_tests(rng, K, (12, 1))
    opts = S.options(K, critic_widths=(12, 1), batch_size=5, capacity=5, seed=1)
    st = S.fresh_state(pol, critics, opts)
    x = (rng.standard_normal((5, 5 * K + 2)) * 0.5).astype(F)
    g, lpa, s4 = S.twin_actor_grad(lib, pol, st["theta"], st["psi"], 0.5, 1, 0, x, opts)
    rg, _, r4 = S.actor_grad(T3.Shapes(pol, opts), pol.log_std_clamp, st["theta"], st["psi"], 0.5, 1, 0, x, opts)
    assert np.isfinite(g).all() and np.isfinite(lpa).all() and _same(g, rg) and _same(s4, r4)


def test_alpha_lr_zero_leaves_log_alpha(lib):
    """alpha_lr == 0: the twin leaves log_alpha and its moments bit for bit and reports exp(log_alpha).  (The target_update_interval
    gate and the skipped temperature step of the device are tests/test_gpu_sac_trainer.py's.)"""
    K, B = 2, 7
    opts = S.options(K, critic_widths=(12, 1), batch_size=B, capacity=20, seed=2, alpha_lr=0.0, init_alpha=0.7, target_update_interval=3)
    la3 = np.array([S.log_alpha_init(0.7), 0.25, 0.5], F)
    new, alpha = S.twin_alpha_step(lib, K, la3, -12.5, B, 0, opts)
    assert _same(new, la3) and _same(np.array([alpha], F), np.array([S.alpha_of(la3[0])], F))
    assert _same(S.alpha_step(la3, -12.5, B, 0, opts), la3)


def test_interval_three_moves_the_targets_on_every_third_update(lib):
    """target_update_interval = 3 through whole updates built from the host twins (target, both gradients, the temperature's step;
    the optimiser step and Polyak are adc_pg_step_host's and adc_td3_polyak_host's): the state equals the restatement's after each
    of six updates, and the target critics move on updates 3 and 6 alone.  The device's gate is tests/test_gpu_sac_trainer.py's."""
    K, act, hidden, widths, B, size = 2, "tanh", (12,), (12, 1), 7, 20
    rng = np.random.default_rng(11)
    pol, _, buf = _setup(rng, K, act, hidden, widths, size)
    opts = S.options(K, critic_widths=widths, batch_size=B, capacity=size, seed=2, alpha_lr=3e-3, init_alpha=0.7, target_update_interval=3, tau=0.05)
    ref = S.fresh_state(pol, T3.random_critics_for_tests(rng, K, widths), opts)
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
    moved = []
    for u in range(6):
        alpha = S.alpha_of(st["log_alpha"][0])
        idx = T3.twin_batch_indices(lib, 2, u, size, B)
        x = buf["x"][idx]
        y, _ = S.twin_target(lib, pol, st["theta"], st["psi_target"], alpha, 2, u, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
        g, _ = S.twin_critic_grad(lib, pol, st["psi"], x, buf["a"][idx], y, opts)
        st["psi"], st["m_psi"], st["v_psi"] = T3._step(st["psi"], st["m_psi"], st["v_psi"], g, u, opts["critic_lr"], opts)
        g, _, s4 = S.twin_actor_grad(lib, pol, st["theta"], st["psi"], alpha, 2, u, x, opts)
        st["theta"], st["m_theta"], st["v_theta"] = T3._step(st["theta"], st["m_theta"], st["v_theta"], g, u, opts["actor_lr"], opts)
        st["log_alpha"], _ = S.twin_alpha_step(lib, K, st["log_alpha"], s4[1], B, u, opts)
        before = st["psi_target"].copy()
        if (u + 1) % 3 == 0:
            st["psi_target"] = T3.twin_polyak(lib, st["psi_target"], st["psi"], opts["tau"])
        st["updates"] = u + 1
        ref, _ = S.update(pol, ref, buf, 2, opts)
        for k in S.STATE_KEYS:
            assert _same(st[k], ref[k]), (k, u)
        moved.append(not _same(before, ref["psi_target"]))
    assert moved == [False, False, True, False, False, True]


BAD = [(dict(gamma=1.5), "gamma: 0 to 1"), (dict(gamma=float("nan")), "gamma: 0 to 1"), (dict(tau=0.0), "tau: above 0, at most 1"),
       (dict(tau=1.5), "tau: above 0, at most 1"), (dict(target_update_interval=0), "target_update_interval >= 1"),
       (dict(init_alpha=0.0), "init_alpha: above 0, finite"), (dict(init_alpha=float("inf")), "init_alpha: above 0, finite"),
       (dict(target_entropy=float("nan")), "target_entropy must be finite"), (dict(target_entropy=float("-inf")), "target_entropy must be finite"),
       (dict(alpha_lr=-1e-3), "alpha_lr >= 0 (0: alpha stays)"), (dict(eps_sq=0.0), "eps_sq: above 0, finite"),
       (dict(eps_sq=float("nan")), "eps_sq: above 0, finite"), (dict(reward_scale=0.0), "reward_scale must be finite and not 0"),
       (dict(reward_scale=float("inf")), "reward_scale must be finite and not 0"), (dict(batch_size=0), "batch_size: 1 to 2^20"),
       (dict(batch_size=(1 << 20) + 1), "batch_size: 1 to 2^20"), (dict(capacity=0), "capacity: 1 to 2^30"),
       (dict(n_critic_layers=0), "n_critic_layers: 1 to 4"), (dict(n_critic_layers=5), "n_critic_layers: 1 to 4"),
       (dict(critic_widths=(256, 256, 2, 0)), "the last critic layer has one output"),
       (dict(critic_widths=(257, 256, 1, 0)), "hidden critic widths: 1 to 256"), (dict(critic_widths=(0, 256, 1, 0)), "hidden critic widths: 1 to 256"),
       (dict(actor_lr=-1e-3), "actor_lr >= 0"), (dict(critic_lr=float("nan")), "critic_lr >= 0"), (dict(beta1=1.0), "Adam: 0 <= beta1, beta2 < 1"),
       (dict(beta2=-0.5), "Adam: 0 <= beta1, beta2 < 1"), (dict(eps=0.0), "Adam: eps > 0"), (dict(optimiser=7), "unknown optimiser"),
       (dict(max_grad_norm=-1.0), "max_grad_norm >= 0 (0: off)"), (dict(struct_size=4), "adc_sac_config: NULL or struct_size mismatch")]


@pytest.mark.parametrize("bad,message", BAD, ids=[next(iter(b)) + "=" + str(next(iter(b.values()))) for b, _ in BAD])
def test_config_check_rejects_each_bad_field(lib, bad, message):
    from adcraft_amd import _ffi
    good = S.sac_config(9)
    msg = C.c_char_p()
    assert lib.adc_sac_config_check(C.byref(good), C.byref(msg)) == _ffi.ADC_OK and msg.value is None
    for k, v in bad.items():
        if k == "critic_widths":
            for i, w in enumerate(v):
                good.critic_widths[i] = w
        else:
            setattr(good, k, v)
    assert lib.adc_sac_config_check(C.byref(good), C.byref(msg)) == _ffi.ADC_EINVAL
    assert msg.value.decode() == message
    assert lib.adc_sac_config_check(None, C.byref(msg)) == _ffi.ADC_EINVAL and msg.value.decode() == "adc_sac_config: NULL or struct_size mismatch"


def test_preset_and_python_surface():
    from adcraft_amd.engine import StepEngine
    c = StepEngine.sac_config(num_keywords=9)
    assert (c.tau, c.init_alpha, c.target_entropy, c.batch_size) == (F(5e-3), 1.0, -10.0, 256)
    assert c.actor_lr == c.critic_lr == c.alpha_lr == F(3e-4)
    with pytest.raises(ValueError, match="tau"):
        StepEngine.sac_config(num_keywords=9, tau=0.0)
    with pytest.raises(ValueError, match="target_entropy"):
        StepEngine.sac_config()


def test_the_trainers_preset_is_rllibs_sac():
    """baselines/sac_trainer.sac(): tau 5e-3, the three learning rates 3e-4, init_alpha 1, target_entropy -A, batch 256 - and the
    engine's configuration built from it carries them"""
    from adcraft_amd.baselines.sac_trainer import SquashedPolicy, sac
    from adcraft_amd.engine import StepEngine
    K = 9
    p = sac(K)
    assert (p["tau"], p["actor_lr"], p["critic_lr"], p["alpha_lr"], p["init_alpha"], p["target_entropy"], p["batch_size"]) == \
        (5e-3, 3e-4, 3e-4, 3e-4, 1.0, -float(K + 1), 256)
    assert p["critic_hidden"] == (256, 256) and p["target_update_interval"] == 1 and p["gamma"] == 0.99
    assert sac(K, tau=0.01)["tau"] == 0.01
    trainer_only = ("critic_hidden", "learning_starts", "updates_per_iteration")
    c = StepEngine.sac_config(num_keywords=K, critic_widths=p["critic_hidden"] + (1,), **{k: v for k, v in p.items() if k not in trainer_only})
    assert (c.tau, c.actor_lr, c.critic_lr, c.alpha_lr, c.init_alpha, c.target_entropy, c.batch_size) == (F(5e-3), F(3e-4), F(3e-4), F(3e-4), 1.0, -10.0, 256)
    assert list(c.critic_widths)[:3] == [256, 256, 1] and c.n_critic_layers == 3
    rng = np.random.default_rng(3)
    pol = S.sac_policy(rng, K, (8,))
    sq = SquashedPolicy(pol, np.zeros(K + 1), np.ones(K + 1))
    assert sq.policy is pol and sq.action_lo.dtype == F and sq.action_hi.shape == (K + 1,)
