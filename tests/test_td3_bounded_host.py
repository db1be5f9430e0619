"""The bounded act and bounded TD3 on the host: the twins adc_mlp_bounded_host / adc_mlp_unbox_host / adc_td3_bounded_target_host /
adc_td3_bounded_actor_grad_host (the code the device kernels run: adc_mlp.h "bounded", adc_td3.h "bounded") against the numpy
restatement in tests/td3_bounded_ref.py bit for bit, the bounded actor gradient against PyTorch autograd, the warm-up's uniform
draws, and the refusals that need no device (the engine's own refusals need an engine, and an engine needs a device: they are in
tests/test_gpu_td3_bounded.py).  None of these symbols exists before this feature: every test here fails on the parent commit."""
import ctypes as C

import numpy as np
import pytest

from tests import mlp_ref as R
from tests import td3_bounded_ref as BR
from tests import td3_ref as T3
from tests.test_td3_host import _terms, _torch_forward, _torch_nets

F = np.float32
NAMES = ("B1", "B2", "B3")


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _state(c):
    """a state whose targets differ from the live networks, and a ring of 2 * batch rows with actions in the box's units"""
    rng, K = c["rng"], c["K"]
    st = T3.fresh_state(c["pol"], c["crit"])
    for k in ("theta_target", "psi_target"):
        st[k] = (st[k] + rng.standard_normal(st[k].size).astype(F) * F(0.05)).astype(F)
    size, D, A = 2 * c["batch"], 5 * K + 2, K + 1
    buf = dict(x=(rng.standard_normal((size, D)) * 0.7).astype(F), a=np.clip(rng.standard_normal((size, A)) * 0.7, -1, 1).astype(F),
               r=(rng.standard_normal(size) * 3).astype(F), done=rng.random(size) < 0.3, x2=(rng.standard_normal((size, D)) * 0.7).astype(F))
    buf["done"][0], buf["done"][1] = True, False
    return st, buf


@pytest.mark.parametrize("name", NAMES)
def test_the_act_twin_equals_the_restatement_in_the_three_modes(lib, name):
    """adc_mlp_act_host gives the raw means; adc_mlp_bounded_host's head on them is the restatement's n and e, with drawn and with
    handed-in normals; the means are scaled so that tanh(mean) + noise leaves the box on both sides in places.  A deterministic
    bounded act's e is adc_mlp_squash_host's of the raw mean"""
    c = BR.case(name)
    rng, pol, K, lo, hi = c["rng"], c["pol"], c["K"], c["lo"], c["hi"]
    A = K + 1
    pol.log_std = np.full(A, np.log(0.8), F)
    obs = R.realistic_obs(rng, 3, K)
    obs[0] = 0
    keys, ticks = [R.agent_key(7 + n) for n in range(3)], [0, 5, 2 ** 32 - 1]
    z_drawn, w = R.normals(keys, ticks, A), BR.words(keys, ticks, A)
    z_given = rng.standard_normal((3, A)).astype(F)
    clipped = 0
    for mode, z, handed in ((BR.GAUSSIAN, z_drawn, False), (BR.GAUSSIAN, z_given, True), (BR.DETERMINISTIC, None, False), (BR.RANDOM, None, False)):
        ref = BR.act(pol, obs, lo, hi, mode, z=z, w=w)
        for n in range(3):
            raw = R.twin_act(lib, pol, obs[n], deterministic=True)
            assert _same(raw["mean"][0], ref["mean"][n])
            got_n, got_e = BR.twin_head(lib, raw["mean"][0], pol.log_std, mode, lo, hi, z=z[n] if handed else None, key=keys[n], tick=ticks[n])
            assert _same(got_n, ref["action"][n]) and _same(got_e, ref["env"][n]), (name, mode, n)
        assert np.all(np.abs(ref["action"]) <= 1) and np.all(ref["env"] >= lo) and np.all(ref["env"] <= hi)
        if mode == BR.GAUSSIAN:
            clipped += int((ref["action"] == 1).sum() > 0) + int((ref["action"] == -1).sum() > 0)
        if mode == BR.DETERMINISTIC:
            sq = np.zeros(A, F)
            for n in range(3):
                assert lib.adc_mlp_squash_host(A, ref["mean"][n].ctypes.data, lo.ctypes.data, hi.ctypes.data, sq.ctypes.data) == 0
                assert _same(sq, ref["env"][n])
    assert clipped >= 2, "the Gaussian cases never reached the clip on both sides"


def test_the_teacher_mapping_inside_on_and_outside_the_box(lib):
    """e inside, on both faces, outside on both sides, and the exact middle: n = clamp((e - lo) * (1 / half) - 1)"""
    for name in NAMES:
        c = BR.case(name)
        lo, hi, rng = c["lo"], c["hi"], c["rng"]
        mid = BR.to_box(np.zeros(lo.size, F), lo, hi)
        for e in (lo, hi, mid, (lo - F(0.5)).astype(F), (hi + F(7)).astype(F), (lo + (hi - lo) * rng.random(lo.size).astype(F)).astype(F),
                  BR.to_box(np.clip(rng.standard_normal(lo.size), -1, 1).astype(F), lo, hi)):
            assert _same(BR.twin_unbox(lib, e, lo, hi), BR.unbox(e, lo, hi)), name
        assert np.all(BR.unbox(lo, lo, hi) == -1) and np.all(BR.unbox((lo - F(0.5)).astype(F), lo, hi) == -1) and np.all(BR.unbox((hi + F(7)).astype(F), lo, hi) == 1)
        assert np.all(np.abs(BR.unbox(hi, lo, hi) - 1) <= 2.0 ** -22) and np.all(np.abs(BR.unbox(mid, lo, hi)) <= 2.0 ** -22)
    # cent bids: what the action buffers hold
    lo, hi = BR.box(6)
    e = R.cent_bids(np.linspace(0.0, 4.0, 7).astype(F))
    assert _same(BR.twin_unbox(lib, e, lo, hi), BR.unbox(e, lo, hi))


@pytest.mark.parametrize("name", NAMES)
def test_target_and_actor_gradient_twins_equal_the_restatement(lib, name):
    c = BR.case(name)
    st, buf = _state(c)
    opts, pol, B = c["opts"], c["pol"], c["batch"]
    sh = T3.Shapes(pol, opts)
    for u in (0, 3):
        idx = T3.batch_indices(opts["seed"], u, len(buf["r"]), B)
        y = BR.twin_target(lib, pol, st["theta_target"], st["psi_target"], opts["seed"], u, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
        assert _same(y, BR.target(sh, st["theta_target"], st["psi_target"], None, opts["seed"], u, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)), (name, u)
        ap = BR.target_action(sh, st["theta_target"], opts["seed"], u, buf["x2"][idx], opts)
        assert np.all(np.abs(ap) <= 1)
    # (the unbounded twin on the same arrays gives another y: the mode is not a no-op)
    assert not _same(y, T3.twin_target(lib, pol, st["theta_target"], st["psi_target"], None, opts["seed"], 3, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts))
    g, sums = BR.twin_actor_grad(lib, pol, st["theta"], st["psi"], buf["x"][idx], opts)
    rg, rsums = BR.actor_grad(sh, st["theta"], st["psi"], None, buf["x"][idx])
    assert _same(g, rg) and _same(sums, rsums), name
    assert np.abs(g).max() > 0
    # one whole update of the restatement is the twins' steps (the critic's is td3_ref's own, on the ring's n as stored)
    st2, _ = BR.update(pol, dict(st, updates=1), buf, opts["seed"], opts)
    assert st2["actor_steps"] == 1 and not _same(st2["theta"], st["theta"])


def test_the_bounded_twins_refuse(lib):
    c = BR.case("B1")
    st, buf = _state(c)
    pol, K = c["pol"], c["K"]
    mcfg = pol.config(K)
    bad = T3.td3_config(**dict(c["opts"], action_lo=0.1, action_hi=0.9))
    y, dn = np.zeros(4, F), np.zeros(4, np.uint8)
    args = (st["theta_target"].ctypes.data, st["psi_target"].ctypes.data, 4, buf["x2"].ctypes.data, buf["r"].ctypes.data, dn.ctypes.data, y.ctypes.data)
    assert lib.adc_td3_bounded_target_host(C.byref(mcfg), K, C.byref(bad), 1, 0, *args) != 0          # action_lo / action_hi set
    ok = T3.td3_config(**c["opts"])
    assert lib.adc_td3_bounded_target_host(C.byref(mcfg), K, C.byref(ok), 1, 0, *args) == 0
    assert lib.adc_td3_bounded_target_host(C.byref(mcfg), K, C.byref(ok), 1, -1, *args) != 0
    m, n = np.zeros(3, F), np.zeros(3, F)
    lo, hi = np.zeros(3, F), np.ones(3, F)
    assert lib.adc_mlp_bounded_host(3, m.ctypes.data, m.ctypes.data, None, 0, 0, 3, lo.ctypes.data, hi.ctypes.data, n.ctypes.data, None) != 0     # unknown mode
    assert lib.adc_mlp_bounded_host(0, m.ctypes.data, m.ctypes.data, None, 0, 0, 0, lo.ctypes.data, hi.ctypes.data, n.ctypes.data, None) != 0
    assert lib.adc_mlp_unbox_host(3, None, lo.ctypes.data, hi.ctypes.data, n.ctypes.data) != 0


def _torch_actor_grad(sh, st, x, dtype, pre=None):
    """the gradient of -mean Q1(x, tanh(mu(x))) in theta by autograd in `dtype`"""
    import torch
    t = lambda v: torch.tensor(np.asarray(v, dtype=np.float64), dtype=dtype)
    (actor,), ap = _torch_nets([sh.actor(st["theta"])], dtype)
    (q1, _), _ = _torch_nets(sh.critics(st["psi"]), dtype)
    mu = _torch_forward(actor, t(x), sh.act, pre)
    (-_torch_forward(q1, torch.cat([t(x), torch.tanh(mu)], dim=1), sh.act, pre)[:, 0].mean()).backward()
    return np.concatenate([p.grad.detach().numpy().astype(np.float64).reshape(-1) for p in ap])


@pytest.mark.parametrize("name", NAMES)
def test_the_bounded_actor_gradient_against_pytorch_autograd(lib, name):
    """against float64 autograd of -Q1(x, tanh(mu(x))) with the yardstick of tests/test_td3_host.py: the twin's error (largest
    absolute difference over the largest float64 entry) is at most twice float32 autograd's own, over the whole gradient and in
    every term on its own, the per-term yardstick not taken below 2^-23; relu pre-activations are checked to be away from the kink"""
    import torch
    c = BR.case(name)
    st, buf = _state(c)
    opts, pol = c["opts"], c["pol"]
    sh = T3.Shapes(pol, opts)
    x = buf["x"][:c["batch"]]
    pre = []
    g64 = _torch_actor_grad(sh, st, x, torch.float64, pre)
    if c["act"] == "relu":
        assert min(float(p.abs().min()) for p in pre) > 1e-6, "a relu pre-activation sits on its kink: choose another seed"
    g32 = _torch_actor_grad(sh, st, x, torch.float32)
    g, _ = BR.twin_actor_grad(lib, pol, st["theta"], st["psi"], x, opts)
    assert g.shape == g64.shape
    scale = np.abs(g64).max()
    err_twin, err_f32 = np.abs(g.astype(np.float64) - g64).max() / scale, np.abs(g32 - g64).max() / scale
    print(f"{name} actor whole : twin {err_twin:.3e}  float32 autograd {err_f32:.3e}  ratio {err_twin / err_f32:.3f}")
    assert err_twin <= 2 * err_f32
    failed = []
    for term, lo, hi in _terms("actor", sh.D, sh.pol_widths)[0]:
        scale = np.abs(g64[lo:hi]).max()
        assert scale > 0, term
        err_twin = np.abs(g[lo:hi].astype(np.float64) - g64[lo:hi]).max() / scale
        err_f32 = np.abs(g32[lo:hi] - g64[lo:hi]).max() / scale
        print(f"{name} {term:12s}: twin {err_twin:.3e}  float32 autograd {err_f32:.3e}")
        if not err_twin <= 2 * max(err_f32, 2.0 ** -23):
            failed.append((term, err_twin, err_f32))
    assert not failed, failed


def test_the_random_mode_is_uniform_strictly_inside_the_box(lib):
    """m = 2^16 counter-addressed draws (64 ticks of A = 1024 components under one agent key): every n strictly inside (-1, 1),
    every e inside [lo, hi]; the mean within 5 / sqrt(3 m) of 0 and the mean square within 5 sqrt(4 / (45 m)) of 1 / 3 (the
    uniform's mean 0, variance 1 / 3, and its square's variance 4 / 45: five standard errors).  The draws are deterministic"""
    A, T = 1024, 64
    m = A * T
    lo, hi = np.full(A, 0.01, F), np.full(A, 3.0, F)
    hi[::2] = F(1e-3) + F(0.01)                                   # (a narrow box too)
    mean = np.zeros(A, F)
    key = R.agent_key(2024)
    ns, es = [], []
    for tick in range(T):
        n, e = BR.twin_head(lib, mean, mean, BR.RANDOM, lo, hi, key=key, tick=tick)
        ns.append(n)
        es.append(e)
        if tick < 2:
            assert _same(n, BR.uniform_unit(BR.words([key], [tick], A))[0])
    n, e = np.concatenate(ns).astype(np.float64), np.stack(es)
    assert n.min() > -1 and n.max() < 1 and np.all(e >= lo) and np.all(e <= hi)
    m1, m2 = n.mean(), (n * n).mean()
    b1, b2 = 5 / np.sqrt(3 * m), 5 * np.sqrt(4 / (45 * m))
    print(f"mean {m1:+.5f} (bound {b1:.5f})  mean square {m2:.5f} (1/3 +- {b2:.5f})  min {n.min():.6f} max {n.max():.6f}")
    assert abs(m1) <= b1 and abs(m2 - 1 / 3) <= b2
    # the extreme words: strictly inside, exact
    assert BR.uniform_unit(np.array([0, 0xFFFFFFFF], np.uint32)).tolist() == [-1 + 2.0 ** -23, 1 - 2.0 ** -23]


def test_the_trainers_refuse_before_touching_an_engine():
    """the Python side's refusals: they are raised before the first engine call, so `None` serves as the engine"""
    from adcraft_amd.baselines import td3_trainer as TT
    rng = np.random.default_rng(3)
    pol = R.random_policy(rng, 3, (4,))
    norm = (np.zeros(4, F), np.ones(4, F))
    with pytest.raises(ValueError, match="random_timesteps needs action_bounds"):
        TT.TD3Trainer(None, pol, random_timesteps=10)
    with pytest.raises(ValueError, match="action_bounds with action_norm"):
        TT.TD3Trainer(None, pol, action_bounds=(0.01, 3.0), action_norm=norm)
    with pytest.raises(ValueError, match="hi > lo"):
        TT.TD3Trainer(None, pol, action_bounds=(3.0, 0.01))
    with pytest.raises(ValueError, match="hi > lo"):
        TT.TD3Trainer(None, pol, action_bounds=(0.0, float("inf")))
    with pytest.raises(ValueError, match="a pair"):
        TT.TD3Trainer(None, pol, action_bounds=(0.0, 1.0, 2.0))
    with pytest.raises(ValueError, match="random_timesteps: an integer"):
        TT.TD3Trainer(None, pol, action_bounds=(0.01, 3.0), random_timesteps=-1)
    cfg = TT.rllib_td3(0.01, 3.0)
    assert cfg["gamma"] == 0.995 and cfg["actor_lr"] == cfg["critic_lr"] == 1e-3 and cfg["batch_size"] == 2048 and cfg["tau"] == 0.005
    assert cfg["random_timesteps"] == cfg["learning_starts"] == 10000 and cfg["critic_hidden"] == (256, 256)
    assert abs(cfg["exploration_sigma"] - 0.1 / 1.495) < 1e-12 and 0.066 < cfg["exploration_sigma"] < 0.068
    assert TT.rllib_td3(0.01, 3.0, gamma=0.9, exploration_sigma=0.2)["exploration_sigma"] == 0.2
    with pytest.raises(ValueError, match="widths differ"):
        TT.rllib_td3([0.0, 0.0], [1.0, 2.0])
    assert TT.rllib_td3([0.0, 0.0], [1.0, 2.0], exploration_sigma=0.1)["action_bounds"] == ([0.0, 0.0], [1.0, 2.0])
