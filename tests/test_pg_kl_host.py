"""The PPO learners' KL penalty and value-loss clip on the host: the twins adc_pg_kl_grad_host / adc_pg_kl_adapt_host (the code
the device kernels run, adc_pg_kl.h) against the numpy restatement in tests/pg_kl_ref.py bit for bit, the gradient against
PyTorch autograd over torch.distributions' own KL divergence, the two degenerate cases in which the add-on must be the trainer it
is attached to, the adaptation's thresholds, the configuration check and the Python surface.  No device is needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mlp_ref as R
from tests import pg_kl_ref as KR
from tests import pg_ref as P

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


CLAMP = (-0.4, 0.3)
# activation, two heads, clamp, K, samples, kl_coef, value clip on.  Every value the issue names occurs: tanh / relu, the free
# head / two heads, the clamp off / on, K = 3 (fewer components than chains), 9, 256 (more components than a workgroup has
# lanes), S = 5 and 1030 (crosses one 1024-chunk), kl_coef 0 / 1 / 0.3, the value clip off / on.  Hidden (8,) throughout.
CASES = [
    ("tanh", False, None, 3, 5, 1.0, False),
    ("relu", True, CLAMP, 3, 1030, 0.3, True),
    ("tanh", True, None, 9, 5, 0.0, True),
    ("relu", False, CLAMP, 9, 1030, 1.0, True),
    ("tanh", False, CLAMP, 256, 5, 0.3, True),
    ("relu", True, None, 256, 1030, 1.0, False),
    ("tanh", True, CLAMP, 9, 1030, 1.0, True),
    ("relu", False, None, 3, 1030, 0.0, False),
    ("tanh", True, CLAMP, 256, 5, 1.0, True),
]
IDS = [f"{a}-{'two' if t else 'free'}-{'clamp' if c else 'noclamp'}-K{k}-S{s}-c{kc}-{'vf' if v else 'novf'}" for a, t, c, k, s, kc, v in CASES]
_made = {}


def _case(i, drift=0.03):
    """the policy that collected, a batch as a record would hold it, the snapshot of the collecting distribution, a theta a few
    updates away, and a value clip for which no sample's squared error lies within 1e-3 (relative) of the cap"""
    if (i, drift) in _made:
        return _made[(i, drift)]
    act, two, clamp, K, S, coef, vf = CASES[i]
    rng = np.random.default_rng(500 + i)
    pol = R.random_policy(rng, K, (8,), activation=act, two_heads=two, value=True, log_std_clamp=clamp)
    if clamp is not None and not two:                          # (a free log_std on both sides of both bounds)
        pol.log_std = np.linspace(clamp[0] - 0.5, clamp[1] + 0.5, K + 1).astype(F)
    obs = (rng.standard_normal((S, 5 * K + 2)) * 0.7).astype(F)
    a = R.act(pol, obs, rng.standard_normal((S, K + 1)).astype(F), deterministic=False)
    theta0 = P.flat_params(pol)
    theta = (theta0 + rng.standard_normal(theta0.size).astype(F) * F(drift)).astype(F)
    adv = rng.standard_normal(S).astype(F)
    ret = (rng.standard_normal(S) * 2).astype(F)
    value_old = (ret + rng.standard_normal(S)).astype(F)
    mean_old, ls_old = KR.old_dist(pol, theta0, obs)
    batch = (theta, obs, a["action"], a["logp"], adv, ret, value_old, mean_old, ls_old)
    # the cap: the widest relative gap between neighbours in the middle half of the sorted squared errors, at its geometric middle
    sq = np.sort(KR.grad(pol, *batch)[5]["sq"].astype(np.float64))
    lo, hi = (S // 4, 3 * S // 4) if S > 8 else (1, S - 1)
    j = lo + int(np.argmax(sq[lo + 1:hi + 1] / sq[lo:hi]))
    cap = float(F(np.sqrt(sq[j] * sq[j + 1]))) if vf else 0.0
    _made[(i, drift)] = (pol, theta0, batch, dict(kl_coef=coef, vf_clip=cap))
    return _made[(i, drift)]


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_twin_equals_the_restatement_bit_for_bit(lib, case):
    act, two, clamp, K, S, coef, vf = CASES[case]
    pol, _, batch, kl = _case(case)
    opts = P.options(vf_coef=1.0, ent_coef=0.01)
    rg, rsums, rsk, rst, rkst, aux = KR.grad(pol, *batch, **kl, **opts)
    # the restatement's own value-clipped fraction lies strictly between 0 and 1 where the clip is on
    frac = float(rkst["vf_clip_fraction"])
    assert (0.0 < frac < 1.0) if vf else frac == 0.0
    g, sums, sk, st, kst = KR.twin_grad(lib, pol, *batch, **kl, **opts)
    assert _same(g, rg)
    assert _same(sums, rsums) and _same(sk, rsk)
    for k in P.STAT_KEYS:
        assert _same(np.float64(st[k]), np.float64(rst[k])), k
    for k in ("kl", "vf_clip_fraction"):
        assert _same(np.float64(kst[k]), np.float64(rkst[k])), k
    assert _same(F(kst["kl_coef"]), F(coef)) and _same(F(kst["kl_coef_next"]), F(coef))
    assert np.isfinite(g).all() and np.abs(g).max() > 0 and kst["kl"] > 0
    if clamp is not None:           # the clamp moves some raw values below lo and some above hi, and leaves some
        layers, _, log_std = P.unflatten(pol, batch[0])
        raw = R.network(batch[1], layers, pol.activation)[:, K + 1:] if two else log_std
        assert (raw < F(clamp[0])).any() and (raw > F(clamp[1])).any() and ((raw >= F(clamp[0])) & (raw <= F(clamp[1]))).any()


@pytest.mark.parametrize("case", [0, 1, 3, 4, 6], ids=[IDS[i] for i in (0, 1, 3, 4, 6)])
def test_nothing_moved(lib, case):
    """mean_old / ls_old equal to the current distribution's: the KL of every sample is exactly +0, and the gradient compares
    equal to the trainer's own (a sum with a zero product may turn a -0 into +0: they compare equal)"""
    pol, theta0, batch, kl = _case(case)
    batch = (theta0,) + batch[1:]
    opts = P.options()
    g, _, sk, _, kst = KR.twin_grad(lib, pol, *batch, kl_coef=1.0, vf_clip=0.0, **opts)
    g0, _, _ = P.twin_grad(lib, pol, *batch[:7], **opts)
    per_sample = KR.grad(pol, *batch, kl_coef=1.0, **opts)[5]["kl"]
    assert np.all(per_sample == 0) and not np.signbit(per_sample).any()
    assert sk[0] == 0.0 and not np.signbit(sk[0]) and kst["kl"] == 0.0
    assert np.array_equal(g, g0) and np.abs(g0).max() > 0


@pytest.mark.parametrize("case", [1, 3, 5], ids=[IDS[i] for i in (1, 3, 5)])
def test_zero_coefficient(lib, case):
    """kl_coef = 0 and vf_clip = 0 under moved parameters: the trainer's own gradient bit for bit, and the KL is measured"""
    pol, _, batch, _ = _case(case)
    opts = P.options(ent_coef=0.01)
    g, sums, _, st, kst = KR.twin_grad(lib, pol, *batch, kl_coef=0.0, vf_clip=0.0, **opts)
    g0, sums0, st0 = P.twin_grad(lib, pol, *batch[:7], **opts)
    assert _same(g, g0) and _same(sums, sums0)
    assert kst["kl"] > 0 and kst["vf_clip_fraction"] == 0.0
    assert all(_same(np.float64(st[k]), np.float64(st0[k])) for k in P.STAT_KEYS)


def _torch_grad(pol, theta, obs, action, logp_old, adv, ret, value_old, mean_old, ls_old, dtype, opts, kl_coef, vf_clip):
    """test_pg_host.py's loss in PyTorch with the penalty written through torch.distributions and the value clip through
    torch.where; the flat gradient by autograd in `dtype`"""
    import torch
    from torch.distributions import Normal, kl_divergence
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
    old = Normal(t(mean_old), torch.exp(t(np.broadcast_to(ls_old, mean_old.shape))))
    kl = kl_divergence(old, Normal(mean, torch.exp(ls))).sum(-1)
    loss = loss + float(F(kl_coef)) * kl.mean()
    sq = (forward(vl, x)[:, 0] - t(ret)) ** 2
    if vf_clip > 0:
        cap = torch.tensor(float(F(vf_clip)), dtype=dtype)
        sq = torch.where(sq > cap, cap, sq)
    loss = loss + float(F(opts["vf_coef"])) * 0.5 * sq.mean()
    loss.backward()
    return np.concatenate([p.grad.detach().numpy().astype(np.float64).reshape(-1) for p in params]), kl.detach().numpy().astype(np.float64)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_gradient_against_pytorch_autograd(lib, case):
    """test_pg_host.py's method exactly: the yardstick is float32 autograd's own error against float64 autograd on the same
    arrays, the twin's error against float64 autograd at most twice that - over the whole flat gradient, and in every term on
    its own with the yardstick not taken below 2^-23.  The cases are the first test's with kl_coef = 1.  Measured ratios:
    profiles/pr_pg_kl.txt."""
    import torch
    act, two, clamp, K, S, _, vf = CASES[case]
    pol, _, batch, kl = _case(case)
    cap = kl["vf_clip"]
    opts = P.options(vf_coef=1.0, ent_coef=0.01)
    if vf:          # float32 and float64 agree on which side of the cap every sample falls: none within 1e-3 (relative) of it
        sq = KR.grad(pol, *batch, **opts)[5]["sq"].astype(np.float64)
        assert np.abs(sq / cap - 1.0).min() > 1e-3
    g, _, _, _, kst = KR.twin_grad(lib, pol, *batch, kl_coef=1.0, vf_clip=cap, **opts)
    g64, kl64 = _torch_grad(pol, *batch, torch.float64, opts, 1.0, cap)
    g32, _ = _torch_grad(pol, *batch, torch.float32, opts, 1.0, cap)
    assert g64.shape == g.shape
    # the measured KL is torch.distributions'.  A component's term is non-negative, formed in six roundings of magnitudes below
    # term + |ls - ls_old| + 1 <= 2 term + 2, and a chain of the sum8 adds A / 8 + 3 more on partial sums below the KL: the
    # float32 KL of a sample is within (A / 8 + 9) 2^-24 (2 kl + 2 A) of the exact one, and so is the mean
    A = K + 1
    assert abs(kst["kl"] - kl64.mean()) <= (A / 8 + 9) * 2.0 ** -24 * (2 * kl64.mean() + 2 * A)
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
    print(f"case {IDS[case]} whole     : twin {err_twin:.3e}  float32 autograd {err_f32:.3e}  ratio {err_twin / err_f32:.3f}")
    assert err_twin <= 2 * err_f32
    failed = []
    for name, a, b in terms:
        scale = np.abs(g64[a:b]).max()
        assert scale > 0, name
        err_twin = np.abs(g[a:b].astype(np.float64) - g64[a:b]).max() / scale
        err_f32 = np.abs(g32[a:b] - g64[a:b]).max() / scale
        print(f"case {IDS[case]} {name:10s}: twin {err_twin:.3e}  float32 autograd {err_f32:.3e}  ratio {err_twin / err_f32 if err_f32 else float('nan'):.3f}")
        if not err_twin <= 2 * max(err_f32, 2.0 ** -23):
            failed.append((name, err_twin, err_f32))
    assert not failed, failed


def test_adaptation(lib):
    target = 0.01
    t = np.float64(F(target))
    up, kept, down = F(F(0.7) * F(1.5)), F(0.7), F(F(0.7) * F(0.5))
    ad = lambda kl, **kw: KR.twin_adapt(lib, 0.7, kl, **dict(dict(kl_target=target, adaptive=True), **kw))
    assert _same(ad(2.0000001 * t), up)
    assert _same(ad(2.0 * t), kept) and _same(ad(0.5 * t), kept) and _same(ad(t), kept)
    assert _same(ad(np.nextafter(0.5 * t, 0.0)), down) and _same(ad(0.0), down)
    assert _same(ad(np.nextafter(2.0 * t, 1.0)), up)
    # custom factors, and the defaults named explicitly
    assert _same(ad(1.0, factor_up=2.5), F(F(0.7) * F(2.5))) and _same(ad(0.0, factor_down=0.125), F(F(0.7) * F(0.125)))
    assert _same(ad(1.0, factor_up=1.5, factor_down=0.5), up)
    # adaptive = 0: the coefficient stays, whatever the KL and the target are
    assert _same(ad(1.0, adaptive=False), kept) and _same(ad(0.0, adaptive=False, kl_target=0.0), kept)
    # ten updates against the restatement: the coefficient rises, stays and falls
    rng = np.random.default_rng(9)
    for kw in (dict(), dict(factor_up=1.3, factor_down=0.9)):
        c_tw = c_ref = F(0.3)
        seen = set()
        for kl in list(t * np.array([3.0, 2.5, 1.0, 0.1, 0.2, 0.49, 0.5, 2.0, 4.0])) + [float(rng.random() * 0.05)]:
            nxt = KR.adapt(c_ref, kl, kl_target=target, **kw)
            seen.add(int(np.sign(float(nxt) - float(c_ref))))
            c_ref = nxt
            c_tw = KR.twin_adapt(lib, c_tw, kl, kl_target=target, **kw)
            assert _same(c_tw, c_ref)
        assert {-1, 0, 1} <= seen


BAD = [dict(kl_coef=-0.1), dict(kl_coef=float("nan")), dict(kl_coef=float("inf")), dict(kl_target=0.0), dict(kl_target=-1.0),
       dict(kl_target=float("nan")), dict(factor_up=1.0), dict(factor_up=0.5), dict(factor_down=1.0), dict(factor_down=-0.5),
       dict(factor_down=1.5), dict(vf_clip=-1.0), dict(vf_clip=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=[next(iter(b)) + "=" + str(next(iter(b.values()))) for b in BAD])
def test_config_check_rejects_each_bad_field(lib, bad):
    from adcraft_amd import _ffi
    from adcraft_amd.engine import StepEngine
    good = StepEngine.pg_kl_config()
    msg = C.c_char_p()
    assert lib.adc_pg_kl_config_check(C.byref(good), C.byref(msg)) == 0 and msg.value is None
    for k, v in bad.items():
        setattr(good, k, v)
    assert lib.adc_pg_kl_config_check(C.byref(good), C.byref(msg)) == _ffi.ADC_EINVAL
    assert msg.value
    with pytest.raises(ValueError):
        StepEngine.pg_kl_config(**bad)
    good = StepEngine.pg_kl_config()
    good.struct_size += 4
    assert lib.adc_pg_kl_config_check(C.byref(good), C.byref(msg)) == _ffi.ADC_EINVAL and b"struct_size" in msg.value
    assert lib.adc_pg_kl_config_check(None, C.byref(msg)) == _ffi.ADC_EINVAL
    # the target is not looked at when the coefficient stays
    if "kl_target" in bad:
        StepEngine.pg_kl_config(adaptive=False, **bad)


def test_python_surface(lib):
    from adcraft_amd import _ffi
    from adcraft_amd.baselines import pg_trainer as T
    from adcraft_amd.engine import ShardedStepEngine, StepEngine
    cfg = T.rllib_ppo()
    assert (cfg["gamma"], cfg["lam"], cfg["lr"], cfg["eps_clip"], cfg["epochs"], cfg["vf_coef"]) == (0.995, 0.95, 1e-4, 0.5, 20, 2.0)
    assert cfg["kl_penalty"] == dict(kl_coef=1.0, kl_target=0.01, adaptive=True, vf_clip=10.0)
    assert T.rllib_ppo(lr=3e-4, epochs=5)["lr"] == 3e-4 and T.rllib_ppo(epochs=5)["epochs"] == 5 and "rllib_ppo" in T.__all__
    StepEngine.pg_config(**{k: v for k, v in cfg.items() if k not in ("epochs", "minibatches", "kl_penalty")})
    c = StepEngine.pg_kl_config(**cfg["kl_penalty"])
    assert c.struct_size == C.sizeof(_ffi.PGKLConfig) == 28 and c.kl_coef == 1.0 and c.adaptive == 1 and c.vf_clip == 10.0
    assert C.sizeof(_ffi.PGKLStats) == 24
    # the trainers check the options before they touch the engine
    assert T._kl_options(None) is None and T._kl_options(dict(kl_coef=0.5)) == dict(kl_coef=0.5)
    with pytest.raises(ValueError, match="unknown"):
        T._kl_options(dict(kl_coeff=0.5))
    with pytest.raises(TypeError):
        T._kl_options(0.5)
    with pytest.raises(TypeError):
        T._kl_options([dict(kl_coef=0.5)])                      # (a list only for a population)
    with pytest.raises(ValueError, match="one per member"):
        T._kl_options([dict(kl_coef=0.5)] * 2, members=3)
    assert T._kl_options([dict(kl_coef=0.5), dict(vf_clip=1.0)], members=2) == [dict(kl_coef=0.5), dict(vf_clip=1.0)]
    with pytest.raises(ValueError, match="unknown"):
        T.PGTrainer(None, None, 4, kl_penalty=dict(target=0.1))
    # the new symbols are declared in the header, exported by the library and bound
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adcraft_engine.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(adc_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.library_path()], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    new = {"adc_pg_kl_config_check", "adc_engine_pg_kl_init", "adc_engine_pg_kl_stats", "adc_engine_pg_kl_coef_get", "adc_engine_pg_kl_coef_set",
           "adc_engine_pg_kl_old_dist_fetch", "adc_pg_kl_grad_host", "adc_pg_kl_adapt_host"}
    for n in new:
        assert n in declared and n in exported and getattr(lib, n).argtypes is not None, n
    sharded = object.__new__(ShardedStepEngine)
    for name in ("pg_kl_init", "pg_kl_stats", "pg_kl_coef", "pg_kl_old_dist"):
        with pytest.raises(NotImplementedError, match="engine_shards=1"):
            getattr(sharded, name)
