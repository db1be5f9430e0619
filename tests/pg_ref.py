"""The policy-gradient law (adcraft_amd/csrc/adc_pg.h) restated in numpy from the header's comments: GAE, the advantage
normalisation, the forward recompute, the PPO-clip loss pieces, the backward pass, the chunked float64 sums over samples, the
norm clip and the Adam / SGD descent step, one float32 rounding at a time.  The host twins (adc_pg_gae_host, adc_pg_grad_host,
adc_pg_step_host) and the device kernels must give these very bits.  `policy` is an MLPPolicy used as a container of shapes and
options; the parameters come as the flat vector theta."""
import ctypes as C

import numpy as np

from tests import mlp_ref as R
from tests.es_ref import bias_correction

F = np.float32
D64 = np.float64
CHUNK = 1024
DEFAULTS = dict(gamma=0.99, lam=0.95, eps_clip=0.2, vf_coef=0.5, ent_coef=0.0, reward_scale=1.0, normalize_advantages=True,
                max_grad_norm=0.5, optimiser="adam", lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, minibatch_envs=0)
STAT_KEYS = ("policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "grad_norm", "explained_variance")


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def flat_params(policy):
    """theta: the policy layers (W input-major, then b), the value layers in the same form, log_std when the head is free"""
    parts = [np.concatenate([w.reshape(-1), b]) for w, b in list(policy.layers) + list(policy.value_layers)]
    if policy.log_std is not None:
        parts.append(policy.log_std)
    return np.concatenate(parts).astype(F)


def unflatten(policy, theta):
    """(layers, value_layers, log_std) of theta in the shapes of `policy`"""
    theta = np.asarray(theta, dtype=F)
    pos, nets = 0, []
    for net in (policy.layers, policy.value_layers):
        out = []
        for w, b in net:
            nw = w.size
            out.append((theta[pos:pos + nw].reshape(w.shape).copy(), theta[pos + nw:pos + nw + b.size].copy()))
            pos += nw + b.size
        nets.append(out)
    log_std = None
    if policy.log_std is not None:
        log_std = theta[pos:pos + policy.log_std.size].copy()
        pos += policy.log_std.size
    assert pos == theta.size
    return nets[0], nets[1], log_std


def with_params(policy, theta):
    """a copy of `policy` holding theta"""
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    layers, value_layers, log_std = unflatten(policy, theta)
    return MLPPolicy(layers, activation=policy.activation, value_layers=value_layers, log_std=log_std, shift=policy.shift, scale=policy.scale,
                     log_std_clamp=policy.log_std_clamp, bid_clip=policy.bid_clip, deterministic=policy.deterministic)


def csum(terms):
    """the chunked float64 sum over axis 0: chunks of 1024 consecutive indices, each a chain from +0, joined by a chain from +0"""
    terms = np.asarray(terms, dtype=D64)
    total = np.zeros(terms.shape[1:], D64)
    for c0 in range(0, terms.shape[0], CHUNK):
        part = np.zeros(terms.shape[1:], D64)
        for i in range(c0, min(c0 + CHUNK, terms.shape[0])):
            part = part + terms[i]
        total = total + part
    return total


def gae(reward, terminated, truncated, value, bootstrap, gamma=0.99, lam=0.95, reward_scale=1.0, normalize_advantages=True, **_):
    """adv, ret [T, N] float32"""
    reward, value = np.asarray(reward, F), np.asarray(value, F)
    T, N = reward.shape
    done = np.asarray(terminated, bool) | np.asarray(truncated, bool)
    g, gl = F(gamma), F(gamma) * F(lam)
    adv, ret = np.zeros((T, N), F), np.zeros((T, N), F)
    a_next, nxt = np.zeros(N, F), np.asarray(bootstrap, F)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            r = reward[t] * F(reward_scale)
            nt = np.where(done[t], F(0), F(1))
            delta = (r + ((g * nxt) * nt)) - value[t]
            a_next = (delta + ((gl * nt) * a_next)).astype(F)
            adv[t] = a_next
            ret[t] = a_next + value[t]
            nxt = value[t]
        if normalize_advantages:
            flat = adv.reshape(-1).astype(D64)
            n = D64(flat.size)
            mean = csum(flat) / n
            d = flat - mean
            var = csum(d * d) / n
            adv = ((flat - mean) / (np.sqrt(var) + 1e-8)).astype(F).reshape(T, N)
    return adv, ret


def grad(policy, theta, obs, action, logp_old, adv, ret, value_old, eps_clip=0.2, vf_coef=0.5, ent_coef=0.0, **_):
    """the flat gradient [Q] float32, the law's ten sums and the statistics of S samples: obs [S, D] (the recorded input),
    action [S, A], logp_old, adv, ret, value_old [S]"""
    layers, value_layers, log_std = unflatten(policy, theta)
    x = np.ascontiguousarray(obs, dtype=F)
    action, logp_old, adv, ret, value_old = (np.asarray(a, F) for a in (action, logp_old, adv, ret, value_old))
    S, A, act = x.shape[0], policy.num_keywords + 1, policy.activation
    with np.errstate(all="ignore"):
        def forward(net):
            ys, h = [], x
            for i, (w, b) in enumerate(net):
                h = R.layer(h, w, b, act if i + 1 < len(net) else None)
                ys.append(h)
            return ys
        yp, yv = forward(layers), forward(value_layers)
        o = yp[-1]
        two = o.shape[1] == 2 * A
        mean = o[:, :A]
        raw = o[:, A:] if two else np.broadcast_to(log_std, mean.shape).astype(F)
        ls, moved = raw, np.zeros(raw.shape, bool)
        if policy.log_std_clamp is not None:
            lo, hi = F(policy.log_std_clamp[0]), F(policy.log_std_clamp[1])
            ls = np.where(ls < lo, lo, ls)
            ls = np.where(ls > hi, hi, ls).astype(F)
            moved = (raw < lo) | (raw > hi)
        sd = R.exp32(ls)
        z = ((action - mean) / sd).astype(F)
        logp = (R.sum8(((-((z * z) * F(0.5))) - ls).T) - F(A) * R.HALF_LOG_2PI).astype(F)
        entropy = (R.sum8(ls.T) + F(A) * (F(0.5) + R.HALF_LOG_2PI)).astype(F)
        ratio = R.exp32(logp - logp_old)
        s1 = ratio * adv
        if eps_clip > 0:
            lo, hi = F(1) - F(eps_clip), F(1) + F(eps_clip)
            rc = np.where(ratio < lo, lo, np.where(ratio > hi, hi, ratio)).astype(F)
            s2 = rc * adv
            clipped = (ratio < lo) | (ratio > hi)
            surr = np.where(s1 < s2, s1, s2)
            passes = ~clipped | (s1 < s2)
        else:
            surr, clipped, passes = s1, np.zeros(S, bool), np.ones(S, bool)
        g = np.where(passes, -(adv * ratio), F(0)).astype(F)
        V = yv[-1][:, 0] if value_layers else np.zeros(S, F)
        dv = V - ret
        val_loss = F(0.5) * (dv * dv)
        dV = F(vf_coef) * dv
        pieces = np.stack([-surr, val_loss, entropy, logp_old - logp, clipped.astype(F), ret, ret - value_old], axis=1).astype(F)
        d_mean = g[:, None] * (z / sd)
        d_ls = np.where(moved, F(0), (g[:, None] * ((z * z) - F(1))) - F(ent_coef)).astype(F)

        def backward(net, ys, d_out):
            deltas = [None] * len(net)
            deltas[-1] = d_out.astype(F)
            for l in range(len(net) - 2, -1, -1):
                w = net[l + 1][0]                                  # [n (this layer's outputs), n_out]
                s = R.sum8(w.T[:, None, :] * deltas[l + 1].T[:, :, None])
                y = ys[l]
                dact = (F(1) - y * y) if act == "tanh" else np.where(y > 0, F(1), F(0)).astype(F)
                deltas[l] = (dact * s).astype(F)
            return deltas
        dp = backward(layers, yp, np.concatenate([d_mean, d_ls], axis=1) if two else d_mean)
        dvs = backward(value_layers, yv, dV[:, None]) if value_layers else []

        def term(xin, delta):
            x1 = np.concatenate([xin, np.ones((S, 1), F)], axis=1).astype(D64) if xin is not None else np.ones((S, 1), D64)
            return csum(x1[:, :, None] * delta.astype(D64)[:, None, :]).reshape(-1)
        parts = []
        for ys, ds in ((yp, dp), (yv, dvs)):
            for l, d in enumerate(ds):
                parts.append(term(x if l == 0 else ys[l - 1], d))
        if not two:
            parts.append(term(None, d_ls))
        gq = (np.concatenate(parts) / D64(S)).astype(F)
        p64 = pieces.astype(D64)
        sums = np.concatenate([csum(p64), csum(p64[:, 5:7] * p64[:, 5:7]), [csum(gq.astype(D64) * gq.astype(D64))]])
    return gq, sums, stats_of(sums, S)


def stats_of(sums, S):
    n = D64(S)
    with np.errstate(all="ignore"):
        mr, me, qr, qe = sums[5] / n, sums[6] / n, sums[7] / n, sums[8] / n
        ev = 1.0 - (qe - me * me) / (qr - mr * mr)
    return dict(policy_loss=sums[0] / n, value_loss=sums[1] / n, entropy=sums[2] / n, approx_kl=sums[3] / n, clip_fraction=sums[4] / n,
                grad_norm=np.sqrt(sums[9]), explained_variance=ev)


def step(theta, m, v, g, steps, max_grad_norm=0.5, optimiser="adam", lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, **_):
    """the norm clip and one descent step; steps: the count before it.  Returns new (theta, m, v)"""
    theta, m, v, g = (np.array(a, dtype=F) for a in (theta, m, v, g))
    with np.errstate(all="ignore"):
        if max_grad_norm > 0:
            norm = np.sqrt(csum(g.astype(D64) * g.astype(D64)))
            q = D64(F(max_grad_norm)) / (norm + 1e-6)
            g = g * F(q if q < 1.0 else 1.0)
        if optimiser == "sgd":
            return (theta - F(lr) * g).astype(F), m, v
        b1, b2 = F(beta1), F(beta2)
        m = (b1 * m) + ((F(1) - b1) * g)
        v = (b2 * v) + ((F(1) - b2) * (g * g))
        c1, c2 = bias_correction(beta1, steps + 1), bias_correction(beta2, steps + 1)
        theta = theta - F(lr) * ((m / c1) / (np.sqrt(v / c2) + F(eps)))
    return theta.astype(F), m.astype(F), v.astype(F)


def minibatch(policy, state, rec, adv, ret, n0, B, opts):
    """what adc_engine_pg_minibatch does to state = dict(theta, m, v, steps) on the record `rec` (rollout_fetch's dict with obs):
    sample s = t * B + (env - n0).  Returns (new state, statistics)"""
    sl = slice(n0, n0 + B)
    flat = lambda a: np.ascontiguousarray(a[:, sl]).reshape((-1,) + a.shape[2:])
    g, _, st = grad(policy, state["theta"], flat(rec["obs"]), flat(rec["action"]), flat(rec["logp"]), flat(adv), flat(ret), flat(rec["value"]), **opts)
    theta, m, v = step(state["theta"], state["m"], state["v"], g, state["steps"], **opts)
    return dict(theta=theta, m=m, v=v, steps=state["steps"] + 1), st


def update(policy, state, rec, bootstrap, epochs, opts):
    """adc_engine_pg_update: advantages once, then epochs x the minibatches in ascending env order"""
    adv, ret = gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], bootstrap, **opts)
    N = rec["reward"].shape[1]
    mb = opts["minibatch_envs"] or N
    for _ in range(epochs):
        acc = dict.fromkeys(STAT_KEYS, D64(0.0))
        for n0 in range(0, N, mb):
            state, st = minibatch(policy, state, rec, adv, ret, n0, mb, opts)
            with np.errstate(all="ignore"):
                acc = {k: acc[k] + st[k] for k in STAT_KEYS}
        with np.errstate(all="ignore"):
            mean = {k: acc[k] / D64(N // mb) for k in STAT_KEYS}      # the last epoch's statistics: the mean over its minibatches, in order
    return state, mean


# ---- the host twins ---------------------------------------------------------------------------------------------------------------
def pg_config(**kw):
    from adcraft_amd.engine import StepEngine
    return StepEngine.pg_config(**kw)


def twin_gae(lib, reward, terminated, truncated, value, bootstrap, **kw):
    cfg = pg_config(**kw)
    reward, value, bootstrap = (np.ascontiguousarray(a, dtype=F) for a in (reward, value, bootstrap))
    te, tr = (np.ascontiguousarray(a, dtype=np.uint8) for a in (terminated, truncated))
    T, N = reward.shape
    adv, ret = np.zeros((T, N), F), np.zeros((T, N), F)
    rc = lib.adc_pg_gae_host(C.byref(cfg), T, N, reward.ctypes.data, te.ctypes.data, tr.ctypes.data, value.ctypes.data, bootstrap.ctypes.data,
                             adv.ctypes.data, ret.ctypes.data)
    assert rc == 0, rc
    return adv, ret


def twin_grad(lib, policy, theta, obs, action, logp_old, adv, ret, value_old, **kw):
    from adcraft_amd import _ffi
    cfg, K = pg_config(**kw), policy.num_keywords
    mcfg = policy.config(K)
    arrs = [np.ascontiguousarray(a, dtype=F) for a in (theta, obs, action, logp_old, adv, ret, value_old)]
    q = C.c_int64(0)
    assert lib.adc_pg_param_count_host(C.byref(mcfg), K, C.byref(q)) == 0 and q.value == arrs[0].size, (q.value, arrs[0].size)
    g, sums, st = np.zeros(q.value, F), np.zeros(10, D64), _ffi.PGStats()
    rc = lib.adc_pg_grad_host(C.byref(mcfg), K, C.byref(cfg), arrs[0].ctypes.data, arrs[1].shape[0], *(a.ctypes.data for a in arrs[1:]),
                              g.ctypes.data, sums.ctypes.data, C.byref(st))
    assert rc == 0, rc
    return g, sums, {k: getattr(st, k) for k in STAT_KEYS}


def twin_step(lib, theta, m, v, g, steps, **kw):
    cfg = pg_config(**kw)
    theta, m, v = (np.array(a, dtype=F) for a in (theta, m, v))
    g = np.ascontiguousarray(g, dtype=F)
    rc = lib.adc_pg_step_host(C.byref(cfg), theta.size, int(steps), g.ctypes.data, theta.ctypes.data, m.ctypes.data, v.ctypes.data)
    assert rc == 0, rc
    return theta, m, v
