"""The imitation law (adcraft_amd/csrc/adc_imitation.h) restated in numpy from the header's comments: the teacher's returns, the
moving scale, the weight, the imitation loss's pieces and output deltas, one float32 rounding at a time; the forward pass, the
head, the backward pass, the chunked sums, the norm clip and the step are the policy-gradient law's (tests/pg_ref.py).  The host
twins (adc_im_weight_host, adc_im_grad_host) and the device kernels must give these very bits.  `policy` is an MLPPolicy used as
a container of shapes and options; the parameters come as the flat vector theta."""
import ctypes as C

import numpy as np

from tests import mlp_ref as R
from tests import pg_ref as P

F = np.float32
D64 = np.float64
IM_DEFAULTS = dict(beta=0.0, vf_coef=1.0, w_max=20.0, ma_start=100.0, ma_rate=1e-8, train_log_std=True)
STAT_KEYS = ("policy_loss", "value_loss", "entropy", "logp", "weight", "grad_norm", "explained_variance")


def im_options(**kw):
    o = dict(IM_DEFAULTS)
    o.update(kw)
    return o


def returns(reward, terminated, truncated, value, bootstrap, gamma=0.99, reward_scale=1.0, **_):
    """(adv, ret) [T, N] float32: GAE with lambda = 1, no normalisation"""
    return P.gae(reward, terminated, truncated, value, bootstrap, gamma=gamma, lam=1.0, reward_scale=reward_scale, normalize_advantages=False)


def scale(ma, adv, ma_rate=1e-8, **_):
    """one advantages call: (new ma, c) from all recorded advantages in the order t * N + env"""
    flat = np.asarray(adv, F).reshape(-1).astype(D64)
    with np.errstate(all="ignore"):
        msq = P.csum(flat * flat) / D64(flat.size)
        ma = D64(ma) + D64(ma_rate) * (msq - D64(ma))
        c = F(D64(1e-8) + np.sqrt(ma))
    return float(ma), c


def weight(adv, c, beta=0.0, w_max=20.0, **_):
    adv = np.asarray(adv, F)
    if beta == 0:
        return np.ones(adv.shape, F)
    with np.errstate(all="ignore"):
        w = R.exp32((F(beta) * (adv / F(c)).astype(F)).astype(F))
        if w_max > 0:
            w = np.where(w > F(w_max), F(w_max), w)
    return w.astype(F)


def grad(policy, theta, obs, action, adv, ret, value_old, c, beta=0.0, vf_coef=1.0, w_max=20.0, train_log_std=True, **_):
    """the flat gradient [Q] float32, the ten sums and the statistics of S samples of the imitation loss under the scale c"""
    layers, value_layers, log_std = P.unflatten(policy, theta)
    x = np.ascontiguousarray(obs, dtype=F)
    action, adv, ret, value_old = (np.asarray(a, F) for a in (action, adv, ret, value_old))
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
        w = weight(adv, c, beta=beta, w_max=w_max)
        pol_loss = -(w * logp)
        g = (-w).astype(F)
        V = yv[-1][:, 0] if value_layers else np.zeros(S, F)
        dv = V - ret
        val_loss = F(0.5) * (dv * dv)
        dV = F(vf_coef) * dv
        pieces = np.stack([pol_loss, val_loss, entropy, logp, w, ret, ret - value_old], axis=1).astype(F)
        d_mean = g[:, None] * (z / sd)
        d_ls = np.where(moved, F(0), (g[:, None] * ((z * z) - F(1))) - F(0)).astype(F)
        if not train_log_std:
            d_ls = np.zeros(d_ls.shape, F)

        def backward(net, ys, d_out):
            deltas = [None] * len(net)
            deltas[-1] = d_out.astype(F)
            for l in range(len(net) - 2, -1, -1):
                wn = net[l + 1][0]
                s = R.sum8(wn.T[:, None, :] * deltas[l + 1].T[:, :, None])
                y = ys[l]
                dact = (F(1) - y * y) if act == "tanh" else np.where(y > 0, F(1), F(0)).astype(F)
                deltas[l] = (dact * s).astype(F)
            return deltas
        dp = backward(layers, yp, np.concatenate([d_mean, d_ls], axis=1) if two else d_mean)
        dvs = backward(value_layers, yv, dV[:, None]) if value_layers else []

        def term(xin, delta):
            x1 = np.concatenate([xin, np.ones((S, 1), F)], axis=1).astype(D64) if xin is not None else np.ones((S, 1), D64)
            return P.csum(x1[:, :, None] * delta.astype(D64)[:, None, :]).reshape(-1)
        parts = []
        for ys, ds in ((yp, dp), (yv, dvs)):
            for l, d in enumerate(ds):
                parts.append(term(x if l == 0 else ys[l - 1], d))
        if not two:
            parts.append(term(None, d_ls))
        gq = (np.concatenate(parts) / D64(S)).astype(F)
        p64 = pieces.astype(D64)
        sums = np.concatenate([P.csum(p64), P.csum(p64[:, 5:7] * p64[:, 5:7]), [P.csum(gq.astype(D64) * gq.astype(D64))]])
    return gq, sums, stats_of(sums, S)


def stats_of(sums, S):
    st = P.stats_of(sums, S)
    st["logp"], st["weight"] = st.pop("approx_kl"), st.pop("clip_fraction")
    return st


def minibatch(policy, state, rec, adv, ret, c, n0, B, opts, im):
    """what adc_engine_im_minibatch does to state = dict(theta, m, v, steps): sample s = t * B + (env - n0)"""
    sl = slice(n0, n0 + B)
    flat = lambda a: np.ascontiguousarray(a[:, sl]).reshape((-1,) + a.shape[2:])
    g, _, st = grad(policy, state["theta"], flat(rec["obs"]), flat(rec["action"]), flat(adv), flat(ret), flat(rec["value"]), c, **im)
    theta, m, v = P.step(state["theta"], state["m"], state["v"], g, state["steps"], **opts)
    return dict(theta=theta, m=m, v=v, steps=state["steps"] + 1), st


def update(policy, state, rec, adv, ret, c, epochs, opts, im):
    """adc_engine_im_update after the advantages: epochs x the minibatches in ascending env order, the last epoch's mean statistics"""
    N = rec["reward"].shape[1]
    mb = opts["minibatch_envs"] or N
    mean = None
    for _ in range(epochs):
        acc = dict.fromkeys(STAT_KEYS, D64(0.0))
        for n0 in range(0, N, mb):
            state, st = minibatch(policy, state, rec, adv, ret, c, n0, mb, opts, im)
            with np.errstate(all="ignore"):
                acc = {k: acc[k] + st[k] for k in STAT_KEYS}
        with np.errstate(all="ignore"):
            mean = {k: acc[k] / D64(N // mb) for k in STAT_KEYS}
    return state, mean


# ---- the host twins ---------------------------------------------------------------------------------------------------------------
def im_config(**kw):
    from adcraft_amd.engine import StepEngine
    return StepEngine.im_config(**kw)


def twin_weight(lib, ma, adv, **im):
    cfg = im_config(**im)
    adv = np.ascontiguousarray(np.asarray(adv, F).reshape(-1))
    ma_c, c, w = C.c_double(ma), C.c_float(0.0), np.zeros(adv.size, F)
    rc = lib.adc_im_weight_host(C.byref(cfg), adv.size, adv.ctypes.data, C.byref(ma_c), C.byref(c), w.ctypes.data)
    assert rc == 0, rc
    return ma_c.value, F(c.value), w


def twin_grad(lib, policy, theta, obs, action, adv, ret, value_old, c, **im):
    from adcraft_amd import _ffi
    cfg, K = im_config(**im), policy.num_keywords
    mcfg = policy.config(K)
    arrs = [np.ascontiguousarray(a, dtype=F) for a in (theta, obs, action, adv, ret, value_old)]
    q = C.c_int64(0)
    assert lib.adc_pg_param_count_host(C.byref(mcfg), K, C.byref(q)) == 0 and q.value == arrs[0].size, (q.value, arrs[0].size)
    g, sums, st = np.zeros(q.value, F), np.zeros(10, D64), _ffi.IMStats()
    rc = lib.adc_im_grad_host(C.byref(mcfg), K, C.byref(cfg), C.c_float(c), arrs[0].ctypes.data, arrs[1].shape[0], *(a.ctypes.data for a in arrs[1:]),
                              g.ctypes.data, sums.ctypes.data, C.byref(st))
    assert rc == 0, rc
    return g, sums, {k: getattr(st, k) for k in STAT_KEYS}
