"""The law of the PPO learners' KL penalty and value-loss clip (adcraft_amd/csrc/adc_pg_kl.h) restated in numpy from the header's
comments, one float32 rounding at a time: the snapshot of the collecting distribution, the per-sample analytic KL and its
gradient's share of the output deltas, the capped value error, the two statistics and the adaptation of the coefficient.  What is
adc_pg.h's - forward, head, surrogate, backward, chunked sums, the step - is restated here once more, in tests/pg_ref.py's words,
because the deltas change in the middle of it.  The host twins (adc_pg_kl_grad_host, adc_pg_kl_adapt_host) and the device kernels
must give these very bits."""
import ctypes as C

import numpy as np

from tests import mlp_ref as R
from tests import pg_ref as P

F = np.float32
D64 = np.float64
KL_DEFAULTS = dict(kl_coef=0.2, kl_target=0.01, adaptive=True, vf_clip=0.0, factor_up=0.0, factor_down=0.0)


def kl_options(**kw):
    o = dict(KL_DEFAULTS)
    o.update(kw)
    return o


def _head(policy, layers, log_std, x):
    """forward of the policy network and the head on the rows x: (layer outputs, mean, raw, ls, moved, two heads)"""
    A, act = policy.num_keywords + 1, policy.activation
    ys, h = [], x
    for i, (w, b) in enumerate(layers):
        h = R.layer(h, w, b, act if i + 1 < len(layers) else None)
        ys.append(h)
    o = ys[-1]
    two = o.shape[1] == 2 * A
    mean = o[:, :A]
    raw = o[:, A:] if two else np.broadcast_to(log_std, mean.shape).astype(F)
    ls, moved = raw, np.zeros(raw.shape, bool)
    if policy.log_std_clamp is not None:
        lo, hi = F(policy.log_std_clamp[0]), F(policy.log_std_clamp[1])
        ls = np.where(ls < lo, lo, ls)
        ls = np.where(ls > hi, hi, ls).astype(F)
        moved = (raw < lo) | (raw > hi)
    return ys, mean, raw, ls, moved, two


def old_dist(policy, theta, obs):
    """the snapshot under theta of the recorded input rows obs [S, D]: mean_old [S, A]; ls_old [S, A] with two heads, else the
    clamped log_std vector [A]"""
    layers, _, log_std = P.unflatten(policy, theta)
    with np.errstate(all="ignore"):
        _, mean, _, ls, _, two = _head(policy, layers, log_std, np.ascontiguousarray(obs, dtype=F))
    return mean.astype(F).copy(), (ls.astype(F).copy() if two else ls[0].astype(F).copy())


def kl_per_sample(mean, ls, mean_old, ls_old):
    """kl [S] and the per-component pieces the gradient needs; ls_old [S, A] or [A]"""
    ls_old = np.broadcast_to(np.asarray(ls_old, F), mean.shape)
    sd, sd_old = R.exp32(ls), R.exp32(ls_old)
    v, vo = sd * sd, sd_old * sd_old
    dm, dl = mean_old - mean, ls - ls_old
    num = vo + (dm * dm)
    term = ((dl + (num / (F(2) * v))) - F(0.5)).astype(F)
    return R.sum8(term.T).astype(F), dm, v, num


def grad(policy, theta, obs, action, logp_old, adv, ret, value_old, mean_old, ls_old, kl_coef=0.0, vf_clip=0.0, eps_clip=0.2, vf_coef=0.5,
         ent_coef=0.0, **_):
    """the flat gradient [Q] float32, adc_pg.h's ten sums, the add-on's two sums, the statistics of both, of S samples"""
    layers, value_layers, log_std = P.unflatten(policy, theta)
    x = np.ascontiguousarray(obs, dtype=F)
    action, logp_old, adv, ret, value_old, mean_old = (np.asarray(a, F) for a in (action, logp_old, adv, ret, value_old, mean_old))
    S, A, act = x.shape[0], policy.num_keywords + 1, policy.activation
    with np.errstate(all="ignore"):
        yp, mean, raw, ls, moved, two = _head(policy, layers, log_std, x)
        yv, h = [], x
        for i, (w, b) in enumerate(value_layers):
            h = R.layer(h, w, b, act if i + 1 < len(value_layers) else None)
            yv.append(h)
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
        sq = dv * dv
        vf_clipped = (sq > F(vf_clip)) if vf_clip > 0 else np.zeros(S, bool)
        val_loss = np.where(vf_clipped, F(0.5) * F(vf_clip), F(0.5) * sq).astype(F)
        dV = np.where(vf_clipped, F(0), F(vf_coef) * dv).astype(F)
        pieces = np.stack([-surr, val_loss, entropy, logp_old - logp, clipped.astype(F), ret, ret - value_old], axis=1).astype(F)
        kl, dm, v, num = kl_per_sample(mean, ls, mean_old, ls_old)
        d_mean = g[:, None] * (z / sd)
        d_ls = np.where(moved, F(0), (g[:, None] * ((z * z) - F(1))) - F(ent_coef)).astype(F)
        if F(kl_coef) != 0:                                         # (a zero coefficient adds nothing: adc_pg.h's bits)
            k_mean = -(dm / v)
            k_ls = np.where(moved, F(0), F(1) - (num / v)).astype(F)
            d_mean = (d_mean + (F(kl_coef) * k_mean)).astype(F)
            d_ls = (d_ls + (F(kl_coef) * k_ls)).astype(F)

        def backward(net, ys, d_out):
            deltas = [None] * len(net)
            deltas[-1] = d_out.astype(F)
            for l in range(len(net) - 2, -1, -1):
                w = net[l + 1][0]
                s = R.sum8(w.T[:, None, :] * deltas[l + 1].T[:, :, None])
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
        sums_kl = P.csum(np.stack([kl, vf_clipped.astype(F)], axis=1).astype(D64))
        kl_stats = dict(kl=sums_kl[0] / D64(S), vf_clip_fraction=sums_kl[1] / D64(S), kl_coef=F(kl_coef), kl_coef_next=F(kl_coef))
    return gq, sums, sums_kl, P.stats_of(sums, S), kl_stats, dict(kl=kl, vf_clipped=vf_clipped, sq=sq)


def adapt(coef, kl, kl_target=0.01, adaptive=True, factor_up=0.0, factor_down=0.0, **_):
    """the coefficient after an update whose last epoch's mean KL was kl (float64)"""
    coef = F(coef)
    if not adaptive:
        return coef
    up, down = F(factor_up) if factor_up else F(1.5), F(factor_down) if factor_down else F(0.5)
    t = D64(F(kl_target))
    if D64(kl) > 2.0 * t:
        return F(coef * up)
    if D64(kl) < 0.5 * t:
        return F(coef * down)
    return coef


def snapshot(policy, theta, rec):
    """old_dist over the whole record: mean_old [T, N, A]; ls_old [T, N, A] or [A]"""
    T, N = rec["obs"].shape[:2]
    mean, ls = old_dist(policy, theta, rec["obs"].reshape(T * N, -1))
    return mean.reshape(T, N, -1), (ls.reshape(T, N, -1) if ls.ndim == 2 else ls)


def minibatch(policy, state, rec, adv, ret, snap, n0, B, opts, kl_opts, coef):
    """what adc_engine_pg_minibatch does under the add-on to state = dict(theta, m, v, steps): sample s = t * B + (env - n0).
    Returns (new state, statistics, the add-on's statistics)"""
    sl = slice(n0, n0 + B)
    flat = lambda a: np.ascontiguousarray(a[:, sl]).reshape((-1,) + a.shape[2:])
    mean_old, ls_old = snap
    g, _, _, st, kst, _ = grad(policy, state["theta"], flat(rec["obs"]), flat(rec["action"]), flat(rec["logp"]), flat(adv), flat(ret), flat(rec["value"]),
                               flat(mean_old), flat(ls_old) if ls_old.ndim == 3 else ls_old, kl_coef=coef, vf_clip=kl_opts["vf_clip"], **opts)
    theta, m, v = P.step(state["theta"], state["m"], state["v"], g, state["steps"], **opts)
    return dict(theta=theta, m=m, v=v, steps=state["steps"] + 1), st, kst


def update(policy, state, rec, bootstrap, epochs, opts, kl_opts, coef):
    """adc_engine_pg_update under the add-on: advantages and the snapshot once, epochs x the minibatches ascending, then the
    adaptation.  Returns (new state, the last epoch's statistics, the add-on's statistics with kl_coef_next)"""
    adv, ret = P.gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], bootstrap, **opts)
    snap = snapshot(policy, state["theta"], rec)
    N = rec["reward"].shape[1]
    mb = opts["minibatch_envs"] or N
    for _ in range(epochs):
        acc = dict.fromkeys(P.STAT_KEYS, D64(0.0))
        kacc = dict(kl=D64(0.0), vf_clip_fraction=D64(0.0))
        for n0 in range(0, N, mb):
            state, st, kst = minibatch(policy, state, rec, adv, ret, snap, n0, mb, opts, kl_opts, coef)
            with np.errstate(all="ignore"):
                acc = {k: acc[k] + st[k] for k in P.STAT_KEYS}
                kacc = {k: kacc[k] + kst[k] for k in kacc}
        with np.errstate(all="ignore"):
            mean = {k: acc[k] / D64(N // mb) for k in P.STAT_KEYS}
            kmean = {k: kacc[k] / D64(N // mb) for k in kacc}
    kmean.update(kl_coef=F(coef), kl_coef_next=adapt(coef, kmean["kl"], **kl_opts))
    return state, mean, kmean


# ---- the host twins ---------------------------------------------------------------------------------------------------------------
def kl_config(**kw):
    from adcraft_amd.engine import StepEngine
    return StepEngine.pg_kl_config(**kw)


KL_STAT_KEYS = ("kl", "vf_clip_fraction", "kl_coef", "kl_coef_next")


def twin_grad(lib, policy, theta, obs, action, logp_old, adv, ret, value_old, mean_old, ls_old, kl_coef=0.0, vf_clip=0.0, **kw):
    from adcraft_amd import _ffi
    cfg, K = P.pg_config(**kw), policy.num_keywords
    klc = kl_config(kl_coef=kl_coef, vf_clip=vf_clip)
    mcfg = policy.config(K)
    arrs = [np.ascontiguousarray(a, dtype=F) for a in (theta, obs, action, logp_old, adv, ret, value_old)]
    mean_old, ls_old = np.ascontiguousarray(mean_old, dtype=F), np.ascontiguousarray(ls_old, dtype=F)
    g, sums, sums_kl, st, kst = np.zeros(arrs[0].size, F), np.zeros(10, D64), np.zeros(2, D64), _ffi.PGStats(), _ffi.PGKLStats()
    rc = lib.adc_pg_kl_grad_host(C.byref(mcfg), K, C.byref(cfg), arrs[0].ctypes.data, arrs[1].shape[0], *(a.ctypes.data for a in arrs[1:]),
                                 C.byref(klc), float(F(kl_coef)), mean_old.ctypes.data, ls_old.ctypes.data, 1 if ls_old.ndim == 2 else 0,
                                 g.ctypes.data, sums.ctypes.data, sums_kl.ctypes.data, C.byref(st), C.byref(kst))
    assert rc == 0, rc
    return g, sums, sums_kl, {k: getattr(st, k) for k in P.STAT_KEYS}, {k: getattr(kst, k) for k in KL_STAT_KEYS}


def twin_adapt(lib, coef, kl, **kw):
    klc = kl_config(**dict(kw, kl_coef=0.0))
    out = C.c_float(0.0)
    rc = lib.adc_pg_kl_adapt_host(C.byref(klc), float(F(coef)), float(kl), C.byref(out))
    assert rc == 0, rc
    return F(out.value)
