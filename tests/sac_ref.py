"""The soft actor-critic law (adcraft_amd/csrc/adc_sac.h) and the squashed act (adc_mlp.h's `squash`) restated in numpy from the
headers' comments, one float32 rounding at a time, on top of tests/mlp_ref.py, tests/pg_ref.py and tests/td3_ref.py (networks,
chunked sums, optimiser step, ring, batch indices).  The host twins (adc_sac_*_host, adc_mlp_squash_host) and the device kernels
must give these very bits.  theta / psi are the flat vectors; det_log is the oracle's."""
import ctypes as C

import numpy as np

from tests import mlp_ref as R
from tests import pg_ref as P
from tests import td3_ref as T3

F = np.float32
D64 = np.float64
ST_SAC_NEXT, ST_SAC_PI = 20, 21
DEFAULTS = dict(gamma=0.99, tau=0.005, target_update_interval=1, init_alpha=1.0, target_entropy=None, alpha_lr=3e-4, eps_sq=1e-6, reward_scale=1.0,
                batch_size=256, capacity=100000, critic_widths=(256, 256, 1), actor_lr=3e-4, critic_lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                optimiser="adam", max_grad_norm=0.0, seed=0)
STATE_KEYS = ("theta", "psi", "psi_target", "m_theta", "v_theta", "m_psi", "v_psi", "log_alpha")
STAT_KEYS = ("critic_loss", "q1_mean", "q2_mean", "y_mean", "actor_loss", "logp_mean", "alpha", "log_alpha", "critic_grad_norm", "actor_grad_norm")


def options(K, **kw):
    o = dict(DEFAULTS)
    o.update(kw)
    if o["target_entropy"] is None:
        o["target_entropy"] = -float(K + 1)
    return o


# ---- the squashed act ---------------------------------------------------------------------------------------------------------------
def squash(u, lo, hi):
    """e = lo + half * (tanh(u) + 1), half = 0.5 * (hi - lo): a sum, a product, a sum after the law's tanh"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(all="ignore"):
        half = F(0.5) * (hi - lo)
        return (lo + half * (R.tanh32(u) + F(1))).astype(F)


def squashed_act(policy, obs, z, lo, hi, deterministic=None, budget_override=0.0):
    """mlp_ref.act with the env's action taken from the squashed one; mean, log_std, action, logp, value are untouched"""
    ref = R.act(policy, obs, z, deterministic=deterministic, budget_override=budget_override)
    e = squash(ref["action"], lo, hi)
    with np.errstate(invalid="ignore"):
        budget = np.where(e[:, 0] > F(0.01), e[:, 0], F(0.01)).astype(F)
    if budget_override > 0:
        budget = np.full(len(e), F(budget_override))
    ref.update(bids=R.cent_bids(e[:, 1:], policy.bid_clip), budget=budget, env_action=e)
    return ref


def twin_squash(lib, u, lo, hi):
    u, lo, hi = (np.ascontiguousarray(a, dtype=F) for a in (u, lo, hi))
    out = np.zeros_like(u)
    assert lib.adc_mlp_squash_host(u.size, u.ctypes.data, lo.ctypes.data, hi.ctypes.data, out.ctypes.data) == 0
    return out


# ---- the law ------------------------------------------------------------------------------------------------------------------------
def det_log(x):
    from oracle import capi as orc
    L = orc.lib()
    x = np.asarray(x, F)
    return np.array([L.orc_det_logf(float(v)) for v in x.reshape(-1)], F).reshape(x.shape)


def noise(seed, stage, update, B, A):
    """z [B, A]: normal_from_word(word a % 4 of draw(td3 key, a / 4, stage, b, update))"""
    from oracle import capi as orc
    L, key, n = orc.lib(), T3.td3_key(seed), np.zeros((B, A), F)
    for b in range(B):
        for q in range((A + 3) // 4):
            w = T3._words(key, q, stage, b, int(update))
            for h in range(4):
                if 4 * q + h < A:
                    n[b, 4 * q + h] = L.orc_normal_from_word(int(w[h]))
    return n


def head(o, z, clamp, eps_sq):
    """from the policy's outputs o [B, 2A] and z [B, A]: dict of ls, sd, u, t, w, lp, moved"""
    A = o.shape[1] // 2
    mean, raw = o[:, :A], o[:, A:]
    lo, hi = F(clamp[0]), F(clamp[1])
    with np.errstate(all="ignore"):
        moved = (raw < lo) | (raw > hi)
        ls = np.where(raw < lo, lo, raw)
        ls = np.where(ls > hi, hi, ls).astype(F)
        sd = R.exp32(ls)
        u = (mean + sd * z).astype(F)
        t = R.tanh32(u)
        w = (F(1) - t * t).astype(F)
        c = det_log((w + F(eps_sq)).astype(F))
        terms = ((-((z * z) * F(0.5))) - ls).astype(F)
        lp = ((R.sum8(terms.T) - F(A) * R.HALF_LOG_2PI) - R.sum8(c.T)).astype(F)
    return dict(ls=ls, sd=sd, u=u, t=t, w=w, lp=lp, moved=moved, z=np.asarray(z, F))


def target(sh, clamp, theta, psi_t, alpha, seed, update, x2, r, done, opts):
    """y [B], lp' [B] float32 under the LIVE actor theta"""
    x2, r, B = np.ascontiguousarray(x2, F), np.asarray(r, F), len(r)
    with np.errstate(all="ignore"):
        o = T3.forward(x2, sh.actor(theta), sh.act)[-1]
        h = head(o, noise(seed, ST_SAC_NEXT, update, B, sh.A), clamp, opts["eps_sq"])
        row = np.concatenate([x2, h["t"]], axis=1)
        q1, q2 = (T3.forward(row, net, sh.act)[-1][:, 0] for net in sh.critics(psi_t))
        q = np.where(q1 < q2, q1, q2)
        nt = np.where(np.asarray(done, bool), F(0), F(1))
        v = q - (F(alpha) * h["lp"])
        y = (r * F(opts["reward_scale"])) + ((F(opts["gamma"]) * v) * nt)
    return y.astype(F), h["lp"]


def critic_grad(sh, psi, x, u, y):
    """as td3_ref.critic_grad on [x | tanh(u)]"""
    return T3.critic_grad(sh, psi, None, x, R.tanh32(np.asarray(u, F)), y)


def actor_grad(sh, clamp, theta, psi, alpha, seed, update, x, opts):
    """grad [P] float32, lp [B], and the four sums: the loss piece, lp, grad^2, the elements that took critic 2"""
    x, B, al, eps = np.ascontiguousarray(x, F), len(x), F(alpha), F(opts["eps_sq"])
    actor, critics = sh.actor(theta), sh.critics(psi)
    with np.errstate(all="ignore"):
        yp = T3.forward(x, actor, sh.act)
        h = head(yp[-1], noise(seed, ST_SAC_PI, update, B, sh.A), clamp, opts["eps_sq"])
        row = np.concatenate([x, h["t"]], axis=1)
        yqs = [T3.forward(row, net, sh.act) for net in critics]
        q1, q2 = yqs[0][-1][:, 0], yqs[1][-1][:, 0]
        pick = q2 < q1                                                    # a tie takes critic 1
        gq = np.zeros((B, sh.A), F)
        for i, net in enumerate(critics):
            dq = T3.backward(net, yqs[i], np.ones((B, 1), F), sh.act)
            din = R.sum8(net[0][0][sh.D:, :].T[:, None, :] * dq[0].T[:, :, None])
            gq[pick == bool(i)] = din[pick == bool(i)]
        t, w = h["t"], h["w"]
        k = ((t + t) * w).astype(F)
        k = (k / (w + eps)).astype(F)
        du = ((al * k) - (gq * w)).astype(F)
        dls = np.where(h["moved"], F(0), (du * (h["sd"] * h["z"])) - al).astype(F)
        g = T3.net_grad(x, yp, T3.backward(actor, yp, np.concatenate([du, dls], axis=1), sh.act))
        loss = ((al * h["lp"]) - np.where(pick, q2, q1)).astype(F)
        sums = np.array([P.csum(loss.astype(D64)), P.csum(h["lp"].astype(D64)), P.csum(g.astype(D64) * g.astype(D64)), D64(pick.sum())])
    return g, h["lp"], sums


def log_alpha_init(init_alpha):
    return det_log(np.array([init_alpha], F))[0]


def alpha_of(log_alpha):
    return R.exp32(np.array([log_alpha], F))[0]


def alpha_step(la3, lp_sum, B, steps, opts):
    """la3 = (log_alpha, m, v) float32 -> the new three; alpha_lr == 0: unchanged"""
    la3 = np.array(la3, F)
    if not opts["alpha_lr"] > 0:
        return la3
    g = F(-(D64(lp_sum) / D64(B) + D64(F(opts["target_entropy"]))))
    la, m, v = P.step(la3[0:1], la3[1:2], la3[2:3], np.array([g], F), steps, max_grad_norm=0.0, optimiser=opts["optimiser"], lr=opts["alpha_lr"],
                      beta1=opts["beta1"], beta2=opts["beta2"], eps=opts["eps"])
    return np.array([la[0], m[0], v[0]], F)


def fresh_state(policy, critics, opts):
    """the state right after sac_init and sac_set_critics(sync_targets=True)"""
    theta, psi = T3.flat_of(policy.layers), np.concatenate([T3.flat_of(c) for c in critics])
    st = dict(theta=theta, psi=psi, psi_target=psi.copy(), updates=0, log_alpha=np.array([log_alpha_init(opts["init_alpha"]), 0, 0], F))
    st.update(m_theta=np.zeros_like(theta), v_theta=np.zeros_like(theta), m_psi=np.zeros_like(psi), v_psi=np.zeros_like(psi))
    return st


def update(policy, state, buf, seed, opts):
    """one adc_engine_sac_update(1) on state (fresh_state's keys) and the ring buf = dict(x, a, r, done, x2).  Returns (new state,
    statistics)"""
    sh, st, u = T3.Shapes(policy, opts), dict(state), state["updates"]
    clamp, B, size = policy.log_std_clamp, opts["batch_size"], len(buf["r"])
    alpha = alpha_of(st["log_alpha"][0])
    idx = T3.batch_indices(seed, u, size, B)
    x = buf["x"][idx]
    y, _ = target(sh, clamp, st["theta"], st["psi_target"], alpha, seed, u, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
    g, s6 = critic_grad(sh, st["psi"], x, buf["a"][idx], y)
    st["psi"], st["m_psi"], st["v_psi"] = T3._step(st["psi"], st["m_psi"], st["v_psi"], g, u, opts["critic_lr"], opts)
    g, _, s4 = actor_grad(sh, clamp, st["theta"], st["psi"], alpha, seed, u, x, opts)
    st["theta"], st["m_theta"], st["v_theta"] = T3._step(st["theta"], st["m_theta"], st["v_theta"], g, u, opts["actor_lr"], opts)
    st["log_alpha"] = alpha_step(st["log_alpha"], s4[1], B, u, opts)
    if (u + 1) % opts["target_update_interval"] == 0:
        st["psi_target"] = T3.polyak(st["psi_target"], st["psi"], opts["tau"])
    st["updates"] = u + 1
    n = D64(B)
    stats = dict(critic_loss=s6[0] / n + s6[1] / n, q1_mean=s6[2] / n, q2_mean=s6[3] / n, y_mean=s6[4] / n, critic_grad_norm=np.sqrt(s6[5]),
                 actor_loss=s4[0] / n, logp_mean=s4[1] / n, actor_grad_norm=np.sqrt(s4[2]), alpha=D64(alpha_of(st["log_alpha"][0])),
                 log_alpha=D64(st["log_alpha"][0]), picked2=s4[3])
    return st, stats


# ---- the host twins -----------------------------------------------------------------------------------------------------------------
def sac_config(K, **kw):
    from adcraft_amd.engine import StepEngine
    return StepEngine.sac_config(num_keywords=K, **kw)


def twin_logp(lib, policy, eps_sq, mean, raw, z):
    mean, raw, z = (np.ascontiguousarray(a, dtype=F) for a in (mean, raw, z))
    mcfg, u, t, lp = policy.config(policy.num_keywords), np.zeros_like(mean), np.zeros_like(mean), np.zeros(len(mean), F)
    rc = lib.adc_sac_logp_host(C.byref(mcfg), policy.num_keywords, float(eps_sq), len(mean), mean.ctypes.data, raw.ctypes.data, z.ctypes.data,
                               u.ctypes.data, t.ctypes.data, lp.ctypes.data)
    assert rc == 0, rc
    return u, t, lp


def twin_target(lib, policy, theta, psi_t, alpha, seed, update, x2, r, done, opts):
    K = policy.num_keywords
    cfg, mcfg = sac_config(K, **opts), policy.config(K)
    th, ps, x2, r = (np.ascontiguousarray(a, dtype=F) for a in (theta, psi_t, x2, r))
    dn, y, lp = np.ascontiguousarray(done, dtype=np.uint8), np.zeros(len(r), F), np.zeros(len(r), F)
    rc = lib.adc_sac_target_host(C.byref(mcfg), K, C.byref(cfg), int(seed), int(update), float(alpha), th.ctypes.data, ps.ctypes.data, len(r),
                                 x2.ctypes.data, r.ctypes.data, dn.ctypes.data, y.ctypes.data, lp.ctypes.data)
    assert rc == 0, rc
    return y, lp


def twin_critic_grad(lib, policy, psi, x, u, y, opts):
    K = policy.num_keywords
    cfg, mcfg = sac_config(K, **opts), policy.config(K)
    ps, x, u, y = (np.ascontiguousarray(v, dtype=F) for v in (psi, x, u, y))
    g, sums = np.zeros(ps.size, F), np.zeros(6, D64)
    rc = lib.adc_sac_critic_grad_host(C.byref(mcfg), K, C.byref(cfg), ps.ctypes.data, len(y), x.ctypes.data, u.ctypes.data, y.ctypes.data, g.ctypes.data,
                                      sums.ctypes.data)
    assert rc == 0, rc
    return g, sums


def twin_actor_grad(lib, policy, theta, psi, alpha, seed, update, x, opts):
    K = policy.num_keywords
    cfg, mcfg = sac_config(K, **opts), policy.config(K)
    th, ps, x = (np.ascontiguousarray(v, dtype=F) for v in (theta, psi, x))
    g, lp, sums = np.zeros(th.size, F), np.zeros(len(x), F), np.zeros(4, D64)
    rc = lib.adc_sac_actor_grad_host(C.byref(mcfg), K, C.byref(cfg), int(seed), int(update), float(alpha), th.ctypes.data, ps.ctypes.data, len(x),
                                     x.ctypes.data, g.ctypes.data, lp.ctypes.data, sums.ctypes.data)
    assert rc == 0, rc
    return g, lp, sums


def twin_alpha_step(lib, K, la3, lp_sum, B, steps, opts):
    cfg, la3, alpha = sac_config(K, **opts), np.array(la3, F), C.c_float(0)
    rc = lib.adc_sac_alpha_step_host(C.byref(cfg), int(steps), float(lp_sum), int(B), la3.ctypes.data, C.byref(alpha))
    assert rc == 0, rc
    return la3, F(alpha.value)


def sac_policy(rng, K, hidden, activation="tanh", clamp=(-5.0, 2.0), scale=0.5, **kw):
    """a seeded two-headed policy with the log-std clamp on"""
    return R.random_policy(rng, K, hidden, activation, two_heads=True, scale=scale, log_std_clamp=clamp, **kw)
