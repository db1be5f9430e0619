"""The off-policy law (adcraft_amd/csrc/adc_td3.h) restated in numpy from the header's comments: the replay ring, the batch
indices, the TD3 target, the twin critics' gradient, the deterministic policy gradient through critic 1's action inputs, the
optimiser steps and Polyak averaging, one float32 rounding at a time, on top of tests/mlp_ref.py and tests/pg_ref.py.  The host
twins (adc_td3_*_host) and the device kernels must give these very bits.  Networks are lists of (W [n_in, n_out], b [n_out]);
theta / psi are the flat vectors."""
import ctypes as C

import numpy as np

from tests import mlp_ref as R
from tests import pg_ref as P

F = np.float32
D64 = np.float64
ST_TD3_BATCH, ST_TD3_NOISE = 16, 17
DEFAULTS = dict(gamma=0.99, tau=0.005, policy_delay=2, target_noise=0.2, target_noise_clip=0.5, action_lo=0.0, action_hi=0.0, reward_scale=1.0,
                batch_size=256, capacity=100000, critic_widths=(256, 256, 1), actor_lr=1e-3, critic_lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
                optimiser="adam", max_grad_norm=0.0, seed=0)
STATE_KEYS = ("theta", "psi", "theta_target", "psi_target", "m_theta", "v_theta", "m_psi", "v_psi")
STAT_KEYS = ("critic_loss", "q1_mean", "q2_mean", "y_mean", "actor_loss", "critic_grad_norm", "actor_grad_norm")


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def td3_key(seed):
    return R._mix64(int(seed) ^ 0x6A09E667F3BCC908)


def _words(key, index, stage, keyword, tick):
    from oracle import capi as orc
    return orc.philox([index, stage, keyword, tick], [key & 0xFFFFFFFF, key >> 32])


def batch_indices(seed, update, size, B):
    """idx [B] int32: (uint64(word b % 4 of draw(key, b / 4, 16, 0, update)) * size) >> 32"""
    key, idx = td3_key(seed), np.zeros(B, np.int32)
    for q in range((B + 3) // 4):
        w = _words(key, q, ST_TD3_BATCH, 0, int(update))
        for h in range(4):
            if 4 * q + h < B:
                idx[4 * q + h] = (int(w[h]) * int(size)) >> 32
    return idx


def noise(seed, update, B, A):
    """n [B, A]: normal_from_word(word a % 4 of draw(key, a / 4, 17, b, update))"""
    from oracle import capi as orc
    L, key, n = orc.lib(), td3_key(seed), np.zeros((B, A), F)
    for b in range(B):
        for q in range((A + 3) // 4):
            w = _words(key, q, ST_TD3_NOISE, b, int(update))
            for h in range(4):
                if 4 * q + h < A:
                    n[b, 4 * q + h] = L.orc_normal_from_word(int(w[h]))
    return n


# ---- networks ---------------------------------------------------------------------------------------------------------------------
def flat_of(layers):
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in layers]).astype(F)


def unflat(flat, n_in, widths):
    flat, pos, out = np.asarray(flat, F), 0, []
    for n_out in widths:
        nw = n_in * n_out
        out.append((flat[pos:pos + nw].reshape(n_in, n_out).copy(), flat[pos + nw:pos + nw + n_out].copy()))
        pos += nw + n_out
        n_in = n_out
    assert pos == flat.size, (pos, flat.size)
    return out


def forward(x, layers, act):
    ys, h = [], x
    for i, (w, b) in enumerate(layers):
        h = R.layer(h, w, b, act if i + 1 < len(layers) else None)
        ys.append(h)
    return ys


def backward(layers, ys, d_out, act):
    """the deltas of every layer from the last layer's (adc_pg.h's backward)"""
    deltas = [None] * len(layers)
    deltas[-1] = d_out.astype(F)
    for l in range(len(layers) - 2, -1, -1):
        w = layers[l + 1][0]
        s = R.sum8(w.T[:, None, :] * deltas[l + 1].T[:, :, None])
        y = ys[l]
        dact = (F(1) - y * y) if act == "tanh" else np.where(y > 0, F(1), F(0)).astype(F)
        deltas[l] = (dact * s).astype(F)
    return deltas


def net_grad(x, ys, deltas):
    """the flat gradient of one network over the batch: float32(csum over b / f64(B)) per parameter, bias the row x = 1"""
    S, parts = x.shape[0], []
    for l, d in enumerate(deltas):
        xin = x if l == 0 else ys[l - 1]
        x1 = np.concatenate([xin, np.ones((S, 1), F)], axis=1).astype(D64)
        parts.append(P.csum(x1[:, :, None] * d.astype(D64)[:, None, :]).reshape(-1))
    return (np.concatenate(parts) / D64(S)).astype(F)


def action_norm(a, norm):
    if norm is None:
        return np.asarray(a, F)
    return ((np.asarray(a, F) - norm[0][None, :]) * norm[1][None, :]).astype(F)


class Shapes:
    """what the law needs of the policy and the configuration: K, the activation, the widths of the actor and of a critic"""

    def __init__(self, policy, opts):
        self.K, self.act = policy.num_keywords, policy.activation
        self.D, self.A = 5 * self.K + 2, self.K + 1
        self.pol_widths = [w.shape[1] for w, _ in policy.layers]
        self.q_widths = list(opts["critic_widths"])
        self.P = sum((i + 1) * o for i, o in zip([self.D] + self.pol_widths[:-1], self.pol_widths))
        self.Qc = sum((i + 1) * o for i, o in zip([self.D + self.A] + self.q_widths[:-1], self.q_widths))

    def actor(self, theta):
        return unflat(theta, self.D, self.pol_widths)

    def critics(self, psi):
        return [unflat(np.asarray(psi, F)[i * self.Qc:(i + 1) * self.Qc], self.D + self.A, self.q_widths) for i in range(2)]


# ---- the law's steps ----------------------------------------------------------------------------------------------------------------
def target(sh, theta_t, psi_t, norm, seed, update, x2, r, done, opts):
    """y [B] float32"""
    x2, r, B = np.ascontiguousarray(x2, F), np.asarray(r, F), len(r)
    with np.errstate(all="ignore"):
        mu = forward(x2, sh.actor(theta_t), sh.act)[-1]
        c = F(opts["target_noise_clip"])
        e = F(opts["target_noise"]) * noise(seed, update, B, sh.A)
        e = np.where(e < -c, -c, e)
        e = np.where(e > c, c, e).astype(F)
        a = (mu + e).astype(F)
        lo, hi = F(opts["action_lo"]), F(opts["action_hi"])
        if hi > lo:
            a = np.where(a < lo, lo, a)
            a = np.where(a > hi, hi, a).astype(F)
        row = np.concatenate([x2, action_norm(a, norm)], axis=1)
        q1, q2 = (forward(row, net, sh.act)[-1][:, 0] for net in sh.critics(psi_t))
        q = np.where(q1 < q2, q1, q2)
        nt = np.where(np.asarray(done, bool), F(0), F(1))
        y = (r * F(opts["reward_scale"])) + ((F(opts["gamma"]) * q) * nt)
    return y.astype(F)


def critic_grad(sh, psi, norm, x, a, y):
    """grad [2 Qc] float32 and the six sums: both loss pieces, Q1, Q2, y, grad^2"""
    x, y = np.ascontiguousarray(x, F), np.asarray(y, F)
    row = np.concatenate([x, action_norm(a, norm)], axis=1)
    parts, pieces = [], []
    with np.errstate(all="ignore"):
        for net in sh.critics(psi):
            ys = forward(row, net, sh.act)
            q = ys[-1][:, 0]
            d = q - y
            pieces.append((F(0.5) * (d * d), q))
            parts.append(net_grad(row, ys, backward(net, ys, d[:, None], sh.act)))
        g = np.concatenate(parts)
        cols = np.stack([pieces[0][0], pieces[1][0], pieces[0][1], pieces[1][1], y], axis=1).astype(D64)
        sums = np.concatenate([P.csum(cols), [P.csum(g.astype(D64) * g.astype(D64))]])
    return g, sums


def actor_grad(sh, theta, psi, norm, x):
    """grad [P] float32 and the two sums: Q1(x, mu(x)), grad^2"""
    x = np.ascontiguousarray(x, F)
    actor, q1 = sh.actor(theta), sh.critics(psi)[0]
    with np.errstate(all="ignore"):
        yp = forward(x, actor, sh.act)
        row = np.concatenate([x, action_norm(yp[-1], norm)], axis=1)
        yq = forward(row, q1, sh.act)
        dq = backward(q1, yq, np.ones((len(x), 1), F), sh.act)
        w0a = q1[0][0][sh.D:, :]                                        # the action inputs' rows of the first critic layer
        din = R.sum8(w0a.T[:, None, :] * dq[0].T[:, :, None])
        dmu = (-(din * norm[1][None, :]) if norm is not None else -din).astype(F)
        g = net_grad(x, yp, backward(actor, yp, dmu, sh.act))
        sums = np.array([P.csum(yq[-1][:, 0].astype(D64)), P.csum(g.astype(D64) * g.astype(D64))])
    return g, sums


def polyak(t, p, tau):
    t, p = np.asarray(t, F), np.asarray(p, F)
    with np.errstate(all="ignore"):
        return (t + (F(tau) * (p - t))).astype(F)


def _step(vec, m, v, g, steps, lr, opts):
    return P.step(vec, m, v, g, steps, max_grad_norm=opts["max_grad_norm"], optimiser=opts["optimiser"], lr=lr, beta1=opts["beta1"],
                  beta2=opts["beta2"], eps=opts["eps"])


def fresh_state(policy, critics):
    """the state right after td3_init and td3_set_critics(sync_targets=True)"""
    theta, psi = flat_of(policy.layers), np.concatenate([flat_of(c) for c in critics])
    st = dict(theta=theta, psi=psi, theta_target=theta.copy(), psi_target=psi.copy(), updates=0, actor_steps=0)
    st.update(m_theta=np.zeros_like(theta), v_theta=np.zeros_like(theta), m_psi=np.zeros_like(psi), v_psi=np.zeros_like(psi))
    return st


def update(policy, state, buf, norm, seed, opts):
    """one adc_engine_td3_update(1) on state (fresh_state's keys) and the ring buf = dict(x, a, r, done, x2) holding `size` rows.
    Returns (new state, statistics)"""
    sh, st, u = Shapes(policy, opts), dict(state), state["updates"]
    B, size = opts["batch_size"], len(buf["r"])
    idx = batch_indices(seed, u, size, B)
    x, a = buf["x"][idx], buf["a"][idx]
    y = target(sh, st["theta_target"], st["psi_target"], norm, seed, u, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
    g, s6 = critic_grad(sh, st["psi"], norm, x, a, y)
    st["psi"], st["m_psi"], st["v_psi"] = _step(st["psi"], st["m_psi"], st["v_psi"], g, u, opts["critic_lr"], opts)
    n = D64(B)
    stats = dict(critic_loss=s6[0] / n + s6[1] / n, q1_mean=s6[2] / n, q2_mean=s6[3] / n, y_mean=s6[4] / n, critic_grad_norm=np.sqrt(s6[5]),
                 actor_loss=-D64(0.0), actor_grad_norm=D64(0.0))
    if (u + 1) % opts["policy_delay"] == 0:
        g, s2 = actor_grad(sh, st["theta"], st["psi"], norm, x)
        st["theta"], st["m_theta"], st["v_theta"] = _step(st["theta"], st["m_theta"], st["v_theta"], g, st["actor_steps"], opts["actor_lr"], opts)
        st["theta_target"] = polyak(st["theta_target"], st["theta"], opts["tau"])
        st["psi_target"] = polyak(st["psi_target"], st["psi"], opts["tau"])
        st["actor_steps"] += 1
        stats.update(actor_loss=-(s2[0] / n), actor_grad_norm=np.sqrt(s2[1]))
    st["updates"] = u + 1
    return st, stats


# ---- the ring ---------------------------------------------------------------------------------------------------------------------
class Ring:
    """the replay ring on the host: store() appends a record's days [t0, T) as adc_engine_td3_store does"""

    def __init__(self, capacity, D, A):
        self.C, self.written = int(capacity), 0
        self.x, self.a, self.x2 = np.zeros((self.C, D), F), np.zeros((self.C, A), F), np.zeros((self.C, D), F)
        self.r, self.done = np.zeros(self.C, F), np.zeros(self.C, bool)

    @property
    def size(self):
        return min(self.written, self.C)

    def store(self, rec, current_input, t0=0):
        """rec: rollout_fetch's dict with obs; current_input [N, D]: the input row an act would read now"""
        T, N = rec["reward"].shape
        for t in range(t0, T):
            for n in range(N):
                slot = (self.written + (t - t0) * N + n) % self.C
                self.x[slot], self.a[slot], self.r[slot] = rec["obs"][t, n], rec["action"][t, n], rec["reward"][t, n]
                self.done[slot] = rec["terminated"][t, n] or rec["truncated"][t, n]
                self.x2[slot] = rec["obs"][t + 1, n] if t + 1 < T else current_input[n]
        self.written += (T - t0) * N

    def buffer(self):
        n = self.size
        return dict(x=self.x[:n], a=self.a[:n], r=self.r[:n], done=self.done[:n], x2=self.x2[:n], size=n, written=self.written, capacity=self.C)


def current_input(policy, out, first):
    """the input row an act would read from a step's output dict: zeros where `first` [N] (the first day of an episode), normalised"""
    x = R.flat_obs(out)
    x[np.asarray(first, bool)] = 0
    if policy.shift is not None:
        with np.errstate(all="ignore"):
            x = ((x - policy.shift[None, :]) * policy.scale[None, :]).astype(F)
    return x.astype(F)


# ---- the host twins -----------------------------------------------------------------------------------------------------------------
def td3_config(**kw):
    from adcraft_amd.engine import StepEngine
    return StepEngine.td3_config(**kw)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _norm_arrays(norm):
    if norm is None:
        return None, None
    return np.ascontiguousarray(norm[0], dtype=F), np.ascontiguousarray(norm[1], dtype=F)


def twin_batch_indices(lib, seed, update, size, B):
    idx = np.zeros(B, np.int32)
    assert lib.adc_td3_batch_indices_host(int(seed), int(update), int(size), B, idx.ctypes.data) == 0
    return idx


def twin_target(lib, policy, theta_t, psi_t, norm, seed, update, x2, r, done, opts):
    cfg, mcfg, K = td3_config(**opts), policy.config(policy.num_keywords), policy.num_keywords
    th, ps, x2, r = (np.ascontiguousarray(a, dtype=F) for a in (theta_t, psi_t, x2, r))
    dn, (sh, sc) = np.ascontiguousarray(done, dtype=np.uint8), _norm_arrays(norm)
    y = np.zeros(len(r), F)
    rc = lib.adc_td3_target_host(C.byref(mcfg), K, C.byref(cfg), int(seed), int(update), th.ctypes.data, ps.ctypes.data, _ptr(sh), _ptr(sc), len(r),
                                 x2.ctypes.data, r.ctypes.data, dn.ctypes.data, y.ctypes.data)
    assert rc == 0, rc
    return y


def twin_critic_grad(lib, policy, psi, norm, x, a, y, opts):
    cfg, mcfg, K = td3_config(**opts), policy.config(policy.num_keywords), policy.num_keywords
    ps, x, a, y = (np.ascontiguousarray(v, dtype=F) for v in (psi, x, a, y))
    (sh, sc), g, sums = _norm_arrays(norm), np.zeros(ps.size, F), np.zeros(6, D64)
    rc = lib.adc_td3_critic_grad_host(C.byref(mcfg), K, C.byref(cfg), ps.ctypes.data, _ptr(sh), _ptr(sc), len(y), x.ctypes.data, a.ctypes.data,
                                      y.ctypes.data, g.ctypes.data, sums.ctypes.data)
    assert rc == 0, rc
    return g, sums


def twin_actor_grad(lib, policy, theta, psi, norm, x, opts):
    cfg, mcfg, K = td3_config(**opts), policy.config(policy.num_keywords), policy.num_keywords
    th, ps, x = (np.ascontiguousarray(v, dtype=F) for v in (theta, psi, x))
    (sh, sc), g, sums = _norm_arrays(norm), np.zeros(th.size, F), np.zeros(2, D64)
    rc = lib.adc_td3_actor_grad_host(C.byref(mcfg), K, C.byref(cfg), th.ctypes.data, ps.ctypes.data, _ptr(sh), _ptr(sc), len(x), x.ctypes.data,
                                     g.ctypes.data, sums.ctypes.data)
    assert rc == 0, rc
    return g, sums


def twin_polyak(lib, t, p, tau):
    t, p = np.array(t, dtype=F), np.ascontiguousarray(p, dtype=F)
    assert lib.adc_td3_polyak_host(float(tau), t.size, p.ctypes.data, t.ctypes.data) == 0
    return t


def random_critics_for_tests(rng, K, widths, scale=0.6):
    """two seeded random critics on the D + A inputs: weights ~ N(0, scale^2 / n_in), small biases"""
    out = []
    for _ in range(2):
        layers, n_in = [], 6 * K + 3
        for n_out in widths:
            layers.append(((rng.standard_normal((n_in, n_out)) * scale / np.sqrt(n_in)).astype(F), (rng.standard_normal(n_out) * 0.1).astype(F)))
            n_in = n_out
        out.append(layers)
    return out
