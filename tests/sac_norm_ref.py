"""The law of the SAC learners' running normalisers (adcraft_amd/csrc/adc_sac_norm.h) restated in numpy, one rounded IEEE operation
per line as the header's comment block states them, for the bit-exact tests of the host twin adc_sac_y_norm_host and of the device
kernels.  The moments are tests/td3_norm_ref.py's (the law is the same: tests/norm_ref.py's merge over raw rows,
tests/rew_norm_ref.py's update under the learner's discount), the SAC update tests/sac_ref.py's with the batch normalised as it is
sampled and sac_y_norm in the place of sac_y.  Nothing here calls the library except the twin_* functions."""
import ctypes as C

import numpy as np

from tests import per_ref as PER
from tests import sac_ref as S
from tests import td3_norm_ref as TN
from tests import td3_ref as T3

F, D64 = np.float32, np.float64

# ---- the moments: adc_td3_norm.h's, unchanged ---------------------------------------------------------------------------------------
obs_fresh, obs_update, normalize = TN.obs_fresh, TN.obs_update, TN.normalize
rew_fresh, rew_update = TN.rew_fresh, TN.rew_update
obs_same, rew_same, split = TN.obs_same, TN.rew_same, TN.split
twin_obs, twin_rew = TN.twin_obs, TN.twin_rew


# ---- the target under the normalisers ------------------------------------------------------------------------------------------------
def y_norm(r, done, q, alpha, lp, gamma, reward_scale, scale, clip):
    """sac_y_norm: rs = r * reward_scale; rs = rs * scale; the clip; al = alpha * lp; v = q - al; gv = gamma * v; gvn = gv * nt;
    y = rs + gvn.  The entropy term is not scaled."""
    r, q, lp, cl = np.asarray(r, F), np.asarray(q, F), np.asarray(lp, F), F(clip)
    with np.errstate(all="ignore"):
        rs = r * F(reward_scale)
        rs = rs * F(scale)
        if cl > 0:
            rs = np.where(rs < -cl, -cl, rs)
            rs = np.where(rs > cl, cl, rs)
        nt = np.where(np.asarray(done, bool), F(0), F(1))
        al = (F(alpha) * lp).astype(F)
        v = (q - al).astype(F)
        gv = (F(gamma) * v).astype(F)
        gvn = (gv * nt).astype(F)
        y = rs.astype(F) + gvn
    return y.astype(F)


def y_plain(r, done, q, alpha, lp, gamma, reward_scale):
    """adc_sac.h's sac_y (tests/sac_ref.py's last lines of target())"""
    r, q, lp = np.asarray(r, F), np.asarray(q, F), np.asarray(lp, F)
    with np.errstate(all="ignore"):
        nt = np.where(np.asarray(done, bool), F(0), F(1))
        v = q - (F(alpha) * lp)
        return ((r * F(reward_scale)) + ((F(gamma) * v) * nt)).astype(F)


def target(sh, clamp, theta, psi_t, alpha, seed, update, x2n, r, done, opts, scale, clip):
    """sac_ref.target with sac_y_norm in the place of sac_y; x2n: the rows already normalised.  Returns (y, lp', q)"""
    x2n, r, B = np.ascontiguousarray(x2n, F), np.asarray(r, F), len(r)
    with np.errstate(all="ignore"):
        o = T3.forward(x2n, sh.actor(theta), sh.act)[-1]
        h = S.head(o, S.noise(seed, S.ST_SAC_NEXT, update, B, sh.A), clamp, opts["eps_sq"])
        row = np.concatenate([x2n, h["t"]], axis=1)
        q1, q2 = (T3.forward(row, net, sh.act)[-1][:, 0] for net in sh.critics(psi_t))
        q = np.where(q1 < q2, q1, q2)
    return y_norm(r, done, q, alpha, h["lp"], opts["gamma"], opts["reward_scale"], scale, clip), h["lp"], q


def update(policy, state, buf, seed, opts, vectors=None, rew_scale=None, rew_clip=0.0, tree=None, per=None):
    """one adc_engine_sac_update(1) under live normalisers on the RAW ring buf: vectors = (shift, scale) [D] in force (None: the
    ring holds network inputs), rew_scale the multiplier in force (None: sac_y).  tree / per: prioritised replay's tree (updated in
    place) and options - the batch is tests/per_ref.py's draw, the critics' deltas are weighted and the leaves follow the |d| of the
    normalised inputs; None: the uniform law.  Returns (new state, statistics, dict(idx, w, y))."""
    sh, st, u = T3.Shapes(policy, opts), dict(state), state["updates"]
    clamp, B, size = policy.log_std_clamp, opts["batch_size"], len(buf["r"])
    alpha = S.alpha_of(st["log_alpha"][0])
    if tree is None:
        idx, w = T3.batch_indices(seed, u, size, B), None
    else:
        idx, w = PER.sample(tree, seed, u, B, size, per["beta"])
    x, x2 = buf["x"][idx], buf["x2"][idx]
    if vectors is not None:
        x, x2 = normalize(x, *vectors), normalize(x2, *vectors)
    r, done = buf["r"][idx], buf["done"][idx]
    if rew_scale is None:
        y, _ = S.target(sh, clamp, st["theta"], st["psi_target"], alpha, seed, u, x2, r, done, opts)
    else:
        y, _, _ = target(sh, clamp, st["theta"], st["psi_target"], alpha, seed, u, x2, r, done, opts, rew_scale, rew_clip)
    if tree is None:
        g, s6 = S.critic_grad(sh, st["psi"], x, buf["a"][idx], y)
    else:
        g, s6, d1, d2 = PER.critic_grad(sh, st["psi"], None, x, S.R.tanh32(np.asarray(buf["a"][idx], F)), y, w)
        PER._after_critics(tree, idx, d1, d2, per)
    st["psi"], st["m_psi"], st["v_psi"] = T3._step(st["psi"], st["m_psi"], st["v_psi"], g, u, opts["critic_lr"], opts)
    g, _, s4 = S.actor_grad(sh, clamp, st["theta"], st["psi"], alpha, seed, u, x, opts)
    st["theta"], st["m_theta"], st["v_theta"] = T3._step(st["theta"], st["m_theta"], st["v_theta"], g, u, opts["actor_lr"], opts)
    st["log_alpha"] = S.alpha_step(st["log_alpha"], s4[1], B, u, opts)
    if (u + 1) % opts["target_update_interval"] == 0:
        st["psi_target"] = T3.polyak(st["psi_target"], st["psi"], opts["tau"])
    st["updates"] = u + 1
    n = D64(B)
    stats = dict(critic_loss=s6[0] / n + s6[1] / n, q1_mean=s6[2] / n, q2_mean=s6[3] / n, y_mean=s6[4] / n, critic_grad_norm=np.sqrt(s6[5]),
                 actor_loss=s4[0] / n, logp_mean=s4[1] / n, actor_grad_norm=np.sqrt(s4[2]), alpha=D64(S.alpha_of(st["log_alpha"][0])),
                 log_alpha=D64(st["log_alpha"][0]), picked2=s4[3])
    return st, stats, dict(idx=np.asarray(idx), w=w, y=y)


# ---- the host twins -----------------------------------------------------------------------------------------------------------
def config(observations=True, rewards=True, per_member=False, obs_min_std=1e-2, obs_count_cap=0, rew_min_std=1e-2, rew_count_cap=0, rew_clip=10.0):
    from adcraft_amd import _ffi
    c = _ffi.SACNormConfig()
    c.struct_size = C.sizeof(_ffi.SACNormConfig)
    c.observations, c.rewards, c.per_member = int(observations), int(rewards), int(per_member)
    c.obs_min_std, c.obs_count_cap, c.rew_min_std, c.rew_count_cap, c.rew_clip = obs_min_std, obs_count_cap, rew_min_std, rew_count_cap, rew_clip
    return c


def twin_y(lib, r, done, q, alpha, lp, gamma, reward_scale, scale, clip, K=3):
    cfg = S.sac_config(K, **S.options(K, gamma=gamma, reward_scale=reward_scale))
    r, q, lp = (np.ascontiguousarray(a, dtype=F) for a in (r, q, lp))
    dn = np.ascontiguousarray(done, dtype=np.uint8)
    y = np.zeros(r.size, F)
    rc = lib.adc_sac_y_norm_host(C.byref(cfg), r.size, r.ctypes.data, dn.ctypes.data, q.ctypes.data, lp.ctypes.data, float(F(alpha)), float(F(scale)),
                                 float(F(clip)), y.ctypes.data)
    assert rc == 0, rc
    return y
