"""The law of the TD3 learners' running normalisers (adcraft_amd/csrc/adc_td3_norm.h) restated in numpy, one rounded IEEE
operation per line as the header's comment block states them, for the bit-exact tests of the host twins adc_td3_norm_obs_host /
adc_td3_norm_rew_host / adc_td3_y_norm_host and of the device kernels.  The merge is tests/norm_ref.py's lines, the reward part
tests/rew_norm_ref.py's update under the TD3 discount, the TD3 update tests/td3_ref.py's with the batch normalised as it is
sampled.  Nothing here calls the library except the twin_* functions."""
import ctypes as C

import numpy as np

from tests import norm_ref as NR
from tests import rew_norm_ref as RR
from tests import td3_ref as T3
from tests.pg_ref import csum

F, D64 = np.float32, np.float64


# ---- the observation part: raw rows ---------------------------------------------------------------------------------------------
def obs_fresh(D, shift=None, scale=None):
    return NR.fresh(D, shift, scale)


def obs_update(state, x, min_std=1e-2, count_cap=0):
    """x [S, D] float32: the batch's RAW rows.  Returns the new state (the vectors in state are not read: no back-conversion)."""
    x = np.ascontiguousarray(x, dtype=F)
    S, fs = x.shape[0], D64(x.shape[0])
    x64 = x.astype(D64)
    with np.errstate(all="ignore"):
        sx = csum(x64)
        qx = csum(x64 * x64)                                  # (the product of two float32 values is exact in float64)
        mx = sx / fs
        qm, mm = qx / fs, mx * mx
        vx = qm - mm
        vx = np.where(vx > 0.0, vx, 0.0)
        M2b = vx * fs
        count = int(state["count"])
        if count == 0:
            mean, M2 = mx, M2b
        else:
            fc = D64(count)
            nt = fc + fs
            d = mx - state["mean"]
            w = fs / nt
            dw = d * w
            mean = state["mean"] + dw
            m2s, dd = state["M2"] + M2b, d * d
            cs = fc * fs
            k = cs / nt
            t = dd * k
            M2 = m2s + t
        count += S
        if count_cap > 0 and count > count_cap:
            f = D64(count_cap) / D64(count)
            M2 = M2 * f
            count = int(count_cap)
        var = M2 / D64(count)
        sd = np.sqrt(var)
        sd = np.where(sd < D64(min_std), D64(min_std), sd)
        shift = mean.astype(F)
        scale = (D64(1.0) / sd).astype(F)
    return dict(count=count, mean=np.asarray(mean, D64), M2=np.asarray(M2, D64), shift=shift, scale=scale)


def normalize(x, shift, scale):
    """(x - shift) * scale: a difference, a product"""
    with np.errstate(all="ignore"):
        return ((np.asarray(x, F) - np.asarray(shift, F)[None, :]).astype(F) * np.asarray(scale, F)[None, :]).astype(F)


# ---- the reward part: adc_rew_norm.h's law under the TD3 discount -----------------------------------------------------------------
rew_fresh = RR.fresh


def rew_update(state, reward, terminated, truncated, gamma, min_std=1e-2, count_cap=0):
    return RR.update(state, reward, terminated, truncated, gamma, min_std=min_std, count_cap=count_cap)


# ---- the target and the update under the normalisers -----------------------------------------------------------------------------
def y_norm(r, done, q, gamma, reward_scale, scale, clip):
    """td3_y_norm: rs = r * reward_scale; rs = rs * scale; the clip; y = rs + ((gamma * q) * nt)"""
    r, q, cl = np.asarray(r, F), np.asarray(q, F), F(clip)
    with np.errstate(all="ignore"):
        rs = r * F(reward_scale)
        rs = rs * F(scale)
        if cl > 0:
            rs = np.where(rs < -cl, -cl, rs)
            rs = np.where(rs > cl, cl, rs)
        nt = np.where(np.asarray(done, bool), F(0), F(1))
        y = rs.astype(F) + ((F(gamma) * q) * nt)
    return y.astype(F)


def y_plain(r, done, q, gamma, reward_scale):
    """adc_td3.h's td3_y (tests/td3_ref.py's last lines of target())"""
    r, q = np.asarray(r, F), np.asarray(q, F)
    with np.errstate(all="ignore"):
        nt = np.where(np.asarray(done, bool), F(0), F(1))
        return ((r * F(reward_scale)) + ((F(gamma) * q) * nt)).astype(F)


def target(sh, theta_t, psi_t, norm, seed, update, x2n, r, done, opts, scale, clip):
    """td3_ref.target with td3_y_norm in the place of td3_y; x2n: the rows already normalised"""
    x2n, r, B = np.ascontiguousarray(x2n, F), np.asarray(r, F), len(r)
    with np.errstate(all="ignore"):
        mu = T3.forward(x2n, sh.actor(theta_t), sh.act)[-1]
        c = F(opts["target_noise_clip"])
        e = F(opts["target_noise"]) * T3.noise(seed, update, B, sh.A)
        e = np.where(e < -c, -c, e)
        e = np.where(e > c, c, e).astype(F)
        a = (mu + e).astype(F)
        lo, hi = F(opts["action_lo"]), F(opts["action_hi"])
        if hi > lo:
            a = np.where(a < lo, lo, a)
            a = np.where(a > hi, hi, a).astype(F)
        row = np.concatenate([x2n, T3.action_norm(a, norm)], axis=1)
        q1, q2 = (T3.forward(row, net, sh.act)[-1][:, 0] for net in sh.critics(psi_t))
        q = np.where(q1 < q2, q1, q2)
    return y_norm(r, done, q, opts["gamma"], opts["reward_scale"], scale, clip), q


def update(policy, state, buf, norm, seed, opts, vectors=None, rew_scale=None, rew_clip=0.0):
    """one adc_engine_td3_update(1) under live normalisers on the RAW ring buf: vectors = (shift, scale) [D] in force (None: the
    ring holds network inputs), rew_scale the multiplier in force (None: td3_y).  Returns (new state, statistics, (rs, q) of the
    batch: the scaled rewards before the clip and the target critics' minimum)."""
    sh, st, u = T3.Shapes(policy, opts), dict(state), state["updates"]
    B, size = opts["batch_size"], len(buf["r"])
    idx = T3.batch_indices(seed, u, size, B)
    x, x2, a = buf["x"][idx], buf["x2"][idx], buf["a"][idx]
    if vectors is not None:
        x, x2 = normalize(x, *vectors), normalize(x2, *vectors)
    r, done = buf["r"][idx], buf["done"][idx]
    if rew_scale is None:
        y, q = target(sh, st["theta_target"], st["psi_target"], norm, seed, u, x2, r, done, opts, F(1.0), 0.0)
        rs = (np.asarray(r, F) * F(opts["reward_scale"])).astype(F)
    else:
        y, q = target(sh, st["theta_target"], st["psi_target"], norm, seed, u, x2, r, done, opts, rew_scale, rew_clip)
        rs = ((np.asarray(r, F) * F(opts["reward_scale"])).astype(F) * F(rew_scale)).astype(F)
    g, s6 = T3.critic_grad(sh, st["psi"], norm, x, a, y)
    st["psi"], st["m_psi"], st["v_psi"] = T3._step(st["psi"], st["m_psi"], st["v_psi"], g, u, opts["critic_lr"], opts)
    n = D64(B)
    stats = dict(critic_loss=s6[0] / n + s6[1] / n, q1_mean=s6[2] / n, q2_mean=s6[3] / n, y_mean=s6[4] / n, critic_grad_norm=np.sqrt(s6[5]),
                 actor_loss=-D64(0.0), actor_grad_norm=D64(0.0))
    if (u + 1) % opts["policy_delay"] == 0:
        g, s2 = T3.actor_grad(sh, st["theta"], st["psi"], norm, x)
        st["theta"], st["m_theta"], st["v_theta"] = T3._step(st["theta"], st["m_theta"], st["v_theta"], g, st["actor_steps"], opts["actor_lr"], opts)
        st["theta_target"] = T3.polyak(st["theta_target"], st["theta"], opts["tau"])
        st["psi_target"] = T3.polyak(st["psi_target"], st["psi"], opts["tau"])
        st["actor_steps"] += 1
        stats.update(actor_loss=-(s2[0] / n), actor_grad_norm=np.sqrt(s2[1]))
    st["updates"] = u + 1
    return st, stats, (rs, q)


# ---- the host twins -----------------------------------------------------------------------------------------------------------
def config(observations=True, rewards=True, per_member=False, obs_min_std=1e-2, obs_count_cap=0, rew_min_std=1e-2, rew_count_cap=0, rew_clip=10.0):
    from adcraft_amd import _ffi
    c = _ffi.TD3NormConfig()
    c.struct_size = C.sizeof(_ffi.TD3NormConfig)
    c.observations, c.rewards, c.per_member = int(observations), int(rewards), int(per_member)
    c.obs_min_std, c.obs_count_cap, c.rew_min_std, c.rew_count_cap, c.rew_clip = obs_min_std, obs_count_cap, rew_min_std, rew_count_cap, rew_clip
    return c


def twin_obs(lib, state, x, min_std=1e-2, count_cap=0):
    """adc_td3_norm_obs_host on a copy of state"""
    x = np.ascontiguousarray(x, dtype=F)
    cfg = config(obs_min_std=min_std, obs_count_cap=count_cap)
    cnt = C.c_int64(int(state["count"]))
    mean, M2 = np.array(state["mean"], D64), np.array(state["M2"], D64)
    shift, scale = np.array(state["shift"], F), np.array(state["scale"], F)
    rc = lib.adc_td3_norm_obs_host(C.byref(cfg), x.shape[0], x.shape[1], x.ctypes.data, C.byref(cnt), mean.ctypes.data, M2.ctypes.data,
                                   shift.ctypes.data, scale.ctypes.data)
    assert rc == 0, rc
    return dict(count=cnt.value, mean=mean, M2=M2, shift=shift, scale=scale)


def twin_rew(lib, state, reward, terminated, truncated, gamma, min_std=1e-2, count_cap=0):
    """adc_td3_norm_rew_host on a copy of state"""
    reward = np.ascontiguousarray(reward, dtype=F)
    te, tr = (np.ascontiguousarray(a, dtype=np.uint8) for a in (terminated, truncated))
    T, n = reward.shape
    gm = np.ascontiguousarray(np.broadcast_to(np.asarray(gamma, F), (n,)))
    cfg = config(rew_min_std=min_std, rew_count_cap=count_cap)
    cnt, mean, m2, sc = C.c_int64(int(state["count"])), C.c_double(float(state["mean"])), C.c_double(float(state["M2"])), C.c_float(float(state["scale"]))
    carry = np.array(state["returns"], D64)
    rc = lib.adc_td3_norm_rew_host(C.byref(cfg), T, n, gm.ctypes.data, reward.ctypes.data, te.ctypes.data, tr.ctypes.data, C.byref(cnt), C.byref(mean),
                                   C.byref(m2), C.byref(sc), carry.ctypes.data)
    assert rc == 0, rc
    return dict(count=cnt.value, mean=D64(mean.value), M2=D64(m2.value), scale=F(sc.value), returns=carry)


def twin_y(lib, r, done, q, gamma, reward_scale, scale, clip):
    cfg = T3.td3_config(**T3.options(gamma=gamma, reward_scale=reward_scale))
    r, q = np.ascontiguousarray(r, dtype=F), np.ascontiguousarray(q, dtype=F)
    dn = np.ascontiguousarray(done, dtype=np.uint8)
    y = np.zeros(r.size, F)
    rc = lib.adc_td3_y_norm_host(C.byref(cfg), r.size, r.ctypes.data, dn.ctypes.data, q.ctypes.data, float(F(scale)), float(F(clip)), y.ctypes.data)
    assert rc == 0, rc
    return y


obs_same = NR.same
rew_same = RR.same


def split(state):
    """StepEngine.td3_norm_state's dict (plus `returns`) as (observation state, reward state) in this module's keys"""
    o = dict(count=state["obs_count"], mean=state["obs_mean"], M2=state["obs_M2"], shift=state["shift"], scale=state["scale"]) if "obs_count" in state else None
    r = dict(count=state["rew_count"], mean=state["rew_mean"], M2=state["rew_M2"], scale=state["rew_scale"], returns=state.get("returns")) if "rew_count" in state else None
    return o, r
