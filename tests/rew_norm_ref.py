"""The law of the running reward normaliser (adcraft_amd/csrc/adc_rew_norm.h) restated in numpy, one rounded IEEE operation
per line as the header's comment block states them, for the bit-exact tests of the host twins adc_rew_norm_host /
adc_pg_gae_norm_host and of the device kernels.  The merge is tests/norm_ref.py's lines (the header shares adc_norm.h's code),
the GAE tail tests/pg_ref.py's.  Nothing here calls the library except twin() and twin_gae()."""
import ctypes as C

import numpy as np

from tests import pg_ref as P
from tests.pg_ref import csum

F, D64 = np.float32, np.float64


def fresh(N):
    """an empty normaliser and its N envs' carry"""
    return dict(count=0, mean=D64(0.0), M2=D64(0.0), scale=F(1.0), returns=np.zeros(N, D64))


def scan(reward, done, gamma, carry):
    """reward [T, n] float32, done [T, n] bool, gamma scalar or [n] float32, carry [n] float64 -> (g [T, n] float64, new carry)"""
    reward = np.asarray(reward, F)
    T, n = reward.shape
    gm = np.broadcast_to(np.asarray(gamma, F), (n,)).astype(D64)
    G = np.array(carry, D64)
    g = np.zeros((T, n), D64)
    with np.errstate(all="ignore"):
        for t in range(T):
            G = gm * G
            G = G + reward[t].astype(D64)
            g[t] = G
            G = np.where(done[t], D64(0.0), G)
    return g, G


def update(state, reward, terminated, truncated, gamma, min_std=1e-2, count_cap=0, **_):
    """one update of one normaliser over its envs' days [T, n] not yet consumed.  Returns the new state."""
    done = np.asarray(terminated, bool) | np.asarray(truncated, bool)
    g, carry = scan(reward, done, gamma, state["returns"])
    g = g.reshape(-1)                                           # (sample s = (t - t0) * n + local env)
    S, fs = g.size, D64(g.size)
    with np.errstate(all="ignore"):
        sx = csum(g)
        qx = csum(g * g)                                        # (the square rounded, then added)
        mb = sx / fs
        qm, mm = qx / fs, mb * mb
        vb = qm - mm
        vb = vb if vb > 0.0 else D64(0.0)
        M2b = vb * fs
        count = int(state["count"])
        if count == 0:
            mean, M2 = mb, M2b
        else:
            fc = D64(count)
            nt = fc + fs
            d = mb - state["mean"]
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
        sd = D64(min_std) if sd < D64(min_std) else sd
        scale = F(D64(1.0) / sd)
    return dict(count=count, mean=D64(mean), M2=D64(M2), scale=scale, returns=carry)


def gae(reward, terminated, truncated, value, bootstrap, scale, clip, gamma=0.99, lam=0.95, reward_scale=1.0, normalize_advantages=True, **_):
    """adv, ret [T, N] float32 under the multiplier scale (scalar or [N]) and clip; the tail is pg_ref.gae's lines"""
    reward, value = np.asarray(reward, F), np.asarray(value, F)
    T, N = reward.shape
    done = np.asarray(terminated, bool) | np.asarray(truncated, bool)
    sc = np.broadcast_to(np.asarray(scale, F), (N,))
    g, gl, cl = F(gamma), F(gamma) * F(lam), F(clip)
    adv, ret = np.zeros((T, N), F), np.zeros((T, N), F)
    a_next, nxt = np.zeros(N, F), np.asarray(bootstrap, F)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            r = reward[t] * F(reward_scale)
            r = r * sc
            if cl > 0:
                r = np.where(r < -cl, -cl, r)
                r = np.where(r > cl, cl, r)
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


def pg_update(policy, state, rec, bootstrap, scale, clip, epochs, opts):
    """adc_engine_pg_update under a live normaliser: gae() above once, then pg_ref's minibatches as pg_ref.update runs them"""
    adv, ret = gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], bootstrap, scale, clip, **opts)
    N = rec["reward"].shape[1]
    mb = opts["minibatch_envs"] or N
    for _ in range(epochs):
        for n0 in range(0, N, mb):
            state, _st = P.minibatch(policy, state, rec, adv, ret, n0, mb, opts)
    return state


# ---- the host twins -----------------------------------------------------------------------------------------------------------
def config(min_std=1e-2, clip=10.0, count_cap=0, per_member=False):
    from adcraft_amd import _ffi
    c = _ffi.RewNormConfig()
    c.struct_size = C.sizeof(_ffi.RewNormConfig)
    c.per_member, c.min_std, c.clip, c.count_cap = int(per_member), min_std, clip, count_cap
    return c


def twin(lib, state, reward, terminated, truncated, gamma, min_std=1e-2, count_cap=0, **_):
    """adc_rew_norm_host on a copy of state"""
    reward = np.ascontiguousarray(reward, dtype=F)
    te, tr = (np.ascontiguousarray(a, dtype=np.uint8) for a in (terminated, truncated))
    T, n = reward.shape
    gm = np.ascontiguousarray(np.broadcast_to(np.asarray(gamma, F), (n,)))
    cfg = config(min_std, 0.0, count_cap)
    cnt, mean, m2, sc = C.c_int64(int(state["count"])), C.c_double(float(state["mean"])), C.c_double(float(state["M2"])), C.c_float(float(state["scale"]))
    carry = np.array(state["returns"], D64)
    rc = lib.adc_rew_norm_host(C.byref(cfg), T, n, gm.ctypes.data, reward.ctypes.data, te.ctypes.data, tr.ctypes.data, C.byref(cnt), C.byref(mean),
                               C.byref(m2), C.byref(sc), carry.ctypes.data)
    assert rc == 0, rc
    return dict(count=cnt.value, mean=D64(mean.value), M2=D64(m2.value), scale=F(sc.value), returns=carry)


def twin_gae(lib, reward, terminated, truncated, value, bootstrap, scale, clip, **kw):
    cfg = P.pg_config(**kw)
    reward, value, bootstrap = (np.ascontiguousarray(a, dtype=F) for a in (reward, value, bootstrap))
    te, tr = (np.ascontiguousarray(a, dtype=np.uint8) for a in (terminated, truncated))
    T, N = reward.shape
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, F), (N,)))
    adv, ret = np.zeros((T, N), F), np.zeros((T, N), F)
    rc = lib.adc_pg_gae_norm_host(C.byref(cfg), T, N, reward.ctypes.data, te.ctypes.data, tr.ctypes.data, value.ctypes.data, bootstrap.ctypes.data,
                                  sc.ctypes.data, clip, adv.ctypes.data, ret.ctypes.data)
    assert rc == 0, rc
    return adv, ret


def _bits(x, t):
    return np.ascontiguousarray(x, dtype=t).reshape(-1).view(np.uint8)


def same(a, b, returns=True):
    """two states, bit for bit (returns=False: the moments and the multiplier alone)"""
    if int(a["count"]) != int(b["count"]):
        return False
    keys = (("mean", D64), ("M2", D64), ("scale", F)) + ((("returns", D64),) if returns else ())
    for k, t in keys:
        x, y = _bits(a[k], t), _bits(b[k], t)
        if x.shape != y.shape or not np.array_equal(x, y):
            return False
    return True


def member_days(rec, m, n, t0=0, t1=None):
    """(reward, terminated, truncated) [t1 - t0, n] of member m's envs"""
    return tuple(np.ascontiguousarray(rec[k][t0:t1, m * n:(m + 1) * n]) for k in ("reward", "terminated", "truncated"))
