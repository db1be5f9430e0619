"""numpy restatement of n-step returns for the TD3 / SAC learners, from the comment "n-step" of csrc/adc_td3.h: the window of one
sample in float32 scalars, operation by operation; the ring's store under a window; the targets with a per-element bootstrap
discount gn (td3_ref / sac_ref / td3_norm_ref / sac_norm_ref's own target code, handed gn where it reads gamma); the updates; and
the ctypes front ends of the host twins adc_replay_nstep_host / adc_td3_y_nstep_host / adc_sac_y_nstep_host."""
import ctypes as C

import numpy as np

from tests import per_ref as PR
from tests import sac_norm_ref as SN
from tests import sac_ref as S
from tests import td3_norm_ref as TN
from tests import td3_ref as T3

F = np.float32
N_MAX = 16


# ---- the law ------------------------------------------------------------------------------------------------------------------------
def window_of(reward, done, t, e, t1, n, gamma):
    """the sample of recorded day t and env e of a store that ends at day t1: (R, g, d, m).
    R = r[t]; g = gamma; m = 1; d = done[t]; while m < n and not d and t + m < t1: p = g * r[t + m]; R = R + p; g = g * gamma;
    d = done[t + m]; m = m + 1"""
    gamma = F(gamma)
    R, g, m, d = F(reward[t, e]), gamma, 1, bool(done[t, e])
    with np.errstate(all="ignore"):
        while m < n and not d and t + m < t1:
            p = F(g * F(reward[t + m, e]))
            R = F(R + p)
            g = F(g * gamma)
            d = bool(done[t + m, e])
            m = m + 1
    return R, g, d, m


def windows(n, gamma, reward, terminated, truncated, t0=0, t1=None):
    """every sample s = (t - t0) * N + e of the days [t0, t1) of a record [T, N]: dict of R [S] float32, done [S] bool, gn [S]
    float32, m [S] int32"""
    reward = np.asarray(reward, F)
    done = np.asarray(terminated, bool) | np.asarray(truncated, bool)
    T, N = reward.shape
    t1 = T if t1 is None else t1
    S_ = (t1 - t0) * N
    out = dict(R=np.zeros(S_, F), done=np.zeros(S_, bool), gn=np.zeros(S_, F), m=np.zeros(S_, np.int32))
    for t in range(t0, t1):
        for e in range(N):
            s = (t - t0) * N + e
            out["R"][s], out["gn"][s], out["done"][s], out["m"][s] = window_of(reward, done, t, e, t1, n, gamma)
    return out


class Ring(T3.Ring):
    """td3_ref.Ring with n-step windows: store() appends a record's days [t0, T) as adc_engine_td3_store does after
    adc_engine_replay_nstep_init(n); gn [C] rides along.  A sample with s + C < count is not written (a later sample of the same
    store lands on its slot)"""

    def __init__(self, capacity, D, A, n, gamma):
        super().__init__(capacity, D, A)
        self.n, self.gamma = int(n), F(gamma)
        self.gn = np.zeros(self.C, F)

    def store(self, rec, current_input, t0=0):
        T, N = rec["reward"].shape
        w = windows(self.n, self.gamma, rec["reward"], rec["terminated"], rec["truncated"], t0, T)
        count = (T - t0) * N
        for t in range(t0, T):
            for e in range(N):
                s = (t - t0) * N + e
                if s + self.C < count:
                    continue
                slot, m = (self.written + s) % self.C, int(w["m"][s])
                self.x[slot], self.a[slot] = rec["obs"][t, e], rec["action"][t, e]
                self.r[slot], self.done[slot], self.gn[slot] = w["R"][s], w["done"][s], w["gn"][s]
                self.x2[slot] = rec["obs"][t + m, e] if t + m < T else current_input[e]
        self.written += count

    def buffer(self):
        return dict(super().buffer(), gn=self.gn[:self.size])


# ---- the targets: the refs' own code with gn[element] where it reads gamma (they multiply F(gamma) * q elementwise) ---------------
def _opts(opts, gn_b):
    return dict(opts, gamma=np.asarray(gn_b, F))


def td3_y(r, done, q, gn_b, reward_scale, scale=None, clip=0.0):
    """td3_y with gn (scale None), or td3_y_norm with gn"""
    if scale is None:
        return TN.y_plain(r, done, q, np.asarray(gn_b, F), reward_scale)
    return TN.y_norm(r, done, q, np.asarray(gn_b, F), reward_scale, scale, clip)


def sac_y(r, done, q, alpha, lp, gn_b, reward_scale, scale=None, clip=0.0):
    if scale is None:
        return SN.y_plain(r, done, q, alpha, lp, np.asarray(gn_b, F), reward_scale)
    return SN.y_norm(r, done, q, alpha, lp, np.asarray(gn_b, F), reward_scale, scale, clip)


def td3_target(sh, theta_t, psi_t, norm, seed, update, x2, r, done, gn_b, opts):
    return T3.target(sh, theta_t, psi_t, norm, seed, update, x2, r, done, _opts(opts, gn_b))


def sac_target(sh, clamp, theta, psi_t, alpha, seed, update, x2, r, done, gn_b, opts):
    return S.target(sh, clamp, theta, psi_t, alpha, seed, update, x2, r, done, _opts(opts, gn_b))


# ---- the updates: buf carries gn [size]; the batch's slots are the law's, so the elements' gn are known before the ref's update runs ----
def td3_update(policy, state, buf, norm, seed, opts, rew_scale=None, rew_clip=0.0, tree=None, per=None):
    """one adc_engine_td3_update(1) under n-step returns: td3_ref.update (rew_scale: td3_norm_ref.update's multiplier and clip on a
    ring of network inputs; tree, per: per_ref.td3_update's prioritised batch) with the sampled slots' gn in gamma's place"""
    u, B, size = state["updates"], opts["batch_size"], len(buf["r"])
    idx = PR.sample(tree, seed, u, B, size, per["beta"])[0] if tree is not None else T3.batch_indices(seed, u, size, B)
    o = _opts(opts, np.asarray(buf["gn"], F)[idx])
    if tree is not None:
        return PR.td3_update(policy, state, buf, norm, seed, o, tree, per)
    if rew_scale is not None:
        return TN.update(policy, state, buf, norm, seed, o, None, rew_scale, rew_clip)[:2]
    return T3.update(policy, state, buf, norm, seed, o)


def sac_update(policy, state, buf, seed, opts):
    u, B, size = state["updates"], opts["batch_size"], len(buf["r"])
    idx = T3.batch_indices(seed, u, size, B)
    return S.update(policy, state, buf, seed, _opts(opts, np.asarray(buf["gn"], F)[idx]))


# ---- the host twins -----------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def twin_windows(lib, n, gamma, reward, terminated, truncated, t0=0, t1=None):
    from adcraft_amd import _ffi
    reward = np.ascontiguousarray(reward, F)
    term, trunc = np.ascontiguousarray(terminated, np.uint8), np.ascontiguousarray(truncated, np.uint8)
    T, N = reward.shape
    t1 = T if t1 is None else t1
    S_ = max((t1 - t0) * N, 0)
    R, done, gn, m = np.zeros(S_, F), np.zeros(S_, np.uint8), np.zeros(S_, F), np.zeros(S_, np.int32)
    rc = lib.adc_replay_nstep_host(int(n), float(F(gamma)), T, N, int(t0), int(t1), _ptr(reward), _ptr(term), _ptr(trunc), _ptr(R), _ptr(done), _ptr(gn), _ptr(m))
    if rc != _ffi.ADC_OK:
        return rc
    return dict(R=R, done=done.astype(bool), gn=gn, m=m)


def twin_td3_y(lib, r, done, q, gn_b, gamma, reward_scale, scale=1.0, clip=0.0):
    from adcraft_amd import _ffi
    cfg = T3.td3_config(**T3.options(gamma=gamma, reward_scale=reward_scale))
    r, q, gn_b, d = np.ascontiguousarray(r, F), np.ascontiguousarray(q, F), np.ascontiguousarray(gn_b, F), np.ascontiguousarray(done, np.uint8)
    y = np.zeros(len(r), F)
    assert lib.adc_td3_y_nstep_host(C.byref(cfg), len(r), _ptr(r), _ptr(d), _ptr(q), _ptr(gn_b), float(F(scale)), float(F(clip)), _ptr(y)) == _ffi.ADC_OK
    return y


def twin_sac_y(lib, r, done, q, alpha, lp, gn_b, gamma, reward_scale, scale=1.0, clip=0.0, K=3):
    from adcraft_amd import _ffi
    cfg = S.sac_config(K, **S.options(K, gamma=gamma, reward_scale=reward_scale))
    r, q, lp, gn_b = (np.ascontiguousarray(v, F) for v in (r, q, lp, gn_b))
    d = np.ascontiguousarray(done, np.uint8)
    y = np.zeros(len(r), F)
    assert lib.adc_sac_y_nstep_host(C.byref(cfg), len(r), _ptr(r), _ptr(d), _ptr(q), _ptr(lp), _ptr(gn_b), float(F(alpha)), float(F(scale)), float(F(clip)),
                                    _ptr(y)) == _ffi.ADC_OK
    return y
