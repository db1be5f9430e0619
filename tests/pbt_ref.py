"""The population-based training scheduler's law (adcraft_amd/csrc/adc_pbt.h) restated in numpy from the header's comments: the
fitness chains over the record, the smoothing, the ranking, the donor draw and the explored hyperparameters.  The host twins
(adc_pbt_fitness_host, adc_pbt_plan_host, adc_pbt_explore_host), the device's fitness kernel and adc_engine_pbt_step must give
these very bits."""
import ctypes as C

import numpy as np

from tests.mlp_ref import _mix64

F = np.float32
ST_PBT = 18
PG, TD3 = 0, 1
PG_IDS = ("lr", "ent_coef", "eps_clip", "vf_coef")
TD3_IDS = ("actor_lr", "critic_lr", "target_noise", "tau", "sigma")
SIGMA = 4


def pbt_key(seed):
    return _mix64(int(seed) ^ 0xBB67AE8584CAA73B)


def fitness(reward_tn, M):
    """[M] float64: an env's return chains over the days ascending from +0; a member's fitness chains over its envs ascending
    from +0 and is divided by their number"""
    r = np.asarray(reward_tn, dtype=F)
    T, N = r.shape
    n = N // M
    out = np.zeros(M, np.float64)
    with np.errstate(all="ignore"):
        for m in range(M):
            acc = np.float64(0.0)
            for env in range(m * n, (m + 1) * n):
                ret = np.float64(0.0)
                for t in range(T):
                    ret = ret + np.float64(r[t, env])
                acc = acc + ret
            out[m] = acc / np.float64(n)
    return out


def smooth(ema, s, f, first):
    f = np.asarray(f, dtype=np.float64)
    if first or F(ema) == 0:
        return f.copy()
    e = np.float64(F(ema))
    with np.errstate(all="ignore"):
        return (e * np.asarray(s, np.float64)) + ((np.float64(1.0) - e) * f)


def order(s):
    """the members by rank: ascending by (s, index), NaNs first by index"""
    s = np.asarray(s, dtype=np.float64)
    return sorted(range(s.size), key=lambda m: (0, 0.0, m) if np.isnan(s[m]) else (1, s[m], m))


def draw(seed, member, round_):
    from oracle import capi as orc
    key = pbt_key(seed)
    return orc.philox([int(member), ST_PBT, 0, int(round_)], [key & 0xFFFFFFFF, key >> 32])


def plan(seed, round_, q, s):
    """rank [M], src [M] (-1: kept), bits [M] (the replaced member's w.y) from the smoothed fitness"""
    M = len(s)
    o = order(s)
    rank, src, bits = np.zeros(M, np.int32), np.full(M, -1, np.int32), np.zeros(M, np.uint32)
    for r, m in enumerate(o):
        rank[m] = r
    for r in range(q):
        d = o[r]
        w = draw(seed, d, round_)
        src[d] = o[M - q + ((int(w[0]) * q) >> 32)]
        bits[d] = w[1]
    return rank, src, bits


def clamp(v, lo, hi):
    v = F(lo) if v < F(lo) else v
    return F(hi) if v > F(hi) else v


def explore(cfg, kind, bits, donor, own):
    """[8] float32: the replaced member's values by id from its donor's and its own (TD3's id 4: one log_std component)"""
    out = np.array(own, dtype=F)
    with np.errstate(all="ignore"):
        for h in range(8):
            if not (int(cfg["tuned_mask"]) >> h) & 1:
                continue
            up = (int(bits) >> h) & 1
            if kind == TD3 and h == SIGMA:
                v = F(donor[h]) + F(cfg["log_factor_hi"] if up else cfg["log_factor_lo"])
            else:
                v = F(donor[h]) * F(cfg["factor_hi"] if up else cfg["factor_lo"])
            out[h] = clamp(F(v), cfg["lo"][h], cfg["hi"][h])
    return out


def round_(cfg, kind, seed, state, fit, hp):
    """one round on (state = dict(round, smoothed [M]), fit [M], hp [M, 8] the members' values by id - TD3's id 4 ignored).
    Returns (new state, result dict as StepEngine.pbt_step's; hp's id 4 of TD3: the log shift of a replaced member, 0 else)"""
    M = len(fit)
    s = smooth(cfg["fitness_ema"], state["smoothed"], fit, state["round"] == 0)
    rank, src, bits = plan(seed, state["round"], cfg["replace_count"], s)
    hp_new = np.array(hp, dtype=F)
    if kind == TD3:
        hp_new[:, SIGMA] = 0
    s_new = s.copy()
    for m in range(M):
        if src[m] < 0:
            continue
        mask = dict(cfg, tuned_mask=int(cfg["tuned_mask"]) & ~(1 << SIGMA)) if kind == TD3 else cfg
        hp_new[m] = explore(mask, kind, bits[m], hp[src[m]], hp[m])
        if kind == TD3:
            tuned = (int(cfg["tuned_mask"]) >> SIGMA) & 1
            hp_new[m, SIGMA] = F(0) if not tuned else F(cfg["log_factor_hi"] if (int(bits[m]) >> SIGMA) & 1 else cfg["log_factor_lo"])
        s_new[m] = s[src[m]]
    return (dict(round=state["round"] + 1, smoothed=s_new),
            dict(fitness=np.asarray(fit, np.float64).copy(), smoothed=s_new, rank=rank, src=src, hp=hp_new, bits=bits))


def log_std_after(cfg, bits, donor_log_std):
    """a replaced member's log_std from its donor's (sigma tuned)"""
    up = (int(bits) >> SIGMA) & 1
    lf = F(cfg["log_factor_hi"] if up else cfg["log_factor_lo"])
    return np.array([clamp(F(F(x) + lf), cfg["lo"][SIGMA], cfg["hi"][SIGMA]) for x in donor_log_std], dtype=F)


def config_dict(c):
    """a ctypes PBTConfig as the dict the functions above take"""
    return dict(replace_count=int(c.replace_count), fitness_ema=F(c.fitness_ema), factor_lo=F(c.factor_lo), factor_hi=F(c.factor_hi),
                log_factor_lo=F(c.log_factor_lo), log_factor_hi=F(c.log_factor_hi), tuned_mask=int(c.tuned_mask),
                lo=np.array(list(c.lo), F), hi=np.array(list(c.hi), F), with_ring=int(c.with_ring), seed=int(c.seed))


def twin_fitness(lib, reward_tn, M):
    r = np.ascontiguousarray(reward_tn, dtype=F)
    out = np.zeros(M, np.float64)
    assert lib.adc_pbt_fitness_host(r.shape[0], r.shape[1], M, r.ctypes.data, out.ctypes.data) == 0
    return out


def twin_plan(lib, c, seed, round_no, fit, s_prev):
    fit = np.ascontiguousarray(fit, dtype=np.float64)
    M = fit.size
    s = np.array(s_prev, dtype=np.float64)
    rank, src, bits = np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros(M, np.uint32)
    rc = lib.adc_pbt_plan_host(C.byref(c), int(seed), M, int(round_no), fit.ctypes.data, s.ctypes.data, rank.ctypes.data, src.ctypes.data, bits.ctypes.data)
    assert rc == 0, rc
    return s, rank, src, bits


def twin_explore(lib, c, kind, bits, donor, own):
    donor, own = np.ascontiguousarray(donor, dtype=F), np.ascontiguousarray(own, dtype=F)
    out = np.zeros(8, F)
    assert lib.adc_pbt_explore_host(C.byref(c), int(kind), int(bits), donor.ctypes.data, own.ctypes.data, out.ctypes.data) == 0
    return out
