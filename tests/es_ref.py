"""The evolution strategy's law (adcraft_amd/csrc/adc_es.h) restated in numpy from the header's comments: counter-addressed
noise, antithetic members, fitness, shaping, the float64 gradient sum by pair, Adam / SGD one float32 rounding at a time.  The
host twins (adc_es_noise_host, adc_es_update_host) and the device kernels must give these very bits."""
import ctypes as C

import numpy as np

from tests.mlp_ref import _mix64

F = np.float32
ST_ES = 15


def es_key(seed):
    return _mix64(int(seed) ^ 0x3C6EF372FE94F82B)


def noise(seed, pair, generation, P, p0=0):
    """eps(pair, generation)[p0 : P]: normal_from_word of word p % 4 of Philox call (p / 4, stage 15, pair, generation)"""
    from oracle import capi as orc
    L = orc.lib()
    key = es_key(seed)
    out = np.zeros(P - p0, dtype=F)
    for q in range(p0 // 4, (P + 3) // 4):
        w = orc.philox([q, ST_ES, int(pair), int(generation)], [key & 0xFFFFFFFF, key >> 32])
        for h in range(4):
            p = 4 * q + h
            if p0 <= p < P:
                out[p - p0] = L.orc_normal_from_word(int(w[h]))
    return out


def noise_rows(seed, generation, pairs, P, p0=0):
    """[pairs, P - p0]: eps(i, generation)[p0 : P] of the pairs i in order - what members() and update() draw, for a caller that
    draws it once for both"""
    return np.stack([noise(seed, i, generation, P, p0) for i in range(pairs)])


def members(theta, seed, generation, M, sigma, rows=None):
    """[M, P]: member 2i = theta + sigma * eps(i), member 2i + 1 = theta + sigma * (-eps(i)); rows: noise_rows, if drawn already"""
    theta = np.asarray(theta, dtype=F)
    out = np.zeros((M, theta.size), dtype=F)
    for i in range(M // 2):
        e = noise(seed, i, generation, theta.size) if rows is None else rows[i]
        out[2 * i] = theta + F(sigma) * e
        out[2 * i + 1] = theta + F(sigma) * (-e)
    return out


def fitness(returns, member_of_env, M):
    """float64 mean of a member's envs' returns: summed envs ascending from +0, divided by their number"""
    f, n = np.zeros(M, np.float64), np.zeros(M, np.int64)
    for env, m in enumerate(member_of_env):
        f[m] = f[m] + np.float64(returns[env])
        n[m] += 1
    with np.errstate(all="ignore"):
        return f / n.astype(np.float64)


def shape(fit, shaping):
    fit = np.asarray(fit, dtype=np.float64)
    M = fit.size
    if shaping == "raw":
        return fit.copy()
    order = sorted(range(M), key=lambda m: (0, 0.0, m) if np.isnan(fit[m]) else (1, fit[m], m))
    u = np.zeros(M, np.float64)
    for r, m in enumerate(order):
        u[m] = np.float64(r) / np.float64(M - 1) - 0.5
    return u


def bias_correction(beta, t):
    p = np.float64(1.0)
    for _ in range(t):
        p = p * np.float64(F(beta))
    return F(np.float64(1.0) - p)


def update(theta, m, v, fit, seed, generation, sigma=0.02, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, l2=0.0, shaping="centered_rank",
           optimiser="adam", p0=0, rows=None):
    """one generation: returns (theta, m, v, g) - new arrays, float32.  A parameter's update reads nothing of another's, so a range
    of a longer flat vector is restated on its own: p0 > 0 says that theta, m and v are the entries [p0, p0 + theta.size) of one.
    rows: noise_rows of those entries, if drawn already"""
    theta, m, v = (np.array(a, dtype=F) for a in (theta, m, v))
    fit = np.asarray(fit, dtype=np.float64)
    M, P = fit.size, theta.size
    u = shape(fit, shaping)
    acc = np.zeros(P, np.float64)
    with np.errstate(all="ignore"):
        for i in range(M // 2):
            du = u[2 * i] - u[2 * i + 1]
            e = noise(seed, i, generation, p0 + P, p0) if rows is None else rows[i]
            acc = acc + du * e.astype(np.float64)
        g = (acc / (np.float64(M) * np.float64(F(sigma)))).astype(F)
        if l2 > 0:
            g = g - F(l2) * theta
        if optimiser == "sgd":
            return theta + F(lr) * g, m, v, g
        t = generation + 1
        b1, b2 = F(beta1), F(beta2)
        m = (b1 * m) + ((F(1) - b1) * g)
        v = (b2 * v) + ((F(1) - b2) * (g * g))
        c1, c2 = bias_correction(beta1, t), bias_correction(beta2, t)
        theta = theta + F(lr) * ((m / c1) / (np.sqrt(v / c2) + F(eps)))
    return theta.astype(F), m.astype(F), v.astype(F), g.astype(F)


def draw_fitness(rng, M, ties=False, nans=False, tie_in_pair=True):
    """[M] float64 as tests/test_es_host.py draws it: normals times 100; ties: two members tied with member 0 - member M - 1 and
    member 1, or (tie_in_pair off: under raw shaping a tie inside a pair is a pair without a term) member 2; nans: two NaNs (ranked
    lowest, by index)"""
    fit = rng.standard_normal(M) * 100
    if ties:
        fit[1 if tie_in_pair else 2] = fit[0]
        fit[M - 1] = fit[0]
    if nans:
        fit[M // 2] = np.nan
        fit[0 if M == 2 else 2] = np.nan
    return fit


def flat_params(policy):
    """the flat parameter order: the policy layers in order, each W input-major (j * n_out + h) followed by its b"""
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in policy.layers]).astype(F)


def es_config(seed=0, **kw):
    from adcraft_amd.engine import StepEngine
    return StepEngine.es_config(seed=seed, **kw)


def twin_noise(lib, seed, pair, generation, p0, n):
    out = np.zeros(n, dtype=F)
    assert lib.adc_es_noise_host(int(seed), int(pair), int(generation), int(p0), int(n), out.ctypes.data) == 0
    return out


def twin_update(lib, theta, m, v, fit, seed, generation, **kw):
    theta, m, v = (np.array(a, dtype=F) for a in (theta, m, v))
    fit = np.ascontiguousarray(fit, dtype=np.float64)
    g = np.zeros_like(theta)
    cfg = es_config(**kw)
    rc = lib.adc_es_update_host(C.byref(cfg), int(seed), int(fit.size), int(theta.size), fit.ctypes.data, int(generation),
                                theta.ctypes.data, m.ctypes.data, v.ctypes.data, g.ctypes.data)
    assert rc == 0, rc
    return theta, m, v, g
