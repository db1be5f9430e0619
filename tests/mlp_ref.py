"""The MLP policy's law (adcraft_amd/csrc/adc_mlp.h) restated in numpy from the header's comments: float32 operations one
rounding at a time, the float64 exp / tanh by the header's formula, heads, normals, log-probability, cent bids.  The host twin
(adc_mlp_act_host) and the device kernel must give these very bits.  `policy` is an adcraft_amd.baselines.mlp_policy.MLPPolicy
(used as a container of arrays and options only)."""
import ctypes as C
import math

import numpy as np

F = np.float32
ST_MLP = 14
HALF_LOG_2PI = F(0.918938517570495605)


def sum8(terms):
    """sum over axis 0: eight chains (index mod 8, ascending, from +0), joined ((0+1)+(2+3))+((4+5)+(6+7))"""
    terms = np.asarray(terms, dtype=F)
    s = np.zeros((8,) + terms.shape[1:], dtype=F)
    n = terms.shape[0]
    for i in range(0, n, 8):
        m = min(8, n - i)
        s[:m] = s[:m] + terms[i:i + m]
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))


_C = [1.0 / math.factorial(k) for k in range(15)]


def expm1_poly(r):
    r = np.asarray(r, dtype=np.float64)
    q = np.full(r.shape, _C[14])
    for k in range(13, 1, -1):
        q = q * r + _C[k]
    return r + (r * r) * q


def exp64(x):
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(x * 1.4426950408889634)
    r = (x - n * 0.693145751953125) - n * 1.4286068203094173e-06
    return (1.0 + expm1_poly(r)) * np.ldexp(1.0, n.astype(np.int64))


def tanh32(x):
    x = np.asarray(x, dtype=F)
    nan = np.isnan(x)
    a = np.abs(np.where(nan, F(0), x).astype(np.float64))
    a2 = a + a
    small = a2 < 0.34
    m = expm1_poly(np.where(small, a2, 0.0))
    e = exp64(np.where(small | (a >= 10.0), 1.0, a2))
    with np.errstate(all="ignore"):
        t = np.where(a >= 10.0, 1.0, np.where(small, m / (m + 2.0), 1.0 - 2.0 / (e + 1.0)))
    out = np.copysign(t.astype(F), x)
    return np.where(nan, x, out).astype(F)


def exp32(x):
    x = np.asarray(x, dtype=F)
    nan = np.isnan(x)
    c = np.minimum(np.maximum(np.where(nan, F(0), x), F(-87)), F(88))
    return np.where(nan, x, exp64(c.astype(np.float64)).astype(F)).astype(F)


def layer(x, w, b, act):
    """x [B, n_in], w [n_in, n_out], b [n_out]; act: 'tanh', 'relu' or None"""
    with np.errstate(all="ignore"):
        y = sum8(w[:, None, :] * x.T[:, :, None]) + b[None, :]
    if act == "tanh":
        return tanh32(y)
    if act == "relu":
        return np.where(y > 0, y, F(0)).astype(F)
    return y


def network(x, layers, activation):
    for i, (w, b) in enumerate(layers):
        x = layer(x, w, b, activation if i + 1 < len(layers) else None)
    return x


def normals(keys, ticks, A):
    """z [N, A]: normal_from_word of word a % 4 of Philox call (a / 4, stage 14, 0, tick) under each agent key"""
    from oracle import capi as orc
    L = orc.lib()
    z = np.zeros((len(keys), A), dtype=F)
    for n, (key, tick) in enumerate(zip(keys, ticks)):
        key = int(key)
        for q in range((A + 3) // 4):
            w = orc.philox([q, ST_MLP, 0, int(tick)], [key & 0xFFFFFFFF, key >> 32])
            for h in range(4):
                if 4 * q + h < A:
                    z[n, 4 * q + h] = L.orc_normal_from_word(int(w[h]))
    return z


def _mix64(x):
    x = (int(x) + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def agent_key(seed):
    return _mix64(int(seed) ^ 0x1F83D9ABFB41BD6B)


def default_agent_key(engine_seed, global_env_id):
    """without per-env seeds: from the engine's seed and env_id_base + env"""
    return _mix64(int(engine_seed) ^ _mix64(int(global_env_id) + 0x5BE0CD19137E2179))


def cent_bids(v, clip=None):
    v = np.asarray(v, dtype=F)
    with np.errstate(invalid="ignore"):
        v = np.where(v > F(0.01), v, F(0.01)).astype(F)
        if clip:
            v = np.where(v < F(clip), v, F(clip)).astype(F)
        c = np.rint(v.astype(np.float64) * 100.0)
    c = np.where(c >= 1.0, c, 1.0)
    c = np.where(c < 1.0e9, c, 1.0e9)
    return (c / 100.0).astype(F)


def act(policy, obs, z=None, deterministic=None, budget_override=0.0):
    """obs [B, D] float32 (rows of zeros on a first day); z [B, A] normals (ignored when deterministic).  Returns dict of mean,
    log_std, action [B, A], logp, value [B], bids [B, K], budget [B]."""
    det = policy.deterministic if deterministic is None else deterministic
    x = np.ascontiguousarray(obs, dtype=F)
    if policy.shift is not None:
        with np.errstate(all="ignore"):
            x = ((x - policy.shift[None, :]) * policy.scale[None, :]).astype(F)
    A = policy.num_keywords + 1
    out = network(x, policy.layers, policy.activation)
    value = network(x, policy.value_layers, policy.activation)[:, 0] if policy.value_layers else np.zeros(len(x), F)
    mean = out[:, :A]
    ls = out[:, A:] if out.shape[1] == 2 * A else np.broadcast_to(policy.log_std, mean.shape).astype(F)
    if policy.log_std_clamp is not None:
        lo, hi = F(policy.log_std_clamp[0]), F(policy.log_std_clamp[1])
        with np.errstate(invalid="ignore"):
            ls = np.where(ls < lo, lo, ls)
            ls = np.where(ls > hi, hi, ls).astype(F)
    z = np.zeros(mean.shape, F) if det else np.asarray(z, dtype=F)
    with np.errstate(all="ignore"):
        action = mean if det else (mean + exp32(ls) * z).astype(F)
        terms = (-((z * z) * F(0.5))) - ls
        logp = sum8(terms.T) - F(A) * HALF_LOG_2PI
        a0 = action[:, 0]
        budget = np.where(a0 > F(0.01), a0, F(0.01)).astype(F)
    if budget_override > 0:
        budget = np.full(len(x), F(budget_override))
    return dict(mean=mean, log_std=ls, action=action, logp=logp.astype(F), value=value.astype(F),
                bids=cent_bids(action[:, 1:], policy.bid_clip), budget=budget, x=x)


def flat_obs(out, n=None):
    """the FlatArrayWrapper rows [N, 5K+2] of a step's output dict (tests/helpers' / StepEngine.step's names)"""
    cols = [np.asarray(out["buyside_clicks"], F), np.asarray(out["cost"], F),
            np.asarray(out["cumulative_profit"], np.float64).astype(F)[:, None], np.asarray(out["days_passed"]).astype(F)[:, None],
            np.asarray(out["impressions"], F), np.asarray(out["revenue"], F), np.asarray(out["sellside_conversions"], F)]
    return np.concatenate(cols, axis=1)


def twin_act(lib, policy, obs_row, z_row=None, key=0, tick=0, deterministic=None, budget_override=0.0):
    """adc_mlp_act_host for one env; same dict as act() with a leading axis of one"""
    K = policy.num_keywords
    A = K + 1
    cfg = policy.config(K, deterministic)
    ptrs = lambda arrs: (C.c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
    pw, pb = ptrs([w for w, _ in policy.layers]), ptrs([b for _, b in policy.layers])
    vw, vb = ptrs([w for w, _ in policy.value_layers]), ptrs([b for _, b in policy.value_layers])
    o = dict(mean=np.zeros((1, A), F), log_std=np.zeros((1, A), F), action=np.zeros((1, A), F), logp=np.zeros(1, F), value=np.zeros(1, F),
             bids=np.zeros((1, K), F), budget=np.zeros(1, F))
    obs_row = None if obs_row is None else np.ascontiguousarray(obs_row, dtype=F)
    z_row = None if z_row is None else np.ascontiguousarray(z_row, dtype=F)
    p = lambda a: None if a is None else a.ctypes.data
    rc = lib.adc_mlp_act_host(C.byref(cfg), K, p(obs_row), pw, pb, vw, vb, p(policy.shift), p(policy.scale), p(policy.log_std), p(z_row),
                              int(key), int(tick), float(budget_override),
                              *(o[k].ctypes.data for k in ("mean", "log_std", "action", "logp", "value", "bids", "budget")))
    assert rc == 0, rc
    return o


def random_policy(rng, K, hidden, activation="tanh", two_heads=False, value=False, normalize=False, scale=0.5, **kw):
    """a seeded random MLPPolicy: weights ~ N(0, scale^2 / n_in), small biases"""
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    D, A = 5 * K + 2, K + 1

    def net(widths):
        layers, n_in = [], D
        for n_out in widths:
            layers.append(((rng.standard_normal((n_in, n_out)) * scale / np.sqrt(n_in)).astype(F),
                           (rng.standard_normal(n_out) * 0.1).astype(F)))
            n_in = n_out
        return layers

    if normalize:
        kw["shift"] = (rng.random(D) * 3).astype(F)
        kw["scale"] = (0.01 + rng.random(D) * 0.2).astype(F)
    if not two_heads:
        kw.setdefault("log_std", (rng.standard_normal(A) * 0.5 - 1.0).astype(F))
    return MLPPolicy(net(list(hidden) + [2 * A if two_heads else A]), activation=activation,
                     value_layers=net(list(hidden) + [1]) if value else (), **kw)


def ragged_policy(rng, K, two_heads=False, hidden=(5, 3), value_hidden=(6,)):
    """random_policy whose two networks differ in depth and whose hidden widths (and the value head's 1) are no multiple of the
    4 floats the device's stores are padded to"""
    pol = random_policy(rng, K, hidden, two_heads=two_heads, value=False)
    val = random_policy(rng, K, value_hidden, value=True)
    pol.value_layers = val.value_layers
    return pol


def realistic_obs(rng, B, K):
    """observation rows of the magnitude a day leaves: counts in the tens to thousands, dollars in the tens, some zeros"""
    clicks = rng.poisson(rng.gamma(2.0, 20.0, (B, K))) * (rng.random((B, K)) < 0.8)
    imp = clicks + rng.poisson(rng.gamma(2.0, 150.0, (B, K)))
    conv = rng.binomial(clicks, 0.1)
    cost = (clicks * rng.random((B, K)) * 0.8).astype(F)
    rev = (conv * rng.random((B, K)) * 9).astype(F)
    cum = (rng.standard_normal(B) * 3000).astype(F)
    day = rng.integers(1, 60, B).astype(F)
    return np.concatenate([clicks.astype(F), cost, cum[:, None], day[:, None], imp.astype(F), rev, conv.astype(F)], axis=1)


def realistic_norm(K):
    """shift / scale that bring realistic_obs to O(1), as a trainer's running normaliser would"""
    D = 5 * K + 2
    shift, scale = np.zeros(D, F), np.ones(D, F)
    scale[:K], scale[K:2 * K] = 1 / 40.0, 1 / 20.0
    scale[2 * K], scale[2 * K + 1] = 1 / 3000.0, 1 / 30.0
    scale[2 * K + 2:3 * K + 2], scale[3 * K + 2:4 * K + 2], scale[4 * K + 2:] = 1 / 300.0, 1 / 20.0, 1 / 4.0
    shift[:K], shift[2 * K + 2:3 * K + 2] = 30.0, 300.0
    return shift, scale
