"""The recurrent policy's law (adcraft_amd/csrc/adc_gru.h) restated in numpy from the header's comments, over tests/mlp_ref.py for
what the header takes from adc_mlp.h (sum8, tanh, exp64, the heads): the sigmoid, the cell, the act with a cell in front of the
output layer, and the state rule.  The host twins (adc_gru_cell_host, adc_mlp_act_recurrent_host, adc_gru_state_host) and the
device kernel must give these very bits.  `policy` is an MLPPolicy with gru=(Wi, bi, Wh, bh)."""
import ctypes as C
import types

import numpy as np

from tests import mlp_ref as R

F = np.float32
NONE = -2                                   # `last` of an env that has not acted since its explicit reset


def sigmoid32(v):
    """float32 -> float32: a = min(max(v, -87), 88) as float64; float32(1 / (1 + exp64(-a))); NaN -> NaN"""
    v = np.asarray(v, dtype=F)
    nan = np.isnan(v)
    a = np.minimum(np.maximum(np.where(nan, F(0), v), F(-87)), F(88)).astype(np.float64)
    out = (1.0 / (1.0 + R.exp64(-a))).astype(F)
    return np.where(nan, v, out).astype(F)


def cell(x, h, gru):
    """x [B, n_in], h [B, G] -> h' [B, G]; gates r, z, n, row q = gate * G + g"""
    wi, bi, wh, bh = gru
    G = wh.shape[0]
    gi = R.layer(np.asarray(x, F), wi, bi, None)
    gh = R.layer(np.asarray(h, F), wh, bh, None)
    with np.errstate(all="ignore"):
        r = sigmoid32(gi[:, :G] + gh[:, :G])
        z = sigmoid32(gi[:, G:2 * G] + gh[:, G:2 * G])
        t = r * gh[:, 2 * G:]
        n = R.tanh32(gi[:, 2 * G:] + t)
        u = F(1) - z
        p = u * n
        s = z * np.asarray(h, F)
        return (p + s).astype(F)


def act(policy, obs, h, z=None, deterministic=None, budget_override=0.0):
    """mlp_ref.act with the cell in front of the output layer: obs [B, D], h [B, G] the input states.  Returns mlp_ref.act's dict
    plus h [B, G], the new states."""
    x = np.ascontiguousarray(obs, dtype=F)
    if policy.shift is not None:
        with np.errstate(all="ignore"):
            x = ((x - policy.shift[None, :]) * policy.scale[None, :]).astype(F)
    t = x
    for w, b in policy.layers[:-1]:
        t = R.layer(t, w, b, policy.activation)
    h1 = cell(t, h, policy.gru)
    # everything after the output layer is the feed-forward law: a policy whose only layer reads the new state, no normalisation
    head = types.SimpleNamespace(layers=[policy.layers[-1]], value_layers=[], shift=None, scale=None, num_keywords=policy.num_keywords,
                                 activation=policy.activation, log_std=policy.log_std, log_std_clamp=policy.log_std_clamp, bid_clip=policy.bid_clip,
                                 deterministic=policy.deterministic)
    out = R.act(head, h1, z, deterministic, budget_override)
    out["value"] = (R.network(x, policy.value_layers, policy.activation)[:, 0] if policy.value_layers else np.zeros(len(x), F)).astype(F)
    out["h"], out["x"] = h1, x
    return out


class State:
    """one env's state under the header's rule: h [2, G], last, from"""

    def __init__(self, G):
        self.h, self.last, self.frm = np.zeros((2, G), F), NONE, 0

    def begin(self, d):
        """the `from` an act on episode day d forms, and the state it reads"""
        frm = 0 if d == 0 else (d if self.last not in (d - 1, d) else self.frm)
        return frm, (np.zeros(self.h.shape[1], F) if frm == d else self.h[(d + 1) & 1].copy())

    def commit(self, d, frm, h_new):
        self.h[d & 1] = h_new
        self.last, self.frm = d, frm

    def forget(self):
        self.last = NONE


def twin_cell(lib, x, h, gru):
    """adc_gru_cell_host on one row"""
    wi, bi, wh, bh = gru
    x, h = np.ascontiguousarray(x, F), np.ascontiguousarray(h, F)
    out = np.zeros(wh.shape[0], F)
    rc = lib.adc_gru_cell_host(wi.shape[0], wh.shape[0], x.ctypes.data, h.ctypes.data, wi.ctypes.data, bi.ctypes.data, wh.ctypes.data, bh.ctypes.data,
                               out.ctypes.data)
    assert rc == 0, rc
    return out


def twin_act(lib, policy, obs_row, h_row, z_row=None, key=0, tick=0, deterministic=None, budget_override=0.0):
    """adc_mlp_act_recurrent_host for one env; act()'s dict with a leading axis of one"""
    K = policy.num_keywords
    A, G = K + 1, policy.gru_width
    cfg = policy.config(K, deterministic)
    ptrs = lambda arrs: (C.c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
    pw, pb = ptrs([w for w, _ in policy.layers]), ptrs([b for _, b in policy.layers])
    vw, vb = ptrs([w for w, _ in policy.value_layers]), ptrs([b for _, b in policy.value_layers])
    o = dict(mean=np.zeros((1, A), F), log_std=np.zeros((1, A), F), action=np.zeros((1, A), F), logp=np.zeros(1, F), value=np.zeros(1, F),
             bids=np.zeros((1, K), F), budget=np.zeros(1, F), h=np.zeros((1, G), F))
    keep = [None if a is None else np.ascontiguousarray(a, dtype=F) for a in (obs_row, z_row, h_row)]
    p = lambda a: None if a is None else a.ctypes.data
    rc = lib.adc_mlp_act_recurrent_host(C.byref(cfg), K, G, p(keep[0]), pw, pb, *(a.ctypes.data for a in policy.gru), vw, vb, p(policy.shift),
                                        p(policy.scale), p(policy.log_std), p(keep[1]), int(key), int(tick), float(budget_override), p(keep[2]),
                                        *(o[k].ctypes.data for k in ("mean", "log_std", "action", "logp", "value", "bids", "budget", "h")))
    assert rc == 0, rc
    return o


def random_gru(rng, n_in, G, scale=1.0):
    """a seeded random cell: uniform in +-scale / sqrt(G), as torch draws it"""
    b = scale / np.sqrt(G)
    return tuple(rng.uniform(-b, b, s).astype(F) for s in ((n_in, 3 * G), (3 * G,), (G, 3 * G), (3 * G,)))


def random_policy(rng, K, hidden, G, activation="tanh", two_heads=False, value=False, normalize=False, scale=0.5, **kw):
    """mlp_ref.random_policy with a cell of width G in front of the output layer (hidden: the trunk's widths, () for none)"""
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    ff = R.random_policy(rng, K, hidden, activation, two_heads, value, normalize, scale, **kw)
    A = K + 1
    n_in = ff.layers[-1][0].shape[0]
    P = 2 * A if two_heads else A
    out = ((rng.standard_normal((G, P)) * scale / np.sqrt(G)).astype(F), (rng.standard_normal(P) * 0.1 + 0.5).astype(F))
    return MLPPolicy(ff.layers[:-1] + [out], activation=activation, value_layers=ff.value_layers, log_std=ff.log_std, shift=ff.shift, scale=ff.scale,
                     log_std_clamp=ff.log_std_clamp, bid_clip=ff.bid_clip, deterministic=ff.deterministic, gru=random_gru(rng, n_in, G))
