"""The prioritised-replay law (adcraft_amd/csrc/adc_per.h) restated in numpy from the header's comments: the radix-64 sum tree with
its Hillis-Steele scans in float64, the counter-addressed descent, the batch's importance weights, the priorities from the critics'
errors and the max-over-duplicates leaf update, and the TD3 / SAC updates of tests/td3_ref.py / tests/sac_ref.py driven by these
slots and weights.  The host twins (adc_per_*_host) and the device kernels must give these very bits."""
import ctypes as C

import numpy as np

from tests import mlp_ref as R
from tests import pg_ref as P
from tests import sac_ref as S
from tests import td3_ref as T3

F = np.float32
D64 = np.float64
ST_PER_BATCH = 22
RADIX = 64
DEFAULTS = dict(alpha=0.6, beta=0.4, eps=1e-6, cap=1e6)


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def shape(capacity):
    """[n_0 = C, n_1, ..., n_L = 1]: n_l = ceil(n_{l-1} / 64), at least one level above the leaves"""
    n = [int(capacity)]
    while True:
        n.append((n[-1] + RADIX - 1) // RADIX)
        if n[-1] <= 1:
            return n


def scan64(v):
    """the inclusive prefix of [..., 64] float64 children: for s = 1, 2, 4, 8, 16, 32, all lanes at once, c_i = c_i + c_{i-s} (i >= s)"""
    c = np.array(v, D64)
    s = 1
    while s < RADIX:
        t = c.copy()
        t[..., s:] = c[..., s:] + c[..., :-s]
        c = t
        s += s
    return c


class Tree:
    """leaf [C] float32 (zeros past the stored slots) and the float64 levels above, every level padded with zeros to a multiple of 64"""

    def __init__(self, capacity, leaf=None, top=1.0):
        self.C, self.n = int(capacity), shape(capacity)
        self.L = len(self.n) - 1
        pad = lambda k: (k + RADIX - 1) // RADIX * RADIX
        self.leaf = np.zeros(pad(self.C), F)
        self.node = [None] + [np.zeros(pad(self.n[l]), D64) for l in range(1, self.L + 1)]
        self.top = F(top)
        if leaf is not None:
            leaf = np.asarray(leaf, F)
            self.leaf[:leaf.size] = leaf
        self.rebuild()

    def children(self, level, i):
        src = self.leaf if level == 1 else self.node[level - 1]
        return src[i * RADIX:(i + 1) * RADIX].astype(D64)

    def rebuild(self):
        for l in range(1, self.L + 1):
            src = (self.leaf if l == 1 else self.node[l - 1]).astype(D64).reshape(-1, RADIX)
            self.node[l][:self.n[l]] = scan64(src)[:self.n[l], RADIX - 1]

    def rebuild_paths(self, slots):
        for l in range(1, self.L + 1):
            for i in sorted({int(s) >> (6 * l) for s in slots}):
                self.node[l][i] = scan64(self.children(l, i))[RADIX - 1]

    @property
    def total(self):
        return self.node[self.L][0]

    def nodes(self):
        """the levels 1 .. L one after the other, n_l values each (adc_per_tree_host's order)"""
        return np.concatenate([self.node[l][:self.n[l]] for l in range(1, self.L + 1)])

    def descend(self, m):
        """the slot a descent with m (float64) reaches, before the guard against the ring's size"""
        m, i = D64(m), 0
        for l in range(self.L, 0, -1):
            v = self.children(l, i)
            c = scan64(v)
            over = np.nonzero(c > m)[0]
            if over.size:
                child = int(over[0])
            else:
                nz = np.nonzero(v != 0)[0]
                child = int(nz[-1]) if nz.size else 0
            if child > 0:
                m = m - c[child - 1]
            i = min(i * RADIX + child, self.n[l - 1] - 1)
        return i

    def fill(self, slots):
        """what a store or a buffer load does to the slots it wrote: leaf = top, the nodes on their paths rebuilt"""
        slots = [int(s) for s in slots]
        self.leaf[slots] = self.top
        self.rebuild_paths(slots)


def u53(seed, update, B):
    """[B] float64: w = draw(td3 key, b / 2, 22, 0, u); hi, lo = words 2 (b % 2), 2 (b % 2) + 1; f64(((hi << 32) | lo) >> 11) * 2^-53"""
    key, out = T3.td3_key(seed), np.zeros(B, D64)
    for q in range((B + 1) // 2):
        w = T3._words(key, q, ST_PER_BATCH, 0, int(update))
        for h in range(2):
            if 2 * q + h < B:
                bits = ((int(w[2 * h]) << 32) | int(w[2 * h + 1])) >> 11
                out[2 * q + h] = D64(bits) * D64(2.0 ** -53)
    return out


def weight(lmin, leaf, beta):
    leaf = np.asarray(leaf, F)
    if F(beta) == 0:
        return np.ones(leaf.shape, F)
    with np.errstate(all="ignore"):
        d = (S.det_log(np.full(leaf.shape, lmin, F)) - S.det_log(leaf)).astype(F)
        return R.exp32((F(beta) * d).astype(F))


def sample(tree, seed, update, B, size, beta):
    """(idx [B] int32, w [B] float32) of update number `update` from the tree as it stands"""
    idx = np.zeros(B, np.int32)
    for b, u in enumerate(u53(seed, update, B)):
        idx[b] = min(tree.descend(u * tree.total), int(size) - 1)
    lf = tree.leaf[idx]
    return idx, weight(lf.min(), lf, beta)


def pa(p, alpha):
    p = np.asarray(p, F)
    if F(alpha) == 0:
        return np.ones(p.shape, F)
    with np.errstate(all="ignore"):
        return R.exp32((F(alpha) * S.det_log(p)).astype(F))


def priority(d1, d2, eps, cap):
    """mm = 0.5 * (|d_1| + |d_2|); p = mm + eps; p = p > cap ? cap : p; p = p >= eps ? p : eps (a NaN becomes eps)"""
    d1, d2, eps, cap = np.asarray(d1, F), np.asarray(d2, F), F(eps), F(cap)
    with np.errstate(all="ignore"):
        p = ((F(0.5) * (np.abs(d1) + np.abs(d2)).astype(F)).astype(F) + eps).astype(F)
        p = np.where(p > cap, cap, p).astype(F)
        return np.where(p >= eps, p, eps).astype(F)


def leaf_update(tree, idx, pab):
    """a slot's new leaf is the maximum of pa(p_b) over the elements that drew it; top follows; the touched paths are rebuilt"""
    idx, pab = np.asarray(idx), np.asarray(pab, F)
    for s in np.unique(idx):
        tree.leaf[s] = pab[idx == s].max()
    tree.top = max(tree.top, F(pab.max()))
    tree.rebuild_paths(idx)


# ---- the learners' updates under prioritised replay -----------------------------------------------------------------------------------
def critic_grad(sh, psi, norm, x, an, y, w):
    """td3_ref.critic_grad with the output deltas w * d and the loss pieces w * (0.5 * (d * d)); also the unweighted d of both critics.
    an: the action inputs as the critics read them"""
    x, y, w = np.ascontiguousarray(x, F), np.asarray(y, F), np.asarray(w, F)
    row = np.concatenate([x, an], axis=1)
    parts, pieces, ds = [], [], []
    with np.errstate(all="ignore"):
        for net in sh.critics(psi):
            ys = T3.forward(row, net, sh.act)
            q = ys[-1][:, 0]
            d = (q - y).astype(F)
            ds.append(d)
            pieces.append(((w * (F(0.5) * (d * d)).astype(F)).astype(F), q))
            parts.append(T3.net_grad(row, ys, T3.backward(net, ys, (w * d).astype(F)[:, None], sh.act)))
        g = np.concatenate(parts)
        cols = np.stack([pieces[0][0], pieces[1][0], pieces[0][1], pieces[1][1], y], axis=1).astype(D64)
        sums = np.concatenate([P.csum(cols), [P.csum(g.astype(D64) * g.astype(D64))]])
    return g, sums, ds[0], ds[1]


def _after_critics(tree, idx, d1, d2, per):
    leaf_update(tree, idx, pa(priority(d1, d2, per["eps"], per["cap"]), per["alpha"]))


def td3_update(policy, state, buf, norm, seed, opts, tree, per):
    """td3_ref.update with the batch drawn from `tree` (updated in place) under the options `per`.  Returns (new state, statistics)"""
    sh, st, u = T3.Shapes(policy, opts), dict(state), state["updates"]
    B, size = opts["batch_size"], len(buf["r"])
    idx, w = sample(tree, seed, u, B, size, per["beta"])
    x, a = buf["x"][idx], buf["a"][idx]
    y = T3.target(sh, st["theta_target"], st["psi_target"], norm, seed, u, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
    g, s6, d1, d2 = critic_grad(sh, st["psi"], norm, x, T3.action_norm(a, norm), y, w)
    _after_critics(tree, idx, d1, d2, per)
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
    return st, stats


def sac_update(policy, state, buf, seed, opts, tree, per):
    """sac_ref.update with the batch drawn from `tree` (updated in place) under the options `per`.  Returns (new state, statistics)"""
    sh, st, u = T3.Shapes(policy, opts), dict(state), state["updates"]
    clamp, B, size = policy.log_std_clamp, opts["batch_size"], len(buf["r"])
    alpha = S.alpha_of(st["log_alpha"][0])
    idx, w = sample(tree, seed, u, B, size, per["beta"])
    x = buf["x"][idx]
    y, _ = S.target(sh, clamp, st["theta"], st["psi_target"], alpha, seed, u, buf["x2"][idx], buf["r"][idx], buf["done"][idx], opts)
    g, s6, d1, d2 = critic_grad(sh, st["psi"], None, x, R.tanh32(np.asarray(buf["a"][idx], F)), y, w)
    _after_critics(tree, idx, d1, d2, per)
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
    return st, stats


# ---- the host twins -----------------------------------------------------------------------------------------------------------------
def prio_config(**kw):
    from adcraft_amd.engine import StepEngine
    return StepEngine.replay_prio_config(**kw)


def _leaves(capacity, leaf):
    out = np.zeros(int(capacity), F)
    leaf = np.asarray(leaf, F)
    out[:leaf.size] = leaf
    return out


def twin_tree(lib, capacity, leaf):
    """(levels, counts [levels + 1], nodes: the levels 1 .. L one after the other)"""
    lf, counts = _leaves(capacity, leaf), np.zeros(7, np.int64)
    L = lib.adc_per_tree_host(int(capacity), lf.ctypes.data, None, counts.ctypes.data)
    assert L >= 1, L
    nodes = np.zeros(int(counts[1:L + 1].sum()), D64)
    assert lib.adc_per_tree_host(int(capacity), lf.ctypes.data, nodes.ctypes.data, None) == L
    return L, counts[:L + 1].copy(), nodes


def twin_descend(lib, capacity, leaf, m):
    lf, slot = _leaves(capacity, leaf), C.c_int64(-1)
    assert lib.adc_per_descend_host(int(capacity), lf.ctypes.data, float(m), C.byref(slot)) == 0
    return slot.value


def twin_sample(lib, capacity, size, leaf, seed, update, B, **per):
    cfg, lf = prio_config(**per), _leaves(capacity, leaf)
    idx, w = np.zeros(B, np.int32), np.zeros(B, F)
    rc = lib.adc_per_sample_host(C.byref(cfg), int(capacity), int(size), lf.ctypes.data, int(seed), int(update), B, idx.ctypes.data, w.ctypes.data)
    assert rc == 0, rc
    return idx, w


def twin_priority(lib, d1, d2, **per):
    cfg, d1, d2 = prio_config(**per), np.ascontiguousarray(d1, dtype=F), np.ascontiguousarray(d2, dtype=F)
    out = np.zeros(d1.size, F)
    assert lib.adc_per_priority_host(C.byref(cfg), d1.size, d1.ctypes.data, d2.ctypes.data, out.ctypes.data) == 0
    return out


def twin_leaf_update(lib, capacity, leaf, top, idx, pab):
    lf, t = _leaves(capacity, leaf), C.c_float(float(top))
    idx, pab = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(pab, dtype=F)
    assert lib.adc_per_leaf_update_host(int(capacity), lf.ctypes.data, C.byref(t), idx.size, idx.ctypes.data, pab.ctypes.data) == 0
    return lf, F(t.value)
