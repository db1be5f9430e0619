"""The law of the PPO learners' shuffled sample-level minibatches and target-KL early stop (adcraft_amd/csrc/adc_pg_shuffle.h)
restated in numpy from the header's comments: the shuffle key, the 4-round Feistel permutation with cycle walking over the
Philox stream, the record rows, the minibatches cut from an epoch's order, the stop rule and the statistics of an update.  The
gradient itself is tests/pg_ref.py's (tests/pg_kl_ref.py's under the KL add-on): their grad(...) take sample arrays in order, so a
gathered minibatch is a call with gathered arrays.  The host twins (adc_pg_shuffle_order_host, adc_pg_shuffle_stop_host) and the
device kernels must give these very bits."""
import ctypes as C

import numpy as np

from tests import pg_kl_ref as KR
from tests import pg_ref as P
from tests.mlp_ref import _mix64

F = np.float32
D64 = np.float64
U32 = np.uint32
U64 = np.uint64
ST_PG_SHUFFLE = 19
PHILOX_ROUNDS = 7
SHUFFLE_DEFAULTS = dict(minibatch_samples=64, seed=0, target_kl=0.0)


def shuffle_options(**kw):
    o = dict(SHUFFLE_DEFAULTS)
    o.update(kw)
    return o


def shuffle_key(seed):
    return _mix64(int(seed) ^ 0xA54FF53A5F1D36F1)


def philox_x(key, index, stage, keyword, tick):
    """word x of draw(key, index, stage, keyword, tick) (adc_law.h's Philox4x32-7) for an array of indices"""
    c0 = np.asarray(index, dtype=U64)
    c1, c2, c3 = (np.full(c0.shape, v, U64) for v in (stage, keyword, tick))
    k0, k1 = int(key) & 0xFFFFFFFF, int(key) >> 32
    m32 = U64(0xFFFFFFFF)
    for _ in range(PHILOX_ROUNDS):
        a, b = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2
        n0 = (b >> U64(32)) ^ c1 ^ U64(k0)
        n2 = (a >> U64(32)) ^ c3 ^ U64(k1)
        c1, c3 = b & m32, a & m32
        c0, c2 = n0, n2
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0.astype(U32)


def half_bits(n_s):
    h = 1
    while (1 << (2 * h)) < n_s:
        h += 1
    return h


def feistel(key, x, h, tick):
    """one application of the network to the array x < 2^(2 h)"""
    mask = U32((1 << h) - 1)
    x = np.asarray(x, dtype=U32)
    L, R = x >> U32(h), x & mask
    for r in range(4):
        f = philox_x(key, R, ST_PG_SHUFFLE, r, tick) & mask
        L, R = R, L ^ f
    return (L << U32(h)) | R


def order(seed, n_s, tick):
    """[n_s] uint32: position i holds sample sigma_tick(i); seed as resolved (the configuration's, or the engine's)"""
    key, h = shuffle_key(seed), half_bits(n_s)
    x = feistel(key, np.arange(n_s, dtype=U32), h, int(tick) & 0xFFFFFFFF)
    while True:
        out = x >= n_s
        if not out.any():
            return x
        x[out] = feistel(key, x[out], h, int(tick) & 0xFFFFFFFF)


def rows(order_, n, N, member=0):
    """the record rows (of the record flattened to [T * N]) of a member's samples"""
    o = np.asarray(order_, dtype=np.int64)
    return ((o // n) * N + member * n + o % n).astype(U32)


def stop(approx_kl, target_kl):
    return bool(F(target_kl) > 0 and D64(approx_kl) > 1.5 * D64(F(target_kl)))


def minibatches(n_s, mb):
    return [(j * mb, min((j + 1) * mb, n_s)) for j in range((n_s + mb - 1) // mb)]


def _gathered(rec, adv, ret, idx):
    """the sample arrays of the record (a member's own columns, [T, n, ...]) at the sample indices idx = t * n + env"""
    flat = lambda a: np.ascontiguousarray(a).reshape((-1,) + a.shape[2:])[idx]
    return flat(rec["obs"]), flat(rec["action"]), flat(rec["logp"]), flat(adv), flat(ret), flat(rec["value"])


def minibatch(policy, state, rec, adv, ret, idx, opts, sh_opts, stopped=False, snap=None, kl_opts=None, coef=None):
    """what adc_engine_pg_shuffle_minibatch does to state = dict(theta, m, v, steps) over the samples idx, in that order.
    snap / kl_opts / coef: under the KL add-on.  Returns (new state, statistics, the KL add-on's statistics or None, stopped)"""
    obs, action, logp, a, r, value = _gathered(rec, adv, ret, idx)
    kst = None
    if snap is not None:
        mean_old, ls_old = snap
        mo = mean_old.reshape((-1, mean_old.shape[-1]))[idx]
        lo = ls_old.reshape((-1, ls_old.shape[-1]))[idx] if ls_old.ndim == 3 else ls_old
        g, _, _, st, kst, _ = KR.grad(policy, state["theta"], obs, action, logp, a, r, value, mo, lo, kl_coef=coef, vf_clip=kl_opts["vf_clip"], **opts)
    else:
        g, _, st = P.grad(policy, state["theta"], obs, action, logp, a, r, value, **opts)
    if stopped or stop(st["approx_kl"], sh_opts["target_kl"]):
        return state, st, kst, True
    theta, m, v = P.step(state["theta"], state["m"], state["v"], g, state["steps"], **opts)
    return dict(theta=theta, m=m, v=v, steps=state["steps"] + 1), st, kst, False


def update(policy, state, rec, bootstrap, epochs, opts, sh_opts, seed, kl_opts=None, coef=None, trace=None):
    """adc_engine_pg_update under the add-on (for a population: one member, rec its own columns): the advantages (and the
    snapshot) once, per epoch the order of tick = the step count and its minibatches, until the stop.  seed: the resolved seed.
    Returns (new state, the statistics of the last epoch begun, the KL statistics or None, the shuffle statistics); trace, a
    list, receives (epoch, j, approx_kl, theta after) per evaluated minibatch"""
    adv, ret = P.gae(rec["reward"], rec["terminated"], rec["truncated"], rec["value"], bootstrap, **opts)
    snap = KR.snapshot(policy, state["theta"], rec) if kl_opts is not None else None
    T, n = rec["reward"].shape
    n_s, mb = T * n, sh_opts["minibatch_samples"]
    sst = dict(epochs_begun=0, minibatches_evaluated=0, steps_taken=0, stopped=0)
    mean = kmean = None
    stopped, samples = False, 0
    for ep in range(epochs):
        if stopped:
            break
        o = order(seed, n_s, state["steps"])
        sst["epochs_begun"] += 1
        acc, kacc, cnt = dict.fromkeys(P.STAT_KEYS, D64(0.0)), dict(kl=D64(0.0), vf_clip_fraction=D64(0.0)), 0
        for j, (i0, i1) in enumerate(minibatches(n_s, mb)):
            state, st, kst, stopped = minibatch(policy, state, rec, adv, ret, o[i0:i1].astype(np.int64), opts, sh_opts, False, snap, kl_opts, coef)
            sst["minibatches_evaluated"] += 1
            sst["steps_taken"] += 0 if stopped else 1
            samples, cnt = i1 - i0, cnt + 1
            if trace is not None:
                trace.append((ep, j, st["approx_kl"], state["theta"].copy()))
            with np.errstate(all="ignore"):
                acc = {k: acc[k] + st[k] for k in P.STAT_KEYS}
                if kst is not None:
                    kacc = {k: kacc[k] + kst[k] for k in kacc}
            if stopped:
                break
        with np.errstate(all="ignore"):
            mean = {k: acc[k] / D64(cnt) for k in P.STAT_KEYS}
            kmean = {k: kacc[k] / D64(cnt) for k in kacc}
    sst["stopped"] = 1 if stopped else 0
    mean = dict(mean, samples=samples, steps=state["steps"])
    if kl_opts is None:
        return state, mean, None, sst
    kmean.update(kl_coef=F(coef), kl_coef_next=KR.adapt(coef, kmean["kl"], **kl_opts))
    return state, mean, kmean, sst


# ---- the host twins ---------------------------------------------------------------------------------------------------------------
def twin_order(lib, seed, n_s, tick):
    out = np.zeros(n_s, U32)
    rc = lib.adc_pg_shuffle_order_host(int(seed), int(n_s), int(tick) & 0xFFFFFFFF, out.ctypes.data)
    assert rc == 0, rc
    return out


def twin_stop(lib, approx_kl, target_kl):
    out = C.c_int32(-1)
    rc = lib.adc_pg_shuffle_stop_host(float(approx_kl), float(F(target_kl)), C.byref(out))
    assert rc == 0, rc
    return bool(out.value)
