"""The law of the running observation normaliser (adcraft_amd/csrc/adc_norm.h) restated in numpy, one rounded IEEE operation
per line as the header's comment block states them, for the bit-exact tests of the host twin adc_obs_norm_host and of the
device kernels.  Nothing here calls the library except twin()."""
import ctypes as C

import numpy as np

from tests.pg_ref import csum

F, D64 = np.float32, np.float64


def fresh(D, shift=None, scale=None):
    """an empty normaliser under the given vectors (default: identity)"""
    return dict(count=0, mean=np.zeros(D, D64), M2=np.zeros(D, D64),
                shift=np.zeros(D, F) if shift is None else np.array(shift, F), scale=np.ones(D, F) if scale is None else np.array(scale, F))


def update(state, x, min_std=1e-2, count_cap=0):
    """x [S, D] float32: the batch's rows, already normalised by state's shift / scale.  Returns the new state."""
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
        sc = state["scale"].astype(D64)
        mr = mx / sc
        mb = state["shift"].astype(D64) + mr
        sc2 = sc * sc
        vb = vx / sc2
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
        sd = np.where(sd < D64(min_std), D64(min_std), sd)
        shift = mean.astype(F)
        scale = (D64(1.0) / sd).astype(F)
    return dict(count=count, mean=np.asarray(mean, D64), M2=np.asarray(M2, D64), shift=shift, scale=scale)


def config(min_std=1e-2, count_cap=0, per_member=False):
    from adcraft_amd import _ffi
    c = _ffi.ObsNormConfig()
    c.struct_size = C.sizeof(_ffi.ObsNormConfig)
    c.per_member, c.min_std, c.count_cap = int(per_member), min_std, count_cap
    return c


def twin(lib, state, x, min_std=1e-2, count_cap=0):
    """adc_obs_norm_host on a copy of state"""
    x = np.ascontiguousarray(x, dtype=F)
    cfg = config(min_std, count_cap)
    cnt = C.c_int64(int(state["count"]))
    mean, M2 = np.array(state["mean"], D64), np.array(state["M2"], D64)
    shift, scale = np.array(state["shift"], F), np.array(state["scale"], F)
    rc = lib.adc_obs_norm_host(C.byref(cfg), x.shape[0], x.shape[1], x.ctypes.data, C.byref(cnt), mean.ctypes.data, M2.ctypes.data,
                               shift.ctypes.data, scale.ctypes.data)
    assert rc == 0, rc
    return dict(count=cnt.value, mean=mean, M2=M2, shift=shift, scale=scale)


def same(a, b):
    """two states, bit for bit"""
    if int(a["count"]) != int(b["count"]):
        return False
    for k, t in (("mean", D64), ("M2", D64), ("shift", F), ("scale", F)):
        x, y = np.ascontiguousarray(a[k], dtype=t), np.ascontiguousarray(b[k], dtype=t)
        if x.shape != y.shape or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            return False
    return True


def member_rows(obs, m, n, t0=0, t1=None):
    """the law's sample order for member m of a record's obs [T, N, D]: days [t0, t1), the member's n envs -> [S, D]"""
    o = obs[t0:t1, m * n:(m + 1) * n]
    return np.ascontiguousarray(o.reshape(-1, obs.shape[2]))
