"""The decision at the end of a minibatch, restated in numpy from the comments of csrc/adc_pg_shuffle.h (pg_decide) and csrc/adc_pg.h
(pg_clip_scale, the two statistics): what the host-driven update decides on the host between a minibatch's sums and its optimiser
step, and k_pg_decide of the queued update on the device.  Every value is float64 unless marked; one IEEE operation each.

    approx_kl   sums[3] / f64(S)
    stop        target_kl > 0 and approx_kl > 1.5 * f64(f32(target_kl)); a NaN approx_kl compares false: no stop
    a stopping minibatch takes no step: clip 0, scale f32(1)
    clip        f32(max_grad_norm) > 0
    grad_norm   sqrt(sums[9])
    scale       q = f64(f32(max_grad_norm)) / (grad_norm + 1e-6); f32(q if q < 1 else 1) - a NaN q compares false: scale 1;
                f32(1) with the clip off
"""
import ctypes as C

import numpy as np

F = np.float32
D64 = np.float64


def decide(max_grad_norm, target_kl, sums, S):
    """(evaluated, stop, clip, scale float32) of a live member's minibatch with the ten sums `sums` over S samples"""
    sums = np.asarray(sums, dtype=D64)
    with np.errstate(all="ignore"):
        approx_kl = sums[3] / D64(S)
        t = F(target_kl)
        if t > 0 and approx_kl > D64(1.5) * D64(t):
            return 1, 1, 0, F(1.0)
        g = F(max_grad_norm)
        if not g > 0:
            return 1, 0, 0, F(1.0)
        norm = np.sqrt(sums[9])
        q = D64(g) / (norm + D64(1e-6))
        return 1, 0, 1, F(q if q < 1.0 else 1.0)


def sums_for(approx_kl=0.0, grad_norm=1.0, S=7):
    """ten sums whose statistics are the given ones: sums[3] = approx_kl * S, sums[9] = grad_norm^2 (the caller checks what
    the roundings made of them where it matters)"""
    s = np.zeros(10, D64)
    with np.errstate(all="ignore"):
        s[3] = D64(approx_kl) * D64(S)
        s[9] = D64(grad_norm) * D64(grad_norm)
    s[[0, 1, 2, 5, 6, 7, 8]] = (0.25, 0.5, 1.5, 3.0, 0.125, 11.0, 0.75)
    return s


def twin_decide(lib, max_grad_norm, target_kl, sums, S):
    from adcraft_amd.engine import StepEngine
    cfg = StepEngine.pg_config(max_grad_norm=float(max_grad_norm))
    sums = np.ascontiguousarray(sums, dtype=D64)
    ev, stop, clip, scale = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_float(-1.0)
    rc = lib.adc_pg_decide_host(C.byref(cfg), float(F(target_kl)), sums.ctypes.data, int(S), C.byref(ev), C.byref(stop), C.byref(clip), C.byref(scale))
    assert rc == 0, rc
    return ev.value, stop.value, clip.value, F(scale.value)
