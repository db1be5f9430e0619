#!/usr/bin/env python3
"""The running observation normaliser measured (profiles/pr_obs_norm.txt).  Every measurement is a child process of its own
under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  device   ms of one obs_norm_update over the T recorded days (the pass over the record and the D-long finish): the engine's
           device events around the call (region_begin / region_end) and the host clock around the synchronised call, after an
           untimed round; and the record's bytes over the device time against the HBM peak of 8.0 TB/s
  host     ms of what there was to do without it: rollout_fetch of the record (with the observations), float64 numpy moments of
           the de-normalised rows, the new vectors, adc_engine_mlp_set_norm - the host clock around the three together, and the
           fetch alone

    python tools/measure_obs_norm.py [--shapes 4096x256x60x1,1024x25x60x16] [--reps 7] [--host-reps 2]
(a shape: envs x keywords x days x members; members > 1: learners with per-member normalisers - the host path is then M times
the moments on M slices and cannot upload per-member vectors at all, so it is measured for the shared normaliser only)
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/measure_obs_norm.py --child device --shape 4096x256x60x1 (a run of its own).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
HBM_PEAK = 8.0e12          # bytes / s (spec)


def engine(N, K, days):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    return e


def policy(K, days):
    from adcraft_amd.baselines.es_trainer import default_policy
    return default_policy(K, hidden=(32, 32), days=days, seed=0)


def line(label, v, extra=""):
    print(f"  {label:44s} ms " + " ".join(f"{x:9.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, spread {max(v) - min(v):.3f}){extra}",
          flush=True)


def setup(a):
    N, K, T, M = (int(x) for x in a.shape.split("x"))
    e = engine(N, K, T)
    e.mlp_init(policy(K, T), deterministic=False)
    if M > 1:
        e.mlp_learners(M)
    e.rollout_enable(T, obs=True)
    return e, N, K, T, M


def child_device(a):
    e, N, K, T, M = setup(a)
    D = 5 * K + 2
    e.obs_norm_init(per_member=M > 1)
    dev, host = [], []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", T, 100000.0)
        e.synchronize()
        t0 = time.perf_counter()
        e.region_begin()
        e.obs_norm_update()
        ms = e.region_end()
        e.synchronize()
        if rep:
            dev.append(ms)
            host.append((time.perf_counter() - t0) * 1e3)
    st = e.obs_norm_state(M - 1)
    assert st["count"] == (a.reps + 1) * T * (N // M) and np.isfinite(st["scale"]).all()
    e.close()
    nbytes = T * N * D * 4
    rate = nbytes / (min(dev) * 1e-3)
    line(f"device {a.shape} (D {D}, {nbytes / 1e6:.1f} MB) events", dev, f"   {rate / 1e9:.0f} GB/s of record = {100 * rate / HBM_PEAK:.1f} % of HBM peak (best)")
    line(f"device {a.shape} host clock", host)


def child_host(a):
    e, N, K, T, M = setup(a)
    pol = policy(K, T)
    shift, scale = pol.shift.astype(np.float64), pol.scale.astype(np.float64)
    total, fetch = [], []
    for rep in range(a.host_reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", T, 100000.0)
        e.synchronize()
        t0 = time.perf_counter()
        obs = e.rollout_fetch()["obs"]
        t1 = time.perf_counter()
        raw = obs.reshape(-1, obs.shape[2]).astype(np.float64) / scale + shift
        mean, sd = raw.mean(axis=0), raw.std(axis=0)
        new_shift, new_scale = mean.astype(np.float32), (1.0 / np.maximum(sd, 1e-2)).astype(np.float32)
        e._lib.adc_engine_mlp_set_norm(e._h, new_shift.ctypes.data, new_scale.ctypes.data)
        e.synchronize()
        t2 = time.perf_counter()
        e._lib.adc_engine_mlp_set_norm(e._h, pol.shift.ctypes.data, pol.scale.ctypes.data)
        if rep:
            total.append((t2 - t0) * 1e3)
            fetch.append((t1 - t0) * 1e3)
    e.close()
    line(f"host   {a.shape} fetch + numpy + set_norm", total)
    line(f"host   {a.shape} of which rollout_fetch (all fields)", fetch)


def run(args, timeout):
    rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=timeout).returncode       # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_obs_norm: child {args} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x256x60x1,1024x25x60x16")
    ap.add_argument("--shape", default="64x5x20x1")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--child", default=None, choices=["device", "host"])
    ap.add_argument("--child-timeout", type=int, default=280)
    a = ap.parse_args()
    if a.child == "device":
        return child_device(a)
    if a.child == "host":
        return child_host(a)
    print("one obs_norm_update against rollout_fetch + numpy moments + mlp_set_norm (envs x keywords x days x members)")
    for shape in a.shapes.split(","):
        common = ["--shape", shape, "--reps", str(a.reps), "--host-reps", str(a.host_reps)]
        run(["--child", "device"] + common, a.child_timeout)
        if shape.endswith("x1"):
            run(["--child", "host"] + common, a.child_timeout)
        else:
            s = "x".join(shape.split("x")[:3]) + "x1"
            run(["--child", "device", "--shape", s] + common[2:], a.child_timeout)
            run(["--child", "host", "--shape", s] + common[2:], a.child_timeout)


if __name__ == "__main__":
    main()
