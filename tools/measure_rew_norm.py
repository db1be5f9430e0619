#!/usr/bin/env python3
"""The running reward normaliser measured (profiles/pr_rew_norm.txt).  Every measurement is a child process of its own under a
time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  device   ms of one rew_norm_update (scan, chunk sums, finish) plus the advantages call that reads the new multiplier
           (pg_advantages / pg_pop_advantages: bootstrap values, GAE, advantage normalisation): the engine's device events around
           the two calls (region_begin / region_end) and the host clock around the synchronised calls, after an untimed round;
           and the update alone
  host     ms of what there was to do without it: the record's reward, terminated and truncated arrays fetched through
           adc_engine_rollout_fetch (those three alone; the Python rollout_fetch, which also brings the observations, is timed
           beside it), a numpy scan of the discounted return and its running moments per normaliser, the new constant written
           as reward_scale (one learner: pg_state, pg_init, pg_state - there is no other way to change it; a population: M calls
           of pg_pop_set_config), then the same advantages call - the host clock around all of it

    python tools/measure_rew_norm.py [--shapes 4096x256x60x1,1024x25x60x16] [--reps 7] [--host-reps 3]
(a shape: envs x keywords x days x members; members > 1: a learner population with per-member normalisers)
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
GAMMA = 0.99


def engine(N, K, days):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    return e


def policy(K, days):
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    pol = default_policy(K, hidden=(32, 32), days=days, seed=0)
    rng = np.random.default_rng(3)
    widths, value = [pol.input_size, 32, 32, 1], []
    for n_in, n_out in zip(widths[:-1], widths[1:]):
        value.append(((rng.standard_normal((n_in, n_out)) / np.sqrt(n_in)).astype(np.float32), np.zeros(n_out, np.float32)))
    return MLPPolicy(pol.layers, activation=pol.activation, value_layers=value, log_std=pol.log_std, shift=pol.shift, scale=pol.scale)


def line(label, v, extra=""):
    print(f"  {label:58s} ms " + " ".join(f"{x:9.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, spread {max(v) - min(v):.3f}){extra}",
          flush=True)


def setup(a):
    N, K, T, M = (int(x) for x in a.shape.split("x"))
    e = engine(N, K, T)
    e.mlp_init(policy(K, T), deterministic=False)
    cfg = dict(gamma=GAMMA, reward_scale=0.1)
    if M > 1:
        e.mlp_learners(M)
        e.rollout_enable(T, obs=True)
        e.pg_pop_init(cfg)
    else:
        e.rollout_enable(T, obs=True)
        e.pg_init(**cfg)
    return e, N, K, T, M, cfg


def collect(e, T):
    e.reset()
    e.rollout_reset()
    e.run_days("mlp", T, 100000.0)
    e.synchronize()


def child_device(a):
    e, N, K, T, M, _ = setup(a)
    e.rew_norm_init(per_member=M > 1)
    adv = e.pg_pop_advantages if M > 1 else e.pg_advantages
    both, both_host, alone = [], [], []
    for rep in range(a.reps + 1):
        collect(e, T)
        t0 = time.perf_counter()
        e.region_begin()
        e.rew_norm_update()
        adv()
        ms = e.region_end()
        e.synchronize()
        t1 = time.perf_counter()
        collect(e, T)
        e.region_begin()
        e.rew_norm_update()
        ms_alone = e.region_end()
        if rep:
            both.append(ms)
            both_host.append((t1 - t0) * 1e3)
            alone.append(ms_alone)
    st = e.rew_norm_state(M - 1)
    assert st["count"] == 2 * (a.reps + 1) * T * (N // M) and np.isfinite(st["M2"]) and st["scale"] > 0
    e.close()
    line(f"device {a.shape} rew_norm_update + advantages, events", both)
    line(f"device {a.shape} rew_norm_update + advantages, host clock", both_host)
    line(f"device {a.shape} rew_norm_update alone, events", alone)


def child_host(a):
    e, N, K, T, M, cfg = setup(a)
    n = N // M
    adv = e.pg_pop_advantages if M > 1 else e.pg_advantages
    count, mean, m2, G = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(N)
    total, fetch3, fetch_all = [], [], []
    for rep in range(a.host_reps + 1):
        collect(e, T)
        t0 = time.perf_counter()
        reward, te, tr = np.zeros((T, N), np.float32), np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
        rc = e._lib.adc_engine_rollout_fetch(e._h, None, None, None, None, reward.ctypes.data, te.ctypes.data, tr.ctypes.data, None)
        assert rc == 0, rc
        t1 = time.perf_counter()
        done = (te | tr).astype(bool)
        g = np.zeros((T, N))
        for t in range(T):
            G = GAMMA * G + reward[t]
            g[t] = G
            G = np.where(done[t], 0.0, G)
        gm = g.reshape(T, M, n).transpose(1, 0, 2).reshape(M, -1)
        mb, vb, S = gm.mean(axis=1), gm.var(axis=1), float(T * n)
        d, nt = mb - mean, count + S
        mean, m2, count = mean + d * S / nt, m2 + vb * S + d * d * count * S / nt, nt
        scale = 1.0 / np.maximum(np.sqrt(m2 / count), 1e-2)
        if M > 1:
            for m in range(M):
                e.pg_pop_set_config(m, **dict(cfg, reward_scale=float(0.1 * scale[m])))
        else:
            st = e.pg_state()
            e.pg_init(**dict(cfg, reward_scale=float(0.1 * scale[0])))
            e.pg_state(st)
        adv()
        e.synchronize()
        t2 = time.perf_counter()
        e.rollout_fetch()
        t3 = time.perf_counter()
        if rep:
            total.append((t2 - t0) * 1e3)
            fetch3.append((t1 - t0) * 1e3)
            fetch_all.append((t3 - t2) * 1e3)
    e.close()
    line(f"host   {a.shape} fetch + numpy + reward_scale + advantages", total)
    line(f"host   {a.shape} of which the fetch of reward, terminated, truncated", fetch3)
    line(f"host   {a.shape} (rollout_fetch of all fields, not in the total)", fetch_all)


def run(args, timeout):
    rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=timeout).returncode       # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_rew_norm: child {args} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x256x60x1,1024x25x60x16")
    ap.add_argument("--shape", default="64x5x20x1")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--child", default=None, choices=["device", "host"])
    ap.add_argument("--child-timeout", type=int, default=200)
    a = ap.parse_args()
    if a.child == "device":
        return child_device(a)
    if a.child == "host":
        return child_host(a)
    print("one rew_norm_update + advantages against fetch + numpy scan and moments + reward_scale + advantages (envs x keywords x days x members)")
    for shape in a.shapes.split(","):
        common = ["--shape", shape, "--reps", str(a.reps), "--host-reps", str(a.host_reps)]
        run(["--child", "device"] + common, a.child_timeout)
        run(["--child", "host"] + common, a.child_timeout)


if __name__ == "__main__":
    main()
