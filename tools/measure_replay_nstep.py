#!/usr/bin/env python3
"""N-step returns for the TD3 / SAC learners, measured (profiles/pr_replay_nstep.txt).  Every measurement is a child process of its
own under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  variants  parent  with --parent-tree (a checkout of the parent commit, its library built): that tree's package and library
            off     this checkout, adc_engine_replay_nstep_init never called
            n3      this checkout after replay_nstep_init(3)
  figures   ms of td3_store per recorded day (10 days a store), and per update of a td3_update(64) and of a sac_update(64); host
            clock around synchronised calls, after an untimed round; medians of --reps (default 10) with max - min.  The variants
            alternate within a shape, so that all are taken in the same session.

    python tools/measure_replay_nstep.py [--shapes 64x25,4096x256] [--reps 10] [--parent-tree DIR]
Kernel counts and names of an update with the add-on off against the parent's: rocprofv3 --kernel-trace --stats -- python
tools/measure_replay_nstep.py --child td3 --variant off --shape 64x25 (a run of its own; and the same with --tree DIR --variant
parent).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAYS, CRITIC, BATCH = 10, (32, 32), 256


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else HERE)
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    N, K = (int(x) for x in a.shape.split("x"))
    e = eng.StepEngine(N, K, seed=7, max_days=DAYS)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    common = dict(critic_hidden=CRITIC, batch_size=BATCH, capacity=4 * DAYS * N, learning_starts=1 << 40, reward_scale=0.1, seed=3, horizon=DAYS)
    if a.child == "td3":
        from adcraft_amd.baselines.td3_trainer import TD3Trainer, td3
        TD3Trainer(e, default_policy(K, hidden=(32, 32), days=DAYS), **td3(**common))
        store, update = e.td3_store, e.td3_update
    else:
        from adcraft_amd.baselines.mlp_policy import MLPPolicy
        from adcraft_amd.baselines.sac_trainer import SACTrainer, sac
        base, rng, A = default_policy(K, hidden=(32, 32), days=DAYS), np.random.default_rng(0), K + 1
        w, _ = base.layers[-1]                      # (tools/measure_sac.py's two-headed policy)
        last = (np.concatenate([w, (rng.standard_normal(w.shape) * 0.01).astype(np.float32)], axis=1),
                np.concatenate([np.zeros(A, np.float32), np.full(A, -1.0, np.float32)]))
        pol = MLPPolicy(list(base.layers[:-1]) + [last], activation="tanh", shift=base.shift, scale=base.scale, log_std_clamp=(-5.0, 1.0))
        SACTrainer(e, pol, np.full(A, 0.01, np.float32), np.full(A, 3.0, np.float32), **sac(K, **common))
        store, update = e.sac_store, e.sac_update
    if a.variant == "n3":
        e.replay_nstep_init(3)
    rows = {"store per day": [], "per update of 64": []}
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", DAYS, 100000.0)
        t = {"store per day": timed(store, e.synchronize) / DAYS, "per update of 64": timed(lambda: update(64), e.synchronize) / 64}
        if rep:
            for k, v in t.items():
                rows[k].append(v)
    e.close()
    for k, v in rows.items():
        print(f"  {a.child} {a.shape:9s} {a.variant:6s} {k:16s} ms  median {np.median(v):9.4f}  max - min {max(v) - min(v):8.4f}   "
              + " ".join(f"{x:.4f}" for x in v), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x25,4096x256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--child", default=None, choices=["td3", "sac"])
    ap.add_argument("--variant", default="off", choices=["parent", "off", "n3"])
    ap.add_argument("--shape", default="64x25")
    ap.add_argument("--tree", default=None, help="--child: the checkout whose package and library the child runs")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    a = ap.parse_args()
    if a.child:
        return child(a)
    print(f"critics {CRITIC}, batch {BATCH}, actor (32, 32), {DAYS} days a store, ring of {4 * DAYS} days; medians of {a.reps}")
    variants = (["parent"] if a.parent_tree else []) + ["off", "n3"]
    for shape in a.shapes.split(","):
        for what in ("td3", "sac"):
            for variant in variants:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--variant", variant, "--shape", shape, "--reps", str(a.reps)]
                env = dict(os.environ)
                if variant == "parent":
                    cmd += ["--tree", a.parent_tree]
                    env["ADCRAFT_HIP_LIB"] = os.path.join(os.path.abspath(a.parent_tree), "adcraft_amd", "lib", "libadcraft_hip.so")
                rc = subprocess.run(cmd, timeout=a.child_timeout, env=env).returncode      # (a timeout raises: nothing more is started)
                if rc != 0:
                    sys.exit(f"measure_replay_nstep: child {what} {variant} {shape} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
