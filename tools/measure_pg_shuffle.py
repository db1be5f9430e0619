#!/usr/bin/env python3
"""The PPO learners' shuffled sample-level minibatches, measured (profiles/pr_pg_shuffle.txt).  Every measurement is a child
process of its own under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  minibatch  ms of one minibatch of S samples, host clock around synchronised calls, after an untimed round: the parent commit's
             tree (--parent-tree, its library built) and this tree without the add-on over an env range of B envs x T days, this
             tree with the add-on over S = B T gathered samples - the same number of samples, the same bytes of the record, less
             locality - and ms of k_pg_shuffle_rows' launch (pg_shuffle_epoch) per epoch.  A single learner at 4096 envs x 256
             keywords x 60 days, S = 61440; 16 learners of 64 envs x 25 keywords x 60 days, S = 960 (and S = 64 gathered, next to
             the env range of one env: 60 samples).  Alternating, `--rounds` times over.
  update     a whole rllib_ppo(minibatch_size=64) update at the reference's train batch of 2048 samples (128 envs x 16 days x 25
             keywords): 32 minibatches x 20 epochs = 640 steps, each with its host round trip; ms per update and per step
  launches   `--child launches --tree DIR`: one update WITHOUT the add-on of a single learner and of four learners - run it under a
             kernel trace (rocprofv3 --kernel-trace) in this tree and in the parent's and compare the two launch lists

    python tools/measure_pg_shuffle.py --parent-tree DIR [--rounds 3] [--reps 7]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def line(label, what, v):
    print(f"{label:16s} {what:22s} ms " + " ".join(f"{x:9.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, max {max(v):.3f})", flush=True)


def engine(a, N, K, days, hidden, M=0):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from tools.measure_pg import policy
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    pol = policy(K, hidden, days)
    e.mlp_init(pol, deterministic=False)
    if M:
        e.mlp_learners(M)
    e.rollout_enable(days, obs=True)
    return e, pol


def child_minibatch(a):
    """one variant at one shape, in the tree a.tree"""
    N, K, M, B, days = a.envs, a.keywords, a.members, a.range_envs, a.days
    e, _ = engine(a, N, K, days, tuple(int(x) for x in a.hidden.split(",")), M)
    cfg = dict(lr=3e-4, minibatch_envs=B)
    if M:
        e.pg_pop_init(cfg)
        advantages, ranged = e.pg_pop_advantages, lambda: e.pg_pop_minibatch(0)
    else:
        e.pg_init(**cfg)
        advantages, ranged = e.pg_advantages, lambda: e.pg_minibatch(0, B)
    S = a.samples or B * days
    if a.shuffle:
        e.pg_shuffle_init(minibatch_samples=S)
    rows = {}
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", days, 100000.0)
        advantages()
        t = {}
        if a.shuffle:
            t["k_pg_shuffle_rows"] = timed(e.pg_shuffle_epoch, e.synchronize)
            t[f"gathered S={S}"] = timed(lambda: e.pg_shuffle_minibatch(0), e.synchronize)
        else:
            t[f"env range S={B * days}"] = timed(ranged, e.synchronize)
        if rep:
            for k, v in t.items():
                rows.setdefault(k, []).append(v)
    e.close()
    for k, v in rows.items():
        line(a.label, k, v)


def child_update(a):
    from adcraft_amd.baselines import pg_trainer
    N, K, days = 128, 25, 16
    e, pol = engine(a, N, K, days, (32, 32))
    tr = pg_trainer.PGTrainer(e, pol, days, **pg_trainer.rllib_ppo(minibatch_size=64))
    total, steps = [], []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", days, 100000.0)
        before = e.pg_state()["steps"]
        ms = timed(lambda: e.pg_update(tr.epochs), e.synchronize)
        if rep:
            total.append(ms)
            steps.append(e.pg_state()["steps"] - before)
    e.close()
    line(a.label, "rllib_ppo(64) update", total)
    line(a.label, "... per step", [t / s for t, s in zip(total, steps)])
    print(f"{a.label:16s} steps per update: {steps}", flush=True)


def child_launches(a):
    """one update without the add-on, for a kernel trace (4 env-range minibatches x 2 epochs, single learner, then 4 learners)"""
    for M in (0, 4):
        e, _ = engine(a, 64, 25, 8, (32, 32), M)
        cfg = dict(lr=3e-4, minibatch_envs=(64 // max(M, 1)) // 4)
        e.pg_pop_init(cfg) if M else e.pg_init(**cfg)
        e.run_days("mlp", 8, 100000.0)
        e.pg_pop_update(2) if M else e.pg_update(2)
        e.close()
    print("one update each of a single learner and of 4 learners, without the add-on", flush=True)


def run_child(a, tree, mode, label, extra):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree, "--label", label, "--days", str(a.days), "--hidden", a.hidden,
           "--reps", str(a.reps)] + [str(x) for x in extra]
    env = dict(os.environ, ADCRAFT_HIP_LIB=os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so"))
    rc = subprocess.run(cmd, cwd=tree, env=env, timeout=a.child_timeout).returncode          # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_pg_shuffle: child {mode} {label} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--hidden", default="32,32")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--child", default=None, choices=["minibatch", "update", "launches"])
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="this")
    ap.add_argument("--shuffle", type=int, default=0)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--keywords", type=int, default=256)
    ap.add_argument("--members", type=int, default=0)
    ap.add_argument("--range-envs", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, a.tree)
        return dict(minibatch=child_minibatch, update=child_update, launches=child_launches)[a.child](a)
    if not a.parent_tree:
        sys.exit("measure_pg_shuffle: --parent-tree DIR (the baseline is the parent commit's minibatch in the same session)")
    parent = os.path.abspath(a.parent_tree)
    # (envs, keywords, learners, envs of the range, gathered samples when they are not range x days)
    for N, K, M, B, S in ((4096, 256, 0, 1024, 0), (64 * 16, 25, 16, 16, 0), (64 * 16, 25, 16, 1, 64)):
        print(f"--- {N} envs x {K} keywords x {a.days} days, hidden ({a.hidden})" + (f", {M} learners of {N // M} envs" if M else ", one learner")
              + f": env range of {B} envs against {S or B * a.days} gathered samples", flush=True)
        shape = ["--envs", N, "--keywords", K, "--members", M, "--range-envs", B, "--samples", S]
        for _ in range(a.rounds):
            run_child(a, parent, "minibatch", "parent", shape)
            run_child(a, HERE, "minibatch", "this", shape)
            run_child(a, HERE, "minibatch", "this + add-on", shape + ["--shuffle", 1])
    print("--- rllib_ppo(minibatch_size=64): 128 envs x 25 keywords x 16 days = 2048 samples, 20 epochs x 32 minibatches", flush=True)
    for _ in range(a.rounds):
        run_child(a, HERE, "update", "this + add-on", [])


if __name__ == "__main__":
    main()
