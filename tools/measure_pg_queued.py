#!/usr/bin/env python3
"""The queued PPO / A2C update, measured (profiles/pr_pg_queued.txt).  Every measurement is a child process of its own under a time
limit; the parent process never opens the GPU, and the first child that fails ends the run.

  update   ms of a whole update (the advantages included), host clock around synchronised calls, after an untimed round: the parent
           commit's tree (--parent-tree, its library built) host-driven, this tree host-driven, this tree queued - alternating,
           `--rounds` times over.  Shapes:
             solo64   rllib_ppo(minibatch_size=64), one learner, 128 envs x 25 keywords x 16 days = 2048 samples, 20 epochs x 32
                      minibatches = 640 steps
             pop64    16 learners of that size each in one population (2048 envs), the same 640 steps in the same launches
             big      one learner, 4096 envs x 256 keywords x 60 days, rllib_ppo(minibatch_size=61440, epochs=4): 16 steps
  trace    `--child trace --shape S --queued 0|1 --updates U`: U updates and nothing else after the set-up, to be run under a plain
           HIP trace (rocprofv3 --hip-trace, no counters); `--count DIR` then counts the trace's calls by name.  The calls of an
           update are (calls at U = 3 - calls at U = 1) / 2.

  equal    `--child equal --shape S`: two engines from the same seeds at a timed shape, two updates each - host-driven on one, queued on
           the other - and whether theta, m, v, the step counts and the returned statistics are the same bits

    python tools/measure_pg_queued.py --parent-tree DIR [--rounds 2] [--reps 5]
"""
import argparse
import csv
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {       # envs of a learner, keywords, days, learners (0: a single one), minibatch_size, epochs (None: the preset's 20)
    "solo64": (128, 25, 16, 0, 64, None),
    "pop64": (128, 25, 16, 16, 64, None),
    "big": (4096, 256, 60, 0, 61440, 4),
}


def line(label, what, v):
    print(f"{label:14s} {what:8s} ms " + " ".join(f"{x:9.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, max {max(v):.3f})", flush=True)


def trainer(shape):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines import pg_trainer
    from tools.measure_pg import policy
    n, K, days, M, mb, epochs = SHAPES[shape]
    N = n * max(M, 1)
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    pol = policy(K, (32, 32), days)
    cfg = pg_trainer.rllib_ppo(minibatch_size=mb, **({} if epochs is None else dict(epochs=epochs)))
    tr = pg_trainer.PGPopulationTrainer(e, pol, days, [cfg] * M) if M else pg_trainer.PGTrainer(e, pol, days, **cfg)
    return e, tr, days, M


def updater(e, tr, M, queued):
    update = e.pg_pop_update if M else e.pg_update
    return (lambda: update(tr.epochs, queued=True)) if queued else (lambda: update(tr.epochs))       # (the parent's has no `queued`)


def child_update(a):
    e, tr, days, M = trainer(a.shape)
    update = updater(e, tr, M, a.queued)
    ms = []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", days, 100000.0)
        e.synchronize()
        t0 = time.perf_counter()
        update()
        e.synchronize()
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3)
    steps = e.pg_pop_state(0)["steps"] if M else e.pg_state()["steps"]
    e.close()
    line(a.label, a.shape, ms)
    print(f"{a.label:14s} {a.shape:8s} optimiser steps per update: {steps // (a.reps + 1)}", flush=True)


def child_trace(a):
    e, tr, days, M = trainer(a.shape)
    update = updater(e, tr, M, a.queued)
    e.run_days("mlp", days, 100000.0)
    for _ in range(a.updates):
        update()
    e.close()
    print(f"{a.shape}: {a.updates} update(s), {'queued' if a.queued else 'host-driven'}", flush=True)


def child_equal(a):
    out = []
    for queued in (0, 1):
        e, tr, days, M = trainer(a.shape)
        update = updater(e, tr, M, queued)
        stats = []
        for _ in range(2):
            e.rollout_reset()
            e.run_days("mlp", days, 100000.0)
            stats.append(update())
        states = [e.pg_pop_state(m) for m in range(M)] if M else [e.pg_state()]
        e.close()
        out.append((states, stats))
    (sa, ta), (sb, tb) = out
    same = all(x["steps"] == y["steps"] and all(np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)) for k in ("theta", "m", "v")) for x, y in zip(sa, sb))
    same_stats = repr(ta) == repr(tb)
    print(f"{a.shape}: after two updates host-driven and queued agree bit for bit: state {same}, statistics {same_stats} "
          f"(steps {[x['steps'] for x in sa]})", flush=True)
    if not (same and same_stats):
        sys.exit(1)


def count(directory):
    """calls by name of every *hip_api_trace.csv under `directory`: the synchronising calls and the copies"""
    calls = {}
    for root, _, files in os.walk(directory):
        for f in files:
            if f.endswith("hip_api_trace.csv"):
                with open(os.path.join(root, f), newline="") as fh:
                    for row in csv.DictReader(fh):
                        name = row.get("Function") or row.get("Name") or ""
                        calls[name] = calls.get(name, 0) + 1
    keep = {k: v for k, v in calls.items() if "Synchronize" in k or "Memcpy" in k or "LaunchKernel" in k}
    print(directory, " ".join(f"{k}={v}" for k, v in sorted(keep.items())), flush=True)


def run_child(a, tree, label, shape, queued):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "update", "--tree", tree, "--label", label, "--shape", shape, "--queued", str(queued),
           "--reps", str(a.reps)]
    env = dict(os.environ, ADCRAFT_HIP_LIB=os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so"))
    rc = subprocess.run(cmd, cwd=tree, env=env, timeout=a.child_timeout).returncode          # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_pg_queued: child {label} {shape} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", default=None, choices=["update", "trace", "equal"])
    ap.add_argument("--count", default=None, metavar="DIR")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="this")
    ap.add_argument("--shape", default="solo64", choices=list(SHAPES))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--queued", type=int, default=0)
    ap.add_argument("--updates", type=int, default=1)
    a = ap.parse_args()
    if a.count:
        return count(a.count)
    if a.child:
        sys.path.insert(0, a.tree)
        return dict(update=child_update, trace=child_trace, equal=child_equal)[a.child](a)
    if not a.parent_tree:
        sys.exit("measure_pg_queued: --parent-tree DIR (the baseline is the parent commit's update in the same session)")
    parent = os.path.abspath(a.parent_tree)
    for shape in a.shapes.split(","):
        n, K, days, M, mb, epochs = SHAPES[shape]
        print(f"--- {shape}: {max(M, 1)} learner(s) of {n} envs x {K} keywords x {days} days, minibatches of {mb} samples, {epochs or 20} epochs", flush=True)
        for _ in range(a.rounds):
            run_child(a, parent, "parent host", shape, 0)
            run_child(a, HERE, "this host", shape, 0)
            run_child(a, HERE, "this queued", shape, 1)


if __name__ == "__main__":
    main()
