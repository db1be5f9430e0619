#!/usr/bin/env python3
"""The PPO learners' KL penalty and value-loss clip, measured (profiles/pr_pg_kl.txt).  Every measurement is a child process of
its own under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  times    ms of pg_advantages (under the add-on: GAE plus the snapshot of the collecting distribution) and of one minibatch,
           on a record of T days: a single learner at 4096 envs x 256 keywords, and 16 learners of 64 envs x 25 keywords; host
           clock around synchronised calls, after an untimed round.  Three variants, alternating, `--rounds` times over: the
           parent commit's tree (--parent-tree, its library built), this tree without the add-on, this tree with it.
  bench    bench.py of the parent's tree and of this one, alternating: ms_per_step, and --dump-outputs compared byte for byte

    python tools/measure_pg_kl.py --parent-tree DIR [--rounds 3] [--reps 7] [--days 60] [--hidden 32,32]
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


def child(a):
    """one variant at one shape, in the tree a.tree: prints `label what ms ...`"""
    sys.path.insert(0, a.tree)
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from tools.measure_pg import policy
    N, K, M = a.envs, a.keywords, a.members
    hidden = tuple(int(x) for x in a.hidden.split(","))
    e = eng.StepEngine(N, K, seed=7, max_days=a.days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    e.mlp_init(policy(K, hidden, a.days), deterministic=False)
    cfg = dict(lr=3e-4, minibatch_envs=(N // max(M, 1)) // a.minibatches)
    if M:
        e.mlp_learners(M)
    e.rollout_enable(a.days, obs=True)
    if M:
        e.pg_pop_init(cfg)
        advantages, minibatch = e.pg_pop_advantages, lambda: e.pg_pop_minibatch(0)
    else:
        e.pg_init(**cfg)
        advantages, minibatch = e.pg_advantages, lambda: e.pg_minibatch(0, cfg["minibatch_envs"])
    if a.kl:
        e.pg_kl_init(kl_coef=1.0, kl_target=0.01, adaptive=True, vf_clip=10.0)
    rows = dict(advantages=[], minibatch=[])
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", a.days, 100000.0)
        t = dict(advantages=timed(advantages, e.synchronize), minibatch=timed(minibatch, e.synchronize))
        if rep:
            for k, v in t.items():
                rows[k].append(v)
    e.close()
    for k, v in rows.items():
        print(f"{a.label:14s} {k:11s} ms " + " ".join(f"{x:9.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, max {max(v):.3f})", flush=True)


def run_child(a, tree, label, kl, shape):
    N, K, M = shape
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--label", label, "--kl", str(kl), "--envs", str(N), "--keywords", str(K),
           "--members", str(M), "--days", str(a.days), "--hidden", a.hidden, "--reps", str(a.reps), "--minibatches", str(a.minibatches)]
    env = dict(os.environ, ADCRAFT_HIP_LIB=os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so"))
    rc = subprocess.run(cmd, cwd=tree, env=env, timeout=a.child_timeout).returncode          # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_pg_kl: child {label} {shape} ended with status {rc}; stopping")


def bench(a, trees):
    import filecmp
    import json
    import tempfile
    dumps = {k: tempfile.mkdtemp(prefix=f"pg_kl_dump_{k}_") for k in trees}
    ms = {k: [] for k in trees}
    for _ in range(a.rounds):
        for label, tree in trees.items():
            env = dict(os.environ, ADCRAFT_HIP_LIB=os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so"))
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "300", "--warmup", "30", "--dump-outputs", dumps[label]],
                                 cwd=tree, env=env, timeout=a.child_timeout, capture_output=True, text=True)
            if out.returncode != 0:
                sys.exit(f"measure_pg_kl: bench.py of {label} ended with status {out.returncode}; stopping\n{out.stderr[-2000:]}")
            ms[label].append(json.loads(out.stdout.strip().splitlines()[-1])["ms_per_step"])
    for label in trees:
        print(f"bench.py ms_per_step {label:6s}: " + " ".join(f"{x:.4f}" for x in ms[label]) + f"  (min {min(ms[label]):.4f}, max {max(ms[label]):.4f})")
    names = sorted(os.listdir(dumps["this"]))
    same = [n for n in names if filecmp.cmp(os.path.join(dumps["this"], n), os.path.join(dumps["parent"], n), shallow=False)]
    print(f"bench.py --dump-outputs: {len(same)} of {len(names)} files byte-identical to the parent's"
          + ("" if len(same) == len(names) else f"; DIFFERENT: {sorted(set(names) - set(same))}"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--hidden", default="32,32")
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="this")
    ap.add_argument("--kl", type=int, default=0)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--keywords", type=int, default=256)
    ap.add_argument("--members", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        sys.exit("measure_pg_kl: --parent-tree DIR (the baseline is the parent commit's minibatch in the same session)")
    parent = os.path.abspath(a.parent_tree)
    for shape in ((4096, 256, 0), (64 * 16, 25, 16)):
        print(f"--- {shape[0]} envs x {shape[1]} keywords x {a.days} days, hidden ({a.hidden})"
              + (f", {shape[2]} learners of {shape[0] // shape[2]} envs" if shape[2] else ", one learner") + f", {a.minibatches} minibatches", flush=True)
        for _ in range(a.rounds):
            run_child(a, parent, "parent", 0, shape)
            run_child(a, HERE, "this", 0, shape)
            run_child(a, HERE, "this + add-on", 1, shape)
    if not a.skip_bench:
        bench(a, dict(parent=parent, this=HERE))


if __name__ == "__main__":
    main()
