#!/usr/bin/env python3
"""DAgger days, measured (profiles/pr_dagger.txt).  Every measurement is a child process of its own under a time limit; the parent
process never opens the GPU, and the first child that fails ends the run.

  days       ms per day, a (32, 32) policy, at 4096 envs x 256 keywords and at 64 x 25: the parent commit's teach_days(teacher) day and
             its recorded run_days("mlp") day (--parent-tree, its library built), this tree's teach_days(teacher) day (an unchanged
             path) and its dagger_days(teacher, beta) day; `days` days in one call, host clock around synchronised calls, after an
             untimed round
  minibatch  ms of im_minibatch over a record of `days` teacher days in both trees (an unchanged path)
  The variants alternate `--rounds` times; a row is the median of `--reps` with max - min.

    python tools/measure_dagger.py --parent-tree DIR [--rounds 1] [--reps 10] [--days 60] [--teacher oracle] [--beta 0.5]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((4096, 256), (64, 25))


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
    N, K, T = a.envs, a.keywords, a.days
    e = eng.StepEngine(N, K, seed=7, max_days=T)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    mb = N // 4
    if a.teacher == "oracle":
        e.bid_curves_build(2048)
    e.mlp_init(policy(K, (32, 32), T), deterministic=False)
    e.rollout_enable(T, obs=True)
    e.pg_init(lr=3e-4, minibatch_envs=mb)
    e.im_init(beta=0.0)
    rows, share = [], None
    for rep in range(a.reps + 1):
        e.reset()
        if a.teacher == "zero_margin":
            e.agent_init(1.0)
        e.rollout_reset()
        if a.what == "mlp":
            ms = timed(lambda: e.run_days("mlp", T, 100000.0), e.synchronize) / T
        elif a.what == "teach":
            ms = timed(lambda: e.teach_days(a.teacher, T, 100000.0), e.synchronize) / T
        elif a.what == "dagger":
            ms = timed(lambda: e.dagger_days(a.teacher, T, a.beta, 100000.0), e.synchronize) / T
            share = float(e.dagger_mask().mean())
        else:
            e.teach_days(a.teacher, T, 100000.0)
            e.im_advantages()
            ms = timed(lambda: e.im_minibatch(0, mb), e.synchronize)
        if rep:
            rows.append(ms)
    e.close()
    print(f"{N:5d} x {K:3d}  {a.label:32s} ms " + " ".join(f"{x:8.3f}" for x in rows) +
          f"   median {np.median(rows):.3f}  max-min {max(rows) - min(rows):.3f}" + ("" if share is None else f"  teacher share {share:.3f}"),
          flush=True)


def run_child(a, tree, label, what, shape):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--label", label, "--what", what, "--envs", str(shape[0]),
           "--keywords", str(shape[1]), "--days", str(a.days), "--reps", str(a.reps), "--teacher", a.teacher, "--beta", str(a.beta)]
    env = dict(os.environ, ADCRAFT_HIP_LIB=os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so"))
    rc = subprocess.run(cmd, cwd=tree, env=env, timeout=a.child_timeout).returncode          # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_dagger: child {label} {shape} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--teacher", default="oracle")
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    for name in ("--tree", "--label", "--what"):
        ap.add_argument(name)
    ap.add_argument("--envs", type=int)
    ap.add_argument("--keywords", type=int)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_tree:
        ap.error("--parent-tree DIR")
    parent = os.path.abspath(a.parent_tree)
    for shape in SHAPES:
        for _ in range(a.rounds):
            run_child(a, parent, f"parent teach_days({a.teacher}) day", "teach", shape)
            run_child(a, parent, "parent run_days(mlp) day, rec.", "mlp", shape)
            run_child(a, HERE, f"teach_days({a.teacher}) day", "teach", shape)
            run_child(a, HERE, f"dagger_days({a.teacher}, {a.beta}) day", "dagger", shape)
            run_child(a, parent, "parent im_minibatch", "im_minibatch", shape)
            run_child(a, HERE, "im_minibatch", "im_minibatch", shape)


if __name__ == "__main__":
    main()
