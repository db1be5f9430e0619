#!/usr/bin/env python3
"""The recurrent policy, measured (profiles/pr_recurrent.txt).  Every measurement is a child process of its own under a time limit;
the parent process never opens the GPU, and the first child that fails ends the run.

  day         ms per recorded run_days("mlp") day at 4096 envs x 256 keywords: the parent commit's library under the (32, 32)
              feed-forward policy (--parent-tree, its library built), this tree's under the same policy (an unchanged path) and under
              trunk (32,) + GRU 32; `days` days in one call, host clock around synchronised calls, after an untimed round
  generation  ms of one ES generation (perturb, `days` days, update) of 256 members at 64 envs x 25 keywords each member
              (16384 envs), the same three variants
  The variants alternate `--rounds` times; a row is the median of `--reps` with max - min.  The extra bytes per env and day - the
  state read and written, and the cell's weights - are printed from the shapes.

    python tools/measure_recurrent.py --parent-tree DIR [--rounds 1] [--reps 10] [--days 60] [--gru 32]
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
    """one variant in the tree a.tree: prints `label ms ...`"""
    sys.path.insert(0, a.tree)
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    N, K, T = a.envs, a.keywords, a.days
    e = eng.StepEngine(N, K, seed=7, max_days=T)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    pol = default_policy(K, hidden=(32,), days=T, gru=a.gru) if a.gru else default_policy(K, hidden=(32, 32), days=T)
    e.mlp_init(pol, deterministic=False)
    if a.what == "day":
        e.rollout_enable(T, obs=True)
    else:
        e.mlp_population(a.members)
        e.es_init(sigma=0.02, lr=0.01, seed=11)
    rows = []
    for rep in range(a.reps + 1):
        e.reset()
        if a.what == "day":
            e.rollout_reset()
            ms = timed(lambda: e.run_days("mlp", T, 100000.0), e.synchronize) / T
        else:
            def generation():
                e.es_perturb()
                e.run_days("mlp", T, 100000.0)
                e.es_update()
            ms = timed(generation, e.synchronize)
        if rep:
            rows.append(ms)
    e.close()
    print(f"{N:5d} x {K:3d}  {a.label:44s} ms " + " ".join(f"{x:8.3f}" for x in rows) +
          f"   median {np.median(rows):.3f}  max-min {max(rows) - min(rows):.3f}", flush=True)


def run_child(a, tree, label, what, shape, gru):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--label", label, "--what", what, "--envs", str(shape[0]),
           "--keywords", str(shape[1]), "--days", str(a.days), "--reps", str(a.reps), "--gru", str(gru), "--members", str(a.members)]
    env = dict(os.environ, ADCRAFT_HIP_LIB=os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so"))
    rc = subprocess.run(cmd, cwd=tree, env=env, timeout=a.child_timeout).returncode          # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_recurrent: child {label} {shape} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--gru", type=int, default=32)
    ap.add_argument("--members", type=int, default=256)
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
    parent, G = os.path.abspath(a.parent_tree), a.gru
    cell = 4 * ((32 + 1) * 3 * G + (G + 1) * 3 * G)
    print(f"extra per env and day under trunk (32,) + GRU {G}: {4 * G} B of state read, {4 * G} B written, 8 B of words read and written; "
          f"the cell's weights, {cell} B, are read by every workgroup (shared by all envs, or a member's)")
    for what, shape in (("day", (4096, 256)), ("generation", (a.members * 64, 25))):
        unit = 'run_days("mlp") day, rec.' if what == "day" else f"ES generation, {a.members} members"
        for _ in range(a.rounds):
            run_child(a, parent, f"parent (32, 32) {unit}", what, shape, 0)
            run_child(a, HERE, f"(32, 32) {unit}", what, shape, 0)
            run_child(a, HERE, f"(32,) + GRU {G} {unit}", what, shape, G)


if __name__ == "__main__":
    main()
