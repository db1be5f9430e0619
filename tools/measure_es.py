#!/usr/bin/env python3
"""Policy populations and the evolution strategy, measured (profiles/pr_es_population.txt).  Every measurement is a child
process of its own under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  day          ms per day of run_days("mlp") with ONE policy (no population) - the [32, 32] policy of tools/measure_mlp_policy.py,
               stochastic, the rollout record on - of this checkout and, with --parent-tree / --parent-lib, of the parent commit's,
               alternating parent / this / parent / this ... in one call, at 4096 x 256 and 16384 x 1024
  population   the same day under a population of M = N, N / 8 and N / 64 members (distinct weights), this checkout
  generation   seconds per generation of ESTrainer (perturb, reset, run_days, update; host clock around a synchronised call)

    python tools/measure_es.py [--parent-tree DIR --parent-lib FILE] [--reps 3] [--shapes 4096x256,16384x1024]
Kernel times of a generation: rocprofv3 --kernel-trace --stats -- python tools/measure_es.py --child generation --shape 4096x100
(a run of its own).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from measure_mlp_policy import implicit_params, mlp_policy  # noqa: E402


def day(eng, N, K, days, members, reps):
    """ms per day of `reps` timed episodes after an untimed one, each on a fresh engine"""
    planes = implicit_params(N, K, seed=77)
    out = []
    for rep in range(reps + 1):
        e = eng.StepEngine(N, K, seed=31, max_days=days)
        e.set_all_params(planes)
        e.reset()
        pol = mlp_policy(K)
        e.mlp_init(pol, np.arange(N, dtype=np.uint64) + 1000)
        if members:
            from adcraft_amd.baselines.es_trainer import flat_params, policy_from_flat
            e.mlp_population(members)
            flat, rng = flat_params(pol), np.random.default_rng(3)
            for m in range(0, members, max(1, members // 64)):      # (distinct weights in a spread of the members; the rest hold the centre)
                e.mlp_set_member(m, policy_from_flat(pol, flat + (rng.standard_normal(flat.size) * 0.01).astype(np.float32)))
        e.rollout_enable(days)
        e.synchronize()
        e.region_begin()
        e.run_days("mlp", days, 0.0)
        ms = e.region_end()
        e.close()
        if rep:
            out.append(ms / days)
    return out


def generation(eng, N, K, members, days, generations):
    from adcraft_amd.baselines.es_trainer import ESTrainer, default_policy
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(implicit_params(N, K, seed=1))
    e.reset()
    tr = ESTrainer(e, default_policy(K, days=days), members, seed=11)
    tr.generation(days, 100000.0)                                  # untimed
    e.synchronize()
    t = []
    for _ in range(generations):
        t0 = time.perf_counter()
        tr.generation(days, 100000.0)                              # (es_update ends in a device synchronise)
        t.append(time.perf_counter() - t0)
    e.close()
    return t


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import adcraft_amd.engine as eng
    N, K = (int(x) for x in a.shape.split("x"))
    if a.child == "day":
        t = day(eng, N, K, a.days, a.members, a.reps)
        print(f"{a.label:8s} day {N} x {K} members {a.members:6d}: ms per day " + " ".join(f"{x:.4f}" for x in t) + f"  (min {min(t):.4f})", flush=True)
    else:
        t = generation(eng, N, K, a.members or N // 8, a.days, 5)
        print(f"{a.label:8s} generation {N} x {K} members {a.members or N // 8} days {a.days}: seconds " + " ".join(f"{x:.4f}" for x in t)
              + f"  (min {min(t):.4f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="4096x256,16384x1024")
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit")
    ap.add_argument("--parent-lib", default=None, help="its built library (ADCRAFT_HIP_LIB of the parent's children)")
    ap.add_argument("--rounds", type=int, default=3, help="parent / this alternations per shape")
    ap.add_argument("--child", default=None, choices=["day", "generation"])
    ap.add_argument("--shape", default="4096x256")
    ap.add_argument("--members", type=int, default=0)
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="this")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        return child(a)

    def run(label, tree, lib, what, shape, members=0, days=a.days):
        env = dict(os.environ)
        if lib:
            env["ADCRAFT_HIP_LIB"] = lib
        cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--shape", shape, "--members", str(members), "--tree", tree,
               "--label", label, "--reps", str(a.reps), "--days", str(days)]
        rc = subprocess.run(cmd, env=env, timeout=a.child_timeout).returncode       # (a timeout raises: nothing more is started)
        if rc != 0:
            sys.exit(f"measure_es: child {label} {what} {shape} ended with status {rc}; stopping")

    for shape in a.shapes.split(","):
        for _ in range(a.rounds):
            if a.parent_tree:
                run("parent", a.parent_tree, a.parent_lib, "day", shape)
            run("this", HERE, os.environ.get("ADCRAFT_HIP_LIB"), "day", shape)
    for shape in a.shapes.split(","):
        N = int(shape.split("x")[0])
        for members in (N, N // 8, N // 64):
            run("this", HERE, os.environ.get("ADCRAFT_HIP_LIB"), "day", shape, members)
    run("this", HERE, os.environ.get("ADCRAFT_HIP_LIB"), "generation", "4096x100", 512, days=10)
    run("this", HERE, os.environ.get("ADCRAFT_HIP_LIB"), "generation", "4096x100", 4096, days=60)


if __name__ == "__main__":
    main()
