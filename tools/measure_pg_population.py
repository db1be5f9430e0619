#!/usr/bin/env python3
"""Learner populations measured (profiles/pr_pg_population.txt).  Every measurement is a child process of its own under a time
limit; the parent process never opens the GPU, and the first child that fails ends the run.

  pop      ms of one pg_pop_update epoch (advantages + the members' minibatches) with M members of `envs` envs x K keywords each,
           T recorded days, one minibatch per member; host clock around synchronised calls, after an untimed round
  solo     ms of one pg_update epoch of ONE learner at the same per-member shape - with --parent-tree (a checkout of the parent
           commit, its library built) the parent's package and library: the reference the gain is measured against
  mini     ms of one solo pg_minibatch at the three shapes of profiles/pr_pg_trainer.txt section 1, this build and the parent's
           alternating: the solo path must not have moved

    python tools/measure_pg_population.py [--members 1,4,16,64] [--envs 64] [--keywords 25] [--days 32] [--hidden 32,32] [--reps 7]
                                          [--parent-tree DIR [--rounds 3]]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/measure_pg_population.py --child pop --members 16 (a run of its own).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child measures the package of --tree: this checkout's, or the parent's)
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE
sys.path.insert(0, TREE)


def policy(K, hidden, days):
    """tools/measure_pg.py's: default_policy plus a value network of the same hidden sizes"""
    from adcraft_amd.baselines.es_trainer import default_policy
    pol = default_policy(K, hidden=hidden, days=days, seed=0)
    rng = np.random.default_rng(1)
    layers, n_in = [], 5 * K + 2
    for n_out in list(hidden) + [1]:
        b = 1.0 / np.sqrt(n_in)
        layers.append((rng.uniform(-b, b, (n_in, n_out)).astype(np.float32), rng.uniform(-b, b, n_out).astype(np.float32)))
        n_in = n_out
    pol.value_layers = layers
    return pol


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3

MINI_SHAPES = (("4096x256", "64,64", 60), ("4096x256", "32,32", 60), ("1024x25", "32,32", 10))


def engine(N, K, days):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    return e


def line(label, v):
    print(f"  {label:34s} ms " + " ".join(f"{x:8.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, spread {max(v) - min(v):.3f})",
          flush=True)


def child_pop(a, M):
    N, K, hidden = M * a.envs, a.keywords, tuple(int(x) for x in a.hidden.split(","))
    e = engine(N, K, a.days)
    e.mlp_init(policy(K, hidden, a.days), deterministic=False)
    e.mlp_learners(M)
    e.rollout_enable(a.days, obs=True)
    e.pg_pop_init(dict(lr=3e-4))
    rows = []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", a.days, 100000.0)
        t = timed(lambda: e.pg_pop_update(1), e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"pop  M {M:3d} x {a.envs} x {K} T {a.days} {hidden}", rows)


def child_solo(a):
    N, K, hidden = a.envs, a.keywords, tuple(int(x) for x in a.hidden.split(","))
    e = engine(N, K, a.days)
    e.mlp_init(policy(K, hidden, a.days), deterministic=False)
    e.rollout_enable(a.days, obs=True)
    e.pg_init(lr=3e-4)
    rows = []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", a.days, 100000.0)
        t = timed(lambda: e.pg_update(1), e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"solo {a.label:6s} {N} x {K} T {a.days} {hidden}", rows)


def child_mini(a):
    (N, K), hidden = (int(x) for x in a.shape.split("x")), tuple(int(x) for x in a.hidden.split(","))
    e = engine(N, K, a.days)
    e.mlp_init(policy(K, hidden, a.days), deterministic=False)
    e.rollout_enable(a.days, obs=True)
    e.pg_init(lr=3e-4, minibatch_envs=N // 4)
    rows = []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", a.days, 100000.0)
        e.pg_advantages()
        t = timed(lambda: e.pg_minibatch(0, N // 4), e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"pg_minibatch {a.label:6s} {a.shape} {hidden} T {a.days}", rows)


def run(args, tree, timeout):
    env = dict(os.environ)
    if tree:
        tree = os.path.abspath(tree)
        env["ADCRAFT_HIP_LIB"] = os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so")
        args = args + ["--tree", tree]
    rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, timeout=timeout).returncode       # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_pg_population: child {args} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="1,4,16,64")
    ap.add_argument("--envs", type=int, default=64, help="envs of a member")
    ap.add_argument("--keywords", type=int, default=25)
    ap.add_argument("--days", type=int, default=32)
    ap.add_argument("--hidden", default="32,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="this / other-library alternations")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: the solo reference")
    ap.add_argument("--tree", default=HERE, help="(children) the checkout whose package is measured")
    ap.add_argument("--skip-mini", action="store_true")
    ap.add_argument("--child", default=None, choices=["pop", "solo", "mini"])
    ap.add_argument("--shape", default="1024x25")
    ap.add_argument("--label", default="this")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child == "pop":
        return child_pop(a, int(a.members))
    if a.child == "solo":
        return child_solo(a)
    if a.child == "mini":
        return child_mini(a)
    common = ["--envs", str(a.envs), "--keywords", str(a.keywords), "--days", str(a.days), "--hidden", a.hidden, "--reps", str(a.reps)]
    print(f"gain: one epoch, per member {a.envs} envs x {a.keywords} keywords, T {a.days} ({a.envs * a.days} samples), hidden ({a.hidden}), one minibatch")
    for _ in range(a.rounds):
        run(["--child", "solo", "--label", "parent" if a.parent_tree else "this"] + common, a.parent_tree, a.child_timeout)
        for M in a.members.split(","):
            run(["--child", "pop", "--members", M] + common, None, a.child_timeout)
    if a.skip_mini:
        return
    print("solo path: one pg_minibatch (a quarter of the envs), the parent's build and this one alternating")
    for shape, hidden, days in MINI_SHAPES:
        for _ in range(a.rounds):
            for label, tree in (("parent", a.parent_tree), ("this", None)) if a.parent_tree else (("this", None),):
                run(["--child", "mini", "--shape", shape, "--hidden", hidden, "--days", str(days), "--reps", str(a.reps), "--label", label], tree, a.child_timeout)


if __name__ == "__main__":
    main()
