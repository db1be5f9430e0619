#!/usr/bin/env python3
"""TD3 learner populations measured (profiles/pr_td3_population.txt).  Every measurement is a child process of its own under a time
limit; the parent process never opens the GPU, and the first child that fails ends the run.

  pop      ms of one td3_pop_update(64) (no statistics fetched, no member clipping: kernels only) with M members of `envs` envs x K
           keywords each, batch B, critics as given; host clock around synchronised calls, after an untimed round
  solo     ms of one td3_update(64) of ONE learner at the same per-member shape - with --parent-tree (a checkout of the parent
           commit, its library built) the parent's package and library: the reference the gain is measured against
  regress  the paths that must not have moved, this build and the parent's alternating: solo td3_update(64) per update at the
           shapes of profiles/pr_td3_trainer.txt, one solo pg_minibatch, one pg_pop_update epoch (tools/measure_pg_population.py's
           children); bench.py and the single-policy day are tools/measure_td3.py --parent-tree

    python tools/measure_td3_population.py [--members 1,4,16,64] [--envs 64] [--keywords 25] [--batch 256] [--critics 32,32;256,256]
                                           [--reps 7] [--parent-tree DIR [--rounds 3]] [--skip-regress]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/measure_td3_population.py --child pop --members 16 (a run of its own).
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
DAYS, UPDATES = 10, 64
SOLO_SHAPES = (("1024x25", "32,32", 256), ("1024x25", "256,256", 256), ("4096x256", "256,256", 256), ("4096x256", "256,256", 2048))


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def engine(N, K):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    e = eng.StepEngine(N, K, seed=7, max_days=DAYS)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    return e


def config(critic, batch, capacity):
    from adcraft_amd.baselines.td3_trainer import td3
    return td3(critic_hidden=critic, batch_size=batch, capacity=capacity, learning_starts=1 << 40, reward_scale=0.1, seed=3)


def line(label, v):
    print(f"  {label:52s} ms " + " ".join(f"{x:8.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, spread {max(v) - min(v):.3f})",
          flush=True)


def child_pop(a, M):
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer
    critic = tuple(int(x) for x in a.critic.split(","))
    e = engine(M * a.envs, a.keywords)
    TD3PopulationTrainer(e, default_policy(a.keywords, hidden=(32, 32), days=DAYS), 0.1, config(critic, a.batch, 4 * DAYS * a.envs), horizon=DAYS, members=M)
    rows = []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", DAYS, 100000.0)
        e.td3_pop_store()
        t = timed(lambda: e.td3_pop_update(UPDATES, stats=False), e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"pop  M {M:3d} x {a.envs} x {a.keywords} critics ({a.critic}) B {a.batch}: {UPDATES} updates", rows)


def child_solo(a):
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.td3_trainer import TD3Trainer
    (N, K), critic = (int(x) for x in a.shape.split("x")), tuple(int(x) for x in a.critic.split(","))
    e = engine(N, K)
    TD3Trainer(e, default_policy(K, hidden=(32, 32), days=DAYS), horizon=DAYS, **config(critic, a.batch, 4 * DAYS * N))
    rows = []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", DAYS, 100000.0)
        e.td3_store()
        t = timed(lambda: e.td3_update(UPDATES), e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"solo {a.label:6s} {N} x {K} critics ({a.critic}) B {a.batch}: {UPDATES} updates", rows)


def run(script, args, tree, timeout):
    env = dict(os.environ)
    if tree:
        tree = os.path.abspath(tree)
        env["ADCRAFT_HIP_LIB"] = os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so")
        args = args + ["--tree", tree]
    rc = subprocess.run([sys.executable, os.path.join(HERE, "tools", script)] + args, env=env, timeout=timeout).returncode      # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_td3_population: child {script} {args} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="1,4,16,64")
    ap.add_argument("--envs", type=int, default=64, help="envs of a member")
    ap.add_argument("--keywords", type=int, default=25)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--critics", default="32,32;256,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="this / other-library alternations")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: the solo reference")
    ap.add_argument("--tree", default=HERE, help="(children) the checkout whose package is measured")
    ap.add_argument("--skip-regress", action="store_true")
    ap.add_argument("--skip-gain", action="store_true")
    ap.add_argument("--child", default=None, choices=["pop", "solo"])
    ap.add_argument("--shape", default="64x25")
    ap.add_argument("--critic", default="256,256")
    ap.add_argument("--label", default="this")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child == "pop":
        return child_pop(a, int(a.members))
    if a.child == "solo":
        return child_solo(a)
    me, reps = os.path.basename(__file__), ["--reps", str(a.reps)]
    trees = (("parent", a.parent_tree), ("this", None)) if a.parent_tree else (("this", None),)
    if not a.skip_gain:
        for critic in a.critics.split(";"):
            print(f"gain: {UPDATES} updates, per member {a.envs} envs x {a.keywords} keywords, batch {a.batch}, critics ({critic}), actor (32, 32)")
            for _ in range(a.rounds):
                run(me, ["--child", "solo", "--shape", f"{a.envs}x{a.keywords}", "--critic", critic, "--batch", str(a.batch),
                         "--label", trees[0][0]] + reps, trees[0][1], a.child_timeout)
                for M in a.members.split(","):
                    run(me, ["--child", "pop", "--members", M, "--envs", str(a.envs), "--keywords", str(a.keywords), "--critic", critic,
                             "--batch", str(a.batch)] + reps, None, a.child_timeout)
    if a.skip_regress:
        return
    print(f"solo paths: td3_update({UPDATES}), one pg_minibatch, one pg_pop_update epoch; the parent's build and this one alternating")
    for shape, critic, batch in SOLO_SHAPES:
        for _ in range(a.rounds):
            for label, tree in trees:
                run(me, ["--child", "solo", "--shape", shape, "--critic", critic, "--batch", str(batch), "--label", label] + reps, tree, a.child_timeout)
    for _ in range(a.rounds):
        for label, tree in trees:
            run("measure_pg_population.py", ["--child", "mini", "--shape", "1024x25", "--hidden", "32,32", "--days", "10", "--label", label] + reps,
                tree, a.child_timeout)
            print(f"  (pg_pop_update of {label}:)", flush=True)
            run("measure_pg_population.py", ["--child", "pop", "--members", "16", "--envs", "64", "--keywords", "25", "--days", "32", "--hidden", "32,32"] + reps,
                tree, a.child_timeout)


if __name__ == "__main__":
    main()
