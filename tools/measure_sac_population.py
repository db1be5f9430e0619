#!/usr/bin/env python3
"""SAC learner populations measured (profiles/pr_sac_population.txt).  Every measurement is a child process of its own under a time
limit; the parent process never opens the GPU, and the first child that fails ends the run.

  pop      ms of one sac_pop_update(64) (no statistics fetched, no member clipping: kernels only) with M members of `envs` envs x K
           keywords each, batch B, critics as given; host clock around synchronised calls, after an untimed round
  solo     ms of M sac_update(64) calls one after another of ONE learner at the same per-member shape (a sweep of M cells done one
           engine at a time pays this much for its updates) - with --parent-tree (a checkout of the parent commit, its library built)
           the parent's package and library: the reference the gain is measured against
  waits    set-up, one update and then one no-clip sac_pop_update(--waits-updates) with its statistics, alone in a process: run it
           under a HIP-API trace with 64 and with 0; the difference of the two traces' calls is what the call of 64 launches and
           waits for
  regress  the paths that must not have moved, the parent's build and this one alternating: bench.py, its dumped outputs and the
           single-policy day (tools/measure_td3.py's), one solo sac_update(64) (this tool's solo child with M = 1) and one
           td3_pop_update(64) (tools/measure_td3_population.py's pop child)

    python tools/measure_sac_population.py [--members 16,64] [--envs 64] [--keywords 25] [--batch 256] [--critics 32,32] [--reps 10]
                                           [--parent-tree DIR [--rounds 3]] [--skip-regress] [--skip-gain]
Launch and wait counts: rocprofv3 --hip-trace --stats -- python tools/measure_sac_population.py --child waits --members 16
--waits-updates 64, and again with --waits-updates 0 (runs of their own, nothing else collected).
"""
import argparse
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child measures the package of --tree: this checkout's, or the parent's)
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(HERE, "tools"))
DAYS, UPDATES = 10, 64


def timed(fn, sync):
    import time
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


def sac_policy(K):
    """tools/measure_sac.py's: the default (32, 32) policy with a log-std head beside its means"""
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    base = default_policy(K, hidden=(32, 32), days=DAYS)
    rng, A = np.random.default_rng(0), K + 1
    w, b = base.layers[-1]
    last = (np.concatenate([w, (rng.standard_normal(w.shape) * 0.01).astype(np.float32)], axis=1),
            np.concatenate([np.zeros(A, np.float32), np.full(A, -1.0, np.float32)]))
    return MLPPolicy(list(base.layers[:-1]) + [last], activation="tanh", shift=base.shift, scale=base.scale, log_std_clamp=(-5.0, 1.0))


def config(K, critic, batch, capacity):
    from adcraft_amd.baselines.sac_trainer import sac
    return sac(K, critic_hidden=critic, batch_size=batch, capacity=capacity, learning_starts=1 << 40, reward_scale=0.1, seed=3)


def bounds(K):
    return np.full(K + 1, 0.01, np.float32), np.full(K + 1, 3.0, np.float32)


def line(label, v):
    print(f"  {label:60s} ms " + " ".join(f"{x:8.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, spread {max(v) - min(v):.3f})",
          flush=True)


def population(a, M):
    from adcraft_amd.baselines.sac_trainer import SACPopulationTrainer
    critic = tuple(int(x) for x in a.critic.split(","))
    e = engine(M * a.envs, a.keywords)
    SACPopulationTrainer(e, sac_policy(a.keywords), config(a.keywords, critic, a.batch, 4 * DAYS * a.envs), *bounds(a.keywords), horizon=DAYS, members=M)
    return e


def child_pop(a, M):
    e = population(a, M)
    rows = []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", DAYS, 100000.0)
        e.sac_pop_store()
        t = timed(lambda: e.sac_pop_update(UPDATES, stats=False), e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"pop  M {M:3d} x {a.envs} x {a.keywords} critics ({a.critic}) B {a.batch}: one call of {UPDATES} updates", rows)


def child_solo(a, M):
    from adcraft_amd.baselines.sac_trainer import SACTrainer
    (N, K), critic = (int(x) for x in a.shape.split("x")), tuple(int(x) for x in a.critic.split(","))
    e = engine(N, K)
    SACTrainer(e, sac_policy(K), *bounds(K), horizon=DAYS, **config(K, critic, a.batch, 4 * DAYS * N))
    rows = []
    for rep in range(a.reps + 1):
        e.reset()
        e.rollout_reset()
        e.run_days("mlp", DAYS, 100000.0)
        e.sac_store()
        t = timed(lambda: [e.sac_update(UPDATES) for _ in range(M)], e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"solo {a.label:6s} {N} x {K} critics ({a.critic}) B {a.batch}: {M} calls of {UPDATES} updates in sequence", rows)


def child_waits(a, M):
    """set-up and one update, then one no-clip call of --waits-updates updates with its statistics (0: none)"""
    e = population(a, M)
    e.run_days("mlp", DAYS, 100000.0)
    e.sac_pop_store()
    e.sac_pop_update(1)
    e.synchronize()
    if a.waits_updates:
        e.sac_pop_update(a.waits_updates)
    print(f"measure_sac_population: waits child, M {M}, ran sac_pop_update({a.waits_updates})" if a.waits_updates
          else f"measure_sac_population: waits child, M {M}, ran no further update", flush=True)
    e.close()


def run(script, args, tree, timeout):
    env = dict(os.environ)
    if tree:
        tree = os.path.abspath(tree)
        env["ADCRAFT_HIP_LIB"] = os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so")
        args = args + ["--tree", tree]
    rc = subprocess.run([sys.executable, os.path.join(HERE, "tools", script)] + args, env=env, timeout=timeout).returncode      # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_sac_population: child {script} {args} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="16,64")
    ap.add_argument("--envs", type=int, default=64, help="envs of a member")
    ap.add_argument("--keywords", type=int, default=25)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--critics", default="32,32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="parent / this alternations of the paths that must not have moved")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: the solo reference")
    ap.add_argument("--tree", default=HERE, help="(children) the checkout whose package is measured")
    ap.add_argument("--skip-regress", action="store_true")
    ap.add_argument("--skip-gain", action="store_true")
    ap.add_argument("--child", default=None, choices=["pop", "solo", "waits"])
    ap.add_argument("--shape", default="64x25")
    ap.add_argument("--critic", default="32,32")
    ap.add_argument("--label", default="this")
    ap.add_argument("--waits-updates", type=int, default=64)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        return dict(pop=child_pop, solo=child_solo, waits=child_waits)[a.child](a, int(a.members))
    me, reps = os.path.basename(__file__), ["--reps", str(a.reps)]
    ref = ("parent", a.parent_tree) if a.parent_tree else ("this", None)
    if not a.skip_gain:
        for critic in a.critics.split(";"):
            print(f"gain: {UPDATES} updates of every learner, per member {a.envs} envs x {a.keywords} keywords, batch {a.batch}, critics ({critic}), actor (32, 32); "
                  f"solo: the {ref[0]} build")
            for M in a.members.split(","):
                run(me, ["--child", "solo", "--members", M, "--shape", f"{a.envs}x{a.keywords}", "--critic", critic, "--batch", str(a.batch),
                         "--label", ref[0]] + reps, ref[1], a.child_timeout)
                run(me, ["--child", "pop", "--members", M, "--envs", str(a.envs), "--keywords", str(a.keywords), "--critic", critic,
                         "--batch", str(a.batch)] + reps, None, a.child_timeout)
    if a.skip_regress or not a.parent_tree:
        return
    print(f"paths that must not have moved: the parent's build and this one alternating, {a.rounds} rounds")
    from measure_td3 import parent as bench_and_day
    bench_and_day(a)
    for _ in range(a.rounds):
        for label, tree in (("parent", a.parent_tree), ("this", None)):
            run(me, ["--child", "solo", "--members", "1", "--shape", "1024x25", "--critic", "256,256", "--batch", "256", "--label", label] + reps, tree,
                a.child_timeout)
            print(f"  (td3_pop_update of {label}:)", flush=True)
            run("measure_td3_population.py", ["--child", "pop", "--members", "16", "--envs", "64", "--keywords", "25", "--critic", "32,32", "--batch", "256"] + reps,
                tree, a.child_timeout)


if __name__ == "__main__":
    main()
