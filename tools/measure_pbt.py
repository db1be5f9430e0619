#!/usr/bin/env python3
"""The population-based training scheduler measured (profiles/pr_pbt.txt).  Every measurement is a child process of its own
under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  new      ms of one StepEngine.pbt_step(): the fitness from the record on the device, the plan, the batched exploit, the
           explore, one wait at the end
  parent   ms of the same round through the parent commit's own primitives - with --parent-tree (a checkout of the parent
           commit, its library built) the parent's package and library: the record's reward array alone fetched to the host
           and summed there (not the full-record returns()), then q copies (pg_pop_copy / td3_pop_copy) and q set_configs

Both on M members of `envs` envs x K keywords each, T recorded days, q = M / 4, hidden (32, 32); TD3: critics (32, 32), a ring
of --capacity transitions, without and with the ring.  Host clock around synchronised calls, after an untimed round.

    python tools/measure_pbt.py [--members 16,64] [--envs 64] [--keywords 25] [--days 32] [--capacity 4096] [--reps 7]
                                [--parent-tree DIR [--rounds 3]]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child measures the package of --tree: this checkout's, or the parent's)
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE
sys.path.insert(0, TREE)
HIDDEN = (32, 32)


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def line(label, v):
    print(f"  {label:58s} ms " + " ".join(f"{x:8.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, spread {max(v) - min(v):.3f})",
          flush=True)


def population(a, M):
    """the engine with a live population trainer and a full record; the members' configuration dicts"""
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    N, K = M * a.envs, a.keywords
    e = eng.StepEngine(N, K, seed=7, max_days=a.days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    pol = default_policy(K, hidden=HIDDEN, days=a.days, seed=0)
    if a.kind == "pg":
        rng = np.random.default_rng(1)
        layers, n_in = [], 5 * K + 2
        for n_out in list(HIDDEN) + [1]:
            b = 1.0 / np.sqrt(n_in)
            layers.append((rng.uniform(-b, b, (n_in, n_out)).astype(np.float32), rng.uniform(-b, b, n_out).astype(np.float32)))
            n_in = n_out
        pol.value_layers = layers
    e.mlp_init(pol, deterministic=False)
    e.mlp_learners(M)
    e.rollout_enable(a.days, obs=True)
    if a.kind == "pg":
        cfgs = [dict(lr=float(np.float32(lr))) for lr in np.logspace(-5, -2, M)]
        e.pg_pop_init(cfgs)
    else:
        cfgs = [dict(critic_widths=HIDDEN + (1,), batch_size=256, capacity=a.capacity, actor_lr=float(np.float32(lr)), reward_scale=0.1, seed=3)
                for lr in np.logspace(-5, -2, M)]
        e.td3_pop_init(cfgs)
    e.run_days("mlp", a.days, 100000.0)
    if a.kind == "td3":
        e.td3_pop_store()
    return e, cfgs


def child_new(a, M):
    e, _ = population(a, M)
    name = "lr" if a.kind == "pg" else "actor_lr"
    e.pbt_init(a.kind, replace_count=M // 4, tuned=(name,), bounds={name: (1e-6, 1e-1)}, with_ring=bool(a.with_ring))
    rows = []
    for rep in range(a.reps + 1):
        t = timed(e.pbt_step, e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"new    {a.kind} ring {a.with_ring} M {M:3d} x {a.envs} x {a.keywords} T {a.days} q {M // 4}", rows)


def child_parent(a, M):
    """the round as a host loop over the primitives the parent commit has"""
    e, cfgs = population(a, M)
    q, N, name = M // 4, M * a.envs, "lr" if a.kind == "pg" else "actor_lr"
    reward, days = np.zeros((a.days, N), np.float32), C.c_int32(0)
    lib, h = e._lib, e._h

    def one_round():
        rc = lib.adc_engine_rollout_fetch(h, C.byref(days), None, None, None, reward.ctypes.data, None, None, None)
        assert rc == 0, rc
        f = reward[:days.value].astype(np.float64).sum(axis=0).reshape(M, -1).mean(axis=1)
        order = np.argsort(f, kind="stable")
        for dst, src in zip(order[:q], order[M - q:]):
            dst, src = int(dst), int(src)
            if a.kind == "pg":
                e.pg_pop_copy(src, dst)
            else:
                e.td3_pop_copy(src, dst, with_ring=bool(a.with_ring))
            cfgs[dst] = dict(cfgs[dst], **{name: min(max(cfgs[src][name] * 1.25, 1e-6), 1e-1)})
            (e.pg_pop_set_config if a.kind == "pg" else e.td3_pop_set_config)(dst, **cfgs[dst])
    rows = []
    for rep in range(a.reps + 1):
        t = timed(one_round, e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"parent {a.kind} ring {a.with_ring} M {M:3d} x {a.envs} x {a.keywords} T {a.days} q {q} ({a.label})", rows)


def run(args, tree, timeout):
    env = dict(os.environ)
    if tree:
        tree = os.path.abspath(tree)
        env["ADCRAFT_HIP_LIB"] = os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so")
        args = args + ["--tree", tree]
    rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, timeout=timeout).returncode       # (a timeout raises: nothing more is started)
    if rc != 0:
        sys.exit(f"measure_pbt: child {args} ended with status {rc}; stopping")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="16,64")
    ap.add_argument("--envs", type=int, default=64, help="envs of a member")
    ap.add_argument("--keywords", type=int, default=25)
    ap.add_argument("--days", type=int, default=32)
    ap.add_argument("--capacity", type=int, default=4096, help="TD3: transitions of a member's ring")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="parent / new alternations")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: the yardstick's package")
    ap.add_argument("--tree", default=HERE, help="(children) the checkout whose package is measured")
    ap.add_argument("--child", default=None, choices=["new", "parent"])
    ap.add_argument("--kind", default="pg", choices=["pg", "td3"])
    ap.add_argument("--with-ring", type=int, default=0)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child == "new":
        return child_new(a, int(a.members))
    if a.child == "parent":
        return child_parent(a, int(a.members))
    common = ["--envs", str(a.envs), "--keywords", str(a.keywords), "--days", str(a.days), "--capacity", str(a.capacity), "--reps", str(a.reps)]
    print(f"one PBT round: per member {a.envs} envs x {a.keywords} keywords, T {a.days}, q = M / 4, hidden {HIDDEN}; TD3: critics {HIDDEN}, capacity {a.capacity}")
    for kind, ring in (("pg", 0), ("td3", 0), ("td3", 1)):
        for M in a.members.split(","):
            for _ in range(a.rounds):
                shape = ["--kind", kind, "--with-ring", str(ring), "--members", M] + common
                run(["--child", "parent", "--label", "parent's tree" if a.parent_tree else "this tree"] + shape, a.parent_tree, a.child_timeout)
                run(["--child", "new"] + shape, None, a.child_timeout)


if __name__ == "__main__":
    main()
