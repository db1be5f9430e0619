#!/usr/bin/env python3
"""Population-based training over SAC learner populations measured (profiles/pr_pbt_sac.txt).  Every measurement is a child
process of its own under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  new      ms of one StepEngine.pbt_step() of kind "sac": the fitness from the record on the device, the plan, the batched exploit
           (actor, critics, target critics, temperature cells and, with the ring, the five ring arrays), the explore, one wait at
           the end; actor_lr and alpha tuned
  parent   ms of the same round through the primitives the parent commit has - with --parent-tree (a checkout of the parent
           commit, its library built) the parent's package and library: the record's reward array alone fetched to the host and
           summed there, then q sac_pop_copy, q sac_pop_set_config and q sac_pop_state get / set for the temperature
  waits    set-up and one round, then --waits-rounds further rounds, alone in a process: run it under a HIP-API trace with 1 and
           with 0; the difference of the two traces' calls is what a round launches and waits for
  regress  the paths that must not have moved, the parent's build and this one alternating: bench.py and its dumped outputs
           (tools/measure_td3.py's), one solo sac_update(64) and one sac_pop_update(64) (tools/measure_sac_population.py's
           children) and one TD3 PBT round with the ring (tools/measure_pbt.py's child)

Per member `envs` envs x K keywords, T recorded days, q = M / 4, actor (32, 32), critics (32, 32), batch 256, a ring of
--capacity transitions, without and with the ring.  Host clock around synchronised calls, after an untimed round.  A gain is
stated only where the new round's slowest repeat lies below the parent sequence's fastest; otherwise "inside the spread".

    python tools/measure_pbt_sac.py [--members 16,64] [--envs 64] [--keywords 25] [--days 32] [--capacity 4096] [--reps 10]
                                    [--parent-tree DIR [--rounds 3]] [--skip-regress] [--skip-gain]
Launch and wait counts: rocprofv3 --hip-trace --stats -- python tools/measure_pbt_sac.py --child waits --members 16 --with-ring 1
--waits-rounds 1, and again with --waits-rounds 0 (runs of their own, nothing else collected); the same at --members 64.
"""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child measures the package of --tree: this checkout's, or the parent's)
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(HERE, "tools"))
HIDDEN = (32, 32)
LR, ALPHA = (1e-6, 1e-1), (0.01, 10.0)


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def line(label, v):
    print(f"  {label:62s} ms " + " ".join(f"{x:8.3f}" for x in v) + f"   (min {min(v):.3f}, median {np.median(v):.3f}, max {max(v):.3f}, "
          f"spread {max(v) - min(v):.3f})", flush=True)


def population(a, M):
    """the trainer over an engine with a full record and a stored ring"""
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.sac_trainer import SACPopulationTrainer, sac
    from measure_sac_population import bounds, sac_policy
    N, K = M * a.envs, a.keywords
    e = eng.StepEngine(N, K, seed=7, max_days=a.days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    cfgs = [sac(K, critic_hidden=HIDDEN, batch_size=256, capacity=a.capacity, learning_starts=1 << 40, reward_scale=0.1, seed=3,
                actor_lr=float(np.float32(lr)), alpha_lr=0.0 if m % 2 else 3e-4) for m, lr in enumerate(np.logspace(-5, -2, M))]
    tr = SACPopulationTrainer(e, sac_policy(K), cfgs, *bounds(K), horizon=a.days, members=M)
    e.run_days("mlp", a.days, 100000.0)
    e.sac_pop_store()
    return tr


def child_new(a, M):
    e = population(a, M).engine
    e.pbt_init("sac", replace_count=M // 4, tuned=("actor_lr", "alpha"), bounds={"actor_lr": LR, "alpha": ALPHA}, with_ring=bool(a.with_ring))
    rows = []
    for rep in range(a.reps + 1):
        t = timed(e.pbt_step, e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"new    sac ring {a.with_ring} M {M:3d} x {a.envs} x {a.keywords} T {a.days} q {M // 4}", rows)


def child_parent(a, M):
    """the round as a host loop over the primitives the parent commit has"""
    tr = population(a, M)
    e, q, N = tr.engine, M // 4, M * a.envs
    reward, days = np.zeros((a.days, N), np.float32), C.c_int32(0)
    lib, h = e._lib, e._h
    lo, hi, shift = np.float32(np.log(ALPHA[0])), np.float32(np.log(ALPHA[1])), np.float32(np.log(1.25))

    def one_round():
        rc = lib.adc_engine_rollout_fetch(h, C.byref(days), None, None, None, reward.ctypes.data, None, None, None)
        assert rc == 0, rc
        f = reward[:days.value].astype(np.float64).sum(axis=0).reshape(M, -1).mean(axis=1)
        order = np.argsort(f, kind="stable")
        for dst, src in zip(order[:q], order[M - q:]):
            dst, src = int(dst), int(src)
            e.sac_pop_copy(src, dst, with_ring=bool(a.with_ring))
            tr.set_config(dst, actor_lr=min(max(tr.configs[src]["actor_lr"] * 1.25, LR[0]), LR[1]))
            st = e.sac_pop_state(dst)
            st["log_alpha"][0] = min(max(np.float32(st["log_alpha"][0] + shift), lo), hi)
            e.sac_pop_state(dst, st)
    rows = []
    for rep in range(a.reps + 1):
        t = timed(one_round, e.synchronize)
        if rep:
            rows.append(t)
    e.close()
    line(f"parent sac ring {a.with_ring} M {M:3d} x {a.envs} x {a.keywords} T {a.days} q {q} ({a.label})", rows)


def child_waits(a, M):
    e = population(a, M).engine
    e.pbt_init("sac", replace_count=M // 4, tuned=("actor_lr", "alpha"), bounds={"actor_lr": LR, "alpha": ALPHA}, with_ring=bool(a.with_ring))
    e.pbt_step()
    e.synchronize()
    for _ in range(a.waits_rounds):
        e.pbt_step()
    print(f"measure_pbt_sac: waits child, M {M}, ring {a.with_ring}, ran {a.waits_rounds} further round(s)", flush=True)
    e.close()


def run(script, args, tree, timeout, capture=False):
    env = dict(os.environ)
    if tree:
        tree = os.path.abspath(tree)
        env["ADCRAFT_HIP_LIB"] = os.path.join(tree, "adcraft_amd", "lib", "libadcraft_hip.so")
        args = args + ["--tree", tree]
    out = subprocess.run([sys.executable, os.path.join(HERE, "tools", script)] + args, env=env, timeout=timeout, capture_output=capture,
                         text=True)      # (a timeout raises: nothing more is started)
    if capture:
        sys.stdout.write(out.stdout)
        sys.stdout.flush()
    if out.returncode != 0:
        sys.exit(f"measure_pbt_sac: child {script} {args} ended with status {out.returncode}; stopping")
    return out.stdout if capture else ""


def figures(text):
    """(min, max) of a child's line of repeats"""
    m = re.search(r"\(min ([0-9.]+), median ([0-9.]+), max ([0-9.]+)", text)
    return float(m.group(1)), float(m.group(2)), float(m.group(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="16,64")
    ap.add_argument("--envs", type=int, default=64, help="envs of a member")
    ap.add_argument("--keywords", type=int, default=25)
    ap.add_argument("--days", type=int, default=32)
    ap.add_argument("--capacity", type=int, default=4096, help="transitions of a member's ring")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="parent / this alternations of the paths that must not have moved")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: the yardstick's package")
    ap.add_argument("--tree", default=HERE, help="(children) the checkout whose package is measured")
    ap.add_argument("--skip-regress", action="store_true")
    ap.add_argument("--skip-gain", action="store_true")
    ap.add_argument("--child", default=None, choices=["new", "parent", "waits"])
    ap.add_argument("--with-ring", type=int, default=0)
    ap.add_argument("--waits-rounds", type=int, default=1)
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        return dict(new=child_new, parent=child_parent, waits=child_waits)[a.child](a, int(a.members))
    me = os.path.basename(__file__)
    common = ["--envs", str(a.envs), "--keywords", str(a.keywords), "--days", str(a.days), "--capacity", str(a.capacity), "--reps", str(a.reps)]
    if not a.skip_gain:
        print(f"one PBT round over SAC: per member {a.envs} envs x {a.keywords} keywords, T {a.days}, q = M / 4, actor {HIDDEN}, critics {HIDDEN}, "
              f"batch 256, capacity {a.capacity}; medians of {a.reps}")
        for ring in (0, 1):
            for M in a.members.split(","):
                shape = ["--with-ring", str(ring), "--members", M] + common
                old = figures(run(me, ["--child", "parent", "--label", "parent's tree" if a.parent_tree else "this tree"] + shape, a.parent_tree,
                                  a.child_timeout, capture=True))
                new = figures(run(me, ["--child", "new"] + shape, None, a.child_timeout, capture=True))
                verdict = (f"gain: the new round's slowest repeat {new[2]:.3f} lies below the parent sequence's fastest {old[0]:.3f}; medians "
                           f"{old[1]:.3f} -> {new[1]:.3f} ms ({old[1] / new[1]:.1f}x)") if new[2] < old[0] else "inside the spread"
                print(f"    ring {ring} M {M}: {verdict}", flush=True)
    if a.skip_regress or not a.parent_tree:
        return
    print(f"paths that must not have moved: the parent's build and this one alternating, {a.rounds} rounds")
    from measure_td3 import parent as bench_and_day
    bench_and_day(a)
    reps = ["--reps", str(a.reps)]
    for _ in range(a.rounds):
        for label, tree in (("parent", a.parent_tree), ("this", None)):
            run("measure_sac_population.py", ["--child", "solo", "--members", "1", "--shape", "1024x25", "--critic", "256,256", "--batch", "256",
                                              "--label", label] + reps, tree, a.child_timeout)
            print(f"  (sac_pop_update of {label}:)", flush=True)
            run("measure_sac_population.py", ["--child", "pop", "--members", "64", "--envs", "64", "--keywords", "25", "--critic", "32,32", "--batch", "256"] + reps,
                tree, a.child_timeout)
            print(f"  (a TD3 PBT round of {label}:)", flush=True)
            run("measure_pbt.py", ["--child", "new", "--kind", "td3", "--with-ring", "1", "--members", "64"] + reps, tree, a.child_timeout)


if __name__ == "__main__":
    main()
