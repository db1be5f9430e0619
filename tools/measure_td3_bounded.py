#!/usr/bin/env python3
"""The bounded act and bounded TD3, measured (profiles/pr_td3_bounded.txt).  Every GPU measurement is a child process of its own
under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

  --resources PARENT.txt THIS.txt   needs no GPU: two builds' `-Rpass-analysis=kernel-resource-usage` remarks (the parent
            commit's and this one's: `python -c "from adcraft_amd import build; build.build(force=True,
            extra=['-Rpass-analysis=kernel-resource-usage'])" 2> FILE` in either tree), kernel by kernel: VGPRs, SGPRs, LDS, scratch,
            occupancy.  k_mlp_policy's instantiations are matched over the template parameter this feature added (its default).
  act       a recorded run_days("mlp") day at 4096 x 256, policy (32, 32): unbounded, bounded (gaussian), bounded (random)
  update    td3_update(64) at 4096 x 256, batch 2048, critics (256, 256), and a population of 16 learners x 64 envs x 25
            keywords, batch 256, critics (32, 32): ms per update, unbounded against bounded
            Host clock around synchronised calls after an untimed round; the variants alternate inside ONE child per shape (their
            engines live side by side), so that every pair is taken in the same session; medians of --reps (default 10) with max - min.
  --learning  examples/train_mlp_policy_td3.py on its default law, unbounded and --bounded 0.01,3, at --actor-lr 1e-3 and 1e-5:
            the same seeds, one run each, the printed tables as found

    python tools/measure_td3_bounded.py [--reps 10] [--learning] [--iterations 100]
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = 0.01, 3.0


# ---- resource usage (no GPU) ----------------------------------------------------------------------------------------------------------
def parse_remarks(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: (?:[^:]*:\d+:\d+: )?Function Name: (\S+)", line)
        if m:
            cur = re.sub(r"(k_mlp_policyILi\dELb\dELb\d)EE", r"\1ELb0EE", m.group(1))      # (the added template parameter at its default)
            out[cur] = {}
            continue
        m = re.search(r"remark: (?:[^:]*:\d+:\d+: )?\s*([A-Za-z][A-Za-z /\[\]-]*?): (\S+)", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def resources(parent, this):
    a, b = parse_remarks(parent), parse_remarks(this)
    print(f"kernels: {len(a)} in the parent's build, {len(b)} in this one")
    gone = [k for k in a if k not in b]
    moved = [k for k in a if k in b and a[k] != b[k]]
    print(f"of the parent's kernels: {len(gone)} gone, {len(moved)} with another VGPR / SGPR / LDS / scratch / occupancy figure")
    for k in gone:
        print("  gone ", k)
    for k in moved:
        print("  moved", k, {f: (a[k][f], b[k].get(f)) for f in a[k] if a[k][f] != b[k].get(f)})
    print("new kernels:")
    for k in b:
        if k not in a:
            r = b[k]
            print(f"  {k}\n      VGPRs {r.get('VGPRs')}  SGPRs {r.get('TotalSGPRs')}  SGPR spills {r.get('SGPRs Spill')}  VGPR spills {r.get('VGPRs Spill')}  "
                  f"scratch {r.get('ScratchSize [bytes/lane]')}  LDS {r.get('LDS Size [bytes/block]')}  occupancy {r.get('Occupancy [waves/SIMD]')}")
    return 1 if gone or moved else 0


# ---- the children ---------------------------------------------------------------------------------------------------------------------
def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def report(what, variant, v):
    print(f"  {what:34s} {variant:18s} ms  median {np.median(v):9.4f}  max - min {max(v) - min(v):8.4f}   " + " ".join(f"{x:.4f}" for x in v), flush=True)


def engine_of(eng, synthetic, N, K, days):
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    return e


def child_solo(reps):
    sys.path.insert(0, HERE)
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.td3_trainer import TD3Trainer, td3
    N, K, days = 4096, 256, 10
    common = dict(critic_hidden=(256, 256), batch_size=2048, capacity=2 * days * N, learning_starts=1 << 40, reward_scale=0.1, seed=3, horizon=days)
    variants = {}
    for name, extra in (("unbounded", {}), ("bounded", dict(action_bounds=(LO, HI)))):
        e = engine_of(eng, synthetic, N, K, days)
        TD3Trainer(e, default_policy(K, hidden=(32, 32), days=days), **td3(**common), **extra)
        variants[name] = e
    day = {"unbounded": [], "bounded gaussian": [], "bounded random": []}
    upd = {"unbounded": [], "bounded": []}
    for rep in range(reps + 1):
        for name, e in variants.items():
            e.reset()
            e.rollout_reset()
            e.run_days("mlp", 1, 100000.0)              # (the first day's input is the zero row: not timed)
            modes = ("gaussian", "random") if name == "bounded" else (None,)
            for mode in modes:
                if mode:
                    e.mlp_set_explore(mode)
                t = timed(lambda: e.run_days("mlp", 4, 100000.0), e.synchronize) / 4
                if rep:
                    day[name if mode is None else "bounded " + mode].append(t)
            if name == "bounded":
                e.mlp_set_explore("gaussian")
            e.td3_store()
            t = timed(lambda: e.td3_update(64), e.synchronize) / 64
            if rep:
                upd[name].append(t)
    for k, v in day.items():
        report("recorded mlp day 4096x256 (32,32)", k, v)
    for k, v in upd.items():
        report("td3_update(64) 4096x256 b2048 (256,256)", k, v)
    for e in variants.values():
        e.close()


def child_pop(reps):
    sys.path.insert(0, HERE)
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer
    M, n, K, days = 16, 64, 25, 10
    cfg = dict(critic_hidden=(32, 32), batch_size=256, capacity=4 * days * n, learning_starts=1 << 40, updates_per_iteration=64, reward_scale=0.1, seed=3)
    variants = {}
    for name, extra in (("unbounded", {}), ("bounded", dict(action_bounds=(LO, HI)))):
        e = engine_of(eng, synthetic, M * n, K, days)
        TD3PopulationTrainer(e, default_policy(K, hidden=(32, 32), days=days), 0.1, cfg, horizon=days, members=M, **extra)
        variants[name] = e
    upd = {k: [] for k in variants}
    for rep in range(reps + 1):
        for name, e in variants.items():
            e.reset()
            e.rollout_reset()
            e.run_days("mlp", days, 100000.0)
            e.td3_pop_store()
            t = timed(lambda: e.td3_pop_update(64, stats=False), e.synchronize) / 64
            if rep:
                upd[name].append(t)
    for k, v in upd.items():
        report("td3_pop_update(64) 16x64x25 b256 (32,32)", k, v)
    for e in variants.values():
        e.close()


def run_child(args, limit):
    r = subprocess.run([sys.executable] + args, cwd=HERE, timeout=limit)
    if r.returncode != 0:
        print(f"a child ended with status {r.returncode}: nothing more is started", flush=True)
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", nargs=2, metavar=("PARENT.txt", "THIS.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--child", choices=["solo", "pop"])
    a = ap.parse_args()
    if a.resources:
        sys.exit(resources(*a.resources))
    if a.child:
        (child_solo if a.child == "solo" else child_pop)(a.reps)
        return
    me = os.path.abspath(__file__)
    print(f"medians of {a.reps}, bounded and unbounded alternated in one process per shape; box [{LO}, {HI}]", flush=True)
    run_child([me, "--child", "solo", "--reps", str(a.reps)], 420)
    run_child([me, "--child", "pop", "--reps", str(a.reps)], 300)
    if a.learning:
        ex = os.path.join(HERE, "examples", "train_mlp_policy_td3.py")
        for lr in ("1e-3", "1e-5"):
            for bounded in ([], ["--bounded", f"{LO},{HI}"]):
                print(f"\nexamples/train_mlp_policy_td3.py --actor-lr {lr} --iterations {a.iterations} " + " ".join(bounded), flush=True)
                run_child([ex, "--actor-lr", lr, "--iterations", str(a.iterations)] + bounded, 600)


if __name__ == "__main__":
    main()
