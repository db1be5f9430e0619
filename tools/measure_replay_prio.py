#!/usr/bin/env python3
"""Prioritised replay, measured (profiles/pr_replay_prio.txt).  Every shape is a child process of its own under a time limit; the
parent process never opens the GPU, and the first child that fails ends the run.

Per shape, in ONE process (the same machine, the same session), two trainers on the same planes, seeds and critics - one with
prioritized_replay, one without - alternating repeat by repeat after an untimed round.  Every shape is run twice, once with the
"on" trainer built and timed first and once with the "off" trainer first: a difference that follows the order and not the feature
belongs to the two instances (where their buffers lie), not to the add-on.

  updates on    ms of a call of --updates (default 64) updates with prioritised replay: the tree's sample, the weights, the weighted
                critics' pass, the priorities, the leaves, the rebuild of the touched nodes
  updates off   the same updates without the add-on (uniform batch indices)
  store on/off  ms of one store of the freshly collected record, ended by a synchronise; on: plus leaf = top over the stored range
                and the rebuild of the nodes above it

Host clock around synchronised calls; repeats, minimum, median and spread (max - min) for each.

  pop    64 envs x 25 keywords x 16 TD3 learners (4 envs each), critics (32, 32), batch 256, capacity 4096
  solo   64 envs x 25 keywords, one TD3 learner, critics (32, 32), batch 2048, capacity 1 000 000 (the ring filled to the brim with
         loaded rows before the first repeat, so that every level of the tree is as wide as it gets)

    python tools/measure_replay_prio.py [--shapes pop,solo] [--reps 7] [--days 10] [--updates 64]
--root DIR --order off: the "off" trainer alone from another checkout's package and library (the parent commit's), for the same
table.  The launches of an update, on and off: rocprofv3 --kernel-trace --stats -- python tools/measure_replay_prio.py --child pop
--order on (then --order off), runs of their own: every kernel's calls over the updates of the run (--reps + 1 calls of --updates).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# envs, keywords, learners, critics, batch, capacity
SHAPES = dict(pop=(64, 25, 16, (32, 32), 256, 4096), solo=(64, 25, 1, (32, 32), 2048, 1000000))
BUDGET = 100000.0
PRIO = dict(alpha=0.6, beta=0.4, eps=1e-6, cap=1e6)


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def trainer(name, days, on):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer, TD3Trainer, td3
    N, K, M, critic, batch, capacity = SHAPES[name]
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    cfg = td3(critic_hidden=critic, batch_size=batch, capacity=capacity, learning_starts=1 << 40, reward_scale=0.1, seed=3)
    pol = default_policy(K, hidden=(32, 32), days=days)
    extra = dict(prioritized_replay=PRIO) if on else {}
    if M == 1:
        tr = TD3Trainer(e, pol, horizon=days, **extra, **cfg)
        # the ring to the brim: the same 50 000 random rows, twenty times
        rng = np.random.default_rng(5)
        D, A, rows = 5 * K + 2, K + 1, 50000
        chunk = dict(x=rng.standard_normal((rows, D), np.float32), a=rng.standard_normal((rows, A), np.float32), r=rng.standard_normal(rows, np.float32),
                     done=rng.random(rows) < 0.1, x2=rng.standard_normal((rows, D), np.float32))
        for slot in range(0, capacity, rows):
            e.td3_buffer_load(chunk, slot=slot, written=slot + rows)
        return e, tr
    sigma = cfg.pop("exploration_sigma")
    return e, TD3PopulationTrainer(e, pol, sigma, cfg, horizon=days, members=M, **extra)


def child(a, name):
    N, K, M, critic, batch, capacity = SHAPES[name]
    pop = M > 1
    pair = {label: trainer(name, a.days, label == "on") for label in a.order.split(",")}
    rows = {f"{what} {label}": [] for what in ("updates", "store") for label in pair}
    for rep in range(a.reps + 1):
        t = {}
        for label, (e, tr) in pair.items():
            e.reset()
            e.rollout_reset()
            e.run_days("mlp", a.days, BUDGET)
            t["store " + label] = timed(e.td3_pop_store if pop else e.td3_store, e.synchronize)
            upd = (lambda e=e: e.td3_pop_update(a.updates, stats=False)) if pop else (lambda e=e: e.td3_update(a.updates))
            t["updates " + label] = timed(upd, e.synchronize)
        if rep:
            for k, v in t.items():
                rows[k].append(v)
    info = ""
    if "on" in pair:
        e = pair["on"][0]
        info = f"; the tree of member 0 after the run: total {e.replay_prio_info(0)['total']:.6g}, top {e.replay_prio_info(0)['top']:.6g}"
    for e, _ in pair.values():
        e.close()
    print(f"{name}: {N} envs x {K} keywords x {M} learner(s), critics {critic}, actor (32, 32), batch {batch}, capacity {capacity}, {a.days} recorded days "
          f"per repeat, built and timed in the order {a.order}, package {os.path.relpath(a.root)}; ms per call ({a.updates} updates; one store of "
          f"{a.days * (N // M)} transitions per learner), {a.reps} repeats after an untimed round{info}")
    for k, v in rows.items():
        print(f"  {k:12s} " + " ".join(f"{x:9.4f}" for x in v) + f"   (min {min(v):.4f}, median {np.median(v):.4f}, spread {max(v) - min(v):.4f})", flush=True)
    if len(pair) == 2:
        for what, per in (("updates", a.updates), ("store", 1)):
            d = np.median(rows[what + " on"]) - np.median(rows[what + " off"])
            s = max(max(rows[what + " " + k]) - min(rows[what + " " + k]) for k in ("on", "off"))
            print(f"  {what}, on - off (medians): {d:+.4f} ms = {d / per * 1e3:+.2f} us per {'update' if per > 1 else 'store'}; the larger run-to-run "
                  f"spread of the two: {s:.4f} ms ({'inside' if abs(d) <= s else 'OUTSIDE'} the spread)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="pop,solo")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--updates", type=int, default=64, help="updates in a timed call")
    ap.add_argument("--order", default=None, choices=["on,off", "off,on", "on", "off"], help="which trainers are built, and which first (default: both orders)")
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are measured")
    ap.add_argument("--child", default=None, choices=sorted(SHAPES))
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    a.root = os.path.abspath(a.root)
    if a.child:
        sys.path.insert(0, a.root)
        return child(a, a.child)
    for name in a.shapes.split(","):
        for order in ([a.order] if a.order else ["on,off", "off,on"]):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--order", order, "--reps", str(a.reps), "--days", str(a.days),
                   "--updates", str(a.updates), "--root", a.root]
            rc = subprocess.run(cmd, timeout=a.child_timeout).returncode                # (a timeout raises: nothing more is started)
            if rc != 0:
                sys.exit(f"measure_replay_prio: child {name} {order} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
