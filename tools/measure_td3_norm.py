#!/usr/bin/env python3
"""The TD3 learners' running normalisers, measured (profiles/pr_td3_norm.txt).  Every shape is a child process of its own under a
time limit; the parent process never opens the GPU, and the first child that fails ends the run.

Per shape, in ONE process (the same machine, the same session), two trainers on the same planes, seeds and critics - one with
td3_norm_init(observations, rewards), one without - and, alternating them repeat by repeat after an untimed round.  Every shape
is run twice, once with the "on" trainer built and timed first and once with the "off" trainer first: a difference that follows
the order and not the feature belongs to the two instances (where their buffers lie), not to the normalisers.

  updates on    ms of a call of --updates (default 256) td3_update's with the normalisers on: raw ring rows normalised in the gather, td3_y_norm
  updates off   the same updates without a normaliser.  This is the baseline: the off path computes the parent commit's
                bits with the parent's loads (tests/test_gpu_td3_norm.py, test_gpu_td3_trainer.py), so it stands for the parent
  norm update   ms of one td3_norm_update alone over a freshly collected record (five launches), ended by a synchronise

Host clock around synchronised calls; repeats, minimum, median and spread (max - min) for each.

  pop    64 envs x 25 keywords x 16 learners (4 envs each), critics (32, 32), per-member normalisers
  solo   4096 envs x 256 keywords, one learner, critics (256, 256), a shared normaliser

    python tools/measure_td3_norm.py [--shapes pop,solo] [--reps 7] [--days 10] [--batch 256] [--updates 256]
Kernel shares: rocprofv3 --kernel-trace --stats -- python tools/measure_td3_norm.py --child solo (a run of its own).
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SHAPES = dict(pop=(64, 25, 16, (32, 32)), solo=(4096, 256, 1, (256, 256)))
BUDGET = 100000.0


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def trainer(N, K, M, critic, days, batch, normalise):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.td3_trainer import TD3PopulationTrainer, TD3Trainer, td3
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    cfg = td3(critic_hidden=critic, batch_size=batch, capacity=4 * days * (N // M), learning_starts=1 << 40, reward_scale=0.1, seed=3)
    pol = default_policy(K, hidden=(32, 32), days=days)
    norm = dict(normalize_observations=normalise, normalize_rewards=normalise)
    if M == 1:
        return e, TD3Trainer(e, pol, horizon=days, **norm, **cfg)
    sigma = cfg.pop("exploration_sigma")
    return e, TD3PopulationTrainer(e, pol, sigma, cfg, horizon=days, members=M, **norm)


def child(a, name):
    N, K, M, critic = SHAPES[name]
    pop = M > 1
    pair = {label: trainer(N, K, M, critic, a.days, a.batch, label == "on") for label in a.order.split(",")}
    rows = {k: [] for k in ("updates on", "updates off", "norm update")}
    for rep in range(a.reps + 1):
        t = {}
        for label, (e, tr) in pair.items():
            e.reset()
            e.rollout_reset()
            e.run_days("mlp", a.days, BUDGET)
            (e.td3_pop_store if pop else e.td3_store)()
            if label == "on":
                t["norm update"] = timed(e.td3_norm_update, e.synchronize)
            upd = (lambda e=e: e.td3_pop_update(a.updates, stats=False)) if pop else (lambda e=e: e.td3_update(a.updates))
            t["updates " + label] = timed(upd, e.synchronize)
        if rep:
            for k, v in t.items():
                rows[k].append(v)
    for e, _ in pair.values():
        e.close()
    print(f"{name}: {N} envs x {K} keywords x {M} learner(s), critics {critic}, actor (32, 32), batch {a.batch}, {a.days} recorded days per repeat, "
          f"{'per-member' if pop else 'shared'} normalisers, built and timed in the order {a.order}; ms per call of {a.updates} updates, "
          f"{a.reps} repeats after an untimed round")
    for k, v in rows.items():
        print(f"  {k:12s} " + " ".join(f"{x:9.4f}" for x in v) + f"   (min {min(v):.4f}, median {np.median(v):.4f}, spread {max(v) - min(v):.4f})", flush=True)
    d = np.median(rows["updates on"]) - np.median(rows["updates off"])
    s = max(max(rows[k]) - min(rows[k]) for k in ("updates on", "updates off"))
    print(f"  {a.updates} updates, on - off (medians): {d:+.4f} ms = {d / a.updates * 1e3:+.2f} us per update; the larger run-to-run spread of the two: {s:.4f} ms "
          f"({'inside' if abs(d) <= s else 'OUTSIDE'} the spread)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="pop,solo")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--updates", type=int, default=256, help="td3_update's in a timed call")
    ap.add_argument("--order", default="on,off", choices=["on,off", "off,on"], help="(child) which trainer is built and timed first")
    ap.add_argument("--child", default=None, choices=sorted(SHAPES))
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        return child(a, a.child)
    for name in a.shapes.split(","):
        for order in ("on,off", "off,on"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--order", order, "--reps", str(a.reps), "--days", str(a.days),
                   "--batch", str(a.batch), "--updates", str(a.updates)]
            rc = subprocess.run(cmd, timeout=a.child_timeout).returncode                # (a timeout raises: nothing more is started)
            if rc != 0:
                sys.exit(f"measure_td3_norm: child {name} {order} ended with status {rc}; stopping")


if __name__ == "__main__":
    main()
