#!/usr/bin/env python3
"""The SAC learners' running normalisers, measured (profiles/pr_sac_norm.txt).  Every measurement is a child process of its own
under a time limit; the parent process never opens the GPU, and the first child that fails ends the run.

Per shape, in ONE process (the same machine, the same session), two trainers on the same planes, seeds and critics - one with
sac_norm_init(observations, rewards), one without - alternating repeat by repeat after an untimed round.  Every shape is run
twice, once with the "on" trainer built and timed first and once with the "off" trainer first: a difference that follows the order
and not the feature belongs to the two instances (where their buffers lie), not to the normalisers.

  updates on    ms of a call of --updates (default 256) sac_update's with the normalisers on: raw ring rows normalised in the
                gather, sac_y_norm
  updates off   the same updates without a normaliser
  norm update   ms of one sac_norm_update alone over a freshly collected record (five launches), ended by a synchronise

With --parent-tree DIR (a checkout of the parent commit with its library built in the same session): "updates off" alone, of this
checkout and of the parent, each in a process of its own run from its own tree, alternating for --rounds rounds (which tree goes first alternates
from round to round); and bench.py's headline of both trees in the same order.  The off path has to equal the parent's inside the run-to-run spread printed next to it.

Host clock around synchronised calls; repeats, minimum, median and spread (max - min) for each.

  pop    64 envs x 25 keywords x 16 learners (4 envs each), critics (32, 32), per-member normalisers
  solo   4096 envs x 256 keywords, one learner, critics (256, 256), a shared normaliser

    python tools/measure_sac_norm.py [--shapes pop,solo] [--reps 7] [--days 10] [--batch 256] [--updates 256]
                                     [--parent-tree DIR [--rounds 4] [--bench-steps 200]]
Kernel shares: rocprofv3 --kernel-trace --stats -- python tools/measure_sac_norm.py --child solo (a run of its own).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = dict(pop=(64, 25, 16, (32, 32)), solo=(4096, 256, 1, (256, 256)))
BUDGET = 100000.0


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def sac_policy(K, days):
    from adcraft_amd.baselines.es_trainer import default_policy
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    base = default_policy(K, hidden=(32, 32), days=days)
    rng, A = np.random.default_rng(0), K + 1
    w, _ = base.layers[-1]
    last = (np.concatenate([w, (rng.standard_normal(w.shape) * 0.01).astype(np.float32)], axis=1),
            np.concatenate([np.zeros(A, np.float32), np.full(A, -1.0, np.float32)]))
    return MLPPolicy(list(base.layers[:-1]) + [last], activation="tanh", shift=base.shift, scale=base.scale, log_std_clamp=(-5.0, 1.0))


def trainer(N, K, M, critic, days, batch, normalise):
    import adcraft_amd.engine as eng
    from adcraft_amd import synthetic
    from adcraft_amd.baselines.sac_trainer import SACPopulationTrainer, SACTrainer, sac
    e = eng.StepEngine(N, K, seed=7, max_days=days)
    e.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=8.0))
    e.reset()
    cfg = sac(K, critic_hidden=critic, batch_size=batch, capacity=4 * days * (N // M), learning_starts=1 << 40, reward_scale=0.1, seed=3)
    lo, hi = np.full(K + 1, 0.01, np.float32), np.full(K + 1, 3.0, np.float32)
    # (the keywords are passed only when on: the off trainer is built by the very call a tree without the feature accepts)
    norm = dict(normalize_observations=True, normalize_rewards=True) if normalise else {}
    if M == 1:
        return e, SACTrainer(e, sac_policy(K, days), lo, hi, horizon=days, **norm, **cfg)
    return e, SACPopulationTrainer(e, sac_policy(K, days), cfg, lo, hi, horizon=days, members=M, **norm)


def child(a, name):
    N, K, M, critic = SHAPES[name]
    pop = M > 1
    pair = {label: trainer(N, K, M, critic, a.days, a.batch, label == "on") for label in a.order.split(",")}
    rows = {"updates " + label: [] for label in pair}
    if "on" in pair:
        rows["norm update"] = []
    for rep in range(a.reps + 1):
        t = {}
        for label, (e, tr) in pair.items():
            e.reset()
            e.rollout_reset()
            e.run_days("mlp", a.days, BUDGET)
            (e.sac_pop_store if pop else e.sac_store)()
            if label == "on":
                t["norm update"] = timed(e.sac_norm_update, e.synchronize)
            upd = (lambda e=e: e.sac_pop_update(a.updates, stats=False)) if pop else (lambda e=e: e.sac_update(a.updates))
            t["updates " + label] = timed(upd, e.synchronize)
        if rep:
            for k, v in t.items():
                rows[k].append(v)
    for e, _ in pair.values():
        e.close()
    print(f"{name}: {N} envs x {K} keywords x {M} learner(s), critics {critic}, actor (32, 32), batch {a.batch}, {a.days} recorded days per repeat, "
          f"{'per-member' if pop else 'shared'} normalisers, built and timed in the order {a.order}, tree {a.tree}; ms per call of {a.updates} "
          f"updates, {a.reps} repeats after an untimed round")
    for k, v in rows.items():
        print(f"  {k:12s} " + " ".join(f"{x:9.4f}" for x in v) + f"   (min {min(v):.4f}, median {np.median(v):.4f}, spread {max(v) - min(v):.4f})", flush=True)
    if "updates on" in rows and "updates off" in rows:
        d = np.median(rows["updates on"]) - np.median(rows["updates off"])
        s = max(max(rows[k]) - min(rows[k]) for k in ("updates on", "updates off"))
        print(f"  {a.updates} updates, on - off (medians): {d:+.4f} ms = {d / a.updates * 1e3:+.2f} us per update; the larger run-to-run spread of the two: "
              f"{s:.4f} ms ({'inside' if abs(d) <= s else 'OUTSIDE'} the spread)", flush=True)
    print("RESULT " + json.dumps({k: [float(np.median(v)), float(min(v)), float(max(v))] for k, v in rows.items()}), flush=True)


def run_child(a, tree, name, order):
    """a child from `tree`: that tree's package and library"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--order", order, "--tree", tree, "--reps", str(a.reps), "--days", str(a.days),
           "--batch", str(a.batch), "--updates", str(a.updates)]
    out = subprocess.run(cmd, timeout=a.child_timeout, stdout=subprocess.PIPE, text=True, cwd=tree)      # (a timeout raises: nothing more is started)
    sys.stdout.write("".join(line + "\n" for line in out.stdout.splitlines() if not line.startswith("RESULT ")))
    sys.stdout.flush()
    if out.returncode != 0:
        sys.exit(f"measure_sac_norm: child {name} {order} of {tree} ended with status {out.returncode}; stopping")
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


def against_parent(a, names):
    trees = (("this", HERE), ("parent", os.path.abspath(a.parent_tree)))
    for name in names:
        med = {label: [] for label, _ in trees}
        for r in range(a.rounds):
            for label, tree in (trees if r % 2 == 0 else trees[::-1]):      # (which tree goes first alternates too)
                med[label].append(run_child(a, tree, name, "off")["updates off"][0])
        line = "; ".join(f"{label} " + " ".join(f"{x:.4f}" for x in v) + f" (median {np.median(v):.4f}, spread {max(v) - min(v):.4f})" for label, v in med.items())
        d = np.median(med["this"]) - np.median(med["parent"])
        s = max(max(v) - min(v) for v in med.values())
        print(f"{name}: updates off, medians of {a.rounds} processes each, ms per call of {a.updates} updates: {line}; this - parent {d:+.4f} ms = "
              f"{d / a.updates * 1e3:+.2f} us per update ({'inside' if abs(d) <= s else 'OUTSIDE'} the larger spread {s:.4f})", flush=True)
    head = {label: [] for label, _ in trees}
    for r in range(a.rounds):
        for label, tree in (trees if r % 2 == 0 else trees[::-1]):
            cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "20"]
            out = subprocess.run(cmd, timeout=a.child_timeout, stdout=subprocess.PIPE, text=True, cwd=tree)
            if out.returncode != 0:
                sys.exit(f"measure_sac_norm: bench.py of {tree} ended with status {out.returncode}; stopping")
            res = json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])
            head[label].append(float(res["value"]))
            unit = res["unit"]
    line = "; ".join(f"{label} " + " ".join(f"{x:.5g}" for x in v) + f" (median {np.median(v):.5g}, spread {max(v) - min(v):.3g})" for label, v in head.items())
    d = np.median(head["this"]) - np.median(head["parent"])
    s = max(max(v) - min(v) for v in head.values())
    print(f"bench.py --gpus 1 --steps {a.bench_steps} --warmup 20, headline [{unit}], {a.rounds} runs each, alternating: {line}; this - parent {d:+.4g} "
          f"({'inside' if abs(d) <= s else 'OUTSIDE'} the larger spread {s:.3g})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="pop,solo")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--updates", type=int, default=256, help="sac_update's in a timed call")
    ap.add_argument("--order", default="on,off", choices=["on,off", "off,on", "off"], help="(child) which trainer is built and timed first; off: that one alone")
    ap.add_argument("--tree", default=HERE, help="(child) the checkout whose package and library are measured")
    ap.add_argument("--child", default=None, choices=sorted(SHAPES))
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=200)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.path.abspath(a.tree))
        return child(a, a.child)
    names = a.shapes.split(",")
    for name in names:
        for order in ("on,off", "off,on"):
            run_child(a, HERE, name, order)
    if a.parent_tree:
        against_parent(a, names)


if __name__ == "__main__":
    main()
