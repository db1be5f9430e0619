#!/usr/bin/env python3
"""ms per day of run_days("interpolation") against run_days("zero_margin") at 4096 x 256, a 60-day episode, the default grid
and the per-step ideal on (profiles/pr_interp_agent.txt).  Each policy runs one untimed episode, then `--reps` timed ones
on fresh engines; the figure is the GPU time of the whole episode / 60.

    python tools/measure_interp_agent.py [--reps 3] [--envs 4096] [--keywords 256]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/measure_interp_agent.py --reps 1   (a run of its own)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def episode(eng, H, N, K, days, policy):
    e = eng.StepEngine(N, K, seed=31, max_days=days)
    e.set_all_params(H.implicit_params(N, K, seed=77, mean_volume=8, cvr=0.5))
    e.reset()
    e.bid_curves_build(2048)
    e.metrics_enable(True)
    e.metrics_reset()
    seeds = np.arange(N, dtype=np.uint64) + 1000
    if policy == "interpolation":
        e.interp_init(-0.2, 0.03, None, 0, seeds)
    else:
        e.agent_init(1.0, seeds)
    e.region_begin()
    e.run_days(policy, days, 100000.0)
    ms = e.region_end()
    e.close()
    return ms / days


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--keywords", type=int, default=256)
    ap.add_argument("--days", type=int, default=60)
    a = ap.parse_args()
    import adcraft_amd.engine as eng
    from tests import helpers as H
    for policy in ("zero_margin", "interpolation"):
        episode(eng, H, a.envs, a.keywords, a.days, policy)
        t = [episode(eng, H, a.envs, a.keywords, a.days, policy) for _ in range(a.reps)]
        print(f"{policy:14s} {a.envs} x {a.keywords}, {a.days} days: ms per day " + " ".join(f"{x:.4f}" for x in t)
              + f"  (min {min(t):.4f})", flush=True)


if __name__ == "__main__":
    main()
