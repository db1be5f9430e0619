#!/usr/bin/env python3
"""ms per day of run_days("mlp") - a [32, 32] tanh policy with a value network, stochastic, the rollout record on - against
run_days with fixed actions and with the zero-margin agent, at 4096 x 256 and 16384 x 1024 (profiles/pr_mlp_policy.txt).
Each policy runs one untimed episode, then `--reps` timed ones on fresh engines; the figure is the GPU time of the whole
episode / days (one event pair around run_days).

    python tools/measure_mlp_policy.py [--reps 3] [--shapes 4096x256,16384x1024] [--policies fixed,zero_margin,mlp]
    python tools/measure_mlp_policy.py --tree <another checkout> --policies fixed,zero_margin     # e.g. the parent commit's build
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/measure_mlp_policy.py --reps 1 --policies mlp   (a run of its own)
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def implicit_params(N, K, seed, mean_volume=8, cvr=0.5):
    """the singleton experiment quantiles' law, sparse volumes: a copy of tests/helpers.py implicit_params, kept here because
    with --tree the script runs against another checkout and must not import this one's tests"""
    rng = np.random.default_rng(seed)
    shape = (N, K)
    pl = lambda lo, mid, hi: np.interp(rng.random(shape), [0.0, 0.5, 1.0], [lo, mid, hi])
    r = rng.random(shape)
    vol_mean = np.full(shape, float(mean_volume))
    vol_std = np.floor(1 + r * 0.5 * mean_volume)
    loc = pl(0.3, 0.55, 1.0)
    scale = np.maximum(0.01, pl(0.01, 0.15, 0.3) * loc)
    bctr = pl(0.1, 0.5, 0.9)
    mu = pl(0.3, 1.0, 1.5)
    sd = np.maximum(0.01, pl(0.01, 0.15, 0.3) * mu)
    return np.stack([vol_mean, vol_std, loc, scale, bctr, np.full(shape, cvr), mu, sd]).astype(np.float32)


def mlp_policy(K, seed=5):
    from adcraft_amd.baselines.mlp_policy import MLPPolicy
    rng = np.random.default_rng(seed)
    D, A = 5 * K + 2, K + 1

    def net(widths):
        layers, n_in = [], D
        for n_out in widths:
            layers.append(((rng.standard_normal((n_in, n_out)) / np.sqrt(n_in)).astype(np.float32), np.zeros(n_out, np.float32)))
            n_in = n_out
        return layers
    pol = MLPPolicy(net([32, 32, A]), activation="tanh", value_layers=net([32, 32, 1]), log_std=np.full(A, -1.5, np.float32),
                    shift=np.zeros(D, np.float32), scale=np.full(D, 0.05, np.float32))
    pol.layers[-1][1][:] = 0.6                     # bids around 60 cents
    pol.layers[-1][1][0] = 1.0e5                   # an ample budget
    return pol


def episode(eng, N, K, days, policy, planes, record=True):
    e = eng.StepEngine(N, K, seed=31, max_days=days)
    e.set_all_params(planes)
    e.reset()
    seeds = np.arange(N, dtype=np.uint64) + 1000
    if policy == "mlp":
        e.mlp_init(mlp_policy(K), seeds)
        if record:
            e.rollout_enable(days)
    elif policy == "zero_margin":
        e.agent_init(1.0, seeds)
    else:
        e.sample_actions(0.3, 1.0, 1.0e5)
    e.synchronize()
    e.region_begin()
    e.run_days(policy, days, 0.0 if policy == "mlp" else 100000.0)
    ms = e.region_end()
    groups = e.env_groups()
    e.close()
    return ms / days, groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="4096x256,16384x1024")
    ap.add_argument("--policies", default="fixed,zero_margin,mlp")
    ap.add_argument("--days", type=int, default=30)
    ap.add_argument("--no-record", action="store_true", help="mlp: without the rollout record")
    ap.add_argument("--tree", default=HERE, help="the checkout whose adcraft_amd package is measured (default: this one)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import adcraft_amd.engine as eng
    print(f"# package {os.path.dirname(os.path.abspath(eng.__file__))}", flush=True)
    for shape in a.shapes.split(","):
        N, K = (int(x) for x in shape.split("x"))
        planes = implicit_params(N, K, seed=77)
        for policy in a.policies.split(","):
            episode(eng, N, K, a.days, policy, planes, not a.no_record)
            runs = [episode(eng, N, K, a.days, policy, planes, not a.no_record) for _ in range(a.reps)]
            t = [r[0] for r in runs]
            print(f"{policy:12s} {N} x {K}, {a.days} days, env groups {runs[-1][1]}: ms per day " + " ".join(f"{x:.4f}" for x in t)
                  + f"  (min {min(t):.4f})", flush=True)


if __name__ == "__main__":
    main()
