#!/usr/bin/env python3
"""Train a learned bidder on the device with an evolution strategy (OpenAI-ES), next to the zero-margin baseline.

The `[32, 32]` tanh policy of examples/evaluate_mlp_policy.py (built in numpy here: nothing but numpy and the engine is
loaded) is trained on the sparse 100-keyword law: every generation perturbs the population's weights on the device, runs one
episode of `run_days("mlp")` and updates the centre policy from the members' returns; no observation, action or noise
crosses the bus.  Every few generations the centre is evaluated deterministically on held-out keyword sets and its episode
return and NCP are printed beside the zero-margin agent's.

Usage: python examples/train_mlp_policy_es.py [--generations 100] [--members 512] [--num-envs 4096] [--num-keywords 100]
                                              [--frames H] [--gru G] [--drift RATE]

--gru G makes the policy recurrent: one trunk layer of 32 and a GRU cell of width G in front of the output layer, its state kept
per env on the device (csrc/adc_gru.h); the strategy needs no back-propagation through time.  --drift RATE lets every keyword's
parameters drift by RATE per day (the engine's updater) in training and in the held-out evaluation alike.
"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines.es_trainer import ESTrainer, default_policy  # noqa: E402
from adcraft_amd.closed_loop import run_baseline_episode  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402


def drifting(e, rate):
    """every keyword of every env drifts by `rate` per day"""
    e.set_drift_mask(None)
    e.set_env_drift(np.float32([rate, rate, rate]))


def evaluate(name, policy, planes, days, budget, drift=0.0):
    """(mean episode return, mean NCP) of an agent on the held-out keyword sets"""
    N, K = planes.shape[1:]
    e = StepEngine(N, K, max_days=days, seed=70, drift_enabled=drift > 0)
    e.set_all_params(planes)
    e.reset()
    if drift > 0:
        drifting(e, drift)
    r = run_baseline_episode(e, name, steps=days, budget=budget, default_rpc=1.0, mlp=policy, deterministic=True, per_keyword_sums=False)
    ret = np.asarray(e.fetch()["cumulative_profit"], np.float64).mean()
    e.close()
    return ret, float(np.mean(r["NCP"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--members", type=int, default=512)
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--num-keywords", type=int, default=100)
    ap.add_argument("--frames", type=int, default=1, metavar="H", help="the policy acts on the last H observations (1 to 8), gathered on the device")
    ap.add_argument("--gru", type=int, default=0, metavar="G", help="a recurrent policy: a trunk of 32 and a GRU cell of width G (1 to 256) in front of the output layer")
    ap.add_argument("--drift", type=float, default=0.0, metavar="RATE", help="every keyword's parameters drift by RATE per day")
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--every", type=int, default=10, help="evaluate the centre every this many generations")
    ap.add_argument("--eval-envs", type=int, default=1024)
    args = ap.parse_args()
    N, K, days, budget = args.num_envs, args.num_keywords, args.days, 100000.0
    held_out = synthetic.implicit_keyword_planes(args.eval_envs, K, seed=999, mean_volume=args.mean_volume)
    zm = evaluate("zero_margin", None, held_out, days, budget, args.drift)
    print(f"{N} envs x {K} keywords, {days} days per generation, {args.members} members; held-out: {args.eval_envs} envs")
    print(f"{'generation':>10} {'fitness':>10} {'return':>10} {'NCP':>8}   zero-margin: return {zm[0]:.2f} NCP {zm[1]:.3f}")
    eng = StepEngine(N, K, max_days=days, seed=7, drift_enabled=args.drift > 0)
    train = synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=args.mean_volume)
    eng.set_all_params(train)
    eng.reset()
    if args.drift > 0:
        drifting(eng, args.drift)
    start = default_policy(K, hidden=(32,), days=days, gru=args.gru) if args.gru else default_policy(K, days=days, frames=args.frames)
    trainer = ESTrainer(eng, start, args.members, sigma=args.sigma, lr=args.lr, seed=11)
    rng = np.random.default_rng(5)
    ret, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget, args.drift)
    print(f"{0:>10} {'':>10} {ret:10.2f} {ncp:8.3f}")
    t0 = time.perf_counter()
    for g in range(1, args.generations + 1):
        if args.drift > 0:
            eng.set_all_params(train)                # (every generation's episode starts from the keywords as drawn, as every evaluation does)
        stats = trainer.generation(days, budget, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        if g % args.every == 0 or g == args.generations:
            ret, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget, args.drift)
            print(f"{g:>10} {stats['fitness_mean']:10.2f} {ret:10.2f} {ncp:8.3f}", flush=True)
    eng.close()
    print(f"{args.generations} generations in {time.perf_counter() - t0:.2f} s (evaluations included)")


if __name__ == "__main__":
    main()
