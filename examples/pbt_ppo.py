#!/usr/bin/env python3
"""Population-based training of PPO on ONE engine: 16 learners whose learning rates are spread over three decades train in
lock-step on the device, once as a fixed grid and once under a PBT scheduler (baselines/pbt.py PBTScheduler: every few iterations
the worst quarter of the learners become copies of learners drawn among the best quarter, with the donor's learning rate times
0.8 or 1.25).

Fitness, copy and perturbation run on the device (StepEngine.pbt_step): the members' returns are reduced from the rollout record
where it lies, every replaced member is copied in the same launch, and the new hyperparameters go up in one copy; the launches
and host round trips of a round do not grow with the number of learners (profiles/pr_pbt.txt).

The script prints the best and the mean final return of both runs.  It passes or fails on nothing: what PBT gains on this
workload has not been established.

Usage: python examples/pbt_ppo.py [--members 16] [--envs-per-member 64] [--num-keywords 25] [--days 10] [--iterations 40] [--every 4]
"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import pg_trainer  # noqa: E402
from adcraft_amd.baselines.es_trainer import default_policy  # noqa: E402
from adcraft_amd.baselines.pbt import PBTScheduler  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402

LR_LO, LR_HI = 1e-5, 1e-2


def member_policy(K, days, hidden, seed):
    """the default policy plus a value network of the same hidden sizes, both drawn from the member's seed"""
    policy = default_policy(K, hidden=hidden, days=days, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    layers, n_in = [], policy.input_size
    for n_out in list(hidden) + [1]:
        b = 1.0 / np.sqrt(n_in)
        layers.append((rng.uniform(-b, b, (n_in, n_out)).astype(np.float32), np.zeros(n_out, np.float32)))
        n_in = n_out
    policy.value_layers = layers
    return policy


def run(args, with_pbt):
    K, days, n, M, budget, hidden = args.num_keywords, args.days, args.envs_per_member, args.members, 100000.0, (32, 32)
    N = M * n
    planes = np.concatenate([synthetic.implicit_keyword_planes(n, K, seed=1 + m, mean_volume=args.mean_volume, cvr=0.8) for m in range(M)], axis=1)
    eng = StepEngine(N, K, max_days=days, seed=7)
    eng.set_all_params(planes)
    eng.reset()
    lrs = np.logspace(np.log10(LR_LO), np.log10(LR_HI), M)
    configs = [pg_trainer.ppo(lr=float(lr), reward_scale=args.reward_scale, epochs=args.epochs, minibatches=args.minibatches) for lr in lrs]
    trainer = pg_trainer.PGPopulationTrainer(eng, [member_policy(K, days, hidden, m) for m in range(M)], days, configs, normalize_rewards=args.normalize_rewards)
    scheduler = PBTScheduler(trainer, replace_fraction=0.25, tuned=("lr",), bounds={"lr": (LR_LO, LR_HI)}, factors=(0.8, 1.25), fitness_ema=0.5,
                             every=args.every, seed=11) if with_pbt else None
    rng = np.random.default_rng(5)
    returns, replaced, t0 = None, 0, time.perf_counter()
    for it in range(1, args.iterations + 1):
        trainer.iteration(days, budget, reset=True, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        returns = trainer.returns()
        if scheduler is not None and it < args.iterations:
            res = scheduler.step()
            if res is not None:
                replaced += int((res["src"] >= 0).sum())
        if it % args.print_every == 0 or it == args.iterations:
            print(f"  {it:<5d} best {returns.max():9.2f}  mean {returns.mean():9.2f}  lr " + " ".join(f"{c['lr']:.0e}" for c in trainer.configs), flush=True)
    dt = time.perf_counter() - t0
    origin = scheduler.origin if scheduler is not None else list(range(M))
    eng.close()
    return dict(best=float(returns.max()), mean=float(returns.mean()), seconds=dt, replaced=replaced, origin=origin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--envs-per-member", type=int, default=64)
    ap.add_argument("--num-keywords", type=int, default=25)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--every", type=int, default=4, help="a PBT round every so many iterations")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--reward-scale", type=float, default=0.1)
    ap.add_argument("--print-every", type=int, default=8)
    ap.add_argument("--normalize-rewards", action="store_true", help="one running reward normaliser per member, on the device")
    args = ap.parse_args()
    print(f"{args.members} PPO learners x {args.envs_per_member} envs x {args.num_keywords} keywords on one engine, lr {LR_LO:.0e} .. {LR_HI:.0e}, "
          f"{args.days} days per iteration, {args.iterations} iterations")
    out = {}
    for name, with_pbt in (("fixed grid", False), ("PBT", True)):
        print(f"{name}:")
        out[name] = run(args, with_pbt)
    for name, r in out.items():
        print(f"{name:10s} final return of the last collected episode: best {r['best']:.2f}, mean {r['mean']:.2f}  ({r['seconds']:.2f} s"
              + (f", {r['replaced']} members replaced, surviving lineages {sorted(set(r['origin']))}" if name == "PBT" else "") + ")")


if __name__ == "__main__":
    main()
