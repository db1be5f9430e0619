#!/usr/bin/env python3
"""A hyperparameter sweep of soft actor-critic as ONE engine: an actor_lr x alpha_lr x seed grid of independent SAC learners that
collect, store and update in lock-step on the device.

Every grid cell is a member of a SAC learner population (baselines/sac_trainer.py SACPopulationTrainer): it owns a contiguous block
of the envs, has its own actor, twin critics, target critics, temperature, Adam moments, hyperparameters and replay ring, and every
kernel launch of a store or an update covers all members (the measured cost against one learner at a time:
profiles/pr_sac_population.txt).  What a member computes is bit for bit what a single SACTrainer computes on an engine of its envs.

The default grid asks what DESIGN.md section 2p left open at its small shape (256 envs x 25 sparse keywords, 10-day episodes, 100
updates per iteration): with the preset's defaults the held-out margin peaks early and drifts down while alpha falls; a slower
actor was not run there.  Every member runs the configuration of examples/train_mlp_policy_sac.py but for its grid cell (the seed
is the one of its batches, its noises and its critics' initialisation).  At the end every member's actor is evaluated
deterministically (the squashed mean) on held-out keyword sets, as that example evaluates it, and the table printed is each
member's paired margin over the zero-margin agent with its standard error.

Usage: python examples/sweep_sac.py [--actor-lrs 3e-4,3e-5] [--alpha-lrs 3e-4,0] [--seeds 7,8] [--envs-per-member 256]
                                    [--num-keywords 25] [--days 10] [--iterations 60] [--updates 100]
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import sac_trainer  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402
from train_mlp_policy_sac import evaluate, two_headed_policy  # noqa: E402

BUDGET = 100000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actor-lrs", default="3e-4,3e-5")
    ap.add_argument("--alpha-lrs", default="3e-4,0")
    ap.add_argument("--seeds", default="7,8")
    ap.add_argument("--envs-per-member", type=int, default=256)
    ap.add_argument("--num-keywords", type=int, default=25)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--updates", type=int, default=100, help="SAC updates per iteration")
    ap.add_argument("--critic-hidden", default="256,256")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--warmup-iterations", type=int, default=2, help="iterations collected before the first update")
    ap.add_argument("--reward-scale", type=float, default=0.1)
    ap.add_argument("--bid-lo", type=float, default=0.01)
    ap.add_argument("--bid-hi", type=float, default=3.0)
    ap.add_argument("--eval-envs", type=int, default=256)
    ap.add_argument("--normalize-observations", action="store_true", help="a running observation filter per member; the rings hold raw rows")
    ap.add_argument("--normalize-rewards", action="store_true",
                    help="per member, the reward divided by the discounted return's running standard deviation (the entropy term is not scaled); what the normalisers gain here has not been measured")
    ap.add_argument("--prioritized-replay", action="store_true",
                    help="prioritised replay on the device (alpha 0.6, beta 0.4 annealed to 1 over the run); what it gains here has not been measured")
    ap.add_argument("--n-step", type=int, default=1, metavar="N",
                    help="n-step returns on the device (1: off; up to 16): a slot holds up to N days' discounted rewards and its own bootstrap discount; what it gains here has not been measured")
    args = ap.parse_args()
    K, days, n = args.num_keywords, args.days, args.envs_per_member
    cells = [(float(a), float(t), int(s)) for a, t, s in itertools.product(args.actor_lrs.split(","), args.alpha_lrs.split(","), args.seeds.split(","))]
    M, N = len(cells), len(cells) * n
    member_planes = synthetic.implicit_keyword_planes(n, K, seed=1, mean_volume=args.mean_volume)       # (every member learns on the same keyword sets)
    held_out = synthetic.implicit_keyword_planes(args.eval_envs, K, seed=999, mean_volume=args.mean_volume)
    zm_ret, zm_ncp = evaluate("zero_margin", None, held_out, days, BUDGET)
    base = sac_trainer.sac(K, critic_hidden=tuple(int(w) for w in args.critic_hidden.split(",")), learning_starts=args.warmup_iterations * days * n,
                           updates_per_iteration=args.updates, batch_size=args.batch_size, reward_scale=args.reward_scale, capacity=100000)
    configs = [dict(base, actor_lr=alr, alpha_lr=tlr, seed=seed, critic_seed=seed, n_step=args.n_step) for alr, tlr, seed in cells]
    lo = np.concatenate([[1.0], np.full(K, args.bid_lo)]).astype(np.float32)          # (the budget is overridden during training and evaluation)
    hi = np.concatenate([[BUDGET], np.full(K, args.bid_hi)]).astype(np.float32)
    policy = two_headed_policy(K, days, args.bid_lo, args.bid_hi)
    eng = StepEngine(N, K, max_days=days, seed=7)
    eng.set_all_params(np.concatenate([member_planes] * M, axis=1))
    eng.reset()
    trainer = sac_trainer.SACPopulationTrainer(eng, policy, configs, lo, hi, horizon=days,
                                               normalize_observations=args.normalize_observations, normalize_rewards=args.normalize_rewards,
                                               prioritized_replay=dict(alpha=0.6, beta=0.4, beta_final=1.0, beta_iterations=args.iterations) if args.prioritized_replay else None)
    print(f"{M} SAC learners x {n} envs x {K} keywords on one engine, {days} days and {args.updates} updates per iteration; held-out: {args.eval_envs} envs; "
          f"zero-margin: return {zm_ret.mean():.2f} NCP {zm_ncp:.3f}")
    start, _ = evaluate("mlp", sac_trainer.SquashedPolicy(policy, lo, hi), held_out, days, BUDGET)
    print(f"the untrained policy's paired margin: {(start - zm_ret).mean():.2f} +- {(start - zm_ret).std(ddof=1) / np.sqrt(len(start)):.2f}")
    rng, stats = np.random.default_rng(5), None
    t0 = time.perf_counter()
    for _ in range(args.iterations):
        stats = trainer.iteration(days, BUDGET, reset=True, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
    dt = time.perf_counter() - t0
    print(f"{args.iterations} iterations of {M} learners on one engine in {dt:.2f} s ({1e3 * dt / args.iterations:.1f} ms per iteration)")
    print(f"{'member':>6} {'actor_lr':>9} {'alpha_lr':>9} {'seed':>5} {'critic loss':>12} {'Q1':>9} {'alpha':>8} {'-logp':>8} {'return':>10} {'NCP':>8} {'margin':>10} {'s.e.':>8}")
    for m, (alr, tlr, seed) in enumerate(cells):
        ret, ncp = evaluate("mlp", trainer.policy(m), held_out, days, BUDGET)
        diff = ret - zm_ret                                      # (paired: the same held-out envs, seeds and days)
        s = stats[m] if isinstance(stats, list) else None
        cols = (s["critic_loss"], s["q1_mean"], s["alpha"], -s["logp_mean"]) if s else (float("nan"),) * 4
        print(f"{m:>6} {alr:9.0e} {tlr:9.0e} {seed:>5} {cols[0]:12.5f} {cols[1]:9.3f} {cols[2]:8.4f} {cols[3]:8.3f} {ret.mean():10.2f} {ncp:8.3f} "
              f"{diff.mean():10.2f} {diff.std(ddof=1) / np.sqrt(len(diff)):8.2f}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
