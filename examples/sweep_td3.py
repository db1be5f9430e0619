#!/usr/bin/env python3
"""A hyperparameter sweep of TD3 as ONE engine: an actor_lr x critic_lr x exploration-sigma grid of independent off-policy
learners that collect, store and update in lock-step on the device.

Every grid cell is a member of a TD3 learner population (baselines/td3_trainer.py TD3PopulationTrainer): it owns a contiguous
block of the envs, has its own actor, exploration sigma, twin critics, targets, Adam moments, hyperparameters and replay ring, and
every kernel launch of a store or an update covers all members (the measured cost against one learner at a time:
profiles/pr_td3_population.txt).  What a member computes is bit for bit what a single TD3Trainer computes on an engine of its envs.

The default grid is the question DESIGN.md section 2e answers for the small shape (256 envs x 25 sparse keywords, 10-day
episodes): TD3 learns there only when the actor is much slower than the critics.  Every member runs the configuration of that
section but for its grid cell; the table printed is each member's training-plane return (the mean recorded episode return under
the stochastic collection policy), and the verdict compares the mean of the last five iterations with the mean of the first three.
With --solo the same grid is then run as solo trainers, one engine after another, for the wall time of the sweep done the old way.

--bounded LO,HI runs every member in the bounded mode (the actor squashed into the box, clipped noise, --random-timesteps of uniform
warm-up; baselines/td3_trainer.py BoundedActions); the sigmas are then in units of the half-range.

Usage: python examples/sweep_td3.py [--actor-lrs 1e-5,1e-3] [--critic-lrs 1e-3,3e-4] [--sigmas 0.1,0.2] [--envs-per-member 256]
                                    [--num-keywords 25] [--days 10] [--iterations 60] [--solo]
"""
import argparse
import itertools
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import td3_trainer  # noqa: E402
from adcraft_amd.baselines.es_trainer import default_policy  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402

BUDGET, HIDDEN = 100000.0, (32, 32)


def base_config(args):
    """DESIGN.md section 2e's configuration of the small shape (tests/test_gpu_td3_trainer.py LEARN)"""
    return dict(critic_hidden=(64, 64), learning_starts=args.days * args.envs_per_member, updates_per_iteration=args.updates, gamma=0.9, tau=0.01,
                policy_delay=2, target_noise=0.05, target_noise_clip=0.1, batch_size=256, capacity=100000, reward_scale=0.1, action_lo=0.01,
                action_hi=3.0, seed=7, critic_seed=1)


def curves_of(trainer_iteration, returns, iterations, N, seed=2024):
    rng, rows = np.random.default_rng(seed), []
    for _ in range(iterations):
        trainer_iteration(rng.integers(0, 2 ** 63, N).astype(np.uint64))
        rows.append(returns())
    return np.array(rows)                                           # [iterations, members]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actor-lrs", default="1e-5,1e-3")
    ap.add_argument("--critic-lrs", default="1e-3,3e-4")
    ap.add_argument("--sigmas", default="0.1,0.2")
    ap.add_argument("--envs-per-member", type=int, default=256)
    ap.add_argument("--num-keywords", type=int, default=25)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--updates", type=int, default=100, help="critic updates per iteration")
    ap.add_argument("--normalize-observations", action="store_true", help="a running observation filter per member; the rings hold raw rows")
    ap.add_argument("--normalize-rewards", action="store_true", help="per member, the reward divided by the discounted return's running standard deviation")
    ap.add_argument("--solo", action="store_true", help="afterwards, the same grid as solo trainers one after another (wall time)")
    ap.add_argument("--prioritized-replay", action="store_true",
                    help="prioritised replay on the device (alpha 0.6, beta 0.4 annealed to 1 over the run); what it gains here has not been measured")
    ap.add_argument("--n-step", type=int, default=1, metavar="N",
                    help="n-step returns on the device (1: off; up to 16): a slot holds up to N days' discounted rewards and its own bootstrap discount; what it gains here has not been measured")
    ap.add_argument("--bounded", default=None, metavar="LO,HI",
                    help="the bounded mode (csrc/adc_td3.h \"bounded\"): every member's actor squashed into [LO, HI], shared by all members; "
                         "--sigmas are then in units of the half-range")
    ap.add_argument("--random-timesteps", type=int, default=0, metavar="N", help="with --bounded: a member's transitions collected uniformly from the box first")
    args = ap.parse_args()
    if args.random_timesteps and not args.bounded:
        ap.error("--random-timesteps needs --bounded")
    K, days, n = args.num_keywords, args.days, args.envs_per_member
    cells = list(itertools.product(*([float(x) for x in s.split(",")] for s in (args.actor_lrs, args.critic_lrs, args.sigmas))))
    M, N = len(cells), len(cells) * n
    member_planes = synthetic.implicit_keyword_planes(n, K, seed=1, mean_volume=args.mean_volume)       # (every member learns on the same keyword sets)
    norm = (np.full(K + 1, 0.5, np.float32), np.full(K + 1, 2.0, np.float32))
    policy = default_policy(K, hidden=HIDDEN, days=days, seed=0)
    configs = [dict(base_config(args), actor_lr=alr, critic_lr=clr, action_norm=norm, n_step=args.n_step) for alr, clr, _ in cells]
    bounded = {}
    if args.bounded:                    # (the box takes the place of the target's clamp and of the critics' action normalisation)
        lo, hi = (float(v) for v in args.bounded.split(","))
        bounded = dict(action_bounds=(lo, hi), random_timesteps=args.random_timesteps)
        for c in configs:
            for k in ("action_lo", "action_hi", "action_norm"):
                del c[k]
    eng = StepEngine(N, K, max_days=days, seed=7)
    eng.set_all_params(np.concatenate([member_planes] * M, axis=1))
    eng.reset()
    prio = dict(alpha=0.6, beta=0.4, beta_final=1.0, beta_iterations=args.iterations) if args.prioritized_replay else None
    trainer = td3_trainer.TD3PopulationTrainer(eng, policy, [s for _, _, s in cells], configs, horizon=days,
                                               normalize_observations=args.normalize_observations, normalize_rewards=args.normalize_rewards,
                                               prioritized_replay=prio, **bounded)
    print(f"{M} TD3 learners x {n} envs x {K} keywords on one engine, {days} days and {args.updates} updates per iteration")
    print("member    " + " ".join(f"{m:>8d}" for m in range(M)))
    print("actor_lr  " + " ".join(f"{a:8.0e}" for a, _, _ in cells))
    print("critic_lr " + " ".join(f"{c:8.0e}" for _, c, _ in cells))
    print("sigma     " + " ".join(f"{s:8.2f}" for _, _, s in cells))
    t0 = time.perf_counter()
    curves = curves_of(lambda seeds: trainer.iteration(days, BUDGET, reset=True, reset_seeds=seeds), trainer.returns, args.iterations, N)
    dt = time.perf_counter() - t0
    eng.close()
    for it, row in enumerate(curves, 1):
        print(f"{it:<9d} " + " ".join(f"{r:8.2f}" for r in row))
    first, last = curves[:3].mean(axis=0), curves[-5:].mean(axis=0)
    print("first 3   " + " ".join(f"{r:8.2f}" for r in first))
    print("last 5    " + " ".join(f"{r:8.2f}" for r in last))
    print("verdict   " + " ".join(f"{'learns' if b > a else 'falls':>8s}" for a, b in zip(first, last)))
    print(f"{args.iterations} iterations of {M} learners on one engine in {dt:.2f} s ({1e3 * dt / args.iterations:.1f} ms per iteration, fetching the rewards included)")
    if args.solo:
        t0 = time.perf_counter()
        solo_last = []
        for (alr, clr, sigma), cfg in zip(cells, configs):
            e = StepEngine(n, K, max_days=days, seed=7)
            e.set_all_params(member_planes)
            e.reset()
            tr = td3_trainer.TD3Trainer(e, policy, horizon=days, exploration_sigma=sigma, normalize_observations=args.normalize_observations,
                                        normalize_rewards=args.normalize_rewards, prioritized_replay=prio, **bounded, **cfg)
            c = curves_of(lambda seeds: tr.iteration(days, BUDGET, reset=True, reset_seeds=seeds),
                          lambda: [e.rollout_fetch()["reward"].astype(np.float64).sum(axis=0).mean()], args.iterations, n)
            solo_last.append(c[-5:].mean())
            e.close()
        ds = time.perf_counter() - t0
        print("solo last5" + " ".join(f"{r:8.2f}" for r in solo_last) + "   (other envs' streams: each solo engine starts at env id 0)")
        print(f"the same grid as {M} solo trainers one after another in {ds:.2f} s: {ds / dt:.2f} x the population's wall time")


if __name__ == "__main__":
    main()
