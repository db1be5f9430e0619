#!/usr/bin/env python3
"""Train a learned bidder on the device with TD3, next to the zero-margin baseline.

The `[32, 32]` tanh policy of examples/evaluate_mlp_policy.py (built in numpy here: nothing but numpy and the engine is loaded)
is the actor; two critics on (observation, action) are drawn with torch's default initialisation.  Every iteration records one
episode of `run_days("mlp")` under exploration noise, appends it to the replay ring on the device and takes a number of TD3
updates there - minibatch sampling, target smoothing, twin critics, the delayed actor step through critic 1's input gradient,
Polyak averaging, Adam - so no transition or gradient crosses the bus.  Every few iterations the actor is evaluated
deterministically on held-out keyword sets and its episode return and NCP are printed beside the zero-margin agent's.

The actor's learning rate defaults to 1e-5, the one seen to learn at 256 envs x 25 keywords (profiles/pr_td3_trainer.txt): with
TD3's usual 1e-3 the actor outruns the critics there and the return falls.  This script's own default shape has not been
measured; lower --actor-lr further if the return falls.

--bounded LO,HI trains the way RLlib's DDPG family and Stable-Baselines3 run TD3 (csrc/adc_td3.h "bounded"): the actor is
tanh-squashed into the box [LO, HI] (one pair for the budget and every bid; give --budget-bounds for the budget's own), the noise
is added to the squashed action and clipped to the box, --sigma and --warmup-sigma are in units of the half-range, and
--random-timesteps transitions are first collected with actions drawn uniformly from the box.  The critics' action_lo /
action_hi / action_norm of the default law are then not used.

Usage: python examples/train_mlp_policy_td3.py [--iterations 100] [--num-envs 1024] [--num-keywords 100] [--warmup-iterations 2]
                                               [--frames H] [--bounded LO,HI [--random-timesteps N]]
"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import td3_trainer  # noqa: E402
from adcraft_amd.baselines.es_trainer import default_policy  # noqa: E402
from adcraft_amd.closed_loop import run_baseline_episode  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402


def evaluate(name, policy, planes, days, budget):
    """(mean episode return, mean NCP) of an agent on the held-out keyword sets"""
    N, K = planes.shape[1:]
    e = StepEngine(N, K, max_days=days, seed=70)
    e.set_all_params(planes)
    e.reset()
    if hasattr(policy, "install"):          # (a bounded trainer's SquashedPolicy: the actor and its box, through the squashed act)
        e.bid_curves_build(2048, None)
        e.metrics_enable(True)
        e.metrics_reset()
        policy.install(e, deterministic=True)
        e.run_days("mlp", days, budget)
        ncp = e.metrics_akncp_ncp(float(days))[1]
        ret = np.asarray(e.fetch()["cumulative_profit"], np.float64).mean()
        e.close()
        return ret, float(np.mean(ncp))
    r = run_baseline_episode(e, name, steps=days, budget=budget, default_rpc=1.0, mlp=policy, deterministic=True, per_keyword_sums=False)
    ret = np.asarray(e.fetch()["cumulative_profit"], np.float64).mean()
    e.close()
    return ret, float(np.mean(r["NCP"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--num-keywords", type=int, default=100)
    ap.add_argument("--frames", type=int, default=1, metavar="H", help="the policy acts on the last H observations (1 to 8), gathered on the device")
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--critic-hidden", default="256,256")
    ap.add_argument("--updates", type=int, default=200, help="TD3 updates after every collected episode")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=0.1, help="exploration noise (dollars)")
    ap.add_argument("--warmup-iterations", type=int, default=2, help="iterations collected under --warmup-sigma before the first update")
    ap.add_argument("--warmup-sigma", type=float, default=0.3)
    ap.add_argument("--reward-scale", type=float, default=0.1)
    ap.add_argument("--actor-lr", type=float, default=1e-5, help="the actor's learning rate (the critics' stays 1e-3)")
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--every", type=int, default=10, help="evaluate the policy every this many iterations")
    ap.add_argument("--eval-envs", type=int, default=1024)
    ap.add_argument("--normalize-observations", action="store_true", help="a running observation filter on the device; the ring holds raw rows")
    ap.add_argument("--normalize-rewards", action="store_true", help="the reward divided by the discounted return's running standard deviation")
    ap.add_argument("--prioritized-replay", action="store_true",
                    help="prioritised replay on the device (alpha 0.6, beta 0.4 annealed to 1 over the run); what it gains here has not been measured")
    ap.add_argument("--n-step", type=int, default=1, metavar="N",
                    help="n-step returns on the device (1: off; up to 16): a slot holds up to N days' discounted rewards and its own bootstrap discount; what it gains here has not been measured")
    ap.add_argument("--bounded", default=None, metavar="LO,HI",
                    help="the bounded mode: the actor squashed into [LO, HI]; --sigma / --warmup-sigma are then in units of the half-range")
    ap.add_argument("--budget-bounds", default=None, metavar="LO,HI", help="with --bounded: the budget component's own box (default: the bids')")
    ap.add_argument("--random-timesteps", type=int, default=0, metavar="N", help="with --bounded: transitions collected uniformly from the box first")
    args = ap.parse_args()
    N, K, days, budget = args.num_envs, args.num_keywords, args.days, 100000.0
    if args.random_timesteps and not args.bounded:
        ap.error("--random-timesteps needs --bounded")
    held_out = synthetic.implicit_keyword_planes(args.eval_envs, K, seed=999, mean_volume=args.mean_volume)
    zm = evaluate("zero_margin", None, held_out, days, budget)
    print(f"td3: {N} envs x {K} keywords, {days} days and {args.updates} updates per iteration; held-out: {args.eval_envs} envs")
    print(f"{'iteration':>10} {'critic loss':>12} {'Q1':>9} {'return':>10} {'NCP':>8}   zero-margin: return {zm[0]:.2f} NCP {zm[1]:.3f}")
    eng = StepEngine(N, K, max_days=days, seed=7)
    eng.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=args.mean_volume))
    eng.reset()
    config = td3_trainer.td3(critic_hidden=tuple(int(w) for w in args.critic_hidden.split(",")), exploration_sigma=args.warmup_sigma,
                             learning_starts=args.warmup_iterations * days * N, updates_per_iteration=args.updates, batch_size=args.batch_size,
                             reward_scale=args.reward_scale, gamma=args.gamma, actor_lr=args.actor_lr, action_lo=0.01, action_hi=3.0,
                             action_norm=(np.full(K + 1, 0.5, np.float32), np.full(K + 1, 2.0, np.float32)))
    if args.bounded:
        lo, hi = (np.full(K + 1, float(v), np.float32) for v in args.bounded.split(","))
        if args.budget_bounds:
            lo[0], hi[0] = (float(v) for v in args.budget_bounds.split(","))
        for k in ("action_lo", "action_hi", "action_norm"):
            del config[k]
        config.update(action_bounds=(lo, hi), random_timesteps=args.random_timesteps)
    trainer = td3_trainer.TD3Trainer(eng, default_policy(K, days=days, frames=args.frames), horizon=days, normalize_observations=args.normalize_observations,
                                     normalize_rewards=args.normalize_rewards,
                                     prioritized_replay=dict(alpha=0.6, beta=0.4, beta_final=1.0, beta_iterations=args.iterations) if args.prioritized_replay else None,
                                     n_step=args.n_step, **config)
    rng = np.random.default_rng(5)
    ret, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
    print(f"{0:>10} {'':>12} {'':>9} {ret:10.2f} {ncp:8.3f}")
    t0 = time.perf_counter()
    for it in range(1, args.iterations + 1):
        if it == args.warmup_iterations + 1:
            trainer.set_exploration(args.sigma)                # (the warm-up's wider noise is over)
        stats = trainer.iteration(days, budget, reset=True, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        if it % args.every == 0 or it == args.iterations:
            ret, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
            loss, q1 = (stats["critic_loss"], stats["q1_mean"]) if stats.get("updates") else (float("nan"), float("nan"))
            print(f"{it:>10} {loss:12.5f} {q1:9.3f} {ret:10.2f} {ncp:8.3f}", flush=True)
    eng.close()
    print(f"{args.iterations} iterations in {time.perf_counter() - t0:.2f} s (evaluations included)")


if __name__ == "__main__":
    main()
