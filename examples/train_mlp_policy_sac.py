#!/usr/bin/env python3
"""Train a learned bidder on the device with soft actor-critic, next to the zero-margin baseline.

A `[32, 32]` tanh policy with two heads (means and log-stds of the K + 1 action components, built in numpy here: nothing but
numpy and the engine is loaded) is the actor; the env is given the squashed action lo + 0.5 (hi - lo) (tanh(u) + 1), so the
agent's bids stay inside [--bid-lo, --bid-hi].  Two critics on (observation, tanh(u)) are drawn with torch's default
initialisation.  Every iteration records one episode of `run_days("mlp")` under the policy's own noise, appends it to the replay
ring on the device and takes a number of SAC updates there - minibatch sampling, the soft target under the live actor, twin
critics, the actor's reparameterised step through the smaller critic, the temperature's step, Polyak averaging, Adam - so no
transition or gradient crosses the bus.  Every few iterations the actor is evaluated deterministically (the squashed mean) on
held-out keyword sets and its episode return and NCP are printed beside the zero-margin agent's, with the paired margin over
the held-out envs and its standard error.

The defaults are the preset's (baselines/sac_trainer.sac: RLlib's SAC defaults).  Whether they learn at a given shape is for a
run to show; profiles/pr_sac_trainer.txt says what has been run.

Usage: python examples/train_mlp_policy_sac.py [--iterations 100] [--num-envs 1024] [--num-keywords 100] [--frames H]
"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import sac_trainer  # noqa: E402
from adcraft_amd.baselines.mlp_policy import MLPPolicy  # noqa: E402
from adcraft_amd.closed_loop import run_baseline_episode  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402


def two_headed_policy(K, days, bid_lo, bid_hi, start_bid=0.5, hidden=(32, 32), seed=0, log_std_clamp=(-5.0, 1.0), frames=1):
    """means and log-stds from one network on the normalised observation: small last-layer weights and mean biases at
    atanh of start_bid's place in [bid_lo, bid_hi], so that the first bids sit about start_bid (examples/evaluate_mlp_policy.py's
    50 cents) with a standard deviation of exp(-1) before the squash"""
    from adcraft_amd.baselines.es_trainer import default_policy
    base = default_policy(K, days=days, frames=frames)
    rng, A, layers, n_in = np.random.default_rng(seed), K + 1, [], frames * (5 * K + 2)
    for n_out in hidden:
        bound = 1.0 / np.sqrt(n_in)
        layers.append((rng.uniform(-bound, bound, (n_in, n_out)).astype(np.float32), np.zeros(n_out, np.float32)))
        n_in = n_out
    u0 = np.arctanh(2.0 * (start_bid - bid_lo) / (bid_hi - bid_lo) - 1.0)
    bias = np.concatenate([np.full(A, u0, np.float32), np.full(A, -1.0, np.float32)])
    layers.append(((rng.standard_normal((n_in, 2 * A)) * 0.01).astype(np.float32), bias))
    return MLPPolicy(layers, activation="tanh", shift=base.shift, scale=base.scale, log_std_clamp=log_std_clamp, frames=frames)


def evaluate(name, squashed, planes, days, budget):
    """(per-env episode return [N], mean NCP) of an agent on the held-out keyword sets"""
    N, K = planes.shape[1:]
    e = StepEngine(N, K, max_days=days, seed=70)
    e.set_all_params(planes)
    e.reset()
    if name == "mlp":
        e.bid_curves_build(2048, None)
        e.metrics_enable(True)
        e.metrics_reset()
        squashed.install(e, deterministic=True)
        e.run_days("mlp", days, budget)
        ncp = e.metrics_akncp_ncp(float(days))[1]
    else:
        ncp = run_baseline_episode(e, name, steps=days, budget=budget, default_rpc=1.0, per_keyword_sums=False)["NCP"]
    ret = np.asarray(e.fetch()["cumulative_profit"], np.float64).copy()
    e.close()
    return ret, float(np.mean(ncp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--num-keywords", type=int, default=100)
    ap.add_argument("--frames", type=int, default=1, metavar="H", help="the policy acts on the last H observations (1 to 8), gathered on the device")
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--critic-hidden", default="256,256")
    ap.add_argument("--updates", type=int, default=200, help="SAC updates after every collected episode")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--warmup-iterations", type=int, default=2, help="iterations collected before the first update")
    ap.add_argument("--reward-scale", type=float, default=0.1)
    ap.add_argument("--bid-lo", type=float, default=0.01)
    ap.add_argument("--bid-hi", type=float, default=3.0)
    ap.add_argument("--every", type=int, default=10, help="evaluate the policy every this many iterations")
    ap.add_argument("--eval-envs", type=int, default=1024)
    ap.add_argument("--set", action="append", default=[], metavar="KEY=VALUE", help="override a float option of the preset (e.g. actor_lr=1e-5)")
    ap.add_argument("--normalize-observations", action="store_true", help="a running observation filter on the device; the ring holds raw rows")
    ap.add_argument("--normalize-rewards", action="store_true",
                    help="the reward divided by the discounted return's running standard deviation (the entropy term is not scaled); what the normalisers gain here has not been measured")
    ap.add_argument("--prioritized-replay", action="store_true",
                    help="prioritised replay on the device (alpha 0.6, beta 0.4 annealed to 1 over the run); what it gains here has not been measured")
    ap.add_argument("--n-step", type=int, default=1, metavar="N",
                    help="n-step returns on the device (1: off; up to 16): a slot holds up to N days' discounted rewards and its own bootstrap discount; what it gains here has not been measured")
    args = ap.parse_args()
    N, K, days, budget = args.num_envs, args.num_keywords, args.days, 100000.0
    held_out = synthetic.implicit_keyword_planes(args.eval_envs, K, seed=999, mean_volume=args.mean_volume)
    zm_ret, zm_ncp = evaluate("zero_margin", None, held_out, days, budget)
    print(f"sac: {N} envs x {K} keywords, {days} days and {args.updates} updates per iteration; held-out: {args.eval_envs} envs")
    print(f"{'iteration':>10} {'critic loss':>12} {'Q1':>9} {'alpha':>8} {'-logp':>8} {'return':>10} {'NCP':>8} {'margin':>10} {'s.e.':>8}"
          f"   zero-margin: return {zm_ret.mean():.2f} NCP {zm_ncp:.3f}")
    eng = StepEngine(N, K, max_days=days, seed=7)
    eng.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=args.mean_volume))
    eng.reset()
    config = sac_trainer.sac(K, critic_hidden=tuple(int(w) for w in args.critic_hidden.split(",")), learning_starts=args.warmup_iterations * days * N,
                             updates_per_iteration=args.updates, batch_size=args.batch_size, reward_scale=args.reward_scale)
    config.update({k: float(v) for k, v in (kv.split("=", 1) for kv in args.set)})
    lo = np.concatenate([[1.0], np.full(K, args.bid_lo)]).astype(np.float32)          # (the budget is overridden during training and evaluation)
    hi = np.concatenate([[budget], np.full(K, args.bid_hi)]).astype(np.float32)
    trainer = sac_trainer.SACTrainer(eng, two_headed_policy(K, days, args.bid_lo, args.bid_hi, frames=args.frames), lo, hi, horizon=days,
                                     normalize_observations=args.normalize_observations, normalize_rewards=args.normalize_rewards,
                                     prioritized_replay=dict(alpha=0.6, beta=0.4, beta_final=1.0, beta_iterations=args.iterations) if args.prioritized_replay else None,
                                     n_step=args.n_step, **config)
    rng = np.random.default_rng(5)

    def report(it, stats):
        ret, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
        diff = ret - zm_ret                                      # (paired: the same held-out envs, seeds and days)
        cols = (stats["critic_loss"], stats["q1_mean"], stats["alpha"], -stats["logp_mean"]) if stats and stats.get("updates") else (float("nan"),) * 4
        print(f"{it:>10} {cols[0]:12.5f} {cols[1]:9.3f} {cols[2]:8.4f} {cols[3]:8.3f} {ret.mean():10.2f} {ncp:8.3f} {diff.mean():10.2f} "
              f"{diff.std(ddof=1) / np.sqrt(len(diff)):8.2f}", flush=True)

    report(0, None)
    t0 = time.perf_counter()
    for it in range(1, args.iterations + 1):
        stats = trainer.iteration(days, budget, reset=True, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        if it % args.every == 0 or it == args.iterations:
            report(it, stats)
    eng.close()
    print(f"{args.iterations} iterations in {time.perf_counter() - t0:.2f} s (evaluations included)")


if __name__ == "__main__":
    main()
