#!/usr/bin/env python3
"""Train a learned bidder on the device with PPO (or A2C), next to the zero-margin baseline.

The `[32, 32]` tanh policy of examples/evaluate_mlp_policy.py plus a value network of the same shape (built in numpy here:
nothing but numpy and the engine is loaded) is trained on the sparse keyword law: every iteration records one episode of
`run_days("mlp")` under the stochastic policy and updates both networks from it on the device - advantages, backward pass,
PPO-clip loss, Adam - so no observation, action or gradient crosses the bus.  Every few iterations the policy is evaluated
deterministically on held-out keyword sets and its episode return and NCP are printed beside the zero-margin agent's.

With --normalize-observations the hand-set input scaling is replaced by a running mean / std filter of the raw observation
that lives on the device too (StepEngine.obs_norm_*): it starts from identity vectors (shift 0, scale 1) and is updated from
every iteration's record after the PPO / A2C update.  With --normalize-rewards the reward in GAE is divided by the running
standard deviation of the discounted return (StepEngine.rew_norm_*), updated from every iteration's record before the update;
--reward-scale then only sets where the first iteration starts.

With --kl-penalty COEF the loss gains RLlib's analytic KL penalty between the collecting and the current policy, whose
coefficient adapts to --kl-target after every update, and with --vf-clip C a sample's squared value error is capped at C
(StepEngine.pg_kl_*; csrc/adc_pg_kl.h).  --rllib takes the whole configuration of the paper's PPO agent as far as this trainer
expresses it (pg_trainer.rllib_ppo(): its docstring says what it leaves out); --lr and --reward-scale then apply only when given.

With --minibatch-size S an update's minibatches are S samples drawn from a new shuffle of the record every epoch instead of four
env ranges (StepEngine.pg_shuffle_*; csrc/adc_pg_shuffle.h), and --target-kl T ends an update before the step of the first
minibatch whose approx_kl exceeds 1.5 T.  --rllib turns on the reference's minibatch size of 64 unless --minibatch-size says otherwise.

Usage: python examples/train_mlp_policy_ppo.py [--iterations 100] [--algo ppo|a2c] [--num-envs 4096] [--num-keywords 100]
                                               [--normalize-observations] [--normalize-rewards]
                                               [--kl-penalty COEF [--kl-target T]] [--vf-clip C] [--rllib]
                                               [--minibatch-size S [--target-kl T]] [--frames H] [--drift]

--frames H (1 to 8): the policy acts on the last H observations, gathered on the device from a per-env history
(MLPPolicy(frames=H); csrc/adc_mlp.h).
"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import pg_trainer  # noqa: E402
from adcraft_amd.baselines.es_trainer import default_policy  # noqa: E402
from adcraft_amd.closed_loop import run_baseline_episode  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402


def with_value_network(policy, hidden, seed=1):
    """the policy plus a value network of the same hidden sizes, drawn like its own layers"""
    rng = np.random.default_rng(seed)
    layers, n_in = [], policy.input_size
    for n_out in list(hidden) + [1]:
        b = 1.0 / np.sqrt(n_in)
        layers.append((rng.uniform(-b, b, (n_in, n_out)).astype(np.float32), np.zeros(n_out, np.float32)))
        n_in = n_out
    policy.value_layers = layers
    return policy


DRIFT = False          # --drift: the held-out sets drift as the training envs do


def evaluate(name, policy, planes, days, budget):
    """(mean episode return, mean NCP) of an agent on the held-out keyword sets"""
    N, K = planes.shape[1:]
    e = StepEngine(N, K, max_days=days, seed=70, drift_enabled=DRIFT)
    e.set_all_params(planes)
    e.reset()
    r = run_baseline_episode(e, name, steps=days, budget=budget, default_rpc=1.0, mlp=policy, deterministic=True, per_keyword_sums=False)
    ret = np.asarray(e.fetch()["cumulative_profit"], np.float64).mean()
    e.close()
    return ret, float(np.mean(r["NCP"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--algo", choices=["ppo", "a2c"], default="ppo")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--num-keywords", type=int, default=100)
    ap.add_argument("--drift", action="store_true", help="non-stationary keywords: the engine's daily parameter drift, in training and on the held-out sets")
    ap.add_argument("--frames", type=int, default=1, metavar="H", help="the policy acts on the last H observations (1 to 8), gathered on the device")
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--lr", type=float, default=None, help="default 1e-3 (--rllib: the preset's 1e-4)")
    ap.add_argument("--reward-scale", type=float, default=None, help="default 0.1 (--rllib: 1)")
    ap.add_argument("--kl-penalty", type=float, default=None, metavar="COEF", help="the starting coefficient of the adaptive KL penalty")
    ap.add_argument("--kl-target", type=float, default=0.01, metavar="T", help="the KL the coefficient adapts to")
    ap.add_argument("--vf-clip", type=float, default=0.0, metavar="C", help="cap of a sample's squared value error (0: off)")
    ap.add_argument("--rllib", action="store_true", help="the paper's PPO configuration (pg_trainer.rllib_ppo())")
    ap.add_argument("--minibatch-size", type=int, default=None, metavar="S", help="shuffled minibatches of S samples (--rllib: 64)")
    ap.add_argument("--target-kl", type=float, default=None, metavar="T", help="end an update when a minibatch's approx_kl exceeds 1.5 T")
    ap.add_argument("--queued-update", action="store_true", help="enqueue every update as one chain on the device, one host wait (the same bits)")
    ap.add_argument("--every", type=int, default=10, help="evaluate the policy every this many iterations")
    ap.add_argument("--eval-envs", type=int, default=1024)
    ap.add_argument("--normalize-observations", action="store_true", help="a running observation filter on the device, from identity vectors")
    ap.add_argument("--normalize-rewards", action="store_true", help="divide the reward by the running std of the discounted return, on the device")
    args = ap.parse_args()
    global DRIFT
    DRIFT = args.drift
    N, K, days, budget = args.num_envs, args.num_keywords, args.days, 100000.0
    held_out = synthetic.implicit_keyword_planes(args.eval_envs, K, seed=999, mean_volume=args.mean_volume)
    zm = evaluate("zero_margin", None, held_out, days, budget)
    print(f"{'rllib_ppo' if args.rllib else args.algo}: {N} envs x {K} keywords, {days} days per iteration; held-out: {args.eval_envs} envs")
    print(f"{'iteration':>10} {'kl':>9} {'kl coef':>9} {'ev':>7} {'return':>10} {'NCP':>8}   zero-margin: return {zm[0]:.2f} NCP {zm[1]:.3f}")
    eng = StepEngine(N, K, max_days=days, seed=7, drift_enabled=args.drift)
    eng.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=args.mean_volume))
    eng.reset()
    if args.target_kl is not None and args.minibatch_size is None and not args.rllib:
        ap.error("--target-kl needs --minibatch-size")
    if args.rllib:
        config = pg_trainer.rllib_ppo(minibatch_size=64 if args.minibatch_size is None else args.minibatch_size, **{k: v for k, v in (("lr", args.lr), ("reward_scale", args.reward_scale)) if v is not None})
    else:
        config = getattr(pg_trainer, args.algo)(lr=1e-3 if args.lr is None else args.lr, reward_scale=0.1 if args.reward_scale is None else args.reward_scale)
    kl = dict(config.get("kl_penalty") or {})
    if args.kl_penalty is not None:
        kl.update(kl_coef=args.kl_penalty, kl_target=args.kl_target, adaptive=True)
    if args.vf_clip > 0:
        kl["vf_clip"] = args.vf_clip
    if kl and "kl_coef" not in kl:          # (the value clip alone: no penalty)
        kl.update(kl_coef=0.0, adaptive=False)
    config["kl_penalty"] = kl or None
    if args.minibatch_size is not None and not args.rllib:
        del config["minibatches"]
        config["minibatch_size"] = args.minibatch_size
    if args.target_kl is not None:
        config["target_kl"] = args.target_kl
    if args.queued_update:
        config["queued_update"] = True
    policy = with_value_network(default_policy(K, days=days, frames=args.frames), (32, 32))
    if args.normalize_observations:
        policy.shift, policy.scale = np.zeros_like(policy.shift), np.ones_like(policy.scale)
    trainer = pg_trainer.PGTrainer(eng, policy, days, normalize_observations=args.normalize_observations,
                                   normalize_rewards=args.normalize_rewards, **config)
    rng = np.random.default_rng(5)
    ret, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
    print(f"{0:>10} {'':>9} {'':>9} {'':>7} {ret:10.2f} {ncp:8.3f}")
    t0 = time.perf_counter()
    for it in range(1, args.iterations + 1):
        stats = trainer.iteration(days, budget, reset=True, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        if it % args.every == 0 or it == args.iterations:
            ret, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
            kl, coef = (stats["kl"], f"{stats['kl_coef']:9.4g}") if "kl" in stats else (stats["approx_kl"], f"{'':>9}")     # (the analytic KL under the add-on)
            print(f"{it:>10} {kl:9.5f} {coef} {stats['explained_variance']:7.3f} {ret:10.2f} {ncp:8.3f}", flush=True)
    eng.close()
    print(f"{args.iterations} iterations in {time.perf_counter() - t0:.2f} s (evaluations included)")


if __name__ == "__main__":
    main()
