#!/usr/bin/env python3
"""DAgger on the device: clone one of the engine's expert bidders on the states the LEARNER visits.

Behaviour cloning (examples/pretrain_mlp_policy_bc.py) trains on the teacher's own days alone, and a clone that drifts to states
the teacher never visits was never told what to do there.  DAgger (Ross, Gordon and Bagnell 2011) lets the learner drive: every
round records one episode of DAgger days (StepEngine.dagger_days) - the `[32, 32]` tanh policy of
examples/train_mlp_policy_ppo.py and the teacher act on the same observation, the record keeps the teacher's action as the
label, and a per-env coin picks whose action the env is stepped by: the teacher's with probability beta_i = beta0 * decay^i in
round i (round 0 at beta0 = 1 is a round of teacher days).  `im_update` then descends the behaviour-cloning loss over every day
recorded so far (--no-aggregate: over the round alone) on the device.  AKNCP / NCP of the random initialisation, of the teacher
and of the clone are printed on held-out keyword sets, next to the share of env-days the teacher drove.

A round of an aggregated record trains on (round + 1) x days days: the record's memory and an update's time grow with the rounds.

Usage: python examples/train_mlp_policy_dagger.py [--teacher oracle|zero_margin] [--rounds 10] [--beta0 1] [--beta-decay 0.5]
                                                  [--no-aggregate] [--frames H] [--num-envs 4096] [--num-keywords 100]
"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import imitation, pg_trainer  # noqa: E402
from adcraft_amd.baselines.es_trainer import default_policy  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402
from examples.pretrain_mlp_policy_bc import evaluate, teacher_ready  # noqa: E402
from examples.train_mlp_policy_ppo import with_value_network  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher", choices=["oracle", "zero_margin"], default="oracle")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--beta0", type=float, default=1.0, help="the teacher's share of round 0")
    ap.add_argument("--beta-decay", type=float, default=0.5, help="round i runs at beta0 * decay^i")
    ap.add_argument("--no-aggregate", action="store_true", help="train on each round's days alone")
    ap.add_argument("--vf-coef", type=float, default=1.0, help="the value loss's coefficient (0 drops it, as RLlib's BC does)")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--reward-scale", type=float, default=0.1)
    ap.add_argument("--train-log-std", action="store_true")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--num-keywords", type=int, default=100)
    ap.add_argument("--frames", type=int, default=1, metavar="H", help="the policy acts on the last H observations (1 to 8)")
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--eval-envs", type=int, default=1024)
    args = ap.parse_args()
    N, K, days, budget = args.num_envs, args.num_keywords, args.days, 100000.0
    held_out = synthetic.implicit_keyword_planes(args.eval_envs, K, seed=999, mean_volume=args.mean_volume)
    policy = with_value_network(default_policy(K, days=days, frames=args.frames), (32, 32))
    print(f"dagger from {args.teacher}: {N} envs x {K} keywords, {args.rounds} rounds of {days} days, beta {args.beta0} x {args.beta_decay}^round, "
          f"{'each round alone' if args.no_aggregate else 'aggregated'}; held-out: {args.eval_envs} envs")
    rows = [("teacher", evaluate(args.teacher, None, held_out, days, budget)), ("random init", evaluate("mlp", policy, held_out, days, budget))]
    for name, (akncp, ncp) in rows:
        print(f"{name:>14}: AKNCP {akncp:8.3f}  NCP {ncp:8.3f}")
    eng = StepEngine(N, K, max_days=days, seed=7)
    eng.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=args.mean_volume))
    eng.reset()
    if args.teacher == "oracle":
        eng.bid_curves_build(2048)
    config = pg_trainer.ppo(lr=args.lr, reward_scale=args.reward_scale)
    config.pop("epochs")
    config.pop("minibatches")
    trainer = imitation.DAggerTrainer(eng, policy, teacher=args.teacher, rounds=args.rounds, days=days, epochs=args.epochs, beta0=args.beta0,
                                      beta_decay=args.beta_decay, aggregate=not args.no_aggregate, budget=budget, minibatches=args.minibatches,
                                      vf_coef=args.vf_coef, train_log_std=args.train_log_std, pg_options=config)
    rng = np.random.default_rng(5)
    print(f"{'round':>6} {'beta':>8} {'teacher':>8} {'days':>6} {'steps':>6} {'logp':>12} {'v loss':>10} {'ev':>7} {'AKNCP':>8} {'NCP':>8}")
    t0 = time.perf_counter()
    for rnd in range(1, args.rounds + 1):
        eng.reset(seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        teacher_ready(eng, args.teacher)
        st = trainer.iteration()
        if rnd % args.every == 0 or rnd == args.rounds:
            akncp, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
            print(f"{st['round']:>6} {st['beta']:8.4f} {st['teacher_share']:8.3f} {st['recorded']:>6} {st['steps']:>6} {st['logp']:12.4f} "
                  f"{st['value_loss']:10.4f} {st['explained_variance']:7.3f} {akncp:8.3f} {ncp:8.3f}", flush=True)
    print(f"{args.rounds} DAgger rounds in {time.perf_counter() - t0:.2f} s (evaluations included)")
    akncp, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
    print(f"{'clone':>14}: AKNCP {akncp:8.3f}  NCP {ncp:8.3f}")
    eng.close()


if __name__ == "__main__":
    main()
