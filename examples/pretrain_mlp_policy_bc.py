#!/usr/bin/env python3
"""Clone one of the engine's expert bidders into the learned agent on the device, then (optionally) go on with PPO.

Every iteration records one episode of teacher days (StepEngine.teach_days): the `[32, 32]` tanh policy of
examples/train_mlp_policy_ppo.py acts on every observation - its input row and value are recorded, its action thrown away - and the
teacher (the oracle bidder, NaiveInterpolationStrategy or the zero-margin agent) acts in its place.  `im_update` then descends
the behaviour-cloning loss (--beta 0) or MARWIL's advantage-weighted one (--beta > 0) on the device; nothing of the record
crosses the bus.  AKNCP / NCP of the random initialisation, of the clone and of the teacher are printed on held-out keyword sets.
--finetune-ppo M continues with M iterations of PPO on the learner's own rollouts: the same trainer, the same theta and Adam
moments, a value network already fitted to the teacher's returns.

The free log_std is left as the policy has it (--train-log-std trains it): it is the scale each action component's error is
divided by.  The budget component is taken from the teacher's budget as it is.

Usage: python examples/pretrain_mlp_policy_bc.py [--teacher oracle|interpolation|zero_margin] [--iterations 50] [--beta 0]
                                                 [--finetune-ppo M] [--frames H] [--num-envs 4096] [--num-keywords 100]
"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import imitation, pg_trainer  # noqa: E402
from adcraft_amd.baselines.es_trainer import default_policy  # noqa: E402
from adcraft_amd.closed_loop import run_baseline_episode  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402
from examples.train_mlp_policy_ppo import with_value_network  # noqa: E402


def evaluate(name, policy, planes, days, budget):
    """(mean AKNCP, mean NCP) of an agent on the held-out keyword sets"""
    N, K = planes.shape[1:]
    e = StepEngine(N, K, max_days=days, seed=70)
    e.set_all_params(planes)
    e.reset()
    r = run_baseline_episode(e, name, steps=days, budget=budget, default_rpc=1.0, mlp=policy, deterministic=True, per_keyword_sums=False)
    e.close()
    return float(np.nanmean(r["AKNCP"])), float(np.mean(r["NCP"]))


def teacher_ready(eng, teacher):
    """what the teacher needs on the training engine, after every reset"""
    if teacher == "zero_margin":
        eng.agent_init(1.0)
    elif teacher == "interpolation":
        eng.interp_init()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher", choices=["oracle", "interpolation", "zero_margin"], default="oracle")
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--beta", type=float, default=0.0, help="0: behaviour cloning; > 0: MARWIL's exp(beta adv / c) weights")
    ap.add_argument("--vf-coef", type=float, default=1.0, help="the value loss's coefficient (0 drops it, as RLlib's BC does)")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--reward-scale", type=float, default=0.1)
    ap.add_argument("--train-log-std", action="store_true")
    ap.add_argument("--finetune-ppo", type=int, default=0, metavar="M", help="M iterations of PPO on the learner's own rollouts afterwards")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--num-keywords", type=int, default=100)
    ap.add_argument("--frames", type=int, default=1, metavar="H", help="the policy acts on the last H observations (1 to 8)")
    ap.add_argument("--days", type=int, default=60)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--eval-envs", type=int, default=1024)
    args = ap.parse_args()
    N, K, days, budget = args.num_envs, args.num_keywords, args.days, 100000.0
    held_out = synthetic.implicit_keyword_planes(args.eval_envs, K, seed=999, mean_volume=args.mean_volume)
    policy = with_value_network(default_policy(K, days=days, frames=args.frames), (32, 32))
    print(f"{'bc' if args.beta == 0 else 'marwil'} from {args.teacher}: {N} envs x {K} keywords, {days} teacher days per iteration; held-out: {args.eval_envs} envs")
    rows = [("teacher", evaluate(args.teacher, None, held_out, days, budget)), ("random init", evaluate("mlp", policy, held_out, days, budget))]
    for name, (akncp, ncp) in rows:
        print(f"{name:>14}: AKNCP {akncp:8.3f}  NCP {ncp:8.3f}")
    eng = StepEngine(N, K, max_days=days, seed=7)
    eng.set_all_params(synthetic.implicit_keyword_planes(N, K, seed=1, mean_volume=args.mean_volume))
    eng.reset()
    if args.teacher == "oracle":
        eng.bid_curves_build(2048)
    # (PPO's own options travel with the trainer: the fine-tuning below runs under them)
    config = pg_trainer.ppo(lr=args.lr, reward_scale=args.reward_scale)
    ppo_epochs = config.pop("epochs")
    config.pop("minibatches")
    trainer = imitation.ImitationTrainer(eng, policy, teacher=args.teacher, horizon=days, epochs=args.epochs, beta=args.beta, budget=budget,
                                         minibatches=args.minibatches, vf_coef=args.vf_coef, train_log_std=args.train_log_std, pg_options=config)
    rng = np.random.default_rng(5)
    print(f"{'iteration':>10} {'logp':>12} {'weight':>8} {'v loss':>10} {'ev':>7} {'AKNCP':>8} {'NCP':>8}")
    t0 = time.perf_counter()
    for it in range(1, args.iterations + 1):
        eng.reset(seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        teacher_ready(eng, args.teacher)
        st = trainer.iteration()
        if it % args.every == 0 or it == args.iterations:
            akncp, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
            print(f"{it:>10} {st['logp']:12.4f} {st['weight']:8.3f} {st['value_loss']:10.4f} {st['explained_variance']:7.3f} {akncp:8.3f} {ncp:8.3f}", flush=True)
    print(f"{args.iterations} imitation iterations in {time.perf_counter() - t0:.2f} s (evaluations included)")
    akncp, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
    print(f"{'clone':>14}: AKNCP {akncp:8.3f}  NCP {ncp:8.3f}")
    for it in range(1, args.finetune_ppo + 1):
        eng.reset(seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        eng.rollout_reset()
        eng.run_days("mlp", days, budget)
        st = eng.pg_update(ppo_epochs)
        if it % args.every == 0 or it == args.finetune_ppo:
            akncp, ncp = evaluate("mlp", trainer.policy(), held_out, days, budget)
            print(f"{'ppo ' + str(it):>10} {'':>12} {'':>8} {st['value_loss']:10.4f} {st['explained_variance']:7.3f} {akncp:8.3f} {ncp:8.3f}", flush=True)
    if args.finetune_ppo:
        print(f"{'clone + ppo':>14}: AKNCP {akncp:8.3f}  NCP {ncp:8.3f}")
    eng.close()


if __name__ == "__main__":
    main()
