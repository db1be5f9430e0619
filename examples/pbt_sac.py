#!/usr/bin/env python3
"""Population-based training of soft actor-critic on ONE engine: a small population of SAC learners trains in lock-step on the
device under a PBT scheduler (baselines/pbt.py PBTScheduler over SACPopulationTrainer).  The members' actor learning rates are
spread over two decades and their starting temperatures over one; half of the members have alpha_lr = 0, so their temperature
never takes a gradient step - for them the scheduler's explore of `alpha` is the search over the fixed temperature itself.
Every few iterations the worst quarter of the members become copies of members drawn among the best quarter (actor, critics,
target critics, optimiser moments, temperature cell and replay ring), with the donor's actor_lr times 0.8 or 1.25 and the
donor's temperature moved by log 0.8 or log 1.25 in the log domain, on the device.

Fitness, copy and perturbation run on the device (StepEngine.pbt_step): the launches and host round trips of a round do not
grow with the number of learners (profiles/pr_pbt_sac.txt).

The script prints the lineage (which starting member each member now descends from), the members' actor_lr and temperature,
and - for the best and the worst member by smoothed fitness - the deterministic policy's margin over the zero-margin agent on
held-out keyword sets, paired over the held-out envs, with its standard error.  It passes or fails on nothing: what PBT gains
in learning on this workload has not been measured.

Usage: python examples/pbt_sac.py [--members 8] [--envs-per-member 64] [--num-keywords 25] [--days 10] [--iterations 24] [--every 4]
"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "examples")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import sac_trainer  # noqa: E402
from adcraft_amd.baselines.pbt import PBTScheduler  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402
from train_mlp_policy_sac import evaluate, two_headed_policy  # noqa: E402

LR_LO, LR_HI = 3e-5, 3e-3
ALPHA_LO, ALPHA_HI = 0.02, 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--envs-per-member", type=int, default=64)
    ap.add_argument("--num-keywords", type=int, default=25)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--mean-volume", type=float, default=8.0)
    ap.add_argument("--iterations", type=int, default=24)
    ap.add_argument("--every", type=int, default=4, help="a PBT round every so many iterations")
    ap.add_argument("--updates", type=int, default=64, help="SAC updates of every member after every collected episode")
    ap.add_argument("--critic-hidden", default="32,32")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--reward-scale", type=float, default=0.1)
    ap.add_argument("--bid-lo", type=float, default=0.01)
    ap.add_argument("--bid-hi", type=float, default=3.0)
    ap.add_argument("--eval-envs", type=int, default=256)
    ap.add_argument("--print-every", type=int, default=4)
    ap.add_argument("--normalize-observations", action="store_true", help="a running observation filter per member; the rings hold raw rows")
    ap.add_argument("--normalize-rewards", action="store_true",
                    help="per member, the reward divided by the discounted return's running standard deviation (the entropy term is not scaled); what the normalisers gain here has not been measured")
    ap.add_argument("--prioritized-replay", action="store_true",
                    help="prioritised replay on the device (alpha 0.6, beta 0.4 annealed to 1 over the run); what it gains here has not been measured")
    ap.add_argument("--n-step", type=int, default=1, metavar="N",
                    help="n-step returns on the device (1: off; up to 16): a slot holds up to N days' discounted rewards and its own bootstrap discount; what it gains here has not been measured")
    args = ap.parse_args()
    K, days, n, M, budget = args.num_keywords, args.days, args.envs_per_member, args.members, 100000.0
    N = M * n
    planes = np.concatenate([synthetic.implicit_keyword_planes(n, K, seed=1 + m, mean_volume=args.mean_volume, cvr=0.8) for m in range(M)], axis=1)
    eng = StepEngine(N, K, max_days=days, seed=7)
    eng.set_all_params(planes)
    eng.reset()
    lrs, alphas = np.logspace(np.log10(LR_LO) + 0.5, np.log10(LR_HI) - 0.5, M), np.logspace(-1.0, 0.0, M)
    hidden = tuple(int(w) for w in args.critic_hidden.split(","))
    configs = [sac_trainer.sac(K, critic_hidden=hidden, learning_starts=days * n, updates_per_iteration=args.updates, batch_size=args.batch_size,
                               capacity=args.capacity, reward_scale=args.reward_scale, actor_lr=float(lrs[m]), init_alpha=float(alphas[m]),
                               alpha_lr=0.0 if m % 2 else 3e-4, critic_seed=m, n_step=args.n_step) for m in range(M)]
    lo = np.concatenate([[1.0], np.full(K, args.bid_lo)]).astype(np.float32)          # (the budget is overridden during training and evaluation)
    hi = np.concatenate([[budget], np.full(K, args.bid_hi)]).astype(np.float32)
    policies = [two_headed_policy(K, days, args.bid_lo, args.bid_hi, seed=m) for m in range(M)]
    trainer = sac_trainer.SACPopulationTrainer(eng, policies, configs, lo, hi, horizon=days,
                                               normalize_observations=args.normalize_observations, normalize_rewards=args.normalize_rewards,
                                               prioritized_replay=dict(alpha=0.6, beta=0.4, beta_final=1.0, beta_iterations=args.iterations) if args.prioritized_replay else None)
    scheduler = PBTScheduler(trainer, replace_fraction=0.25, tuned=("actor_lr", "alpha"), bounds={"actor_lr": (LR_LO, LR_HI), "alpha": (ALPHA_LO, ALPHA_HI)},
                             factors=(0.8, 1.25), fitness_ema=0.5, every=args.every, seed=11, with_ring=True)
    print(f"{M} SAC learners x {n} envs x {K} keywords on one engine, actor_lr {lrs[0]:.0e} .. {lrs[-1]:.0e}, alpha {alphas[0]:.2f} .. {alphas[-1]:.2f}, "
          f"alpha_lr 0 in every second member; {days} days and {args.updates} updates per iteration, a round every {args.every} iterations")
    rng = np.random.default_rng(5)
    replaced, t0, stats = 0, time.perf_counter(), None
    for it in range(1, args.iterations + 1):
        stats = trainer.iteration(days, budget, reset=True, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        returns = trainer.returns()
        if it < args.iterations:
            res = scheduler.step()
            if res is not None:
                replaced += int((res["src"] >= 0).sum())
                print(f"  round {len(scheduler.history)}: " + ", ".join(f"{m} <- {int(s)} (log alpha {res['hp'][m, 4]:+.3f})" for m, s in enumerate(res["src"]) if s >= 0)
                      + f"; lineage {scheduler.origin}", flush=True)
        if (it % args.print_every == 0 or it == args.iterations) and isinstance(stats, list):
            print(f"  {it:<4d} return best {returns.max():9.2f} mean {returns.mean():9.2f}  actor_lr " + " ".join(f"{c['actor_lr']:.0e}" for c in trainer.configs)
                  + "  alpha " + " ".join(f"{s['alpha']:.3f}" for s in stats), flush=True)
    seconds = time.perf_counter() - t0
    smoothed = scheduler.state()["smoothed"] if scheduler.history else trainer.returns()
    order = np.argsort(smoothed, kind="stable")
    print(f"{args.iterations} iterations in {seconds:.2f} s; {replaced} members replaced in {len(scheduler.history)} rounds; lineage {scheduler.origin}, "
          f"surviving {sorted(set(scheduler.origin))}")
    print("alpha_lr per member: " + " ".join(f"{c['alpha_lr']:.0e}" for c in trainer.configs))
    held_out = synthetic.implicit_keyword_planes(args.eval_envs, K, seed=999, mean_volume=args.mean_volume)
    zm_ret, zm_ncp = evaluate("zero_margin", None, held_out, days, budget)
    print(f"held-out ({args.eval_envs} envs): zero-margin return {zm_ret.mean():.2f} NCP {zm_ncp:.3f}")
    for label, m in (("best", int(order[-1])), ("worst", int(order[0]))):
        ret, ncp = evaluate("mlp", trainer.policy(m), held_out, days, budget)
        diff = ret - zm_ret                                      # (paired: the same held-out envs, seeds and days)
        print(f"  {label:5s} member {m} (from {scheduler.origin[m]}): return {ret.mean():10.2f} NCP {ncp:7.3f} margin {diff.mean():10.2f} "
              f"s.e. {diff.std(ddof=1) / np.sqrt(len(diff)):8.2f}")
    eng.close()


if __name__ == "__main__":
    main()
