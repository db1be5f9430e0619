#!/usr/bin/env python3
"""A hyperparameter sweep of PPO as ONE engine: a learning-rate x entropy-coefficient x seed grid of independent learners that
collect and train in lock-step on the device.

Every grid cell is a member of a learner population (baselines/pg_trainer.py PGPopulationTrainer): it owns a contiguous block of
the envs, has its own policy network, value network, log_std, Adam moments and hyperparameters, and every kernel launch of an
update covers all members, so that the launches and host round trips of an update do not grow with the number of learners
(the measured cost against one learner at a time: profiles/pr_pg_population.txt).  What a member computes is bit
for bit what a single PGTrainer computes on an engine of its envs.  Nothing but numpy and the engine is loaded.

With --regimes the members are dealt over the paper's six environment regimes (dense, semi-dense, sparse, very sparse, and the
non-stationary dense and sparse ones), block by block, through the per-env parameter planes and the per-env drift selection: one
learner per (regime, grid cell).

Usage: python examples/sweep_ppo.py [--lrs 3e-4,1e-3,3e-3] [--ent-coefs 0,0.01] [--seeds 2] [--envs-per-member 64]
                                    [--num-keywords 25] [--days 10] [--iterations 20] [--regimes]
"""
import argparse
import itertools
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import synthetic  # noqa: E402
from adcraft_amd.baselines import pg_trainer  # noqa: E402
from adcraft_amd.baselines.es_trainer import default_policy  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402

# name: (mean auctions per keyword and day, conversion rate, keywords drift) - the six regimes of the paper's experiments
REGIMES = {"dense": (128, 0.8, False), "semi_dense": (64, 0.8, False), "sparse": (64, 0.1, False), "very_sparse": (16, 0.1, False),
           "non_stationary_dense": (128, 0.8, True), "non_stationary_sparse": (64, 0.1, True)}
DRIFT = (0.03, 0.03, 0.03)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lrs", default="3e-4,1e-3,3e-3")
    ap.add_argument("--ent-coefs", default="0,0.01")
    ap.add_argument("--seeds", type=int, default=2)
    ap.add_argument("--envs-per-member", type=int, default=64)
    ap.add_argument("--num-keywords", type=int, default=25)
    ap.add_argument("--days", type=int, default=10)
    ap.add_argument("--mean-volume", type=float, default=8.0, help="without --regimes: the sparse keyword law of the small learning shape")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--minibatch-size", type=int, default=None, metavar="S",
                    help="shuffled minibatches of S samples of a member instead of --minibatches env ranges (csrc/adc_pg_shuffle.h)")
    ap.add_argument("--queued-update", action="store_true", help="enqueue every update as one chain on the device, one host wait (the same bits)")
    ap.add_argument("--reward-scale", type=float, default=0.1)
    ap.add_argument("--normalize-rewards", action="store_true", help="one running reward normaliser per member, on the device")
    ap.add_argument("--regimes", action="store_true", help="deal the grid over the paper's six regimes: one learner per (regime, cell)")
    args = ap.parse_args()
    K, days, n, budget, hidden = args.num_keywords, args.days, args.envs_per_member, 100000.0, (32, 32)
    grid = list(itertools.product([float(x) for x in args.lrs.split(",")], [float(x) for x in args.ent_coefs.split(",")], range(args.seeds)))
    regimes = list(REGIMES) if args.regimes else [None]
    cells = [(r, lr, ent, seed) for r in regimes for lr, ent, seed in grid]
    M, N = len(cells), len(cells) * n
    # the envs' keyword sets and drift, block by block
    planes = np.concatenate([synthetic.implicit_keyword_planes(n, K, seed=1 + m, mean_volume=REGIMES[r][0] if r else args.mean_volume,
                                                               cvr=REGIMES[r][1] if r else 0.8) for m, (r, _, _, _) in enumerate(cells)], axis=1)
    eng = StepEngine(N, K, max_days=days, seed=7)
    eng.set_all_params(planes)
    if args.regimes:
        drifting = np.repeat([REGIMES[r][2] for r, _, _, _ in cells], n)
        eng.set_drift(True, DRIFT)
        eng.set_drift_mask(np.broadcast_to(drifting[:, None], (N, K)))
    eng.reset()
    policies = [member_policy(K, days, hidden, seed) for _, _, _, seed in cells]
    configs = [pg_trainer.ppo(lr=lr, ent_coef=ent, reward_scale=args.reward_scale, epochs=args.epochs, minibatches=args.minibatches)
               for _, lr, ent, _ in cells]
    if args.minibatch_size is not None:
        for c in configs:
            del c["minibatches"]
            c["minibatch_size"] = args.minibatch_size
    trainer = pg_trainer.PGPopulationTrainer(eng, policies, days, configs, normalize_rewards=args.normalize_rewards, queued_update=args.queued_update)
    batches = f"{args.minibatches} minibatches" if args.minibatch_size is None else f"shuffled minibatches of {args.minibatch_size} samples"
    print(f"{M} learners x {n} envs x {K} keywords on one engine, {days} days per iteration, {args.epochs} epochs x {batches}")
    print("member  " + " ".join(f"{m:>8d}" for m in range(M)))
    if args.regimes:
        print("regime  " + " ".join(f"{r[:8]:>8s}" for r, _, _, _ in cells))
    print("lr      " + " ".join(f"{lr:8.0e}" for _, lr, _, _ in cells))
    print("ent     " + " ".join(f"{ent:8.3f}" for _, _, ent, _ in cells))
    print("seed    " + " ".join(f"{seed:8d}" for _, _, _, seed in cells))
    rng = np.random.default_rng(5)
    t0 = time.perf_counter()
    for it in range(1, args.iterations + 1):
        trainer.iteration(days, budget, reset=True, reset_seeds=rng.integers(0, 2 ** 63, N).astype(np.uint64))
        print(f"{it:<7d} " + " ".join(f"{r:8.2f}" for r in trainer.returns()), flush=True)     # (the episode just collected, stochastic policy)
    dt = time.perf_counter() - t0
    eng.close()
    print(f"{args.iterations} iterations of {M} learners in {dt:.2f} s ({1e3 * dt / args.iterations:.1f} ms per iteration, fetching the rewards included)")


if __name__ == "__main__":
    main()
