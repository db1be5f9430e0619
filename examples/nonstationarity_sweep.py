#!/usr/bin/env python3
"""A non-stationarity sweep in ONE engine: drift rate x drifting fraction of the keywords, 16 runs per cell.

Every cell is 16 (env seed, agent seed) runs as in examples/heatmap_closed_loop.py, and every run is one env of a single
engine: the cell's drift magnitude goes to its envs through set_env_drift (updater_params' three numbers, per env) and its
drifting fraction through set_drift_mask (per env; here the reference's prefix rule of a partial updater_mask,
gymnasium_kw_utils.effective_updater_mask, applied to a mask of the first `fraction * K` keywords - which it keeps as is).
One run_days("zero_margin") call then plays the whole sweep: the agent, the ideal profit of the drifted keywords and the
step for every env, every day.  Prints AKNCP / NCP per cell (the mean over its runs).

Usage: python examples/nonstationarity_sweep.py [--rates 0 0.03 0.1 0.3] [--fractions 0.25 0.5 1.0] [--num-keywords 100]
"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from adcraft_amd import gymnasium_kw_utils as utils  # noqa: E402
from adcraft_amd.closed_loop import run_baseline_episode  # noqa: E402
from adcraft_amd.engine import StepEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rates", type=float, nargs="+", default=[0.0, 0.03, 0.1, 0.3])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.25, 0.5, 1.0])
    ap.add_argument("--volume", type=float, default=128.0)
    ap.add_argument("--cvr", type=float, default=0.8)
    ap.add_argument("--num-keywords", type=int, default=100)
    ap.add_argument("--days", type=int, default=60)
    args = ap.parse_args()
    runs = [(es, ag) for es in range(5, 9) for ag in range(0, 4)]
    cells = [(r, f) for r in args.rates for f in args.fractions]
    R, K = len(runs), args.num_keywords
    N = len(cells) * R
    cfg = utils.experiment_keyword_config(args.volume, args.cvr)
    one = np.zeros((8, R, K), np.float32)
    for i, (es, _) in enumerate(runs):                                   # env.reset(seed=env_seed): the reference's draws
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(es)))
        one[:, i] = utils.implicit_params_to_planes(utils.sample_implicit_keyword_params(K, rng, cfg))
    planes = np.tile(one, (1, len(cells), 1))                           # every cell starts from the same 16 keyword sets
    rates = np.zeros((N, 3), np.float32)
    masks = np.zeros((N, K), bool)
    for c, (r, f) in enumerate(cells):
        rates[c * R:(c + 1) * R] = r
        masks[c * R:(c + 1) * R, :int(round(f * K))] = True
    t0 = time.perf_counter()
    eng = StepEngine(N, K, max_days=args.days, loss_threshold=10000.0, drift_enabled=True)
    eng.set_all_params(planes)
    eng.reset(seeds=np.array([1000 * es + ag for es, ag in runs] * len(cells), dtype=np.uint64))
    eng.set_drift_mask(utils.effective_updater_mask(masks))
    eng.set_env_drift(rates)
    res = run_baseline_episode(eng, "zero_margin", steps=args.days, budget=100000.0, default_rpc=1.0,
                               agent_seeds=np.array([ag for _, ag in runs] * len(cells), dtype=np.uint64))
    eng.close()
    print(f"{'rate':>6} {'fraction':>8} {'AKNCP':>8} {'NCP':>8}   (mean over {R} runs of {args.days} days, K = {K}, "
          f"volume {args.volume:g}, cvr {args.cvr:g})")
    for c, (r, f) in enumerate(cells):
        s = slice(c * R, (c + 1) * R)
        print(f"{r:6.3f} {f:8.2f} {np.mean(res['AKNCP'][s]):8.3f} {np.mean(res['NCP'][s]):8.3f}")
    print(f"{len(cells)} cells x {R} runs x {args.days} days as {N} envs of one engine in {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()
