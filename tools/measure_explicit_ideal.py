#!/usr/bin/env python3
"""GPU box: the ideal profit of EXPLICIT keywords at cfg2 size (4096 x 256 default-constructor keywords generated on the device, revenue x 12,
the notebooks' 299-point grid, n = 2048): episode-start ideal_profit, the curve build (k_explicit_curves + k_curve_contenders),
the per-step ideal on the contender lists and on the whole grid, and run_days("oracle") per day next to the step alone.
Usage: python tools/measure_explicit_ideal.py"""
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")


def _timed(f, reps, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    sync()
    return (time.perf_counter() - t0) / reps


def main(label):
    from adcraft_amd._ffi import MODEL_EXPLICIT
    from adcraft_amd.engine import StepEngine
    N, K = 4096, 256
    e = StepEngine(N, K, model=MODEL_EXPLICIT, seed=1729, drift_enabled=True, max_days=1 << 20, loss_threshold=1e12)
    e.reset(seeds=np.arange(N, dtype=np.uint64) + np.uint64(1729))
    e.generate_explicit_keywords()
    planes = e.get_all_params()
    planes[6:8] *= np.float32(12.0)         # the constructor's revenue never covers a cost of 2.2 or more: every ideal would be 0
    e.set_all_params(planes)
    e.ideal_profit(2048)                                            # (warm-up: module load, first allocation)
    t_ideal = _timed(lambda: e.ideal_profit(2048), 3, e.synchronize)
    e.bid_curves_build(2048)
    t_build = _timed(lambda: e.bid_curves_build(2048), 3, e.synchronize)
    count = e.bid_curves_contenders()[0]
    listed = count[count != 65535].astype(np.float64)
    e.sample_actions(0.3, 1.0, 1e9)
    for _ in range(5):
        e.ideal_step(fetch=False)
        e.step_device()
    t_step_ideal = _timed(lambda: e.ideal_step(fetch=False), 100, e.synchronize)
    e.metrics_enable(True)
    e.run_days("oracle", 4, budget=1000.0)
    days = 30
    t_day = _timed(lambda: e.run_days("oracle", days, budget=1000.0), 1, e.synchronize) / days
    e.sample_actions(0.3, 1.0, 1000.0)
    t_step = _timed(lambda: e.step_device(), 30, e.synchronize)
    print(f"{label:22s} N={N} K={K} grid=299 n=2048 (EXPLICIT)")
    print(f"  ideal_profit (episode start)      {t_ideal * 1e3:8.3f} ms")
    print(f"  bid_curves_build (+ contenders)   {t_build * 1e3:8.3f} ms")
    print(f"  ideal_step                        {t_step_ideal * 1e3:8.4f} ms")
    print(f"  run_days('oracle') per day        {t_day * 1e3:8.4f} ms   (step alone {t_step * 1e3:.4f} ms)")
    print(f"  contender lists: mean length {listed.mean():.1f}, max {int(listed.max())}, "
          f"whole grid {int((count == 65535).sum())} of {count.size} keywords")
    e.close()


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        for name, env in (("contender lists", {"ADCRAFT_IDEAL_FULL_SCAN": "0"}), ("whole grid", {"ADCRAFT_IDEAL_FULL_SCAN": "1"})):
            subprocess.check_call([sys.executable, __file__, name], env=dict(os.environ, **env))
