#!/usr/bin/env python3
"""Chained step time at the cfg5 shape (2048 x 1024, dense law, drift on, non-binding budget) under three drift settings
(profiles/pr_drift_mask.txt): no selection (every keyword drifts, adc_engine_set_drift's scalars), half of every env's
keywords selected (adc_engine_set_drift_mask, a different random half per env), and per-env magnitudes
(adc_engine_set_env_drift, every keyword).  Every setting runs on a fresh engine with the same keywords and actions; the
settings alternate over `--reps` rounds and each figure is the GPU time of `--steps` step_device() calls (one event pair
around them) / steps, after `--warmup` untimed steps.

With --resource-usage MAIN.txt BRANCH.txt (the stderr of two `hipcc -Rpass-analysis=kernel-resource-usage` builds of
adcraft_amd/csrc/adc_engine.hip) the file also gets the VGPR / scratch / occupancy table of the step kernels of both builds.

    python tools/measure_drift_mask.py [--reps 5] [--steps 200] [--warmup 20] [--resource-usage main.txt branch.txt]
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the kernels whose resources the selection must leave alone (demangled-name prefixes)
KERNELS = ("k_step_implicit_fast", "k_step_implicit_sparse", "k_step_exact_rows", "k_step_rest_of_day", "k_rest_walk",
           "k_step_explicit_fast", "k_step_float_day", "k_step_explicit_rows", "k_step_general_fast", "k_step_general_small",
           "k_materialize_drift", "k_force_drift")


def run(setting, N, K, steps, warmup, planes):
    from adcraft_amd.engine import StepEngine
    e = StepEngine(N, K, seed=1729, max_days=60, loss_threshold=1.0e12, drift_enabled=True, auto_reset=True)
    e.set_all_params(planes)
    e.reset()
    rng = np.random.default_rng(5)
    if setting == "half":
        m = np.zeros((N, K), bool)
        for n in range(N):
            m[n, rng.permutation(K)[:K // 2]] = True
        e.set_drift_mask(m)
    elif setting == "per-env rates":
        e.set_env_drift(rng.uniform(0.01, 0.1, (N, 3)).astype(np.float32))
    e.sample_actions(0.30, 1.00, 1.0e9)
    for _ in range(warmup):
        e.step_device()
    e.synchronize()
    e.region_begin()
    for _ in range(steps):
        e.step_device()
    ms = e.region_end() / steps
    kernel = e.step_kernel_name()
    e.close()
    return ms, kernel


def resource_table(path):
    """{kernel: (VGPRs, AGPRs, scratch bytes/lane, occupancy waves/SIMD)} from -Rpass-analysis=kernel-resource-usage remarks"""
    import subprocess
    out, name = {}, None
    with open(path) as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                try:
                    name = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
                except OSError:
                    pass
                out[name] = {}
                continue
            m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
            if m and name:
                out[name][m.group(1).split()[0]] = int(m.group(2))
    return out


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"^adck::", "", name)
    return re.sub(r"\(.*$", "", name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--keywords", type=int, default=1024)
    ap.add_argument("--resource-usage", nargs=2, metavar=("MAIN", "BRANCH"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_drift_mask.txt"))
    a = ap.parse_args()
    lines = []
    if a.resource_usage:
        tabs = [resource_table(p) for p in a.resource_usage]
        lines.append("resource usage of the step kernels, main -> branch (VGPRs, AGPRs, scratch B/lane, occupancy waves/SIMD):")
        changed = 0
        for name in sorted(set(tabs[0]) | set(tabs[1])):
            if not short(name).startswith(KERNELS):
                continue
            r = [t.get(name, {}) for t in tabs]
            f = ["{}/{}/{}/{}".format(x.get("VGPRs", "-"), x.get("AGPRs", "-"), x.get("ScratchSize", "-"), x.get("Occupancy", "-")) for x in r]
            same = f[0] == f[1]
            changed += not same
            lines.append(f"  {short(name) if len(short(name)) < 60 else short(name)[:57] + '...':60s} {f[0]:>14s} -> {f[1]:<14s}{'' if same else '  CHANGED'}")
            lines.append(f"      {name}")
        lines.append(f"  kernels whose resources changed: {changed}")
        lines.append("")
    if a.reps > 0:
        from adcraft_amd import synthetic
        N, K = a.envs, a.keywords
        planes = synthetic.implicit_keyword_planes(N, K, seed=1729, mean_volume=128, cvr=0.8, no_vol_prob=0.0)
        settings = ("mask None", "half", "per-env rates")
        res = {s: [] for s in settings}
        kern = {}
        for r in range(a.reps):
            for s in (settings if r % 2 == 0 else settings[::-1]):
                ms, kern[s] = run(s, N, K, a.steps, a.warmup, planes)
                res[s].append(ms)
                print(f"rep {r} {s:14s} {ms:.4f} ms/step", flush=True)
        lines.append(f"chained step_device() at {N} x {K} (cfg5 law: mean volume 128, cvr 0.8, drift on, non-binding budget), "
                     f"{a.steps} steps after {a.warmup} warm-up, {a.reps} alternated rounds, GPU ms per step:")
        base = float(np.median(res["mask None"]))
        for s in settings:
            v = np.asarray(res[s])
            lines.append(f"  {s:14s} median {np.median(v):.4f}  min {v.min():.4f}  max {v.max():.4f}  "
                         f"({(np.median(v) / base - 1) * 100:+.1f} % against mask None)   first-pass kernel {kern[s]}")
            lines.append(f"  {'':14s} all: " + " ".join(f"{x:.4f}" for x in v))
        lines.append("  (per-env rates: magnitudes drawn from [0.01, 0.1] instead of 0.03, so the keywords drift elsewhere and the "
                     "auctions' work differs too; half: the same draws, half of them not taken)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
