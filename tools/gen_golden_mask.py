#!/usr/bin/env python3
"""G14: update_keywords() of the REFERENCE (adcraft/gymnasium_kw_env.py:114-158) under partial updater masks, imported
unmodified with the stand-ins of tools/gen_golden.py.

The reference draws three uniform vectors of length num_updates = sum(mask) and zips them with the keyword list, so only
keywords 0..num_updates-1 are visited: keyword k moves iff mask[k] and k < sum(mask), with the k-th entry of each vector
(SURVEY B-6).  The vectors are recorded by drawing them from a clone of the generator state (as gen_g4 does), with
size=(sum(mask),).

Cases: a True beyond the prefix (it must not move), a mask whose only True lies beyond the prefix (nothing moves),
alternating over K = 8, all-False, a sequence that calls set_updater_mask between updates, two updater_params settings.
Stored per step: the mask in force, the three vectors, and keyword_params after the update.

Usage: python tools/gen_golden_mask.py      (rewrites tests/golden/g14_partial_updater_mask.json; byte-reproducible)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

T, F = True, False
UP_A = [["vol", 0.03], ["ctr", 0.03], ["cvr", 0.03]]
UP_B = [["vol", 0.2], ["ctr", 0.5], ["cvr", 0.9]]
CASES = [
    # masks: one per step (a change between two steps is set_updater_mask)
    dict(name="beyond_prefix", seed=41, K=6, mean_volume=128, cvr=0.8, up=UP_A, masks=[[T, F, T, T, F, T]] * 4),
    dict(name="only_beyond_prefix", seed=42, K=6, mean_volume=64, cvr=0.5, up=UP_A, masks=[[F, F, F, T, F, F]] * 3),
    dict(name="alternating", seed=43, K=8, mean_volume=32, cvr=0.5, up=UP_B, masks=[[T, F] * 4] * 4),
    dict(name="all_false", seed=44, K=5, mean_volume=64, cvr=0.8, up=UP_A, masks=[[F] * 5] * 2),
    dict(name="set_between", seed=45, K=7, mean_volume=16, cvr=0.1, up=UP_B,
         masks=[[T] * 7, [T, F, T, T, F, T, F], [F, T, F, T, T, F, T], [T, T, F, F, F, F, F], [F] * 7, [T] * 7]),
]


def gen_g14(env_mod, eq):
    cases = []
    for c in CASES:
        cfg, _ = G.quant_cfg(eq, c["mean_volume"], c["cvr"])
        K, up = c["K"], c["up"]
        env = env_mod.BiddingSimulation(keyword_config=cfg, num_keywords=K, updater_params=up, updater_mask=c["masks"][0])
        env.reset(seed=c["seed"])
        p0 = G.params_to_json(env.keyword_params)
        steps = []
        for mask in c["masks"]:
            if list(mask) != list(env.updater_mask):
                env.set_updater_mask(mask)
            n = int(env.num_updates)
            st = env.np_random.bit_generator.state
            clone = np.random.Generator(np.random.PCG64())
            clone.bit_generator.state = st
            draws = [G.L(clone.uniform(-v[1], v[1], size=(n,))) for v in up]
            env.update_keywords()
            assert env.np_random.bit_generator.state == clone.bit_generator.state      # the clone drew what the env drew
            steps.append(dict(mask=[bool(x) for x in mask], num_updates=n, uniforms=draws,
                              params=G.params_to_json(env.keyword_params)))
        cases.append(dict(name=c["name"], seed=c["seed"], K=K, mean_volume=c["mean_volume"], conversion_rate=c["cvr"],
                          updater_params=up, params0=p0, steps=steps))
    G.dump("g14_partial_updater_mask.json", dict(
        source="adcraft/gymnasium_kw_env.py:105-158 (set_updater_mask, update_keywords) on an env reset with a seed, executed "
               "unmodified; uniforms = the three vectors of length sum(mask) the call drew (vol, ctr, cvr)",
        cases=cases))


def main():
    G.install_standins()
    from adcraft import gymnasium_kw_env as env_mod
    from adcraft.experiment_utils import experiment_quantiles as eq
    gen_g14(env_mod, eq)


if __name__ == "__main__":
    main()
