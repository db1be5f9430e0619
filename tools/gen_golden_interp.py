#!/usr/bin/env python3
"""G13: traces of the REFERENCE's NaiveInterpolationStrategy (adcraft/baselines/interpolated_expectations.py:298-439),
imported unmodified, driven as its notebooks drive it (G10's recipe: update_all_caches -> sample_action -> env step).

The campaign is the reference's simulate_epoch_of_bidding_on_campaign on keywords from its quantile sampler, with the
stand-ins of tools/gen_golden.py.  The agent's rng is wrapped so that every choice() records the one uniform it used,
without restating choice: snapshot bit_generator.state, draw u from a twin generator set to that state, call the real
choice, and assert that both states agree afterwards.  Which keywords drew is read from the agent's own
get_profit_acquisition_function (wrapped on the instance: a keyword draws exactly when it returns a distribution).

Cases: (a) defaults, dense and sparse keyword sets, 60 days; (b) the notebook's run_ie_agent (threshold -0.1, the grid
np.arange(0.01, max_bid + 0.01, 0.01) growing from 0.10 by 0.03 a day up to 3.0, env budget 1000, cache_tensors_to_floats),
rpc_action_replace off and on; (c) a shuffled grid with half cents and points above $3.00, bid_step 0.05; (d) previous
bids supplied by the caller: half-cent float32 values, 0, negative values, values above 3.00.

Stored per step: the previous bids given to the update, the observation (float32 values), the grid in force (its index in
the case's `grids`, or for the growing grid its length: a prefix of np.arange(0.01, 3.01, 0.01)), the uniforms (NaN: no
draw), the bids (float64), the budget, profit_beliefs, cost_beliefs, and per keyword the cache entry the update touched
[key, ave_clicks, n_clicks, ave_cpc (NaN: none), n_cpc].  Full caches every 10th step and after the last:
per keyword [ave_rpc, num_rpc_obs, ave_sctr, num_sctr_obs, [[key, ave_clicks, n], ...], [[key, ave_cpc, n], ...]].

Usage: python tools/gen_golden_interp.py      (rewrites tests/golden/g13_interpolation_agent.json; byte-reproducible)
"""
import json
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

ARANGE = np.arange(0.01, 3.01, 0.01)
_rng = np.random.default_rng(1313)
SHUFFLED = _rng.permutation(np.concatenate([np.arange(0.005, 1.2, 0.01), np.arange(0.01, 1.5, 0.01), [3.05, 3.5, 4.2]]))
GRID_KINDS = ["default", "growing", "shuffled"]      # grid_kind in the file: 0 np.linspace(0.01, 3.00, 300), 1 growing, 2 grids[0]
CALLER_BIDS = [0.015, 0.125, 0.375, 1.005, 2.995, 0.0, -0.4, 3.7, 12.0, 0.005]

CASES = [
    dict(name="a_dense", seed=21, agent_seed=0, K=8, T=60, mean_volume=64, cvr=0.8, threshold=-0.2, bid_step=0.03, grid="default"),
    dict(name="a_sparse", seed=22, agent_seed=1, K=8, T=60, mean_volume=4, cvr=0.2, threshold=-0.2, bid_step=0.03, grid="default"),
    dict(name="b_notebook", seed=23, agent_seed=2, K=6, T=40, mean_volume=32, cvr=0.5, threshold=-0.1, bid_step=0.03, grid="growing",
         budget=1000.0, floats=True, replace=False),
    dict(name="b_notebook_replace", seed=23, agent_seed=2, K=6, T=40, mean_volume=32, cvr=0.5, threshold=-0.1, bid_step=0.03,
         grid="growing", budget=1000.0, floats=True, replace=True),
    dict(name="c_shuffled", seed=25, agent_seed=4, K=6, T=40, mean_volume=32, cvr=0.5, threshold=-0.2, bid_step=0.05, grid="shuffled"),
    dict(name="d_caller_bids", seed=26, agent_seed=5, K=6, T=40, mean_volume=32, cvr=0.5, threshold=-0.2, bid_step=0.03, grid="default",
         caller=True),
]


class RecordingRng:
    """stands where agent.rng stands; sample_action only ever calls .choice()"""

    def __init__(self, rng):
        self.rng, self.draws = rng, []

    def choice(self, a, p=None):
        state = self.rng.bit_generator.state
        twin = np.random.Generator(np.random.PCG64())
        twin.bit_generator.state = state
        u = float(twin.random())
        out = self.rng.choice(a, p=p)
        assert self.rng.bit_generator.state == twin.bit_generator.state, "choice consumed other than one double"
        self.draws.append(u)
        return out


def cache_tensors_to_floats(cache):          # example_compute_metrics.ipynb cell 9, verbatim behaviour
    cache["ave_rpc"] = float(cache["ave_rpc"])
    cache["ave_sctr"] = float(cache["ave_sctr"])
    cache["ave_clicks"] = {k: [float(v[0]), v[1]] for k, v in cache["ave_clicks"].items()}


def f(x):
    return float(x)


def touched(ie, cache, bid):
    key = ie.bidstr(float(np.float32(bid)))
    c = cache["ave_clicks"].get(key)
    p = cache["ave_cpc"].get(key)
    return [float(key), f(c[0]), int(c[1]), f(p[0]) if p else float("nan"), int(p[1]) if p else 0]


def full_caches(caches):
    out = []
    for c in caches:
        out.append([f(c["ave_rpc"]), int(c["num_rpc_obs"]), f(c["ave_sctr"]), f(c["num_sctr_obs"]),
                    [[float(k), f(v[0]), int(v[1])] for k, v in c["ave_clicks"].items()],
                    [[float(k), f(v[0]), int(v[1])] for k, v in c["ave_cpc"].items()]])
    return out


def main():
    warnings.filterwarnings("ignore")
    G.install_standins()
    from adcraft import bidding_simulation as b, gymnasium_kw_utils as u
    from adcraft.experiment_utils import experiment_quantiles as eq
    import adcraft.baselines.interpolated_expectations as ie
    out = []
    for cs in CASES:
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(cs["seed"])))
        cfg, _ = G.quant_cfg(eq, cs["mean_volume"], cs["cvr"], None)
        _, params = u.sample_implicit_keywords_from_quantile_dfs(cs["K"], rng, cfg)
        kws = []
        for p in params:
            vol = (float(p[0][0]), float(p[0][1]))
            kw, _ = u.generate_implicit_keyword_from_params(vol, G.f32x(p[1]), G.f32x(1.0 / p[2]), G.f32x(p[3]), G.f32x(p[4]),
                                                            G.f32x(p[5]), G.f32x(p[6]), rng)
            kw.volume_sampler = (lambda m, s: (lambda: int(np.floor(max(rng.normal(m, max(s, 1e-12)), 0.0) + 0.5))))(vol[0], vol[1])
            kws.append(kw)
        K = cs["K"]
        max_bid = 0.1
        if cs["grid"] == "default":
            grid = np.linspace(0.01, 3.00, 300)
        elif cs["grid"] == "shuffled":
            grid = SHUFFLED.copy()
        else:
            grid = np.arange(0.01, max_bid + 0.01, 0.01)
        agent = ie.NaiveInterpolationStrategy(K, profit_acquisition_threshold=cs["threshold"], allowed_bids=grid,
                                              seed=cs["agent_seed"], bid_step=cs["bid_step"])
        rec = RecordingRng(agent.rng)
        agent.rng = rec
        drew = []
        orig = agent.get_profit_acquisition_function

        def acq(expected_margin, index, _orig=orig, _drew=drew):
            r = _orig(expected_margin, index)
            if r is not None:
                _drew.append(index)
            return r
        agent.get_profit_acquisition_function = acq
        obs = {k: np.zeros(K) for k in ("impressions", "buyside_clicks", "cost", "sellside_conversions", "revenue")}
        action = {"budget": 0.0, "keyword_bids": 0.01 + np.zeros((K,))}
        crng = np.random.default_rng(cs["seed"] + 1000)
        steps = []
        for t in range(cs["T"]):
            prev = np.array(action["keyword_bids"], dtype=np.float64)
            if cs.get("caller") and t % 3 == 1:
                pick = crng.random(K) < 0.6
                prev = np.where(pick, np.array([CALLER_BIDS[i] for i in crng.integers(0, len(CALLER_BIDS), K)]), prev)
                action = {"budget": action["budget"], "keyword_bids": prev}
            agent.update_all_caches(action, obs)
            touch = [touched(ie, agent.caches[i], prev[i]) for i in range(K)]
            if cs["grid"] == "growing":
                agent.allowed_bids = grid
                assert np.array_equal(grid, ARANGE[:len(grid)])
            drew.clear()
            rec.draws = []
            new = agent.sample_action()
            assert len(rec.draws) == len(drew)
            uni = [float("nan")] * K
            for i, d in zip(drew, rec.draws):
                uni[i] = d
            if cs.get("floats"):
                for c in agent.caches:
                    cache_tensors_to_floats(c)
            step = dict(prev_bids=[float(x) for x in prev],
                        clicks=[f(np.float32(x)) for x in obs["buyside_clicks"]], cost=[f(np.float32(x)) for x in obs["cost"]],
                        conversions=[f(np.float32(x)) for x in obs["sellside_conversions"]],
                        revenue=[f(np.float32(x)) for x in obs["revenue"]],
                        grid=len(grid) if cs["grid"] == "growing" else 0,
                        uniforms=uni, bids=[float(x) for x in new["keyword_bids"]], budget=float(new["budget"]),
                        profit_beliefs=float(agent.profit_beliefs), cost_beliefs=float(agent.cost_beliefs), touched=touch)
            if (t + 1) % 10 == 0 or t == cs["T"] - 1:
                step["caches"] = full_caches(agent.caches)
            steps.append(step)
            env_bids = np.array(new["keyword_bids"], dtype=np.float64)
            if cs.get("replace"):
                rpcs = [max([0.01, agent.caches[i]["ave_rpc"] * agent.caches[i]["ave_sctr"]]) for i in range(K)]
                for i, c in enumerate(agent.caches):
                    if c["num_sctr_obs"] > 2 and rpcs[i] > 0.01:
                        env_bids[i] = round(rpcs[i], 2)
            oc = b.simulate_epoch_of_bidding_on_campaign(kws, [float(x) for x in np.round(env_bids, 2)], cs.get("budget", 100000.0))
            obs = dict(
                impressions=np.array([o["impressions"] for o in oc]),
                buyside_clicks=np.array([o["buyside_clicks"] for o in oc]),
                sellside_conversions=np.array([o["sellside_conversions"] for o in oc]),
                cost=np.array([float(np.sum(o["costs"])) if len(o["costs"]) else 0.0 for o in oc]),
                revenue=np.array([float(np.sum(o["revenues"])) if len(o["revenues"]) else 0.0 for o in oc]))
            action = {"budget": new["budget"], "keyword_bids": env_bids}
            if cs["grid"] == "growing":
                max_bid = min([max_bid + 0.03, 3.0])
                grid = np.arange(0.01, max_bid + 0.01, 0.01)
        out.append(dict(K=K, T=cs["T"], threshold=cs["threshold"], bid_step=cs["bid_step"],
                        grid_kind=GRID_KINDS.index(cs["grid"]), grids=[[float(x) for x in SHUFFLED]] if cs["grid"] == "shuffled" else [],
                        steps=steps))
        n_draw = sum(int(np.isfinite(s["uniforms"]).sum()) for s in steps)
        n_cpc = sum(len(c[5]) for c in steps[-1]["caches"])
        print(cs["name"], "done:", n_draw, "draws,", n_cpc, "cpc points at the end")
    path = os.path.join(G.OUT, "g13_interpolation_agent.json")
    with open(path, "w") as fh:
        json.dump(dict(cases=out), fh, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
