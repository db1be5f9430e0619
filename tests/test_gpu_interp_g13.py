"""G13 through the C ABI: the reference's NaiveInterpolationStrategy runs (tools/gen_golden_interp.py) replayed on the device
agent with the reference's previous bids, observations, grids and uniforms - bids to the cent, the action buffer as the env
rounds them, float64 budget and beliefs and the caches bit for bit."""
import math

import numpy as np
import pytest

from tests import interp_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _cent(key):
    return int(round(key * 100))


def _entries(ent, k):
    """{cent: [ave, n]} of both lists of keyword k of env 0"""
    m, q = ent["n_clicks"][0, k], ent["n_cpc"][0, k]
    clicks = {int(c): [float(v), int(n)] for c, v, n in zip(ent["clicks_cent"][0, k, :m], ent["ave_clicks"][0, k, :m],
                                                            ent["clicks_count"][0, k, :m])}
    cpc = {int(c): [float(v), int(n)] for c, v, n in zip(ent["cpc_cent"][0, k, :q], ent["ave_cpc"][0, k, :q], ent["cpc_count"][0, k, :q])}
    return clicks, cpc


def test_g13_through_the_c_abi_with_replayed_uniforms(amd, golden):
    for ci, case in enumerate(golden("g13_interpolation_agent.json")["cases"]):
        K, T = case["K"], case["T"]
        e = amd.StepEngine(1, K, seed=5, max_days=T)
        grid = R.g13_grid(case, case["steps"][0])
        e.interp_init(case["threshold"], case["bid_step"], grid, 0)
        for t, s in enumerate(case["steps"]):
            e.interp_update(np.array([s["prev_bids"]]), np.array([s["clicks"]]), np.array([s["cost"]]), np.array([s["conversions"]]),
                            np.array([s["revenue"]]))
            ent, st = e.interp_entries(), e.interp_state()
            for k in range(K):
                key, clk, n_clk, cpc, n_cpc = s["touched"][k]
                assert st["max_observed"][0, k] >= key
                c = _cent(key)
                if 1 <= c <= 300:
                    clicks, cpcs = _entries(ent, k)
                    assert clicks[c] == [clk, n_clk], (ci, t, k)
                    assert (c not in cpcs and math.isnan(cpc)) if n_cpc == 0 else cpcs[c] == [cpc, n_cpc], (ci, t, k)
            g = R.g13_grid(case, s)
            if case["grid_kind"] == 1:
                e.interp_set_allowed_bids(g)
            u = np.array(s["uniforms"])
            e.interp_act(0.0, np.where(np.isnan(u), 0.5, u)[None, :])
            st = e.interp_state()
            bids, budget = e.get_actions()
            idx = st["bid_index"][0]
            assert list(np.where(idx >= 0, g[np.maximum(idx, 0)], 0.01)) == s["bids"], (ci, t)
            assert np.array_equal(idx >= 0, np.isfinite(u)), (ci, t)
            want = np.maximum(np.rint(np.array(s["bids"]) * 100.0), 1.0) / 100.0
            assert np.array_equal(bids[0], want.astype(np.float32)), (ci, t)
            assert st["budget"][0] == s["budget"] and st["profit_beliefs"][0] == s["profit_beliefs"], (ci, t)
            assert st["cost_beliefs"][0] == s["cost_beliefs"], (ci, t)
            assert budget[0] == np.float32(np.rint(s["budget"] * 100.0) / 100.0), (ci, t)
            if "caches" in s:
                ent = e.interp_entries()
                for k in range(K):
                    ave_rpc, n_rpc, ave_sctr, n_sctr, clicks, cpc = s["caches"][k]
                    assert float(st["ave_rpc"][0, k]) == ave_rpc and st["num_rpc_obs"][0, k] == n_rpc, (ci, t, k)
                    assert st["num_sctr_obs"][0, k] == n_sctr and (n_sctr == 0 or float(st["ave_sctr"][0, k]) == ave_sctr), (ci, t, k)
                    assert st["max_observed"][0, k] == max([key for key, _, _ in clicks] + [0.03]), (ci, t, k)
                    got_clicks, got_cpc = _entries(ent, k)
                    assert got_clicks == {_cent(key): [v, n] for key, v, n in clicks if 1 <= _cent(key) <= 300}, (ci, t, k)
                    assert got_cpc == {_cent(key): [v, n] for key, v, n in cpc if 1 <= _cent(key) <= 300}, (ci, t, k)
        e.close()
