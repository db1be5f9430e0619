"""G13 (tools/gen_golden_interp.py: the reference's NaiveInterpolationStrategy, run unmodified) against the numpy
restatement (tests/interp_ref.py) and the host twin of the device's act (adc_interp_act_host)."""
import math

import numpy as np
import pytest

from tests import interp_ref as R


@pytest.fixture(scope="module")
def g13(golden):
    return golden("g13_interpolation_agent.json")["cases"]


def _cent(key):
    return int(round(key * 100))


def check_touched(cache, t):
    """the entry the update touched: [key, ave_clicks, n_clicks, ave_cpc (NaN: none), n_cpc]"""
    key, clk, n_clk, cpc, n_cpc = t
    assert cache.max_observed >= key
    c = _cent(key)
    if not 1 <= c <= 300:
        return
    assert float(cache.clicks[c][0]) == clk and cache.clicks[c][1] == n_clk
    if n_cpc == 0:
        assert math.isnan(cpc) and c not in cache.cpc
    else:
        assert cache.cpc[c][0] == cpc and cache.cpc[c][1] == n_cpc


def check_full(cache, want):
    """a full cache dump: [ave_rpc, num_rpc_obs, ave_sctr, num_sctr_obs, clicks entries, cpc entries]"""
    ave_rpc, n_rpc, ave_sctr, n_sctr, clicks, cpc = want
    assert float(cache.ave_rpc) == ave_rpc and cache.n_rpc == n_rpc and cache.n_sctr == n_sctr
    assert n_sctr == 0 or float(cache.ave_sctr) == ave_sctr
    assert cache.max_observed == max([k for k, _, _ in clicks] + [0.03])
    assert {_cent(k): [v, n] for k, v, n in clicks if 1 <= _cent(k) <= 300} == \
        {c: [float(v), n] for c, (v, n) in cache.clicks.items()}
    assert {_cent(k): [v, n] for k, v, n in cpc if 1 <= _cent(k) <= 300} == {c: [v, n] for c, (v, n) in cache.cpc.items()}


def replay(case, on_act=None):
    """the restatement through every step of a case; on_act(ref, grid, step, uniforms) runs before each act"""
    K = case["K"]
    ref = R.InterpAgentRef(1, K, case["threshold"], case["bid_step"])
    for t, s in enumerate(case["steps"]):
        ref.update([s["prev_bids"]], [s["clicks"]], [s["cost"]], [s["conversions"]], [s["revenue"]])
        for k in range(K):
            check_touched(ref.caches[0][k], s["touched"][k])
        grid = R.g13_grid(case, s)
        u = np.array(s["uniforms"])
        if on_act:
            on_act(ref, grid, s, u)
        bids, drew = ref.act(grid, [np.where(np.isnan(u), 0.5, u)])
        assert list(bids[0]) == s["bids"], t
        assert np.array_equal(drew[0], np.isfinite(u)), t
        assert ref.budget[0] == s["budget"] and ref.profit_beliefs[0] == s["profit_beliefs"], t
        assert ref.cost_beliefs[0] == s["cost_beliefs"], t
        if "caches" in s:
            for k in range(K):
                check_full(ref.caches[0][k], s["caches"][k])
    return ref


def test_g13_covers_the_cases_it_is_for(g13):
    assert len(g13) == 6
    assert [c["grid_kind"] for c in g13] == [0, 0, 1, 1, 2, 0]
    assert any(b < 0 for b in sum((s["prev_bids"] for s in g13[5]["steps"]), []))
    assert any(b > 3 for b in sum((s["prev_bids"] for s in g13[5]["steps"]), []))
    assert max(len(R.g13_grid(g13[2], s)) for s in g13[2]["steps"]) > 100
    assert sum(len(k[5]) for k in g13[4]["steps"][-1]["caches"]) > 20      # the shuffled case reaches the interpolation


def test_restatement_replays_every_g13_step(g13):
    for case in g13:
        replay(case)


def test_host_twin_gives_g13_bid_for_every_keyword_step(g13):
    from adcraft_amd import _ffi
    lib = _ffi.lib()
    seen = [0]

    def on_act(ref, grid, s, u):
        for k in range(len(s["bids"])):
            _, _, idx, bid, _ = R.twin_act(lib, ref.caches[0][k], grid, ref.threshold, ref.bid_step,
                                           0.5 if np.isnan(u[k]) else float(u[k]))
            assert bid == s["bids"][k] and (idx >= 0) == bool(np.isfinite(u[k]))
            seen[0] += 1
    for case in g13:
        replay(case, on_act)
    assert seen[0] == sum(c["K"] * c["T"] for c in g13)
