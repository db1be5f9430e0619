"""What tests/test_gpu_io_shapes.py holds the device to, checked where no device is needed: every precondition of
tests/io_shapes.py on the oracle and the numpy restatements in the engine's place, the restatements themselves (the flat row,
the packed counts, the float-money models' cents), and the interpolation agent's host twin adc_interp_act_host against
InterpAgentRef on the closed loop at K = 300 and 257, its terms summed in keyword order as the kernel's thread 0 sums them."""
import numpy as np
import pytest

from tests import interp_ref as IR
from tests import io_shapes as S

F = np.float32


@pytest.fixture(scope="module")
def lib():
    from adcraft_amd import _ffi
    return _ffi.lib()


# ---- 1. the zero-margin agent -----------------------------------------------------------------------------------------------------------
def test_zero_margin_precondition_holds_on_the_oracle():
    c = S.AGENT
    o = S.oracle_after_reset(S.planes_for(c), c["env_seeds"], max_days=c["days"])
    run, obs = S.AgentRun(), S.no_observation(c["N"], c["K"])
    for _ in range(c["days"]):
        a = run.day(obs)
        assert a["bids"].dtype == F and np.array_equal(np.rint(a["bids"].astype(np.float64) * 100.0), a["bid_cents"])
        obs = S.observation(o.step(a["bids"], a["budget"]))
    run.precondition("host agent")
    assert np.all(run.ref.max_bids[:, S.LANES:] > 0.01) and np.any(run.ref.num_rpc_obs[:, 2 * S.LANES:] > 0)


# ---- 2. the interpolation agent and its host twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", S.INTERP["Ks"])
def test_interp_twin_equals_the_restatement_on_the_closed_loop(lib, K):
    c = S.INTERP
    o = S.oracle_after_reset(S.interp_planes(K), c["env_seeds"], max_days=c["days"])
    run, obs = S.InterpRun(c["N"], K), S.no_observation(c["N"], K)
    draws = 0
    for t in range(c["days"]):
        a = run.day(obs)
        ref = run.ref
        for n in range(c["N"]):
            ec = ep = 0.0                                   # thread 0 of k_interp_step: the keywords' terms in keyword order
            for k in range(K):
                cache = ref.caches[n][k]
                margin, cost, idx, bid, _ = IR.twin_act(lib, cache, run.GRID, ref.threshold, ref.bid_step, float(run.uniforms[n, k]))
                assert (idx >= 0) == bool(a["drew"][n, k]) and bid == a["grid_bids"][n, k], (t, n, k)
                if idx >= 0:
                    ec = ec + (cost[idx] if cache.n_sctr > 0 else bid)
                    ep = ep + (margin[idx] if cache.n_rpc > 0 else 0.0)
                    draws += 1
            assert ec == ref.cost_beliefs[n] and ep == ref.profit_beliefs[n], (t, n)
        obs = S.observation(o.step(a["bids"], a["budget"]))
    run.precondition(f"host interp K={K}")
    assert draws > c["N"] * K * (c["days"] - 1) // 2


# ---- 3. the outputs ---------------------------------------------------------------------------------------------------------------------
def test_outputs_second_pass_precondition_holds_on_the_oracle():
    c = S.OUTPUTS
    N, K = c["N"], c["K"]
    assert (N * K, K // 4, N * K - c["first_pass"]) == (267168, 253, 5024)
    planes = S.planes_for(c)
    seeds = np.arange(N, dtype=np.uint64) + 100
    o = S.oracle_after_reset(planes, seeds, threads=8)
    bids = o.sample_bids(0.3, 1.0)
    obs = S.observation(o.step(bids, 1.0e9))
    assert S.second_pass("host outputs", obs) == [259, 260, 261, 262, 263]
    counts, clipped = S.packed(obs)
    assert not clipped and all(np.array_equal(p, obs[k]) and p.dtype == np.uint16 for p, k in zip(counts, S.PER_KEYWORD))
    # the engine whose last entry is clipped
    planes2, bids2 = S.clip_last_keyword(planes, bids)
    o = S.oracle_after_reset(planes2, seeds, threads=8)
    obs2 = S.observation(o.step(bids2, 1.0e9))
    S.clipped_entry("host outputs clipped", obs2)
    counts, clipped = S.packed(obs2)
    assert clipped and counts[0][-1, -1] == 65535 and np.array_equal(counts[0].reshape(-1)[:-1], obs2["impressions"].reshape(-1)[:-1])
    assert all(np.array_equal(obs2[k][:-1], obs[k][:-1]) for k in S.PER_KEYWORD), "the other envs are untouched"


# ---- 4. the packing route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,pageable", [s + (False,) for s in S.PACK["shapes"]] + [S.PACK["pageable"] + (True,)])
def test_pack_precondition_holds_on_the_oracle(N, K, pageable):
    o = S.oracle_after_reset(S.planes_for(S.PACK, N, K), np.arange(N, dtype=np.uint64) + 200)
    obs = S.observation(o.step(o.sample_bids(0.3, 1.0), 1.0e9))
    S.pack_route(f"host pack {N}x{K}", obs, pageable)
    assert S.PACK["odd_K"] % 2 == 1


# ---- 5. flat I/O ------------------------------------------------------------------------------------------------------------------------
def test_flat_row_is_the_sorted_key_concatenation():
    K = 5
    obs = dict(impressions=np.arange(K)[None] + 10, buyside_clicks=np.arange(K)[None] + 20, sellside_conversions=np.arange(K)[None] + 30,
               cost=np.arange(K, dtype=F)[None] + F(40.5), revenue=np.arange(K, dtype=F)[None] + F(50.5),
               cumulative_profit=np.array([-7.25]), days_passed=np.array([3]))
    row = S.flat_rows(obs)
    assert row.shape == (1, 5 * K + 2) and row.dtype == F
    want = np.concatenate([obs["buyside_clicks"][0], obs["cost"][0], [-7.25, 3.0], obs["impressions"][0], obs["revenue"][0],
                           obs["sellside_conversions"][0]]).astype(F)
    assert np.array_equal(row[0], want)


@pytest.mark.parametrize("K", S.FLAT["Ks"])
def test_flat_precondition_holds_on_the_oracle(K):
    c = S.FLAT
    N = c["N"]
    o = S.oracle_after_reset(S.planes_for(c, K=K), np.arange(N, dtype=np.uint64) + 300)
    actions = S.flat_actions(o)
    obs = S.observation(o.step(actions[:, 1:], actions[:, 0]))
    S.flat_shape(f"host flat K={K}", obs, actions)
    assert S.flat_rows(obs).shape == (N, 5 * K + 2) and sum(c["mask"]) not in (0, N)


@pytest.mark.parametrize("K", S.FLAT["Ks"])
def test_masked_reset_precondition_holds_on_the_oracle(K):
    """the second of three days on sampled bids and budgets of $900 and $901, where the GPU case resets three envs of seven"""
    c = S.FLAT
    o = S.oracle_after_reset(S.planes_for(c, K=K), np.arange(c["N"], dtype=np.uint64) + 300, max_days=5)
    for step in range(2):
        ref = o.step(o.sample_bids(0.25, 1.25), 900.0 + step)
    S.masked_reset(f"host masked reset K={K}", S.observation(ref), c["mask"])


# ---- 6. the metric readers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["implicit", "explicit"])
def test_metric_precondition_holds_on_the_oracle(model):
    o, planes, implicit = S.metric_oracle(model)
    sums = S.metric_run(o, implicit)
    sums.precondition(f"host metrics {model}")
    N = S.METRICS["N"]
    assert sums.scalars[1] == len(S.METRICS["budgets"]) * N and sums.scalars[2] == N, "every env ends one episode in four days of three"
    if implicit:
        assert sums.scalars[0] == sums.nk.sum(), "integer money: the envs' profit is the keywords'"


def test_float_money_cents_are_the_kernels_roundings():
    """k_metric_accumulate: rintf(revenue * 100.0f) in float32, rint((double)cost * 100.0) in float64"""
    ref = dict(revenue_cents=np.array([[1, 250, 1234567]]), cost=np.array([[0.005, 0.125, 2.675]]), reward=np.array([1.004999]),
               cost_cents=np.zeros((1, 3), np.int64))
    nk, env = S.metric_cents(ref, implicit=False)
    cost32 = ref["cost"].astype(F).astype(np.float64)
    assert nk.tolist() == [[1 - round(cost32[0, 0] * 100), 250 - round(cost32[0, 1] * 100), 1234567 - round(cost32[0, 2] * 100)]]
    assert env.tolist() == [100]
    nk, env = S.metric_cents(dict(ref, cost_cents=np.array([[1, 2, 3]])), implicit=True)
    assert nk.tolist() == [[0, 248, 1234564]] and env.tolist() == [1234812]


# ---- 7. more envs than 65 535 -----------------------------------------------------------------------------------------------------------
def test_many_envs_precondition_holds_on_the_oracle():
    c = S.MANY_ENVS
    N = c["N"]
    o = S.oracle_after_reset(S.planes_for(c), np.arange(N, dtype=np.uint64) + 400, threads=8)
    bids = o.sample_bids(0.3, 1.0)
    S.many_envs("host many envs", S.observation(o.step(bids, 1.0e9)), bids)


def test_reset_keys_are_splitmix64_of_the_seed():
    """(the value the GPU cases compare get_rng_state() with) splitmix64's published first output for state 0"""
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF and S.reset_keys([0]).dtype == np.uint64
