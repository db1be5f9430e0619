"""Every entry point of the engine that stages a host array through a device temporary (DevTemps, csrc/parts/host_api.inc), at the
smallest shapes that reach it - 3 envs x 5 keywords, and 257 keywords for the per-keyword grids that round up to 256 - and the
refusals whose order a shared staging helper could disturb, each by its whole sentence.  The tape's two users (step_replay,
outcomes_replay_tape) run on the reference's recorded tapes in tests/test_gpu_parity.py (test_g3_implicit_replay_on_gpu,
test_g3_explicit_replay_on_gpu, test_g3_outcome_lists_on_gpu_element_for_element); only their drift refusal is here."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

N = 3
SHAPES = [5, 257]


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _engine(amd, K, model=0, seed=5, **kw):
    e = amd.StepEngine(N, K, model=model, seed=seed, **kw)
    e.set_all_params(H.implicit_params(N, K, seed=seed) if model == 0 else H.explicit_params(N, K, seed=seed))
    e.reset(seeds=np.arange(N, dtype=np.uint64) + np.uint64(100))
    return e


def _stepped(amd, K, seed=5):
    """an engine one step after its reset, and that step's observation"""
    e = _engine(amd, K, seed=seed)
    bids = np.random.default_rng(seed).uniform(0.3, 1.0, (N, K)).astype(np.float32)
    return e, e.step(bids, 1.0e9)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _refused(exc, sentence, call):
    with pytest.raises(exc) as info:
        call()
    assert str(info.value) == sentence


@pytest.mark.parametrize("K", SHAPES)
def test_agent_update_with_host_arrays_equals_the_update_on_the_last_observation(amd, K):
    states = []
    for host in (False, True):
        e, out = _stepped(amd, K)
        e.agent_init(seeds=np.arange(N, dtype=np.uint64) + np.uint64(7))
        if host:
            e.agent_update(out["buyside_clicks"], out["sellside_conversions"], out["revenue"])
        else:
            e.agent_update()
        states.append(e.agent_state())
        e.close()
    assert (states[0]["num_rpc_obs"] > 0).any()
    _same(states[0], states[1])


@pytest.mark.parametrize("K", SHAPES)
def test_interp_update_with_host_arrays_equals_the_update_on_the_last_observation(amd, K):
    states, entries = [], []
    for host in (False, True):
        e, out = _stepped(amd, K)
        e.interp_init(seeds=np.arange(N, dtype=np.uint64) + np.uint64(7))
        if host:        # (the agent's own last bid after interp_init is 0.01)
            e.interp_update(np.full((N, K), 0.01), out["buyside_clicks"], out["cost"], out["sellside_conversions"], out["revenue"])
        else:
            e.interp_update()
        states.append(e.interp_state())
        entries.append(e.interp_entries())
        e.close()
    assert (entries[0]["n_clicks"] > 0).any()
    _same(states[0], states[1])
    assert entries[0].pop("capacity") == entries[1].pop("capacity")
    _same(entries[0], entries[1])


def test_acts_on_replay_uniforms_are_repeatable(amd):
    K = 5
    e, _ = _stepped(amd, K)
    u = np.random.default_rng(3).random((N, K))
    e.agent_init()
    e.agent_update()
    e.interp_init()
    e.interp_update()
    for act in (e.agent_act, e.interp_act):
        act(0.0, u)
        first = e.get_actions()
        act(0.0, u)
        again = e.get_actions()
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    e.close()


@pytest.mark.parametrize("K", SHAPES)
def test_reset_with_mask_and_seeds_touches_the_masked_envs_only(amd, K):
    e, _ = _stepped(amd, K)
    keys1, ticks1 = e.get_rng_state()
    mask = np.array([1, 0, 1], np.uint8)
    seeds = np.array([11, 12, 13], np.uint64)
    e.reset(env_mask=mask, seeds=seeds)
    keys2, ticks2 = e.get_rng_state()
    days, _ = e.get_episode_state()
    e.close()
    fresh = _engine(amd, K)
    fresh.reset(seeds=seeds)
    keys_ref, ticks_ref = fresh.get_rng_state()
    fresh.close()
    assert keys2[1] == keys1[1] and ticks2[1] == ticks1[1] and days[1] == 1
    assert ticks1[1] != ticks_ref[1]                    # (the step moved it: untouched is not the same as reset)
    for n in (0, 2):
        assert keys2[n] == keys_ref[n] and ticks2[n] == ticks_ref[n] and days[n] == 0
        assert keys2[n] != keys1[n]


@pytest.mark.parametrize("K", SHAPES)
def test_keyword_generation_with_a_mask_leaves_the_other_envs_bit_identical(amd, K):
    from adcraft_amd import gymnasium_kw_utils as utils
    table = utils.generate_simple_experiment_quantiles(16, 0.1)
    mask = np.array([0, 1, 0], np.uint8)
    for model in (0, 1):
        e = _engine(amd, K, model=model)
        generate = (lambda **kw: e.generate_keywords(table, **kw)) if model == 0 else e.generate_explicit_keywords
        generate()
        before = e.get_all_params()
        generate(env_mask=mask, serial=1)
        after = e.get_all_params()
        e.close()
        assert np.array_equal(after[:, mask == 0], before[:, mask == 0])
        assert not np.array_equal(after[:, mask == 1], before[:, mask == 1])


@pytest.mark.parametrize("model", [0, 1])
def test_ideal_profit_and_the_cached_curves_repeat_on_one_engine(amd, model):
    K = 5
    e = _engine(amd, K, model=model)
    grid = np.arange(0.05, 2.0, 0.05)
    rounds = []
    for _ in range(2):
        ideal = e.ideal_profit(64, grid)
        e.bid_curves_build(64, grid)
        rounds.append((ideal,) + e.bid_curves_fetch())
    e.close()
    assert np.isfinite(rounds[0][0]).all() and (rounds[0][1] > 0).any()
    for a, b in zip(*rounds):
        assert np.array_equal(a, b)


def test_akncp_ncp_twice(amd):
    K = 5
    e = _engine(amd, K)
    e.metrics_enable()
    e.bid_curves_build(64, np.arange(0.05, 2.0, 0.05))
    e.ideal_step(fetch=False)
    e.step(np.full((N, K), 0.6, np.float32), 1.0e9)
    first = e.metrics_akncp_ncp(1.0)
    again = e.metrics_akncp_ncp(1.0)
    e.close()
    for a, b in zip(first, again):
        assert a.shape == (N,) and np.array_equal(a, b, equal_nan=True)


def test_refusals_by_their_whole_sentence(amd):
    from adcraft_amd import _ffi
    from adcraft_amd import gymnasium_kw_utils as utils
    K = 5
    e, out = _stepped(amd, K)
    L, h = e._lib, e._h
    clicks = np.ascontiguousarray(out["buyside_clicks"], dtype=np.int32)
    cost = np.ascontiguousarray(out["cost"], dtype=np.float32)
    prev = np.full((N, K), 0.01)
    # the agent that was never initialised is named before the partial set of arrays is
    _refused(_ffi.EngineStateError, "adc_engine_agent_init has not been called",
             lambda: _ffi.check(L.adc_engine_agent_update(h, clicks.ctypes.data, None, None)))
    e.agent_init()
    _refused(ValueError, "pass all of clicks/conversions/revenue, or none (= the engine's last observation)",
             lambda: _ffi.check(L.adc_engine_agent_update(h, clicks.ctypes.data, None, None)))
    # ... while the interpolation agent counts its arrays first
    _refused(ValueError, "pass all of prev_bids/clicks/cost/conversions/revenue, or none",
             lambda: _ffi.check(L.adc_engine_interp_update(h, prev.ctypes.data, clicks.ctypes.data, cost.ctypes.data, clicks.ctypes.data, None)))
    e.interp_init()
    _refused(ValueError, "pass all of prev_bids/clicks/cost/conversions/revenue, or none",
             lambda: _ffi.check(L.adc_engine_interp_update(h, prev.ctypes.data, clicks.ctypes.data, cost.ctypes.data, clicks.ctypes.data, None)))
    _refused(_ffi.EngineStateError, "adc_engine_bid_curves_build has not been called",
             lambda: _ffi.check(L.adc_engine_bid_curves_fetch(h, None, None)))
    # a table whose fifth quantity has no bucket, with a mask: the four tables before it are already on their way to the device
    before = e.get_all_params()
    table = utils.generate_simple_experiment_quantiles(16, 0.1)
    table["count_sctr"] = [0]
    _refused(ValueError, "every quantity needs at least one bucket",
             lambda: e.generate_keywords(table, env_mask=np.array([1, 0, 1], np.uint8)))
    assert np.array_equal(e.get_all_params(), before)
    # drift uniforms on a tape, drift off on the engine: refused after the tape's other arrays were uploaded
    tape = amd.ReplayTape(N, np.zeros((N, K), np.int32), drift_uniforms=np.zeros((3, N, K)))
    _refused(ValueError, "tape carries drift coefficients but drift is not enabled on this engine",
             lambda: e.step_replay(np.full((N, K), 0.5, np.float32), 1.0, tape))
    _refused(ValueError, "tape carries drift coefficients but drift is not enabled on this engine",
             lambda: e.outcomes_replay(0, np.full(K, 0.5, np.float32), 1.0, tape=tape))
    # the engine works on: the agents update on host arrays, the envs step
    e.agent_update(out["buyside_clicks"], out["sellside_conversions"], out["revenue"])
    e.interp_update(prev, out["buyside_clicks"], out["cost"], out["sellside_conversions"], out["revenue"])
    assert e.step(np.full((N, K), 0.6, np.float32), 1.0e9)["days_passed"].tolist() == [2] * N
    e.close()
