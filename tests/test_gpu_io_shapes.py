"""GPU tests of the step's callers and its host-facing I/O at the shapes where their index arithmetic takes another path (DESIGN
2x; the shapes and their preconditions are tests/io_shapes.py's):

1. the zero-margin agent at K = 600 (passes of 256, 256 and 88 keywords) with the budget it reduces itself, and in env groups;
2. the interpolation agent at K = 300 and 257 with thread 0's ordered sums and its own budget, and in env groups;
3. k_outputs_to_host past one pass of its grid (264 x 1012), with int32 and with packed counts, a clipped count, and the same step
   fetched into pageable memory;
4. k_pack_counts, which no test ran: K mod 4 = 2 and a pageable uint16 target;
5. the flat I/O and the small (ceil(K / 256), N) kernels at K = 257 and 600, with a masked reset;
6. the metric readers at 301 x 300: five envs a slab, empty trailing slabs, a second pass of the reduce; IMPLICIT and EXPLICIT;
7. an engine of 65 537 envs: gridDim.y past 65 535.
Every device result is compared bit for bit with the oracle and the numpy restatements; every case first asserts, on the
reference alone, the precondition that makes it able to fail, and prints what it measured.  Measured figures:
profiles/pr_io_shapes.txt."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import io_shapes as S
from tests.test_gpu_interp_agent import _assert_caches, _grid_bids

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


def _engine(amd, planes, env_seeds, **kw):
    """StepEngine after set_all_params and reset(seeds): its keys are those tests/io_shapes.py gives the oracle without a device"""
    e = amd.StepEngine(planes.shape[1], planes.shape[2], seed=17, **kw)
    e.set_all_params(planes)
    e.reset(seeds=np.asarray(env_seeds, np.uint64))
    keys, ticks = e.get_rng_state()
    assert np.array_equal(keys, S.reset_keys(env_seeds)) and not ticks.any()
    return e


def _seeds(N, base):
    return np.arange(N, dtype=np.uint64) + base


def _assert_obs(got, want, what=""):
    for k, v in want.items():
        assert np.array_equal(got[k], v), (k, what)


# ======================================================================================================================================
# 1. the zero-margin agent past one pass
# ======================================================================================================================================
def test_zero_margin_agent_at_three_passes_reduces_its_own_budget(amd):
    c = S.AGENT
    N, K = c["N"], c["K"]
    e = _engine(amd, S.planes_for(c), c["env_seeds"], max_days=c["days"])
    e.agent_init(c["default_rpc"], np.array(c["agent_seeds"], np.uint64))
    run, obs = S.AgentRun(), S.no_observation(N, K)
    for t in range(c["days"]):
        e.agent_step(0.0)
        want = run.day(obs)
        bids, budget = e.get_actions()
        assert np.array_equal(np.rint(bids.astype(np.float64) * 100.0), want["bid_cents"]), t
        assert np.array_equal(bids, want["bids"]), t
        assert budget.dtype == F and np.array_equal(budget, want["budget"]), (t, budget, want["budget"])
        st, ref = e.agent_state(), run.ref
        assert np.array_equal(st["ave_rpc"], ref.ave_rpc) and np.array_equal(st["num_rpc_obs"], ref.num_rpc_obs), t
        assert np.array_equal(st["num_sctr_obs"], ref.num_sctr_obs) and np.array_equal(st["max_bids"], ref.max_bids), t
        assert np.array_equal(st["ave_sctr"][ref.num_sctr_obs > 0], ref.ave_sctr[ref.num_sctr_obs > 0]), t
        e.step_device()
        obs = e.fetch()
    e.close()
    run.precondition("gpu agent")


def _agent_days(amd, groups):
    c = S.AGENT_GROUPS
    N, K = c["N"], c["K"]
    e = _engine(amd, S.planes_for(S.AGENT, N, K), _seeds(N, 40), max_days=c["days"])
    e.set_env_groups(groups)
    e.agent_init(1.0, _seeds(N, 50))
    e.run_days("zero_margin", c["days"], budget=0.0, graph=False)
    assert e.env_groups() == groups
    out = e.fetch(), e.agent_state(), e.get_actions()
    e.close()
    return out


def test_zero_margin_agent_days_in_env_groups_equal_one_group(amd):
    (oa, sa, aa), (ob, sb, ab) = _agent_days(amd, 1), _agent_days(amd, S.AGENT_GROUPS["groups"])
    _assert_obs(ob, oa)
    _assert_obs(sb, sa)
    assert np.array_equal(aa[0], ab[0]) and np.array_equal(aa[1], ab[1])
    budget = aa[1]
    S.log("gpu agent groups", budgets=budget.tolist(), clicks_past_keyword_512=int(oa["buyside_clicks"][:, 512:].sum()))
    assert len(set(budget.tolist())) > 1 and np.all(budget >= 100.0 * S.AGENT_GROUPS["K"]) and oa["buyside_clicks"][:, 512:].sum() > 0


# ======================================================================================================================================
# 2. the interpolation agent past one pass
# ======================================================================================================================================
@pytest.mark.parametrize("K", S.INTERP["Ks"])
def test_interp_agent_past_one_pass_sums_every_keyword_in_order(amd, K):
    c = S.INTERP
    N = c["N"]
    e = _engine(amd, S.interp_planes(K), c["env_seeds"], max_days=c["days"])
    e.interp_init(-0.2, 0.03, None, 0, np.array(c["agent_seeds"], np.uint64))
    run, obs = S.InterpRun(N, K), S.no_observation(N, K)
    for t in range(c["days"]):
        e.interp_step(0.0)
        want = run.day(obs)
        st, ref = e.interp_state(), run.ref
        assert np.array_equal(_grid_bids(st, run.GRID), want["grid_bids"]) and np.array_equal(st["bid_index"] >= 0, want["drew"]), t
        assert np.array_equal(st["budget"], ref.budget), (t, st["budget"], ref.budget)
        assert np.array_equal(st["cost_beliefs"], ref.cost_beliefs), (t, st["cost_beliefs"], ref.cost_beliefs)
        assert np.array_equal(st["profit_beliefs"], ref.profit_beliefs), (t, st["profit_beliefs"], ref.profit_beliefs)
        bids, budget = e.get_actions()
        assert np.array_equal(bids, want["bids"]), t
        assert budget.dtype == F and np.array_equal(budget, want["budget"]), (t, budget, want["budget"])
        e.step_device()
        obs = e.fetch()
    _assert_caches(e, run.ref)
    e.close()
    run.precondition(f"gpu interp K={K}")


def _interp_days(amd, groups):
    c = S.INTERP_GROUPS
    N, K = c["N"], c["K"]
    e = _engine(amd, S.interp_planes(K, N), _seeds(N, 60), max_days=c["days"])
    e.set_env_groups(groups)
    e.interp_init(-0.2, 0.03, None, 0, _seeds(N, 70))
    e.run_days("interpolation", c["days"], 0.0, graph=False)
    assert e.env_groups() == groups
    out = e.interp_state(), e.interp_entries(), e.fetch(), e.get_actions()
    e.close()
    return out


def test_interp_agent_days_in_env_groups_equal_one_group(amd):
    base, got = _interp_days(amd, 1), _interp_days(amd, S.INTERP_GROUPS["groups"])
    for a, b in zip(base[:3], got[:3]):
        _assert_obs(b, a)
    assert np.array_equal(base[3][0], got[3][0]) and np.array_equal(base[3][1], got[3][1])
    points = int(base[1]["n_cpc"][:, S.LANES:].sum())
    S.log("gpu interp groups", cpc_points_past_keyword_256=points, profit_beliefs=base[0]["profit_beliefs"].tolist())
    assert points >= 20 and len(set(base[0]["profit_beliefs"].tolist())) == S.INTERP_GROUPS["N"]


# ======================================================================================================================================
# 3. k_outputs_to_host's second pass
# ======================================================================================================================================
def _pageable(amd, e, compact):
    """(out, packed, overflow, adc_step_out) over plain numpy arrays laid out as the engine's own output arrays are"""
    out, packed, overflow = amd._alloc_outputs(lambda shape, dt: np.zeros(shape, dt), e.num_envs, e.num_keywords, compact,
                                               *amd._out_offsets(e._lib, e._h))
    return out, packed, overflow, amd._out_struct(out, packed, overflow, 0, e.num_envs)


def _fetch_pageable(amd, e, compact=False):
    from adcraft_amd._ffi import check
    out, packed, overflow, struct = _pageable(amd, e, compact)
    check(e._lib.adc_engine_fetch(e._h, C.byref(struct)))
    return out, overflow


def _assert_packed(e, got, obs, what=""):
    want, _ = S.packed(obs)
    for k, w in zip(S.PER_KEYWORD, want):
        assert got[k].dtype == np.uint16 and np.array_equal(got[k], w), (k, what)
    assert np.array_equal(e._counts_u16, np.stack(want, axis=1)), what


@pytest.mark.parametrize("compact", [False, True], ids=["int32", "compact"])
def test_outputs_to_host_past_one_pass_of_its_grid(amd, compact):
    c = S.OUTPUTS
    N, K = c["N"], c["K"]
    planes = S.planes_for(c)
    e = _engine(amd, planes, _seeds(N, 100), compact_counts=compact)
    o = H.mirror_oracle(e, planes, threads=8)
    bids = o.sample_bids(0.3, 1.0)
    ref = o.step(bids, 1.0e9)
    obs = S.observation(ref)
    S.second_pass(f"gpu outputs compact={compact}", obs)
    got = e.step(bids, 1.0e9)
    H.assert_step_equal(got, ref)
    if compact:
        _assert_packed(e, got, obs)
        assert not e._overflow.any()
    # the same step into pageable memory: the block copy (int32 counts), or the packing kernel and piecewise copies
    out, overflow = _fetch_pageable(amd, e, compact)
    H.assert_step_equal(out, ref)
    if compact:
        assert all(np.array_equal(out[k], w) for k, w in zip(S.PER_KEYWORD, S.packed(obs)[0])) and not overflow.any()
    e.close()


def test_outputs_to_host_clips_the_last_entry_of_its_second_pass(amd):
    c = S.OUTPUTS
    N, K = c["N"], c["K"]
    planes = S.planes_for(c)
    planes, bids = S.clip_last_keyword(planes, S.oracle_after_reset(planes, _seeds(N, 100)).sample_bids(0.3, 1.0))
    e = _engine(amd, planes, _seeds(N, 100), compact_counts=True)
    o = H.mirror_oracle(e, planes, threads=8)
    obs = S.observation(o.step(bids, 1.0e9))
    S.clipped_entry("gpu outputs clipped", obs)
    with pytest.raises(OverflowError):
        e.step(bids, 1.0e9)
    assert e.out["impressions"][-1, -1] == 65535 and obs["impressions"][-1, -1] > 65535
    _assert_packed(e, e.out, obs)
    for k in ("cost", "revenue", "reward", "cumulative_profit", "days_passed"):
        assert np.array_equal(e.out[k], obs[k]), k
    assert not e._overflow.any(), "the flag is cleared for the next step"
    e.close()


# ======================================================================================================================================
# 4. k_pack_counts
# ======================================================================================================================================
@pytest.mark.parametrize("N,K", S.PACK["shapes"])
def test_pack_counts_where_k_is_even_and_no_multiple_of_four(amd, N, K):
    planes = S.planes_for(S.PACK, N, K)
    e = _engine(amd, planes, _seeds(N, 200), compact_counts=True)
    o = H.mirror_oracle(e, planes)
    for step in range(2):
        bids = o.sample_bids(0.3, 1.0)
        ref = o.step(bids, 1.0e9)
        obs = S.observation(ref)
        S.pack_route(f"gpu pack {N}x{K} step {step}", obs)
        got = e.step(bids, 1.0e9)
        H.assert_step_equal(got, ref)
        _assert_packed(e, got, obs, step)
        assert not e._overflow.any()
    e.close()


def test_pack_counts_into_a_pageable_array(amd):
    N, K = S.PACK["pageable"]
    planes = S.planes_for(S.PACK, N, K)
    e = _engine(amd, planes, _seeds(N, 200))
    o = H.mirror_oracle(e, planes)
    bids = o.sample_bids(0.3, 1.0)
    ref = o.step(bids, 1.0e9)
    obs = S.observation(ref)
    S.pack_route(f"gpu pack {N}x{K} pageable", obs, pageable=True)
    H.assert_step_equal(e.step(bids, 1.0e9), ref)
    out, overflow = _fetch_pageable(amd, e, compact=True)
    H.assert_step_equal(out, ref)
    assert all(out[k].dtype == np.uint16 and np.array_equal(out[k], w) for k, w in zip(S.PER_KEYWORD, S.packed(obs)[0]))
    assert not overflow.any()
    e.close()


def test_pack_counts_clips_and_raises(amd):
    N, K = S.PACK["shapes"][0]
    planes = S.planes_for(S.PACK, N, K)
    planes, bids = S.clip_last_keyword(planes, S.oracle_after_reset(planes, _seeds(N, 200)).sample_bids(0.3, 1.0))
    e = _engine(amd, planes, _seeds(N, 200), compact_counts=True)
    o = H.mirror_oracle(e, planes)
    obs = S.observation(o.step(bids, 1.0e9))
    S.clipped_entry("gpu pack clipped", obs)
    with pytest.raises(OverflowError):
        e.step(bids, 1.0e9)
    assert e.out["impressions"][-1, -1] == 65535
    _assert_packed(e, e.out, obs)
    e.close()


def test_compact_counts_refuse_an_odd_keyword_count(amd):
    N, K = 2, S.PACK["odd_K"]
    e = _engine(amd, S.planes_for(S.PACK, N, K), _seeds(N, 200), compact_counts=True)
    with pytest.raises(ValueError, match="even num_keywords"):
        e.step(np.full((N, K), 0.5, F), 1.0e9)
    e.close()


# ======================================================================================================================================
# 5. flat I/O past one tile
# ======================================================================================================================================
def _flat_obs(e, N, K):
    from adcraft_amd import _ffi
    from tests.hip_ctypes import read_device
    p, nbytes = e.device_buffer(_ffi.BUF_FLAT_OBS)
    return read_device(p, nbytes, F, (N, 5 * K + 2))


@pytest.mark.parametrize("K", S.FLAT["Ks"])
def test_step_flat_past_one_tile(amd, K):
    c = S.FLAT
    N = c["N"]
    planes = S.planes_for(c, K=K)
    e = _engine(amd, planes, _seeds(N, 300))
    o = H.mirror_oracle(e, planes)
    for step in range(2):
        actions = S.flat_actions(o)
        ref = o.step(actions[:, 1:], actions[:, 0])
        obs = S.observation(ref)
        if step == 0:
            S.flat_shape(f"gpu step_flat K={K}", obs, actions)
        rows, reward, term, trunc = e.step_flat(actions)
        assert rows.shape == (N, 5 * K + 2) and np.array_equal(rows, S.flat_rows(obs)), step
        assert np.array_equal(reward, ref["reward"]) and np.array_equal(term, ref["terminated"]) and np.array_equal(trunc, ref["truncated"])
        bids, budget = e.get_actions()
        assert np.array_equal(bids, actions[:, 1:]) and np.array_equal(budget, actions[:, 0]), step
    e.close()


@pytest.mark.parametrize("groups", [1, S.FLAT["groups"]])
@pytest.mark.parametrize("K", S.FLAT["Ks"])
def test_device_flat_actions_and_observations_past_one_tile(amd, K, groups):
    from tests.hip_ctypes import DeviceArray
    c = S.FLAT
    N = c["N"]
    planes = S.planes_for(c, K=K)
    e = _engine(amd, planes, _seeds(N, 300))
    e.set_env_groups(groups)
    e.flat_obs_enable(True)
    o = H.mirror_oracle(e, planes)
    held = []
    for step in range(2):
        actions = S.flat_actions(o)
        ref = o.step(actions[:, 1:], actions[:, 0])
        obs = S.observation(ref)
        if step == 0:
            S.flat_shape(f"gpu device flat K={K} groups={groups}", obs, actions)
        d = DeviceArray(actions)
        held.append(d)
        e.set_flat_actions_device(d.ptr)
        bids, budget = e.get_actions()
        assert np.array_equal(bids, actions[:, 1:]) and np.array_equal(budget, actions[:, 0]), step
        e.step_device()
        got = e.fetch()
        assert e.env_groups() == groups
        H.assert_step_equal(got, ref)
        assert np.array_equal(_flat_obs(e, N, K), S.flat_rows(obs)), step
    e.close()
    for d in held:
        d.free()


@pytest.mark.parametrize("K", S.FLAT["Ks"])
def test_sampled_actions_and_a_masked_reset_past_one_tile(amd, K):
    c = S.FLAT
    N, mask = c["N"], np.array(c["mask"], np.uint8)
    planes = S.planes_for(c, K=K)
    e = _engine(amd, planes, _seeds(N, 300), max_days=5)
    o = H.mirror_oracle(e, planes, max_days=5)
    for step in range(3):
        want = o.sample_bids(0.25, 1.25)
        e.sample_actions(0.25, 1.25, 900.0 + step)
        bids, budget = e.get_actions()
        assert np.array_equal(bids, want) and np.all(budget == F(900.0 + step)), step
        assert len(set(want[:, S.LANES:].reshape(-1).tolist())) > 1
        e.step_device()
        ref = o.step(want, 900.0 + step)
        H.assert_step_equal(e.fetch(), ref)
        if step == 1:                                           # mid-episode: the masked envs' observation is reset()'s zeros
            obs = S.observation(ref)
            S.masked_reset(f"gpu masked reset K={K}", obs, mask)
            e.reset(env_mask=mask)
            got = e.fetch()
            for k in S.PER_KEYWORD:
                assert not got[k][mask == 1].any(), k
                assert np.array_equal(got[k][mask == 0], obs[k][mask == 0]), k
            o.day[mask == 1], o.cum_cents[mask == 1], o.cum[mask == 1] = 0, 0, 0.0
            day, cum = e.get_episode_state()
            assert np.array_equal(day, o.day) and o.day[mask == 0].all() and np.array_equal(cum, np.where(mask == 1, 0.0, ref["cum_profit"]))
    e.close()


# ======================================================================================================================================
# 6. the metric readers past one env a slab
# ======================================================================================================================================
def _metric_case(amd, model, groups):
    c = S.METRICS
    o, planes, implicit = S.metric_oracle(model)
    e = _engine(amd, planes, _seeds(c["N"], S.METRIC_SEEDS), model=0 if implicit else 1, max_days=c["max_days"], auto_reset=True)
    e.set_env_groups(groups)
    e.metrics_enable(True)
    e.metrics_reset()

    def on_step(bids, budget, ref):
        H.assert_step_equal(e.step(bids, budget), ref, implicit=implicit)
        assert implicit or e.env_groups() == groups
    sums = S.metric_run(o, implicit, on_step)
    sums.precondition(f"gpu metrics {model} groups={groups}")
    kp, sc = e.metrics_read()
    nk = np.rint(e.metrics_read_nk(ideal=False)[0] * 100).astype(np.int64)
    e.close()
    assert np.array_equal(nk, sums.nk), np.argwhere(nk != sums.nk)[:8]
    assert np.array_equal(kp, sums.columns), np.flatnonzero(kp != sums.columns)[:8]
    assert np.array_equal(sc[:4], sums.scalars), (sc, sums.scalars)
    assert sc[1] == len(c["budgets"]) * c["N"] and sc[2] == c["N"]


def test_metric_readers_past_one_env_a_slab_implicit(amd):
    _metric_case(amd, "implicit", 1)


@pytest.mark.parametrize("groups", [1, S.METRICS["groups"]])
def test_metric_readers_past_one_env_a_slab_explicit(amd, groups):
    _metric_case(amd, "explicit", groups)


# ======================================================================================================================================
# 7. more envs than 65 535
# ======================================================================================================================================
def test_more_envs_than_a_grid_dimension_of_65535(amd):
    """the (ceil(K / 256), N) launches with gridDim.y = 65 537.  Observed on the MI355X with ROCm 7: the runtime accepts the
    launches and every block runs - everything equals the oracle.  An engine that cannot do that must say so when it
    is created, in ADC_EINVAL words that name the env limit; a later bare HIP error or a stale output fails here."""
    c = S.MANY_ENVS
    N, K = c["N"], c["K"]
    planes = S.planes_for(c)
    try:
        e = amd.StepEngine(N, K, seed=17)
    except ValueError as refusal:
        assert "num_envs" in str(refusal) and "65535" in str(refusal), refusal
        return
    e.set_all_params(planes)
    e.reset(seeds=_seeds(N, 400))
    assert np.array_equal(e.get_rng_state()[0], S.reset_keys(_seeds(N, 400)))
    o = H.mirror_oracle(e, planes, threads=8)
    e.flat_obs_enable(True)
    e.sample_actions(0.3, 1.0, 1.0e9)
    want = o.sample_bids(0.3, 1.0)
    bids, budget = e.get_actions()
    assert np.array_equal(bids, want) and np.all(budget == F(1.0e9))
    e.step_device()
    got = e.fetch()
    ref = o.step(want, 1.0e9)
    obs = S.observation(ref)
    S.many_envs("gpu many envs", obs, want)
    H.assert_step_equal(got, ref)
    rows = np.concatenate([obs["buyside_clicks"], obs["cost"], obs["cumulative_profit"][:, None], obs["days_passed"][:, None],
                           obs["impressions"], obs["revenue"], obs["sellside_conversions"]], axis=1).astype(F)
    assert np.array_equal(rows[[0, N - 1]], S.flat_rows({k: v[[0, N - 1]] for k, v in obs.items()}))
    assert np.array_equal(_flat_obs(e, N, K), rows)
    e.reset(env_mask=(np.arange(N) >= 65535).astype(np.uint8))
    cleared = e.fetch()
    for k in S.PER_KEYWORD:
        assert not cleared[k][65535:].any() and np.array_equal(cleared[k][:65535], obs[k][:65535]), k
    e.close()
