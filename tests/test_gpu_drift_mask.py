"""Per-env drift selections (adc_engine_set_drift_mask) and per-env drift magnitudes (adc_engine_set_env_drift) on the device.

The oracle restatement, with oracle/ unchanged: an OracleEngine with drift on is stepped; after every step its parameters
are snapshot, its pending update is materialised, and vol_mean / bctr / sctr of the unselected keywords are put back from
the snapshot - the masked law on the oracle's own draws.  Per-env magnitudes: one N = 1 oracle per env, built with that
env's key and magnitudes.  Every comparison is exact unless it says otherwise."""
import numpy as np
import pytest

from adcraft_amd import gymnasium_kw_utils as utils
from adcraft_amd._ffi import P_BCTR, P_SCTR, P_VOL_MEAN
from oracle import capi as orc
from tests import helpers as H

pytestmark = pytest.mark.gpu

DRIFTING = (P_VOL_MEAN, P_BCTR, P_SCTR)


@pytest.fixture(scope="module")
def amd():
    import adcraft_amd.engine as eng
    from adcraft_amd import _ffi
    assert _ffi.device_count() >= 1, "no HIP device visible: the engine has no CPU path"
    return eng


class MaskedMirror:
    """the masked law on oracles: one oracle for all envs, or (per-env magnitudes) one N = 1 oracle per env"""

    def __init__(self, e, planes, sel, rates=None, model=orc.IMPLICIT, **kw):
        self.sel = np.array(sel, bool)
        keys, ticks = e.get_rng_state()
        N, K = e.num_envs, e.num_keywords
        if rates is None:
            self.parts = [(slice(0, N), H.mirror_oracle(e, planes, drift_on=True, **kw))]
        else:
            self.parts = []
            for n in range(N):
                o = orc.OracleEngine(1, K, model=model, drift=tuple(float(x) for x in rates[n]), drift_on=True, **kw)
                o.params[:] = planes[:, n:n + 1]
                o.key[:], o.tick[:] = keys[n:n + 1], ticks[n:n + 1]
                self.parts.append((slice(n, n + 1), o))

    def set_rates(self, rates):
        for (s, o), r in zip(self.parts, rates):
            o.cfg.drift_vol, o.cfg.drift_ctr, o.cfg.drift_cvr = (float(x) for x in r)

    def _settle(self, o, sel):
        snap = o.params.copy()
        o.materialize_drift()
        for p in DRIFTING:
            o.params[p][~sel] = snap[p][~sel]

    def step(self, bids, budget):
        outs = []
        budget = np.broadcast_to(np.asarray(budget, np.float32), (bids.shape[0],))
        for s, o in self.parts:
            outs.append(o.step(bids[s], budget[s]))
            self._settle(o, self.sel[s])
        return {k: np.concatenate([r[k] for r in outs]) for k in outs[0]}

    def update_keywords(self):
        """k_force_drift: a draw keyed by the current tick, then the tick moves on"""
        for s, o in self.parts:
            o.tick += 1
            o.drift_pending[:] = 1
            self._settle(o, self.sel[s])

    @property
    def params(self):
        return np.concatenate([o.params for _, o in self.parts], axis=1)

    def sample_bids(self, lo, hi):
        return np.concatenate([o.sample_bids(lo, hi) for _, o in self.parts])


def _selection(N, K, seed):
    rng = np.random.default_rng(seed)
    sel = rng.random((N, K)) < 0.5
    sel[0] = True                       # one env selects everything, one nothing
    sel[-1] = False
    return sel


def _assert_outputs(got, ref, implicit):
    H.assert_step_equal(got, ref, implicit=implicit)


PATHS = {
    # name: (model, N, K, law, env overrides, budgets, bid range)
    "dense": (0, 6, 256, dict(mean_volume=40), {}, [1e9] * 5, (0.4, 1.2)),
    "sparse": (0, 5, 300, dict(mean_volume=16, cvr=0.1, no_vol_prob=0.5),
               {"ADCRAFT_FAST_VARIANT": "2", "ADCRAFT_FAST_TILE_KW": "256"}, [1e9] * 5, (0.4, 1.2)),
    "click_walk": (0, 7, 256, dict(mean_volume=40), {}, [900.0] * 6, (0.4, 1.2)),
    "rest_pair": (0, 7, 256, dict(mean_volume=40), {"ADCRAFT_CLICK_WALK": "0", "ADCRAFT_REST_SPLIT": "1"},
                  [700.0, 700.0, 40.0, 700.0, 700.0, 1e9, 700.0], (0.4, 1.2)),
    "row_kernel": (0, 6, 200, dict(mean_volume=40), {"ADCRAFT_CLICK_WALK": "0", "ADCRAFT_REST_SPLIT": "0"},
                   [700.0, 700.0, 700.0, 700.0, 1e9, 700.0], (0.4, 1.2)),
    "at_once": (0, 6, 256, dict(mean_volume=40), {"ADCRAFT_CLICK_WALK": "0", "ADCRAFT_REST_SPLIT": "1"},
                [3.0, 3.0, 3.0, 3.0, 20.0, 3.0, 3.0], (0.4, 1.2)),
    "explicit": (1, 3, 200, None, {}, [300.0, 300.0, 1e9, 20.0, 1e9, 300.0], (0.05, 2.0)),
    "explicit_512": (1, 3, 512, None, {}, [768.0, 768.0, 1e9, 51.0, 1e9, 768.0], (0.05, 2.0)),
    "general_fast": (2, 3, 45, None, {"ADCRAFT_GENERAL_SMALL": "0"}, [1.0, 1.0, 1e9, 1.0, 1e9, 1.0], (0.05, 0.5)),
    "general_small": (2, 3, 45, None, {"ADCRAFT_GENERAL_SMALL": "1"}, [1.0, 1.0, 1e9, 1.0, 1e9, 1.0], (0.05, 0.5)),
}


def _planes(model, N, K, law, seed):
    if model == 0:
        return H.implicit_params(N, K, seed=seed, **law)
    if model == 1:
        return H.explicit_params(N, K, seed=seed)
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 90, (N, K)), rng.random((N, K)) * 6, rng.uniform(0.0, 0.3, (N, K)), rng.uniform(0.05, 0.15, (N, K)),
                     rng.uniform(0.2, 0.9, (N, K)), rng.uniform(0.2, 0.9, (N, K)), rng.uniform(0.3, 1.5, (N, K)),
                     rng.uniform(0.02, 0.3, (N, K))]).astype(np.float32)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_masks_per_env_match_the_oracle_restatement(amd, monkeypatch, path):
    """different selections per env on every path that applies drift: outputs every day, parameters every other day (a read
    materialises the pending update, so the day after it the kernels have nothing to apply) and at the end; the counters
    show the intended path ran"""
    model, N, K, law, env, budgets, (lo, hi) = PATHS[path]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    planes = _planes(model, N, K, law, seed=300 + len(path))
    e = amd.StepEngine(N, K, model=model, seed=41, drift_enabled=True, drift=(0.2, 0.3, 0.4), max_days=1000, loss_threshold=1e9)
    extra = {}
    if model == 2:
        e.set_general_model(30, 0.6, 1)
        extra = dict(max_bidders=30, participation_rate=0.6, num_winners=1)
    e.set_all_params(planes)
    e.reset()
    e.walk_stats(reset=True)
    e.direct_days(reset=True)
    sel = _selection(N, K, seed=7)
    e.set_drift_mask(sel)
    o = MaskedMirror(e, planes, sel, drift=(0.2, 0.3, 0.4), max_days=1000, loss_threshold=1e9, **extra)
    kernels = set()
    for day, budget in enumerate(budgets):
        bids = o.sample_bids(lo, hi)
        _assert_outputs(e.step(bids, budget), o.step(bids, budget), implicit=model == 0)
        kernels.add(e.step_kernel_name())
        if day % 2 == 1:
            assert np.array_equal(e.get_all_params(), o.params)
    assert np.array_equal(e.get_all_params(), o.params)
    moved = (o.params[list(DRIFTING)] != planes[list(DRIFTING)]).any(axis=0)
    assert not moved[~sel].any() and moved[sel].mean() > 0.9
    if path == "dense":
        assert any(k.startswith("k_step_implicit_fast") for k in kernels)
    elif path == "sparse":
        assert "k_step_implicit_sparse" in kernels
    elif path == "click_walk":
        assert e.walk_stats()[0] > 0
    elif path == "at_once":
        assert e.direct_days() > 0
    elif path in ("general_fast", "general_small"):
        assert kernels == {"k_step_general_small" if path == "general_small" else "k_step_general_fast"}
    e.close()


def _pair(amd, N, K, seed, planes, **kw):
    out = []
    for _ in range(2):
        e = amd.StepEngine(N, K, seed=seed, drift_enabled=True, **kw)
        e.set_all_params(planes)
        e.reset()
        out.append(e)
    return out


def test_null_path_equivalences(amd):
    """all-ones bits == no selection, bit for bit (outputs and parameters, ample and binding budgets); all-zero bits keep the
    parameters at their start values"""
    N, K = 5, 256
    planes = H.implicit_params(N, K, seed=11, mean_volume=40)
    a, b = _pair(amd, N, K, 5, planes)
    a.set_drift_mask(None)
    b.set_drift_mask(np.ones(K, bool))
    rng = np.random.default_rng(3)
    for budget in (1e9, 1e9, 900.0, 900.0, 40.0, 1e9):
        bids = rng.uniform(0.4, 1.2, (N, K)).astype(np.float32)
        ga, gb = a.step(bids, budget), b.step(bids, budget)
        for k in ga:
            assert np.array_equal(ga[k], gb[k]), k
    assert np.array_equal(a.get_all_params(), b.get_all_params())
    b.set_drift_mask(np.zeros((N, K), bool))
    start = b.get_all_params()
    for budget in (1e9, 900.0, 1e9):
        b.step(rng.uniform(0.4, 1.2, (N, K)).astype(np.float32), budget)
    b.update_keywords()
    assert np.array_equal(b.get_all_params(), start)
    a.close()
    b.close()


def test_mask_change_between_steps_and_update_keywords(amd):
    """a new selection takes effect from the next update: the update the last step scheduled moves under the old one;
    update_keywords() (k_force_drift) honours the selection in force"""
    N, K = 4, 256
    planes = H.implicit_params(N, K, seed=12, mean_volume=30)
    e = amd.StepEngine(N, K, seed=6, drift_enabled=True, drift=(0.1, 0.2, 0.3))
    e.set_all_params(planes)
    e.reset()
    s1, s2 = _selection(N, K, 1), _selection(N, K, 2)[::-1].copy()
    e.set_drift_mask(s1)
    o = MaskedMirror(e, planes, s1, drift=(0.1, 0.2, 0.3))
    for i in range(7):
        if i == 3:
            e.set_drift_mask(s2)
            o.sel = s2
        if i == 5:
            e.update_keywords()
            o.update_keywords()
        bids = o.sample_bids(0.4, 1.2)
        _assert_outputs(e.step(bids, 1e9 if i % 3 else 800.0), o.step(bids, 1e9 if i % 3 else 800.0), implicit=True)
    e.set_drift_mask(s1)
    o.sel = s1
    e.update_keywords()
    o.update_keywords()
    assert np.array_equal(e.get_all_params(), o.params)
    e.close()


def test_per_env_rates_against_per_env_mirrors(amd):
    """different magnitudes for every env, changed mid-episode (and back to the scalars), with a selection, against one N = 1
    oracle per env built with that env's key and magnitudes"""
    N, K = 5, 200
    planes = H.implicit_params(N, K, seed=13, mean_volume=40)
    e = amd.StepEngine(N, K, seed=8, drift_enabled=True, drift=(0.05, 0.05, 0.05))
    e.set_all_params(planes)
    e.reset()
    rng = np.random.default_rng(9)
    r1 = rng.uniform(0.01, 0.5, (N, 3)).astype(np.float32)
    r2 = rng.uniform(0.01, 0.9, (N, 3)).astype(np.float32)
    sel = _selection(N, K, 4)
    e.set_drift_mask(sel)
    e.set_env_drift(r1)
    o = MaskedMirror(e, planes, sel, rates=r1)
    for i in range(8):
        if i == 3:
            e.set_env_drift(r2)
            o.set_rates(r2)
        if i == 6:
            e.set_env_drift(None)                       # adc_engine_set_drift's scalars again
            o.set_rates(np.tile(np.float32(0.05), (N, 3)))
        bids = o.sample_bids(0.4, 1.2)
        _assert_outputs(e.step(bids, 900.0 if i in (1, 2, 4) else 1e9), o.step(bids, 900.0 if i in (1, 2, 4) else 1e9), implicit=True)
        if i % 3 == 2:
            assert np.array_equal(e.get_all_params(), o.params)
    assert np.array_equal(e.get_all_params(), o.params)
    e.close()


def _grouped_run(amd, monkeypatch, groups, kind):
    monkeypatch.setenv("ADCRAFT_STREAM_GROUPS", str(groups))
    N, K = 7, 256
    planes = H.implicit_params(N, K, seed=14, mean_volume=40)
    sel = _selection(N, K, 5)
    rates = np.random.default_rng(10).uniform(0.01, 0.5, (N, 3)).astype(np.float32)
    e = amd.StepEngine(N, K, seed=23, drift_enabled=True, max_days=4, loss_threshold=1e9, auto_reset=True)
    e.set_all_params(planes)
    e.reset()
    e.set_drift_mask(sel)
    e.set_env_drift(rates)
    res = []
    if kind == "steps":
        rng = np.random.default_rng(11)
        for budget in (1e9, 900.0, 900.0, 1e9, 3.0, 3.0):
            res.append(e.step(rng.uniform(0.4, 1.2, (N, K)).astype(np.float32), budget))
    elif kind == "graph":
        e.agent_init(1.0, np.arange(N, dtype=np.uint64) + 5)
        e.run_days("zero_margin", 3, budget=900.0, graph=True)
        e.set_drift_mask(sel[::-1].copy())
        e.set_env_drift(rates[::-1].copy())
        e.run_days("zero_margin", 3, budget=900.0, graph=True)
        res.append(e.fetch())
    else:
        if kind == "zero_margin":
            e.agent_init(1.0, np.arange(N, dtype=np.uint64) + 5)
        elif kind == "oracle":
            e.bid_curves_build(512, np.arange(0.01, 3.00, 0.01))
        else:
            e.interp_init(-0.2, 0.03, None, 0, np.arange(N, dtype=np.uint64) + 5)
        e.run_days(kind, 5, budget=900.0)
        res.append(e.fetch())
    res.append(dict(params=e.get_all_params()))
    e.close()
    return res


@pytest.mark.parametrize("kind", ["steps", "zero_margin", "oracle", "interpolation"])
def test_env_groups_change_nothing(amd, monkeypatch, kind):
    """forced env groups (2, 3, 4) with per-env selections and magnitudes give the one-group results: group_view offsets both
    arrays like the other per-env ones"""
    ref = _grouped_run(amd, monkeypatch, 1, kind)
    for g in (2, 3, 4):
        got = _grouped_run(amd, monkeypatch, g, kind)
        for a, b in zip(got, ref):
            for k in b:
                assert np.array_equal(a[k], b[k]), (g, k)


def test_day_graph_across_a_selection_change(amd, monkeypatch):
    """run_days(graph=True) across a change of selection and magnitudes == the plain chain (a captured day reads the
    current device copies; setting or clearing either pointer forces a recapture)"""
    outs = []
    for graph in (True, False):
        monkeypatch.setenv("ADCRAFT_STREAM_GROUPS", "1")
        N, K = 5, 96
        planes = H.implicit_params(N, K, seed=15, mean_volume=24, cvr=0.5)
        e = amd.StepEngine(N, K, seed=32, max_days=1 << 20, loss_threshold=1e12, auto_reset=True, drift_enabled=True)
        e.set_all_params(planes)
        e.reset()
        e.agent_init(1.0, np.arange(N, dtype=np.uint64) + 1)
        e.run_days("zero_margin", 4, budget=1e6, graph=graph)
        e.set_drift_mask(_selection(N, K, 8))                       # pointer set: recapture
        e.run_days("zero_margin", 4, budget=1e6, graph=graph)
        e.set_drift_mask(_selection(N, K, 9))                       # same pointer, new bits
        e.set_env_drift(np.full((N, 3), 0.3, np.float32))
        e.run_days("zero_margin", 4, budget=1e6, graph=graph)
        e.set_drift_mask(None)                                      # cleared: recapture
        e.set_env_drift(None)
        e.run_days("zero_margin", 4, budget=1e6, graph=graph)
        outs.append((e.fetch(), e.get_all_params()))
        e.close()
    for k in outs[0][0]:
        assert np.array_equal(outs[0][0][k], outs[1][0][k]), k
    assert np.array_equal(outs[0][1], outs[1][1])


def test_g14_through_step_replay(amd, golden):
    """G14 (the reference's update_keywords() under partial masks) replayed through k_step_exact<., TAPE>: the tape's positions
    k >= sum(mask) hold NaN - never read - and the selection gates the recorded coefficients.  Tolerance as G4's
    (test_g4_drift_replay_on_gpu): the engine holds float32, the reference float64."""
    for c in golden("g14_partial_updater_mask.json")["cases"]:
        K = c["K"]
        up = dict((n, v) for n, v in c["updater_params"])
        e = amd.StepEngine(1, K, seed=1, drift_enabled=True, drift=(up["vol"], up["ctr"], up["cvr"]))
        p0 = c["params0"]
        planes = np.array([[p[0][0] for p in p0], [p[0][1] for p in p0], [p[1] for p in p0], [1.0 / p[2] for p in p0],
                           [p[3] for p in p0], [p[4] for p in p0], [p[5] for p in p0], [p[6] for p in p0]], np.float32).reshape(8, 1, K)
        e.set_all_params(planes)
        e.reset()
        for st in c["steps"]:
            e.set_drift_mask(utils.effective_updater_mask(st["mask"]))
            u = np.full((3, 1, K), np.nan, np.float32)
            n = st["num_updates"]
            u[:, 0, :n] = np.array(st["uniforms"], np.float32).reshape(3, n)
            out = e.step_replay(np.full((1, K), 0.5, np.float32), 10.0, amd.ReplayTape(1, np.zeros((1, K), np.int32), drift_uniforms=u))
            assert out["impressions"].sum() == 0
            got = e.get_all_params()[:, 0]
            ref = st["params"]
            assert np.isfinite(got).all()
            np.testing.assert_allclose(got[0], [p[0][0] for p in ref], rtol=2e-6, atol=2e-6)
            assert np.array_equal(got[1], planes[1, 0])
            np.testing.assert_allclose(got[4], [p[3] for p in ref], rtol=2e-6)
            np.testing.assert_allclose(got[5], [p[4] for p in ref], rtol=2e-6)
        e.close()


def _cfg(mv, cvr):
    return utils.experiment_keyword_config(mv, cvr)


def test_facade_partial_mask_episode(amd):
    """BiddingSimulation with a partial mask: the selected keywords (B-6) move exactly as an all-True twin's, the others keep
    their parameters; set_updater_mask mid-episode takes effect from the next update"""
    import adcraft_amd as pkg
    K = 8
    mask = [True, False, True, True, False, True, False, False]        # sum 4: keyword 5 lies beyond the prefix and stays
    eff = utils.effective_updater_mask(mask)
    assert eff.tolist() == [True, False, True, True, False, False, False, False]
    env = pkg.BiddingSimulation(keyword_config=_cfg(40, 0.5), num_keywords=K, updater_mask=mask,
                                updater_params=[["vol", 0.3], ["ctr", 0.3], ["cvr", 0.3]])
    twin = pkg.BiddingSimulation(keyword_config=_cfg(40, 0.5), num_keywords=K, updater_mask=[True] * K,
                                 updater_params=[["vol", 0.3], ["ctr", 0.3], ["cvr", 0.3]])
    env.reset(seed=3)
    twin.reset(seed=3)

    def f32(p):         # (the facade reports the device's float32 planes once drift has run: compare at that precision)
        return [np.float32(p[0][0]), np.float32(p[0][1])] + [np.float32(x) for x in p[1:]]

    start = [f32(p) for p in env.keyword_params]
    bids = {"keyword_bids": np.full(K, 0.8, np.float32), "budget": 1000.0}
    for _ in range(5):
        env.step(bids)
        twin.step(bids)
        a, b = env.keyword_params, twin.keyword_params
        for k in range(K):
            if eff[k]:
                assert a[k] == b[k]
            else:
                assert f32(a[k]) == start[k]
    assert all(f32(env.keyword_params[k]) != start[k] for k in range(K) if eff[k])
    env.update_keywords()
    twin.update_keywords()
    assert all(env.keyword_params[k] == twin.keyword_params[k] for k in range(K) if eff[k])
    env.set_updater_mask([False] * K)                                  # drift off: nothing moves any more
    frozen = [list(p) for p in env.keyword_params]
    env.step(bids)
    env.step(bids)
    assert [list(p) for p in env.keyword_params] == frozen
    env.close()
    twin.close()


def test_vector_env_masks_and_params_match_the_engine(amd):
    """BiddingSimulationVectorEnv with [N, K] masks and per-env updater_params == a StepEngine given the same planes and seeds,
    the B-6-translated rows and the magnitudes; set_updater_mask / set_updater_params between steps likewise"""
    from adcraft_amd.vector_env import BiddingSimulationVectorEnv
    N, K = 6, 32
    rng = np.random.default_rng(12)
    masks = rng.random((N, K)) < 0.6
    params = [[["vol", float(a)], ["ctr", float(b)], ["cvr", float(c)]] for a, b, c in rng.uniform(0.01, 0.4, (N, 3))]
    venv = BiddingSimulationVectorEnv(N, keyword_config=_cfg(40, 0.5), num_keywords=K, updater_mask=masks, updater_params=params,
                                      engine_shards=1)
    venv.reset(seed=21)
    eng = venv.engine
    planes = eng.get_all_params()
    twin = amd.StepEngine(N, K, model=0, seed=21, max_days=60, loss_threshold=10000.0, drift_enabled=True, auto_reset=True)
    twin.set_all_params(planes)
    twin.reset(seeds=np.arange(N, dtype=np.uint64) + np.uint64(21))
    assert all(np.array_equal(x, y) for x, y in zip(twin.get_rng_state(), eng.get_rng_state()))
    twin.set_drift_mask(utils.effective_updater_mask(masks))
    twin.set_env_drift(np.array([[p[1] for p in row] for row in params], np.float32))
    for i in range(6):
        if i == 3:
            m2 = rng.random(K) < 0.5
            venv.set_updater_mask(m2)
            twin.set_drift_mask(utils.effective_updater_mask(m2))
            p2 = [["vol", 0.5], ["ctr", 0.1], ["cvr", 0.2]]
            venv.set_updater_params(p2)
            twin.set_env_drift(None)
            twin.set_drift(True, (0.5, 0.1, 0.2))
        bids = rng.uniform(0.3, 1.5, (N, K)).astype(np.float32)
        venv.step({"keyword_bids": bids, "budget": np.full(N, 1000.0, np.float32)})
        twin.step(bids, 1000.0)
        assert np.array_equal(eng.get_all_params(), twin.get_all_params())
    assert (eng.get_all_params()[P_BCTR] != planes[P_BCTR]).any()
    venv.close()
    twin.close()


def test_sharded_engine_equals_one_engine(amd):
    N, K = 9, 64
    planes = H.implicit_params(N, K, seed=16, mean_volume=30)
    sel = _selection(N, K, 12)
    rates = np.random.default_rng(13).uniform(0.01, 0.5, (N, 3)).astype(np.float32)
    one = amd.StepEngine(N, K, seed=4, drift_enabled=True)
    sh = amd.ShardedStepEngine(N, K, shards=3, seed=4, drift_enabled=True)
    for e in (one, sh):
        e.set_all_params(planes)
        e.reset()
        e.set_drift_mask(sel)
        e.set_env_drift(rates)
    rng = np.random.default_rng(14)
    for i in range(5):
        if i == 2:
            for e in (one, sh):
                e.set_drift_mask(sel[0])                # [K]: every env
                e.set_env_drift(rates[1])               # [3]: every env
        bids = rng.uniform(0.4, 1.2, (N, K)).astype(np.float32)
        a, b = one.step(bids, 800.0), sh.step(bids, 800.0)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(one.get_all_params(), sh.get_all_params())
    one.close()
    sh.close()
