"""Mirror of adcraft/baselines/interpolated_expectations.py for the part the paper's experiments use:
``NaiveZeroMarginStrategy`` (:442-515) and ``NaiveInterpolationStrategy`` (:298-439).  The caches and the bid rule live in the HIP engine
(``k_agent_step``, adcraft_amd/csrc/parts/kernels_policy.inc), one agent per env; this class is the reference's
Python surface over it (same constructor, ``update_all_caches(prev_action, prev_observation)``, ``sample_action()``,
``caches``, ``max_bids``), usable with any env that returns the reference's observation dict.

For the closed loop without a host round trip per step use ``adcraft_amd.closed_loop`` instead.
"""
import numpy as np

from ..engine import StepEngine


def get_empty_cache():
    """adcraft/baselines/interpolated_expectations.py:286-295"""
    return {"ave_rpc": 0.0, "num_rpc_obs": 0, "ave_sctr": 0.4, "num_sctr_obs": 0.0, "ave_cpc": {}, "ave_clicks": {}}


class NaiveZeroMarginStrategy:
    """Estimates revenue per buyside click (rpc x sctr) and bids it; ramps the bid up while nothing has been observed
    (reference docstring :443-456).  ``engine`` (optional) is a StepEngine whose envs the agent serves: its device
    action buffers then receive the sampled action (``engine.step_device()`` consumes it)."""

    def __init__(self, num_keywords, default_expected_revenue_per_conversion=3.0, initial_caches=None, seed=None, *,
                 engine=None, device_id=0):
        if initial_caches is not None:
            raise NotImplementedError("preseeded caches are not supported by the device agent")
        self._own = engine is None
        self._e = engine if engine is not None else StepEngine(1, int(num_keywords), device_id=device_id)
        if self._e.num_keywords != int(num_keywords):
            raise ValueError("engine.num_keywords != num_keywords")
        self.observation_keys = ["impressions", "buyside_clicks", "cost", "sellside_conversions", "revenue"]
        self.default_rpc = default_expected_revenue_per_conversion
        # the reference draws from np.random.default_rng(seed); the device agent from its Philox stream keyed by `seed`
        self._e.agent_init(default_expected_revenue_per_conversion,
                           None if seed is None else np.full(self._e.num_envs, seed, dtype=np.uint64) + np.arange(self._e.num_envs, dtype=np.uint64))
        self.prev_bids = None

    def update_all_caches(self, prev_action, prev_observation):
        """:485-494; observations of shape [K] (one env) or [N, K]"""
        self.prev_bids = prev_action["keyword_bids"]
        self._e.agent_update(prev_observation["buyside_clicks"], prev_observation["sellside_conversions"], prev_observation["revenue"])

    def sample_action(self, replay_uniforms=None):
        """:496-515 -> {"budget", "keyword_bids"} (arrays squeezed for a single env)"""
        self._e.agent_act(0.0, replay_uniforms)
        bids, budget = self._e.get_actions()
        if self._e.num_envs == 1:
            return {"budget": float(budget[0]), "keyword_bids": bids[0].astype(np.float64)}
        return {"budget": budget.astype(np.float64), "keyword_bids": bids.astype(np.float64)}

    @property
    def max_bids(self):
        mb = self._e.agent_state()["max_bids"]
        return mb[0] if self._e.num_envs == 1 else mb

    @property
    def caches(self):
        """list (one env) or list of lists of the reference's cache dicts (ave_cpc / ave_clicks are not tracked: the
        zero-margin strategy never reads them)"""
        st = self._e.agent_state()

        def one(n):
            return [dict(ave_rpc=float(st["ave_rpc"][n, k]), num_rpc_obs=int(st["num_rpc_obs"][n, k]),
                         ave_sctr=float(st["ave_sctr"][n, k]), num_sctr_obs=float(st["num_sctr_obs"][n, k]),
                         ave_cpc={}, ave_clicks={}) for k in range(self._e.num_keywords)]
        return one(0) if self._e.num_envs == 1 else [one(n) for n in range(self._e.num_envs)]

    def close(self):
        if self._own:
            self._e.close()


class NaiveInterpolationStrategy:
    """Estimates revenue per buyside click, clicks per bid and cost per bid, and samples bids believed to be profitable above
    a threshold (reference docstring :299-314).  The caches, the interpolation, the acquisition function and the draw live in
    the HIP engine (``k_interp_step``, adcraft_amd/csrc/parts/kernel_interp_agent.inc), one agent per env of ``engine``
    (optional; its action buffers then receive the sampled action).

    The agent draws from its own Philox stream keyed by ``seed``, not from np.random.default_rng(seed);
    ``sample_action(replay_uniforms)`` takes the uniform rng.choice would use instead.  ``capacity``: interpolation points
    kept per keyword (default min(300, max_days + 1)); an update that could overflow it raises ValueError."""

    def __init__(self, num_keywords, profit_acquisition_threshold=-0.2, allowed_bids=np.linspace(0.01, 3.00, 300),
                 initial_caches=None, seed=None, bid_step=0.03, *, engine=None, device_id=0, capacity=None):
        if initial_caches is not None:
            raise NotImplementedError("preseeded caches are not supported by the device agent")
        self._own = engine is None
        self._e = engine if engine is not None else StepEngine(1, int(num_keywords), device_id=device_id)
        if self._e.num_keywords != int(num_keywords):
            raise ValueError("engine.num_keywords != num_keywords")
        self.observation_keys = ["impressions", "buyside_clicks", "cost", "sellside_conversions", "revenue"]
        self.profit_acquisition_threshold = profit_acquisition_threshold
        self.bid_step = bid_step
        self._allowed_bids = np.array(allowed_bids, dtype=np.float64).reshape(-1)
        seeds = None if seed is None else (np.full(self._e.num_envs, seed, dtype=np.uint64) + np.arange(self._e.num_envs, dtype=np.uint64))
        self._e.interp_init(profit_acquisition_threshold, bid_step, self._allowed_bids, 0 if capacity is None else int(capacity), seeds)

    @property
    def allowed_bids(self):
        return self._allowed_bids

    @allowed_bids.setter
    def allowed_bids(self, bids):
        g = np.array(bids, dtype=np.float64).reshape(-1)
        self._e.interp_set_allowed_bids(g)
        self._allowed_bids = g

    def update_all_caches(self, prev_action, prev_observations):
        """:400-403; observations of shape [K] (one env) or [N, K]"""
        o = prev_observations
        self._e.interp_update(prev_action["keyword_bids"], o["buyside_clicks"], o["cost"], o["sellside_conversions"], o["revenue"])

    def sample_action(self, replay_uniforms=None):
        """:405-439 -> {"budget", "keyword_bids"}: the agent's float64 budget and its grid bids (arrays squeezed for one env)"""
        self._e.interp_act(0.0, replay_uniforms)
        st = self._e.interp_state()
        idx = st["bid_index"]
        bids = np.where(idx >= 0, self._allowed_bids[np.maximum(idx, 0)], 0.01)
        if self._e.num_envs == 1:
            return {"budget": float(st["budget"][0]), "keyword_bids": bids[0]}
        return {"budget": st["budget"], "keyword_bids": bids}

    @property
    def profit_beliefs(self):
        v = self._e.interp_state()["profit_beliefs"]
        return float(v[0]) if self._e.num_envs == 1 else v

    @property
    def cost_beliefs(self):
        v = self._e.interp_state()["cost_beliefs"]
        return float(v[0]) if self._e.num_envs == 1 else v

    @property
    def caches(self):
        """list (one env) or list of lists of the reference's cache dicts.  ave_cpc / ave_clicks hold only keys in
        $0.01-$3.00, the ones the agent interpolates; bids outside that range are remembered only through the largest key."""
        st, ent = self._e.interp_state(), self._e.interp_entries()

        def key(c):
            return str(round(c / 100.0, 2))

        def one(n):
            out = []
            for k in range(self._e.num_keywords):
                clicks = {key(int(ent["clicks_cent"][n, k, i])): [float(ent["ave_clicks"][n, k, i]), int(ent["clicks_count"][n, k, i])]
                          for i in range(ent["n_clicks"][n, k])}
                cpc = {key(int(ent["cpc_cent"][n, k, i])): [float(ent["ave_cpc"][n, k, i]), int(ent["cpc_count"][n, k, i])]
                       for i in range(ent["n_cpc"][n, k])}
                out.append(dict(ave_rpc=float(st["ave_rpc"][n, k]), num_rpc_obs=int(st["num_rpc_obs"][n, k]),
                                ave_sctr=float(st["ave_sctr"][n, k]), num_sctr_obs=float(st["num_sctr_obs"][n, k]),
                                ave_cpc=cpc, ave_clicks=clicks))
            return out
        return one(0) if self._e.num_envs == 1 else [one(n) for n in range(self._e.num_envs)]

    def close(self):
        if self._own:
            self._e.close()
