"""The shapes at which the step's callers and its host-facing I/O take another path, shared by
tests/test_io_shapes_host.py and tests/test_gpu_io_shapes.py: the two baseline bidders past one pass of 256 lanes, the output
kernels past one pass of their grid and on the packing route, the flat I/O past one keyword tile, the metric readers past one env
a slab, and an engine of more envs than 65 535.  Every function here works on the oracle and the numpy restatements alone: it
states a case's precondition - what makes the case able to fail - measures it, prints the figures (profiles/pr_io_shapes.txt
keeps them) and asserts it.

  agent    3 envs x 600 keywords (passes of 256, 256 and 88), 12 days, the budget the agent's own: 100 x the sum of the codes
  interp   3 envs x 300 and x 257 keywords (a second pass of 44 lanes and of one), 12 days on mean_volume 64, its own budget
  outputs  264 x 1012: 253 quads a row, 66 792 quads, 1 256 of them (5 024 entries, five envs) in k_outputs_to_host's second pass
  pack     5 x 1014 and 3 x 6 (K mod 4 = 2), 5 x 1012 into pageable memory: k_pack_counts
  flat     7 envs x 257 and x 600: rows of 1287 and 3002 floats, action rows of 258 and 601, two and three keyword tiles
  metrics  301 x 300: 5 envs a slab (60 full, one of a single env, three empty), k_metric_reduce's second pass of 45 envs
  envs     65 537 x 4: gridDim.y past 65 535
"""
import numpy as np

from oracle import capi as orc
from oracle import ref_numpy as rn
from tests import helpers as H
from tests import interp_ref as IR

F = np.float32
LOG = "io-shapes:"
LANES = 256
PER_KEYWORD = ("impressions", "buyside_clicks", "sellside_conversions", "cost", "revenue")

AGENT = dict(N=3, K=600, days=12, mean_volume=24, cvr=0.1, planes_seed=91, default_rpc=1.0, agent_seeds=(5, 6, 7), env_seeds=(21, 22, 23))
AGENT_GROUPS = dict(N=7, K=600, days=10, groups=3)
INTERP = dict(N=3, Ks=(300, 257), days=12, mean_volume=64, cvr=0.5, planes_seed=91, agent_seeds=(5, 6, 7), env_seeds=(31, 32, 33))
INTERP_GROUPS = dict(N=7, K=300, days=10, groups=3)
OUTPUTS = dict(N=264, K=1012, mean_volume=8, planes_seed=7, first_pass=LANES * LANES * 4)
PACK = dict(shapes=((5, 1014), (3, 6)), pageable=(5, 1012), odd_K=1013, mean_volume=8, planes_seed=8)
FLAT = dict(N=7, Ks=(257, 600), mean_volume=64, planes_seed=24, mask=(1, 0, 1, 0, 0, 1, 0), groups=3)
METRICS = dict(N=301, K=300, max_days=3, budgets=(1e9, 30.0, 1e9, 30.0), slabs=64, groups=3, planes_seed=10)
MANY_ENVS = dict(N=65537, K=4, mean_volume=8, planes_seed=11)
AGENT_STREAM = (0xA6E27B1D5C3F9E01, 9)          # the zero-margin agent's key constant and Philox stage (kernels_policy.inc)
INTERP_STREAM = (0x3C6EF372FE94F82B, 13)        # the interpolation agent's (kernel_interp_agent.inc)
M64 = 0xFFFFFFFFFFFFFFFF


def log(case, **figures):
    print(LOG, case, " ".join(f"{k}={v}" for k, v in figures.items()), flush=True)


# ---- streams and the oracle in the engine's place -------------------------------------------------------------------------------------
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def reset_keys(env_seeds):
    """the env keys after reset(seeds=env_seeds) (k_reset: splitmix64 of the seed; the tick is 0)"""
    return np.array([splitmix64(int(s)) for s in env_seeds], np.uint64)


def stream_uniforms(agent_seeds, stream, K, tick):
    """the uniforms an agent draws at `tick`: Philox call (0, stage, keyword, tick) under splitmix64(seed ^ const), 53 bits of
    its first two words as numpy's Generator.random() takes them"""
    const, stage = stream
    u = np.zeros((len(agent_seeds), K))
    for n, s in enumerate(agent_seeds):
        key = splitmix64(int(s) ^ const)
        for k in range(K):
            w = orc.philox([0, stage, k, tick], [key & 0xFFFFFFFF, key >> 32])
            u[n, k] = float(((int(w[0]) >> 5) << 26) | (int(w[1]) >> 6)) * 2.0 ** -53
    return u


def oracle_after_reset(planes, env_seeds, model=orc.IMPLICIT, **kw):
    """an OracleEngine in the state of a StepEngine after set_all_params(planes) and reset(seeds=env_seeds)"""
    o = orc.OracleEngine(planes.shape[1], planes.shape[2], model=model, **kw)
    o.params[:] = planes
    o.key[:] = reset_keys(env_seeds)
    o.tick[:] = 0
    return o


def observation(ref, implicit=True):
    """an oracle step under the names and types fetch() returns"""
    cost = H.f32_dollars(ref["cost_cents"]) if implicit else ref["cost"].astype(F)
    return dict(impressions=ref["impressions"], buyside_clicks=ref["clicks"], sellside_conversions=ref["conversions"], cost=cost,
                revenue=H.f32_dollars(ref["revenue_cents"]), reward=ref["reward"], cumulative_profit=ref["cum_profit"],
                days_passed=ref["day"], terminated=ref["terminated"], truncated=ref["truncated"])


def no_observation(N, K):
    """what reset() leaves"""
    z = np.zeros((N, K), np.int32)
    return dict(impressions=z, buyside_clicks=z, sellside_conversions=z, cost=z.astype(F), revenue=z.astype(F))


def handed_bids(bids):
    """the float32 bids an agent kernel writes for its float64 bids: whole cents, at least one"""
    return (np.maximum(np.rint(np.asarray(bids, np.float64) * 100.0), 1.0) / 100.0).astype(F)


def flat_rows(obs):
    """flatten_dict_array of every env's observation dict, float32 [N, 5K + 2]"""
    N = obs["impressions"].shape[0]
    rows = [rn.flatten_dict_array(dict(impressions=obs["impressions"][i], buyside_clicks=obs["buyside_clicks"][i], cost=obs["cost"][i],
                                       sellside_conversions=obs["sellside_conversions"][i], revenue=obs["revenue"][i],
                                       cumulative_profit=np.array([obs["cumulative_profit"][i]]),
                                       days_passed=np.array([obs["days_passed"][i]]))).astype(F) for i in range(N)]
    return np.stack(rows)


def planes_for(case, N=None, K=None):
    return H.implicit_params(N or case["N"], K or case["K"], case["planes_seed"], mean_volume=case["mean_volume"], cvr=case.get("cvr", 0.5))


# ---- 1. the zero-margin agent past one pass ---------------------------------------------------------------------------------------------
class AgentRun:
    """ZeroMarginAgent day by day on the agent's own uniforms; day(obs) -> what the device must hand over"""

    def __init__(self, N=AGENT["N"], K=AGENT["K"], agent_seeds=AGENT["agent_seeds"], default_rpc=AGENT["default_rpc"]):
        self.N, self.K, self.seeds, self.t = N, K, agent_seeds, 0
        self.ref = rn.ZeroMarginAgent(N, K, default_rpc)
        self.codes, self.budgets = None, []

    def day(self, obs):
        ref = self.ref
        ref.update(obs["buyside_clicks"], obs["sellside_conversions"], obs["revenue"])
        u = stream_uniforms(self.seeds, AGENT_STREAM, self.K, self.t)
        no_rpc = ref.num_rpc_obs < 1
        with np.errstate(divide="ignore"):
            ramp = no_rpc & (u <= 1.0 / np.sqrt(ref.num_sctr_obs.astype(np.float64)))
        self.codes = np.where(no_rpc, np.where(ramp, 1, 2), 3)
        bids, budget = ref.act(u)
        assert np.array_equal(budget, 100.0 * self.codes.sum(axis=1))
        self.budgets.append(budget)
        self.t += 1
        return dict(bid_cents=np.maximum(np.rint(bids * 100.0), 1.0), bids=handed_bids(bids), budget=budget.astype(F))

    def precondition(self, case):
        """on the last day each code occurs in each pass of every env, the envs' budgets are not all equal, and on no day is an
        env's budget 100 x the code sum of its first pass"""
        K, codes = self.K, self.codes
        ranges = [(a, min(a + LANES, K)) for a in range(0, K, LANES)]
        counts = [[[int((codes[n, a:b] == c).sum()) for c in (1, 2, 3)] for a, b in ranges] for n in range(self.N)]
        first = [100.0 * float(self.codes[n, :LANES].sum()) for n in range(self.N)]
        log(case, passes=ranges, codes_1_2_3_per_env_and_pass=counts, budgets_last_day=self.budgets[-1].tolist(), first_pass_alone=first)
        assert len(ranges) > 1 and all(min(c) > 0 for env in counts for c in env), counts
        assert len(set(self.budgets[-1].tolist())) > 1
        assert all(b[n] != 100.0 * LANES * c for b in self.budgets for n in range(self.N) for c in (1, 2, 3))
        assert all(self.budgets[-1][n] != first[n] for n in range(self.N))
        assert np.all(self.budgets[-1] == np.float64(F(self.budgets[-1]))), "the budget is a float32"


# ---- 2. the interpolation agent past one pass -------------------------------------------------------------------------------------------
def interp_planes(K, N=None):
    """INTERP's law; the keywords past the first pass meet competitors at 3 cents and are clicked nine times in ten, so that the
    agent's first bids already win there and every day adds a cpc point (at K = 257 one keyword an env has to hold them all)"""
    planes = planes_for(INTERP, N, K)
    planes[2, :, LANES:], planes[3, :, LANES:], planes[4, :, LANES:] = 0.03, 0.01, 0.9
    return planes


class InterpRun:
    """InterpAgentRef day by day on the agent's own uniforms, and beside it the same agent on the first 256 keywords alone:
    its beliefs are the sums thread 0 would have after 256 terms"""
    GRID = np.linspace(0.01, 3.00, 300)

    def __init__(self, N, K, agent_seeds=INTERP["agent_seeds"]):
        self.N, self.K, self.seeds, self.t = N, K, agent_seeds, 0
        self.ref, self.head = IR.InterpAgentRef(N, K), IR.InterpAgentRef(N, LANES)
        self.prev = np.full((N, K), 0.01)
        self.uniforms = None
        self.head_differs = 0

    def day(self, obs):
        a = [self.prev] + [np.asarray(obs[k]) for k in ("buyside_clicks", "cost", "sellside_conversions", "revenue")]
        self.ref.update(*a)
        self.head.update(*(x[:, :LANES] for x in a))
        self.uniforms = u = stream_uniforms(self.seeds, INTERP_STREAM, self.K, self.t)
        bids, drew = self.ref.act(self.GRID, u)
        self.head.act(self.GRID, u[:, :LANES])
        self.head_differs += int(np.any(self.ref.profit_beliefs != self.head.profit_beliefs))
        self.prev = bids
        self.t += 1
        return dict(grid_bids=bids, drew=drew, bids=handed_bids(bids), budget=(np.rint(self.ref.budget * 100.0) / 100.0).astype(F))

    def precondition(self, case):
        """keywords past the first pass hold cpc points, and the beliefs are not the first pass's sums"""
        points = sum(len(c.cpc) for row in self.ref.caches for c in row[LANES:])
        log(case, cpc_points_past_keyword_256=points, profit_beliefs=self.ref.profit_beliefs.tolist(),
            first_256_alone=self.head.profit_beliefs.tolist(), cost_beliefs=self.ref.cost_beliefs.tolist(),
            cost_first_256_alone=self.head.cost_beliefs.tolist(), budget=self.ref.budget.tolist(), days_profit_differs=self.head_differs)
        assert points >= 20, points
        assert np.any(self.ref.profit_beliefs != self.head.profit_beliefs)
        assert np.all(self.ref.cost_beliefs != self.head.cost_beliefs)


# ---- 3. k_outputs_to_host's second pass -------------------------------------------------------------------------------------------------
def second_pass(case, obs, first_pass=OUTPUTS["first_pass"]):
    """each per-keyword output is non-zero somewhere in the flat entries the grid's second pass moves, and those span four envs"""
    N, K = obs["impressions"].shape
    envs = sorted(set((np.arange(first_pass, N * K) // K).tolist()))
    nonzero = {k: int(np.count_nonzero(obs[k].reshape(-1)[first_pass:])) for k in PER_KEYWORD}
    log(case, entries=N * K, second_pass_entries=N * K - first_pass, second_pass_envs=envs, not_zero_there=nonzero,
        largest_count=int(max(obs[k].max() for k in PER_KEYWORD[:3])))
    assert N * K > first_pass and K % 4 == 0 and len(envs) >= 4
    assert all(v > 0 for v in nonzero.values()), nonzero
    return envs


def clip_last_keyword(planes, bids):
    """the last env's last keyword takes 70 000 auctions and wins them all"""
    planes, bids = planes.copy(), np.array(bids, F)
    planes[:, -1, -1] = (70000.0, 0.0, 0.0, 0.1, 0.5, 0.5, 1.0, 0.2)
    bids[-1, -1] = 5.0
    return planes, bids


def packed(obs):
    """the three counts as compact_counts returns them, and whether one was clipped"""
    counts = [obs[k] for k in PER_KEYWORD[:3]]
    return [np.minimum(c, 65535).astype(np.uint16) for c in counts], any(int(c.max()) > 65535 for c in counts)


def clipped_entry(case, obs):
    """only the impressions of the last env's last keyword pass 65 535"""
    over = {k: np.argwhere(obs[k] > 65535).tolist() for k in PER_KEYWORD[:3]}
    N, K = obs["impressions"].shape
    log(case, entries_past_65535=over, impressions_there=int(obs["impressions"][-1, -1]))
    assert over == dict(impressions=[[N - 1, K - 1]], buyside_clicks=[], sellside_conversions=[]), over


# ---- 4. k_pack_counts -------------------------------------------------------------------------------------------------------------------
def pack_route(case, obs, pageable=False):
    """the shape takes the packing kernel (K even and not a multiple of 4, or a pageable target), and every env's three counts
    are non-zero in its last pair of keywords or before: an env taken from the wrong row shows"""
    N, K = obs["impressions"].shape
    rows_differ = all(not np.array_equal(obs[k][a], obs[k][b]) for k in PER_KEYWORD[:3] for a in range(N) for b in range(a))
    nonzero = {k: [int(np.count_nonzero(obs[k][n])) for n in range(N)] for k in PER_KEYWORD[:3]}
    log(case, N=N, K=K, K_mod_4=K % 4, pageable=pageable, counts_not_zero_per_env=nonzero, rows_differ=rows_differ)
    assert K % 2 == 0 and (K % 4 == 2 or pageable)
    assert rows_differ and all(min(v) > 0 for v in nonzero.values())


# ---- 5. flat I/O past one tile ----------------------------------------------------------------------------------------------------------
def flat_shape(case, obs, actions):
    """more than one keyword tile, a row stride and an action stride that are odd or no multiple of 4, and every plane non-zero
    past keyword 256 in every env: a tile left out shows"""
    N, K = obs["impressions"].shape
    tiles = [min(LANES, K - a) for a in range(0, K, LANES)]
    tail = {k: int(min(np.count_nonzero(obs[k][n, LANES:]) for n in range(N))) for k in PER_KEYWORD}
    log(case, tiles=tiles, row_floats=5 * K + 2, action_floats=K + 1, least_not_zero_past_256_per_env=tail,
        bids_distinct_past_256=len(set(actions[:, 1 + LANES:].reshape(-1).tolist())))
    assert len(tiles) > 1 and ((5 * K + 2) % 4 != 0 or (K + 1) % 4 != 0)
    assert all(v > 0 for v in tail.values()), tail
    assert len(set(actions[:, 1 + LANES:].reshape(-1).tolist())) > 1 and len(set(actions[:, 0].tolist())) == N


def masked_reset(case, obs, mask):
    """mid-episode the masked envs hold something to clear in every plane past keyword 256, and the others something to keep"""
    mask = np.asarray(mask) == 1
    clear = {k: int(np.count_nonzero(obs[k][mask][:, LANES:])) for k in PER_KEYWORD}
    keep = {k: int(np.count_nonzero(obs[k][~mask][:, LANES:])) for k in PER_KEYWORD}
    log(case, masked_envs=np.flatnonzero(mask).tolist(), not_zero_past_keyword_256_to_clear=clear, to_keep=keep, days=obs["days_passed"].tolist())
    assert mask.any() and not mask.all() and all(v > 0 for v in clear.values()) and all(v > 0 for v in keep.values())
    assert np.all(obs["days_passed"] > 0) and np.all(obs["cumulative_profit"] != 0)


def flat_actions(o):
    """[N, K + 1] = [budget, bids...]: the oracle's sampled bids and an ample budget that differs from env to env"""
    bids = o.sample_bids(0.3, 1.0)
    return np.concatenate([(1.0e6 + np.arange(o.N, dtype=F))[:, None], bids], axis=1).astype(F)


# ---- 6. the metric readers past one env a slab --------------------------------------------------------------------------------------------
METRIC_SEEDS = 500


def metric_planes(model):
    c = METRICS
    return H.implicit_params(c["N"], c["K"], c["planes_seed"], mean_volume=32) if model == "implicit" else H.explicit_params(c["N"], c["K"], c["planes_seed"])


def metric_oracle(model):
    """(oracle, planes, implicit) of the metric case after reset(seeds = METRIC_SEEDS + env)"""
    c, planes = METRICS, metric_planes(model)
    o = oracle_after_reset(planes, np.arange(c["N"], dtype=np.uint64) + METRIC_SEEDS, model=orc.IMPLICIT if model == "implicit" else orc.EXPLICIT,
                           max_days=c["max_days"], auto_reset=True, threads=8)
    return o, planes, model == "implicit"


def metric_run(o, implicit, on_step=None):
    """the case's four steps on the oracle (and, through on_step(bids, budget, ref), on a device beside it) -> MetricSums"""
    sums = MetricSums(o.N, o.K)
    for budget in METRICS["budgets"]:
        bids = o.sample_bids(0.3, 1.0) if implicit else o.sample_bids(0.05, 2.0)
        ref = o.step(bids, budget)
        if on_step is not None:
            on_step(bids, budget, ref)
        sums.add(ref, implicit)
    return sums



def metric_cents(ref, implicit):
    """a step's profit per (env, keyword) and per env in cents: the oracle's integers (IMPLICIT), or the float-money models'
    rounding of the float32 observation (k_metric_accumulate: rint of the float32 product revenue x 100, less rint of the float64
    product cost x 100; the env's is rint(reward x 100))"""
    if implicit:
        nk = (ref["revenue_cents"] - ref["cost_cents"]).astype(np.int64)
        return nk, nk.sum(axis=1)
    revenue, cost = H.f32_dollars(ref["revenue_cents"]), ref["cost"].astype(F)              # (the float32 observation)
    nk = np.rint(revenue * F(100.0)).astype(np.int64) - np.rint(cost.astype(np.float64) * 100.0).astype(np.int64)
    return nk, np.rint(ref["reward"] * 100.0).astype(np.int64)


class MetricSums:
    """what metrics_read() and metrics_read_nk() must return after the steps added"""

    def __init__(self, N, K):
        self.nk, self.env = np.zeros((N, K), np.int64), np.zeros((4, N), np.int64)
        self.volume = np.zeros(K, np.int64)

    def add(self, ref, implicit):
        nk, env = metric_cents(ref, implicit)
        self.nk += nk
        done = (ref["terminated"] != 0) | (ref["truncated"] != 0)
        self.env += np.stack([env, np.ones_like(env), done.astype(np.int64), (ref["truncated"] != 0).astype(np.int64)])
        self.volume += ref["impressions"].sum(axis=0)

    columns = property(lambda self: self.nk.sum(axis=0))
    scalars = property(lambda self: self.env.sum(axis=1))

    def precondition(self, case, slabs=METRICS["slabs"]):
        """the columns of the first 64 envs alone (every slab cut to one env) differ from the full ones in every keyword that saw
        an impression, and every scalar that is not zero differs from its sum over the first 256 envs (one pass of the reduce)"""
        N, K = self.nk.shape
        per = -(-N // slabs)
        sizes = [max(0, min(N, (s + 1) * per) - s * per) for s in range(slabs)]
        seen = self.volume > 0
        same = int(np.sum(self.nk[:slabs].sum(axis=0)[seen] == self.columns[seen]))
        head = self.env[:, :LANES].sum(axis=1)
        log(case, N=N, K=K, envs_a_slab=per, full_slabs=sizes.count(per), slabs_partly_filled=[s for s in sizes if 0 < s < per],
            empty_slabs=sizes.count(0), keywords_with_impressions=int(seen.sum()), columns_equal_to_the_first_64_envs_alone=same,
            scalars=self.scalars.tolist(), first_256_envs_alone=head.tolist())
        assert per > 1 and sizes.count(0) > 0 and N > LANES and K > LANES
        assert seen.any() and same == 0
        assert all(self.scalars[:3] != 0) and all(h != s for h, s in zip(head, self.scalars) if s != 0)


# ---- 7. more envs than 65 535 -----------------------------------------------------------------------------------------------------------
def many_envs(case, obs, bids):
    """the envs past 65 535 hold counts and bids that are not zero and differ from env 0's: a wrapped block index shows"""
    N = obs["impressions"].shape[0]
    last = {k: int(np.count_nonzero(obs[k][65535:])) for k in PER_KEYWORD}
    log(case, N=N, not_zero_from_env_65535=last, last_env_bids=bids[-1].tolist(), env_0_bids=bids[0].tolist(),
        env_1_bids=bids[N - 65536].tolist())
    assert N > 65535 and all(v > 0 for v in last.values()), last
    assert not np.array_equal(bids[-1], bids[N - 1 - 65536]) and not np.array_equal(bids[-1], bids[0])
