"""A numpy restatement of NaiveInterpolationStrategy (adcraft/baselines/interpolated_expectations.py:298-439), written from
its documented semantics: the checker of the device agent (parts/kernel_interp_agent.inc) and of its host twin.

One agent per env; every keyword keeps the zero-margin agent's rpc / sctr cache (float32), the largest key it has seen,
and dicts {cent: [mean, count]} for the cents 1..300 the agent interpolates: float32 means of the clicks, float64 means of
cost / clicks (only observations with clicks > 0)."""
import numpy as np

ARANGE = np.arange(0.01, 3.01, 0.01)           # the interpolation x values, cents 1..300


def key_of(bid):
    """float(bidstr(bid)): round(float(float32 bid), 2)"""
    return round(float(np.float32(bid)), 2)


def smoothed(values):
    v = np.asarray(values, dtype=np.float64)
    w = np.bartlett(min(5, max(1, len(v) - 1)))
    m = np.sum(w)
    w = w / m if m > 0 else np.array([1.0])
    return np.convolve(v, w, mode="same")


class KeywordCache:
    def __init__(self):
        self.ave_rpc, self.n_rpc = np.float32(0.0), 0
        self.ave_sctr, self.n_sctr = np.float32(0.4), 0
        self.max_observed = 0.03
        self.clicks = {}            # cent -> [np.float32 mean, count]
        self.cpc = {}               # cent -> [float mean, count]

    def update(self, bid, clicks, cost, conversions, revenue):
        bc, sc, rev, cost = np.float32(clicks), np.float32(conversions), np.float32(revenue), np.float32(cost)
        if bc > 0:
            if sc > 0:
                self.ave_rpc = np.float32((rev / sc) + np.float32(float(self.ave_rpc) * self.n_rpc)) / np.float32(self.n_rpc + 1)
                self.n_rpc += 1
            all_convs = (sc / bc) * bc + np.float32(float(self.ave_sctr) * self.n_sctr)
            self.ave_sctr = np.float32(all_convs / np.float32(max(1.0, float(clicks) + self.n_sctr)))
            self.n_sctr += 1
        key = key_of(bid)
        self.max_observed = max(self.max_observed, key)
        cent = int(round(key * 100))
        if not 1 <= cent <= 300:
            return
        if cent in self.clicks:
            a, n = self.clicks[cent]
            self.clicks[cent] = [np.float32((bc + np.float32(a * np.float32(n))) / np.float32(n + 1)), n + 1]
        else:
            self.clicks[cent] = [bc, 1]
        if bc > 0:
            cpc = float(cost) / float(bc)
            if cent in self.cpc:
                a, n = self.cpc[cent]
                self.cpc[cent] = [(cpc + a * n) / (1 + n), n + 1]
            else:
                self.cpc[cent] = [cpc, 1]

    def erpc(self):
        if self.n_rpc < 1 and self.n_sctr < 1:
            return 0.3
        if self.n_rpc < 1:
            return 0.7 * float(self.ave_sctr)
        return float(self.ave_rpc) * float(self.ave_sctr)

    def curves(self, grid):
        """(margin, cost) over the grid"""
        grid = np.asarray(grid, dtype=np.float64)
        cc = sorted(self.cpc)
        if cc:
            xs = ARANGE[np.array(cc) - 1]
            ys = np.array([self.cpc[c][0] for c in cc], dtype=np.float64)
            cpc = np.interp(grid, xs, smoothed(ys), left=0.01, right=np.max(ys))
            kc = sorted(self.clicks)
            xk = ARANGE[np.array(kc) - 1]
            yk = np.array([float(self.clicks[c][0]) for c in kc], dtype=np.float64)
            clicks = np.interp(grid, xk, smoothed(yk), left=yk[0], right=yk[-1])
        else:
            cpc, clicks = 0.9 * grid, 1.0
        return (-cpc + self.erpc()) * (0.01 + clicks), cpc * (0.01 + clicks)

    def acquisition(self, margin, threshold, bid_step):
        thr = -(1 / (1 + self.n_rpc + float(self.n_sctr) / 5)) * np.abs(threshold)
        a = np.maximum(margin, thr) - thr
        end = min(len(a), int(100 * (self.max_observed + bid_step) - 1))
        a[end:] = 0.0
        return a, np.sum(a[:end])


def choice_index(p, u):
    """rng.choice(range(len(p)), p=p) for the uniform u it draws"""
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    return int(np.searchsorted(cdf, u, side="right"))


class InterpAgentRef:
    def __init__(self, num_envs, num_keywords, threshold=-0.2, bid_step=0.03):
        self.N, self.K = num_envs, num_keywords
        self.threshold, self.bid_step = threshold, bid_step
        self.caches = [[KeywordCache() for _ in range(num_keywords)] for _ in range(num_envs)]
        self.budget = np.zeros(num_envs)
        self.profit_beliefs = np.zeros(num_envs)
        self.cost_beliefs = np.zeros(num_envs)

    def update(self, prev_bids, clicks, cost, conversions, revenue):
        for n in range(self.N):
            for k in range(self.K):
                self.caches[n][k].update(prev_bids[n][k], clicks[n][k], cost[n][k], conversions[n][k], revenue[n][k])

    def act(self, grid, uniforms):
        """uniforms [N, K] (read where a draw happens) -> (bids [N, K] float64, drew [N, K] bool)"""
        grid = np.asarray(grid, dtype=np.float64)
        bids = np.full((self.N, self.K), 0.01)
        drew = np.zeros((self.N, self.K), bool)
        for n in range(self.N):
            ec = ep = 0.0
            for k in range(self.K):
                c = self.caches[n][k]
                margin, cost = c.curves(grid)
                a, mass = c.acquisition(margin, self.threshold, self.bid_step)
                if not mass > 0:
                    continue
                i = choice_index(a / mass, uniforms[n][k])
                bids[n, k], drew[n, k] = grid[i], True
                ec += cost[i] if c.n_sctr > 0 else grid[i]
                if c.n_rpc > 0:
                    ep += margin[i]
            base = max(min(ec, 10000), 1000)
            self.budget[n] = 1.5 * base if ep > 0 else (base if ep > self.K * self.threshold else 1000.0)
            self.profit_beliefs[n], self.cost_beliefs[n] = ep, ec
        return bids, drew


def twin_act(lib, cache, grid, threshold, bid_step, u):
    """adc_interp_act_host on a KeywordCache -> (margin [L], cost [L], index (-1: no draw), bid, mass)"""
    import ctypes as C
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    kc, pc = sorted(cache.clicks), sorted(cache.cpc)
    clk_cent = np.array(kc, np.uint16)
    clk_ave = np.array([cache.clicks[c][0] for c in kc], np.float32)
    cpc_cent = np.array(pc, np.uint16)
    cpc_ave = np.array([cache.cpc[c][0] for c in pc], np.float64)
    margin, cost = np.zeros(grid.size), np.zeros(grid.size)
    bid, idx, mass = C.c_double(0.0), C.c_int32(0), C.c_double(0.0)
    rc = lib.adc_interp_act_host(float(cache.ave_rpc), cache.n_rpc, float(cache.ave_sctr), cache.n_sctr, cache.max_observed,
                                 threshold, bid_step, grid.ctypes.data, grid.size, len(kc), clk_cent.ctypes.data, clk_ave.ctypes.data,
                                 len(pc), cpc_cent.ctypes.data, cpc_ave.ctypes.data, u, margin.ctypes.data, cost.ctypes.data,
                                 C.byref(bid), C.byref(idx), C.byref(mass))
    assert rc == 0
    return margin, cost, idx.value, bid.value, mass.value


def g13_grid(case, step):
    """the grid in force at a G13 step"""
    if case["grid_kind"] == 0:
        return np.linspace(0.01, 3.00, 300)
    if case["grid_kind"] == 1:
        return ARANGE[:step["grid"]]
    return np.array(case["grids"][0])
