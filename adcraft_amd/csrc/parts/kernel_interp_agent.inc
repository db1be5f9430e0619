// kernel_interp_agent.inc - NaiveInterpolationStrategy (adcraft/baselines/interpolated_expectations.py:298-439) on the
// device, one agent per env: its update (:349-358 -> full_cache_update :214-235) and its act (:405-439).  The per-keyword
// act is adc::interp_pick / adc::interp_point (adc_interp.h), the code the host twin adc_interp_act_host runs too.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// State.  Per keyword [N*K]: the rpc / sctr cache of the zero-margin agent, max_observed (the largest key of every bid seen,
// 0.03 included), the agent's own last bid as float32, and two lists of interpolation points in cents 1..300, each sorted
// by cent and stored slot-major ([cap][N*K]: 64 lanes walking their slots in lockstep read coalesced):
//   clicks: every observation creates or updates one (cent u16, float32 mean of the clicks, count i32) - 10 bytes a slot
//   cpc:    only observations with clicks > 0 (cent u16, float64 mean of cost / clicks, count i32)    - 14 bytes a slot
// 24 bytes per slot of capacity and 56 per keyword besides.  An update adds at most one point to each list, so a capacity of
// C slots holds every point while the updates since init number at most C (the host counts them; 300 can never overflow).
struct InterpView {
    float *ave_rpc;
    int32_t *n_rpc;
    float *ave_sctr;
    int32_t *n_sctr;
    double *max_obs;           // [N*K] float(max(observed keys + [0.03]))
    float *last_bid;           // [N*K] the bid the agent returned, as torch.Tensor([bid]) holds it
    int32_t *last_index;       // [N*K] its grid index (-1: no draw, bid 0.01)
    int32_t *n_clk, *n_cpc;    // [N*K] points in each list
    uint16_t *clk_cent;        // [cap][N*K]
    float *clk_ave;
    int32_t *clk_cnt;
    uint16_t *cpc_cent;        // [cap][N*K]
    double *cpc_ave;
    int32_t *cpc_cnt;
    double *kw_cost, *kw_profit;     // [N*K] each keyword's term of cost_beliefs / profit_beliefs (+0: none), summed in order
    double *budget, *profit, *cost;  // [N] the agent's float64 budget, profit_beliefs, cost_beliefs
    uint64_t *key;             // [N] the agent's own stream (stage ST_INTERP)
    uint32_t *tick;            // [N]
    const double *grid;        // allowed_bids [n_bids]
    int n_bids;
    int cap;
    size_t slot_stride;        // N*K of the whole engine (env groups offset the base pointers, not the stride)
    double threshold, bid_step;
};

// the slots of one keyword's lists
struct InterpSlots {
    const InterpView &p;
    size_t o;
    __device__ __forceinline__ adc::InterpSeries<float> clicks() const { return {p.clk_cent + o, p.clk_ave + o, p.slot_stride, p.n_clk[o]}; }
    __device__ __forceinline__ adc::InterpSeries<double> cpc() const { return {p.cpc_cent + o, p.cpc_ave + o, p.slot_stride, p.n_cpc[o]}; }
};

// update_cached_rpc_and_sctr (:107-152) for one observation, in the zero-margin agent's float32 order (k_agent_step)
__device__ __forceinline__ void interp_rpc_sctr(float &ave_rpc, int32_t &n_rpc, float &ave_sctr, int32_t &n_sctr, int32_t clicks,
                                                int32_t convs, float rev)
{
    const float bc = (float)clicks, sc = (float)convs;
    if (bc > 0.0f) {
        if (sc > 0.0f) {
            const float rpc_obs = rev / sc;
            const float term = (float)((double)ave_rpc * (double)n_rpc);
            ave_rpc = (rpc_obs + term) / (float)(n_rpc + 1);
            n_rpc += 1;
        }
        const float s_obs = sc / bc;
        const float termc = (float)((double)ave_sctr * (double)n_sctr);
        const float all_convs = s_obs * bc + termc;
        const double all_obs = (double)clicks + (double)n_sctr;
        ave_sctr = all_convs / (float)(all_obs > 1.0 ? all_obs : 1.0);
        n_sctr += 1;
    }
}

// position of `cent` in a sorted list of n slots: its slot if present (found), else where it goes
__device__ __forceinline__ int interp_find(const uint16_t *cent, size_t stride, int n, int c, bool &found)
{
    int i = n - 1;                 // (the agent's own bids sit near the top of its list: scan down from there)
    while (i >= 0 && (int)cent[(size_t)i * stride] > c) --i;
    found = i >= 0 && (int)cent[(size_t)i * stride] == c;
    return found ? i : i + 1;
}

// update_ave_cpc_cache / update_ave_clicks_cache (:22-64) of one keyword for the observation (bid, clicks, cost)
__device__ __forceinline__ void interp_cache_update(const InterpView &p, size_t o, float bid, int32_t clicks_i, float cost)
{
    const double kc = adc::interp_key_cents(bid);
    const double key = kc / 100.0;
    if (key > p.max_obs[o]) p.max_obs[o] = key;
    if (!(kc >= 1.0 && kc <= (double)adc::kInterpCents)) return;      // outside np.arange(0.01, 3.01, 0.01): never read
    const int c = (int)kc;
    const size_t S = p.slot_stride;
    const float clicks = (float)clicks_i;
    {   // ave_clicks: float32 running mean, zero clicks included
        int n = p.n_clk[o];
        bool found;
        const int i = interp_find(p.clk_cent + o, S, n, c, found);
        if (found) {
            const size_t s = o + (size_t)i * S;
            const int32_t m = p.clk_cnt[s];
            p.clk_ave[s] = (clicks + p.clk_ave[s] * (float)m) / (float)(1 + m);
            p.clk_cnt[s] = m + 1;
        } else if (n < p.cap) {
            for (int j = n; j > i; --j) {
                const size_t d = o + (size_t)j * S, q = d - S;
                p.clk_cent[d] = p.clk_cent[q]; p.clk_ave[d] = p.clk_ave[q]; p.clk_cnt[d] = p.clk_cnt[q];
            }
            const size_t s = o + (size_t)i * S;
            p.clk_cent[s] = (uint16_t)c; p.clk_ave[s] = clicks; p.clk_cnt[s] = 1;
            p.n_clk[o] = n + 1;
        }
    }
    if (clicks > 0.0f) {   // ave_cpc: float64 running mean of float32 cost / float32 clicks
        const double cpc = (double)cost / (double)clicks;
        int n = p.n_cpc[o];
        bool found;
        const int i = interp_find(p.cpc_cent + o, S, n, c, found);
        if (found) {
            const size_t s = o + (size_t)i * S;
            const int32_t m = p.cpc_cnt[s];
            p.cpc_ave[s] = (cpc + p.cpc_ave[s] * (double)m) / (double)(1 + m);
            p.cpc_cnt[s] = m + 1;
        } else if (n < p.cap) {
            for (int j = n; j > i; --j) {
                const size_t d = o + (size_t)j * S, q = d - S;
                p.cpc_cent[d] = p.cpc_cent[q]; p.cpc_ave[d] = p.cpc_ave[q]; p.cpc_cnt[d] = p.cpc_cnt[q];
            }
            const size_t s = o + (size_t)i * S;
            p.cpc_cent[s] = (uint16_t)c; p.cpc_ave[s] = cpc; p.cpc_cnt[s] = 1;
            p.n_cpc[o] = n + 1;
        }
    }
}

// update (prev_bids: NULL = the agent's own last bids) and/or act.  One workgroup per env, lanes stride over keywords,
// one lane per keyword (the pairwise mass and the cdf are ordered sums); thread 0 then sums the beliefs in keyword order.
__global__ __launch_bounds__(256) void k_interp_step(View v, InterpView p, const float *__restrict__ prev_bids,
                                                     const int32_t *__restrict__ clicks, const float *__restrict__ cost,
                                                     const int32_t *__restrict__ convs, const float *__restrict__ revenue,
                                                     int do_update, int do_act, const double *__restrict__ replay_u,
                                                     float budget_override, float *__restrict__ bids, float *__restrict__ budgets)
{
    const int env = blockIdx.x, K = v.K;
    const uint64_t key = p.key[env];
    const uint32_t tick = p.tick[env];
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const size_t o = (size_t)env * K + k;
        float ave_rpc = p.ave_rpc[o], ave_sctr = p.ave_sctr[o];
        int32_t n_rpc = p.n_rpc[o], n_sctr = p.n_sctr[o];
        if (do_update) {
            interp_rpc_sctr(ave_rpc, n_rpc, ave_sctr, n_sctr, clicks[o], convs[o], revenue[o]);
            p.ave_rpc[o] = ave_rpc; p.n_rpc[o] = n_rpc; p.ave_sctr[o] = ave_sctr; p.n_sctr[o] = n_sctr;
            interp_cache_update(p, o, prev_bids ? prev_bids[o] : p.last_bid[o], clicks[o], cost[o]);
        }
        if (!do_act) continue;
        const InterpSlots sl{p, o};
        const adc::InterpSeries<float> clk = sl.clicks();
        const adc::InterpSeries<double> cpc = sl.cpc();
        double cpc_right = 0.0;
        for (int i = 0; i < cpc.n; ++i) { const double y = cpc.y(i); cpc_right = (i == 0 || y > cpc_right) ? y : cpc_right; }
        const double erpc = adc::interp_erpc(ave_rpc, n_rpc, ave_sctr, n_sctr);
        const double thr = adc::interp_threshold(n_rpc, n_sctr, p.threshold);
        const int end = adc::interp_end_index(p.max_obs[o], p.bid_step, p.n_bids);
        const double *grid = p.grid;
        auto eval = [&](int j) { return adc::interp_point(clk, cpc, cpc_right, erpc, grid[j]); };
        auto uniform = [&]() {
            if (replay_u) return replay_u[o];
            const adc::U4 w = adc::draw(key, 0u, adc::ST_INTERP, (uint32_t)k, tick);
            return uniform53(w.x, w.y);
        };
        const adc::InterpPick pk = adc::interp_pick(eval, thr, end, uniform);
        double bid = 0.01, kc = 0.0, kp = 0.0;
        if (pk.index >= 0) {
            bid = grid[pk.index];
            const adc::InterpPoint q = eval(pk.index);
            kc = n_sctr > 0 ? q.cost : bid;
            kp = n_rpc > 0 ? q.margin : 0.0;
        }
        p.kw_cost[o] = kc;
        p.kw_profit[o] = kp;
        p.last_bid[o] = (float)bid;
        p.last_index[o] = pk.index;
        // the env rounds the float64 bid to cents (gymnasium_kw_env.py:215); hand over exactly that value
        double c = __builtin_rint(bid * 100.0);
        c = c >= 1.0 ? c : 1.0;
        c = c < 1.0e9 ? c : 1.0e9;
        bids[o] = (float)(c / 100.0);
    }
    if (!do_act) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        double ec = 0.0, ep = 0.0;
        const size_t o0 = (size_t)env * K;
        for (int k = 0; k < K; ++k) { ec = ec + p.kw_cost[o0 + k]; ep = ep + p.kw_profit[o0 + k]; }
        const double clamped = ec < 10000.0 ? ec : 10000.0;
        const double base = clamped > 1000.0 ? clamped : 1000.0;
        double b;
        if (ep > 0.0) b = 1.5 * base;                                      // :433-438
        else if (ep > (double)K * p.threshold) b = base;
        else b = 1000.0;
        p.budget[env] = b;
        p.profit[env] = ep;
        p.cost[env] = ec;
        budgets[env] = budget_override > 0.0f ? budget_override : (float)(__builtin_rint(b * 100.0) / 100.0);
        p.tick[env] = tick + 1u;
    }
}

__global__ void k_interp_init(InterpView p, int K, const uint64_t *seeds, uint64_t seed, int64_t env_id_base)
{
    const int env = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) {
        const size_t o = (size_t)env * K + k;
        p.ave_rpc[o] = 0.0f;           // get_empty_cache, :286-295
        p.n_rpc[o] = 0;
        p.ave_sctr[o] = 0.4f;
        p.n_sctr[o] = 0;
        p.max_obs[o] = 0.03;           // observed_bids.append(0.03), :387
        p.last_bid[o] = 0.01f;         // the notebooks' first previous_action: 0.01 + np.zeros(K)
        p.last_index[o] = -1;
        p.n_clk[o] = 0;
        p.n_cpc[o] = 0;
        p.kw_cost[o] = 0.0;
        p.kw_profit[o] = 0.0;
    }
    if (k == 0) {
        p.key[env] = seeds ? splitmix64(seeds[env] ^ 0x3C6EF372FE94F82Bull)
                           : splitmix64(seed ^ splitmix64((uint64_t)(env_id_base + env) + 0x510E527FADE682D1ull));
        p.tick[env] = 0u;
        p.budget[env] = 0.0;
        p.profit[env] = 0.0;
        p.cost[env] = 0.0;
    }
}
