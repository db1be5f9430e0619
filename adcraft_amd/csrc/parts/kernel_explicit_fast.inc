// kernel_explicit_fast.inc - k_step_explicit_fast: the EXPLICIT model's keyword-parallel pass
// (part of the single translation unit adc_engine.hip; see that file for the overview)
// -------------------------------------------------------------------------------------------------
// The EXPLICIT keyword (ExplicitKeyword, adcraft/synthetic_kw_classes.py:457-575; the default constructor's model)
// keeps money in float64, so every sum must be taken in the reference's order.  Those orders are all per keyword:
// a keyword's observed cost adds its paid clicks' costs cell after cell, left to right (bidding_simulation.py:109,
// 124-147), its profit adds one (revenue - cost) per cell (:118, 141), and the reward adds the keywords' profits in
// keyword order (gymnasium_kw_env.py:222).  Only the budget couples keywords.  So: one lane walks one keyword's 24
// cells in order - which reproduces every float64 sum bit for bit - and the env is handed to the serial reference-order
// walker (k_step_exact<EXPLICIT>) only if its total spend comes within a margin of the budget, i.e. only if one of
// the reference's `budget >= cost` checks (:97-104) or its `remaining_budget <= 0` stop (:230-233) could have
// gone the other way.
// One workgroup per env; lanes stride over keywords; dynamic LDS: profit[K] (float64).
constexpr int kXDayK = 256;          // k_step_float_day (below): keywords it takes, one per lane, at its base width ...
constexpr int kXDayKMax = 1024;      // ... and at its widest (512- and 1024-lane workgroups for K > 256)
constexpr int kXDayInline = 4;       // ... clicked impressions of a cell listed in place; further ones go to chained
constexpr int kXDayPool = 512;       // overflow blocks of four, shared by the row's cells (two per lane)
__global__ __launch_bounds__(256) void k_step_explicit_fast(View v, const float *__restrict__ bids,
                                                            const float *__restrict__ budget_in, int parity)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ double part[256 / kWave];
    double *s_profit = reinterpret_cast<double *>(lds_raw);          // [K]
    const int env = blockIdx.x, K = v.K;
    const int tid = threadIdx.x;
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    const bool drift = v.drift_on && v.drift_pending[env];
    if (env == 0 && tid == 0) { v.flag_count[parity ^ 1] = 0; v.flag_next[parity ^ 1] = 0; v.xover_count[parity ^ 1] = 0; v.retry_count[parity ^ 1] = 0; }
    // the budget bound yesterday (k_step_float_day's hint): this pass's result would be discarded - a scheduling hint only;
    // the day kernel then also applies the pending drift
    if (K <= kXDayKMax && v.exact_hint[env]) {
        if (tid == 0) v.flag_list[atomicAdd(&v.flag_count[parity], 1)] = env;
        return;
    }

    double my_cost = 0.0;
    for (int k = tid; k < K; k += blockDim.x) {
        const size_t o = (size_t)env * K + k;
        float vol_mean = param_at(v, ADC_P_VOL_MEAN, env, k);
        const float vol_std = param_at(v, ADC_P_VOL_STD, env, k);
        float bctr = param_at(v, ADC_P_BCTR, env, k), sctr = param_at(v, ADC_P_SCTR, env, k);
        if (drift && drift_keyword(v, env, key, tick - 1u, k, vol_mean, vol_std, bctr, sctr)) {
            param_at(v, ADC_P_VOL_MEAN, env, k) = vol_mean;
            param_at(v, ADC_P_BCTR, env, k) = bctr;
            param_at(v, ADC_P_SCTR, env, k) = sctr;
        }
        const float mu = param_at(v, ADC_P_REV_MEAN, env, k), sd = param_at(v, ADC_P_REV_STD, env, k);
        const uint64_t t_click = adc::bernoulli_threshold(bctr), t_conv = adc::bernoulli_threshold(sctr);
        const long long bid_c = adc::bid_to_cents(bids[o]);
        const float bid_d = (float)((double)bid_c / 100.0);
        const uint64_t t_imp = adc::bernoulli_threshold(adc::threshold_sigmoid_f32(bid_d, v.imp_thresh, param_at(v, ADC_P_A, env, k),
                                                                                  param_at(v, ADC_P_B, env, k)));
        const int V = adc::volume_from_word(adc::volume_word(key, (uint32_t)k, tick), vol_mean, vol_std, g_norm_table);

        double obs_cost = 0.0, profit = 0.0;
        long long rev_c = 0;
        int imps_k = 0, paid_k = 0, convs_k = 0;
        for (int t = 0; t < adc::kTimesteps; ++t) {
            int32_t j0, n;
            adc::cell_range(V, t, j0, n);
            double cell_cost = 0.0;
            long long cell_rev_c = 0;
            int imps = 0;
            for (int i = 0; i < n; ++i) {
                const adc::U4 w = adc::draw(key, (uint32_t)(j0 + i), adc::ST_AUCTION, (uint32_t)k, tick);
                if (!adc::bernoulli(w.x, t_imp)) continue;                    // Binomial(n, p) as n Bernoullis (src/lib.rs:70-76)
                ++imps;
                if (!adc::bernoulli(w.z, t_click)) continue;
                const double c = (double)adc::explicit_cost(w.y, bid_d);      // cost_create, src/lib.rs:54-67
                cell_cost += c;                                               // every click is affordable here (see the header)
                obs_cost += c;
                ++paid_k;
                if (adc::bernoulli(w.w, t_conv)) {
                    ++convs_k;
                    const adc::U4 w2 = adc::draw(key, (uint32_t)(j0 + i), adc::ST_XREV, (uint32_t)k, tick);
                    cell_rev_c += adc::revenue_cents(w2.x, mu, sd);
                }
            }
            if (imps == 0) {
                // phantom zero-cost click opportunity (synthetic_kw_classes.py:514-515), once per cell
                const adc::U4 w = adc::draw(key, (uint32_t)t, adc::ST_XPHANTOM, (uint32_t)k, tick);
                if (adc::bernoulli(w.x, t_click)) {
                    ++paid_k;
                    if (adc::bernoulli(w.y, t_conv)) {
                        ++convs_k;
                        cell_rev_c += adc::revenue_cents(w.z, mu, sd);
                    }
                }
            }
            imps_k += imps;
            rev_c += cell_rev_c;
            profit += (double)cell_rev_c / 100.0 - cell_cost;                 // combine_outcomes: profit += profit
        }
        v.imp[o] = imps_k;
        v.clk[o] = paid_k;
        v.conv[o] = convs_k;
        v.cost[o] = (float)obs_cost;
        v.rev[o] = (float)rev_c / 100.0f;
        s_profit[k] = profit;
        my_cost += obs_cost;
    }
    // total spend of the env (any order: it is only compared against the budget with a margin)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) my_cost += __shfl_xor(my_cost, s, 64);
    if ((tid & 63) == 0) part[tid >> 6] = my_cost;
    __syncthreads();
    if (tid == 0) {
        double spend = 0.0;
        for (int i = 0; i < (int)(blockDim.x / kWave); ++i) spend += part[i];
        const double budget_d = (double)adc::budget_to_cents(budget_in[env]) / 100.0;     // np.round(budget, 2)
        if (budget_d - spend > 1.0e-6 * (1.0 + budget_d)) {
            double reward = 0.0;                                   // rust.sum_list(profits): left to right (gymnasium_kw_env.py:222)
            for (int k = 0; k < K; ++k) reward += s_profit[k];
            step_tail(v, env, tick, false, 0, reward);
        } else {
            v.flag_list[atomicAdd(&v.flag_count[parity], 1)] = env;          // the budget may bind: reference-order walker
        }
    }
}

// -------------------------------------------------------------------------------------------------
// k_step_general_fast: the keyword-parallel pass of IMPLICIT_GENERAL - the reference's default ImplicitKeyword
// (synthetic_kw_classes.py:610-686: B ~ Binomial(max_bidders, participation) other bidders per (sub-timestep, keyword) call, raw
// Laplace bids, nth_price_auction over the top num_winners + 2, synthetic_kw_helpers.py:116-180).  Same plan as
// k_step_explicit_fast, for the same reason: money is float64 here too (bids are not rounded to cents), every sum is per
// keyword in the reference's order, only the budget couples keywords - so one lane walks one keyword's 24 cells in order, and the
// env is left to the reference-order walker (k_step_exact<IMPLICIT_GENERAL>) only if the budget may bind.  A price can be
// negative (the bids are raw Laplace draws), so the running spend is not monotone: the env is flagged when the sum of the
// POSITIVE costs - an upper bound of every prefix of the spend - comes within the margin of the budget.
// The auction itself is the walker's code: top four competitor bids kept sorted in registers by an insertion network.
__global__ __launch_bounds__(256) void k_step_general_fast(View v, const float *__restrict__ bids,
                                                           const float *__restrict__ budget_in, int parity)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ double part[256 / kWave];
    double *s_profit = reinterpret_cast<double *>(lds_raw);          // [K]
    const int env = blockIdx.x, K = v.K;
    const int tid = threadIdx.x;
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    const bool drift = v.drift_on && v.drift_pending[env];
    if (env == 0 && tid == 0) { v.flag_count[parity ^ 1] = 0; v.flag_next[parity ^ 1] = 0; v.xover_count[parity ^ 1] = 0; v.retry_count[parity ^ 1] = 0; }
    // the budget bound yesterday (the walker's hint): this pass's result would be discarded - a scheduling hint only; the
    // walker then also applies the pending drift
    if (v.exact_hint[env]) {
        if (tid == 0) v.flag_list[atomicAdd(&v.flag_count[parity], 1)] = env;
        return;
    }
    const int top = v.num_winners + 2;
    const uint64_t t_part = adc::bernoulli_threshold(v.participation_rate);
    const adc::BidderLaw bidder_law = adc::general_bidder_law(v.max_bidders, v.participation_rate);
    __shared__ float s_bidder_cdf[adc::kBidderTable];
    if (bidder_law.pmf0 > 0.0f) {
        if (tid == 0) adc::fill_bidder_cdf(s_bidder_cdf, bidder_law);
        __syncthreads();
    }

    double my_spend = 0.0;
    for (int k = tid; k < K; k += blockDim.x) {
        const size_t o = (size_t)env * K + k;
        float vol_mean = param_at(v, ADC_P_VOL_MEAN, env, k);
        const float vol_std = param_at(v, ADC_P_VOL_STD, env, k);
        float bctr = param_at(v, ADC_P_BCTR, env, k), sctr = param_at(v, ADC_P_SCTR, env, k);
        if (drift && drift_keyword(v, env, key, tick - 1u, k, vol_mean, vol_std, bctr, sctr)) {
            param_at(v, ADC_P_VOL_MEAN, env, k) = vol_mean;
            param_at(v, ADC_P_BCTR, env, k) = bctr;
            param_at(v, ADC_P_SCTR, env, k) = sctr;
        }
        const float loc = param_at(v, ADC_P_A, env, k), scale = param_at(v, ADC_P_B, env, k);
        const float mu = param_at(v, ADC_P_REV_MEAN, env, k), sd = param_at(v, ADC_P_REV_STD, env, k);
        const uint64_t t_click = adc::bernoulli_threshold(bctr), t_conv = adc::bernoulli_threshold(sctr);
        const double bid_d = (double)adc::bid_to_cents(bids[o]) / 100.0;
        const int V = adc::volume_from_word(adc::volume_word(key, (uint32_t)k, tick), vol_mean, vol_std, g_norm_table);

        double obs_cost = 0.0, profit = 0.0, spend_pos = 0.0;
        long long rev_c = 0;
        int imps_k = 0, paid_k = 0, convs_k = 0;
        adc::U4 bw{0u, 0u, 0u, 0u};                                       // the bidder-count call of sub-timesteps 4 bw_t .. 4 bw_t + 3
        int bw_t = -1;
        for (int t = 0; t < adc::kTimesteps; ++t) {
            int32_t j0, n;
            adc::cell_range(V, t, j0, n);
            if (n == 0) continue;                                         // (a call without auctions draws nothing that is used)
            int B = 0;                                                    // bidders of this call, :610-621
            if (bidder_law.pmf0 > 0.0f) {                                 // (engine-uniform) by inversion: one call serves four sub-timesteps
                if (bw_t != (t >> 2)) { bw = adc::draw(key, (uint32_t)(t >> 2), adc::ST_GBIDDERS, (uint32_t)k, tick); bw_t = t >> 2; }
                B = adc::bidders_from_table((t & 3) == 0 ? bw.x : (t & 3) == 1 ? bw.y : (t & 3) == 2 ? bw.z : bw.w, s_bidder_cdf, bidder_law.n);
            } else
            for (int b0 = 0; b0 < v.max_bidders; b0 += 4) {
                const adc::U4 w = adc::draw(key, (uint32_t)(64 * t + (b0 >> 2)), adc::ST_GBIDDERS, (uint32_t)k, tick);
                B += (int)adc::bernoulli(w.x, t_part);
                if (b0 + 1 < v.max_bidders) B += (int)adc::bernoulli(w.y, t_part);
                if (b0 + 2 < v.max_bidders) B += (int)adc::bernoulli(w.z, t_part);
                if (b0 + 3 < v.max_bidders) B += (int)adc::bernoulli(w.w, t_part);
            }
            double cell_cost = 0.0;
            long long cell_rev_c = 0;
            for (int i = 0; i < n; ++i) {
                const uint32_t j = (uint32_t)(j0 + i);
                // the auction, decided from the top `num_winners` bids alone (adc_law.h clear_general_auction; the walker and the
                // oracle sort the top num_winners + 2 literally)
                float price;
                if (!adc::clear_general_auction(adc::draw(key, j, adc::ST_GBID, (uint32_t)k, tick), B, top - 2, loc, scale, bid_d, price)) continue;   // :170
                ++imps_k;
                const adc::U4 w3 = adc::draw(key, j, adc::ST_GCLICK, (uint32_t)k, tick);
                if (!adc::bernoulli(w3.x, t_click)) continue;
                const double cost = (double)price;                       // sorted[index - 1], :173-175
                cell_cost += cost;                                        // every click is affordable here (see the header)
                obs_cost += cost;
                if (cost > 0.0) spend_pos += cost;
                ++paid_k;
                if (adc::bernoulli(w3.y, t_conv)) {
                    ++convs_k;
                    cell_rev_c += adc::revenue_cents_tab(w3.z, mu, sd, g_norm_table);
                }
            }
            rev_c += cell_rev_c;
            profit += (double)cell_rev_c / 100.0 - cell_cost;             // combine_outcomes: profit += profit
        }
        v.imp[o] = imps_k;
        v.clk[o] = paid_k;
        v.conv[o] = convs_k;
        v.cost[o] = (float)obs_cost;
        v.rev[o] = (float)rev_c / 100.0f;
        s_profit[k] = profit;
        my_spend += spend_pos;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) my_spend += __shfl_xor(my_spend, s, 64);
    if ((tid & 63) == 0) part[tid >> 6] = my_spend;
    __syncthreads();
    if (tid == 0) {
        double spend = 0.0;
        for (int i = 0; i < (int)(blockDim.x / kWave); ++i) spend += part[i];
        const double budget_d = (double)adc::budget_to_cents(budget_in[env]) / 100.0;     // np.round(budget, 2)
        if (budget_d - spend > 1.0e-6 * (1.0 + budget_d)) {
            double reward = 0.0;                                   // rust.sum_list(profits): left to right (gymnasium_kw_env.py:222)
            for (int k = 0; k < K; ++k) reward += s_profit[k];
            step_tail(v, env, tick, false, 0, reward);
        } else {
            v.flag_list[atomicAdd(&v.flag_count[parity], 1)] = env;          // the budget may bind: reference-order walker
        }
    }
}

// -------------------------------------------------------------------------------------------------
// k_step_general_small + k_general_small_tail: the same pass for a HANDFUL of envs (N K <= kGSmallMaxKeywords; round 4).
// One workgroup walking an env's keywords, a lane per keyword and ~128 auctions per lane one after the other, is latency-bound
// (218 us per step for one env x 100 keywords: ~250 instructions per auction, dependent ones, on one wavefront).  What must run
// in order is only the float64 bookkeeping - a click's cost joins the keyword's sums in auction order - not the auctions
// themselves.  Here a keyword has a WAVEFRONT: 64 consecutive auctions of its day are cleared side by side (bidder count of the
// auction's sub-timestep, top bids, click, conversion, revenue - all addressed by what they are for), and the wave then goes
// through the clicked ones in auction order (a ballot, v_readlane of price / revenue / sub-timestep) - the very additions of
// k_step_general_fast, bit for bit.  The keyword's profit and positive costs go to global memory; k_general_small_tail (one
// wavefront per env) adds the profits in keyword order, tests the budget margin and runs the step tail or flags the env,
// exactly as k_step_general_fast's last lane does.
constexpr int kGSmallMaxKeywords = 16384;            // envs x keywords up to which an engine takes this path
__global__ __launch_bounds__(256) void k_step_general_small(View v, const float *__restrict__ bids)
{
    __shared__ float s_bidder_cdf[adc::kBidderTable];
    const int K = v.K, tid = threadIdx.x, lane = tid & 63;
    const adc::BidderLaw bidder_law = adc::general_bidder_law(v.max_bidders, v.participation_rate);
    if (bidder_law.pmf0 > 0.0f) {
        if (tid == 0) adc::fill_bidder_cdf(s_bidder_cdf, bidder_law);
        __syncthreads();                                 // (the workgroup's only barrier: its four keywords share the table and nothing else)
    }
    const size_t o = (size_t)blockIdx.x * (256 / kWave) + (size_t)(tid >> 6);          // this wavefront's keyword
    if (o >= (size_t)v.N * K) return;
    const int env = (int)(o / K), k = (int)(o - (size_t)env * K);
    if (v.exact_hint[env]) return;                       // the budget bound yesterday: the tail flags the env
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    const int top = v.num_winners + 2;
    const uint64_t t_part = adc::bernoulli_threshold(v.participation_rate);
    float vol_mean = param_at(v, ADC_P_VOL_MEAN, env, k), bctr = param_at(v, ADC_P_BCTR, env, k), sctr = param_at(v, ADC_P_SCTR, env, k);
    const float vol_std = param_at(v, ADC_P_VOL_STD, env, k);
    if (v.drift_on && v.drift_pending[env]) {
        if (drift_keyword(v, env, key, tick - 1u, k, vol_mean, vol_std, bctr, sctr) && lane == 0) {
            param_at(v, ADC_P_VOL_MEAN, env, k) = vol_mean;
            param_at(v, ADC_P_BCTR, env, k) = bctr;
            param_at(v, ADC_P_SCTR, env, k) = sctr;
        }
    }
    const float loc = param_at(v, ADC_P_A, env, k), scale = param_at(v, ADC_P_B, env, k);
    const float mu = param_at(v, ADC_P_REV_MEAN, env, k), sd = param_at(v, ADC_P_REV_STD, env, k);
    const double bid_d = (double)adc::bid_to_cents(bids[o]) / 100.0;
    const int V = adc::volume_from_word(adc::volume_word(key, (uint32_t)k, tick), vol_mean, vol_std, g_norm_table);
    const uint64_t t_click = adc::bernoulli_threshold(bctr), t_conv = adc::bernoulli_threshold(sctr);
    const int cell = V / adc::kTimesteps, first = V - (adc::kTimesteps - 1) * cell;      // adc::cell_range: sub-timestep 0 holds `first` auctions

    double obs_cost = 0.0, profit = 0.0, spend_pos = 0.0, cell_cost = 0.0;
    long long rev_c = 0, cell_rev_c = 0;
    int imps_k = 0, paid_k = 0, convs_k = 0;
    int cur_t = -1;                                      // the sub-timestep whose clicks cell_cost / cell_rev_c are collecting
    for (int base = 0; base < V; base += kWave) {
        // ---- this lane's auction of the 64
        const int j = base + lane;
        float price = 0.0f;
        int rev = 0, t = 0;
        bool win = false, click = false, conv = false;
        if (j < V) {
            t = j < first ? 0 : 1 + (j - first) / cell;               // (cell > 0 whenever an auction lies beyond sub-timestep 0)
            int B = 0;                                                // bidders of the auction's call, :610-621
            if (bidder_law.pmf0 > 0.0f) {
                const adc::U4 bw = adc::draw(key, (uint32_t)(t >> 2), adc::ST_GBIDDERS, (uint32_t)k, tick);
                B = adc::bidders_from_table((t & 3) == 0 ? bw.x : (t & 3) == 1 ? bw.y : (t & 3) == 2 ? bw.z : bw.w, s_bidder_cdf, bidder_law.n);
            } else
            for (int b0 = 0; b0 < v.max_bidders; b0 += 4) {
                const adc::U4 w = adc::draw(key, (uint32_t)(64 * t + (b0 >> 2)), adc::ST_GBIDDERS, (uint32_t)k, tick);
                B += (int)adc::bernoulli(w.x, t_part);
                if (b0 + 1 < v.max_bidders) B += (int)adc::bernoulli(w.y, t_part);
                if (b0 + 2 < v.max_bidders) B += (int)adc::bernoulli(w.z, t_part);
                if (b0 + 3 < v.max_bidders) B += (int)adc::bernoulli(w.w, t_part);
            }
            win = adc::clear_general_auction(adc::draw(key, (uint32_t)j, adc::ST_GBID, (uint32_t)k, tick), B, top - 2, loc, scale, bid_d, price);   // :170
            if (win) {
                const adc::U4 w3 = adc::draw(key, (uint32_t)j, adc::ST_GCLICK, (uint32_t)k, tick);
                click = adc::bernoulli(w3.x, t_click);
                conv = click && adc::bernoulli(w3.y, t_conv);
                if (conv) rev = adc::revenue_cents_tab(w3.z, mu, sd, g_norm_table);
            }
        }
        // ---- the clicked ones folded in auction order.  A sub-timestep without a click adds 0.0 to the keyword's profit in the
        // reference (:141) - nothing - so a sub-timestep is closed when a click of a later one turns up, or at the day's end.
        imps_k += (int)__popcll(__builtin_amdgcn_ballot_w64(win));
        const unsigned long long conv_mask = __builtin_amdgcn_ballot_w64(conv);
        unsigned long long m = __builtin_amdgcn_ballot_w64(click);
        paid_k += (int)__popcll(m);
        convs_k += (int)__popcll(conv_mask);
        while (m) {
            const int l = (int)__builtin_ctzll(m);
            m &= m - 1ull;
            const int ct = __builtin_amdgcn_readlane(t, l);
            if (ct != cur_t && cur_t >= 0) {                          // a new sub-timestep: combine_outcomes of the one before
                rev_c += cell_rev_c;
                profit += (double)cell_rev_c / 100.0 - cell_cost;
                cell_rev_c = 0;
                cell_cost = 0.0;
            }
            cur_t = ct;
            const double cost = (double)__uint_as_float((unsigned int)__builtin_amdgcn_readlane((int)__float_as_uint(price), l));      // sorted[index - 1], :173-175
            cell_cost += cost;
            obs_cost += cost;
            if (cost > 0.0) spend_pos += cost;
            if ((conv_mask >> l) & 1ull) cell_rev_c += (long long)__builtin_amdgcn_readlane(rev, l);
        }
    }
    rev_c += cell_rev_c;
    profit += (double)cell_rev_c / 100.0 - cell_cost;
    if (lane == 0) {
        v.imp[o] = imps_k;
        v.clk[o] = paid_k;
        v.conv[o] = convs_k;
        v.cost[o] = (float)obs_cost;
        v.rev[o] = (float)rev_c / 100.0f;
        v.gs_profit[o] = profit;
        v.gs_spend[o] = spend_pos;
    }
}

__global__ __launch_bounds__(kWave) void k_general_small_tail(View v, const float *__restrict__ budget_in, int parity)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double *s_profit = reinterpret_cast<double *>(lds_raw);          // [K]
    const int env = blockIdx.x, K = v.K, lane = threadIdx.x;
    if (env == 0 && lane == 0) { v.flag_count[parity ^ 1] = 0; v.flag_next[parity ^ 1] = 0; v.xover_count[parity ^ 1] = 0; v.retry_count[parity ^ 1] = 0; }
    if (v.exact_hint[env]) {
        if (lane == 0) v.flag_list[atomicAdd(&v.flag_count[parity], 1)] = env;
        return;
    }
    double spend = 0.0;
    for (int k = lane; k < K; k += kWave) {
        spend += v.gs_spend[(size_t)env * K + k];
        s_profit[k] = v.gs_profit[(size_t)env * K + k];              // (64 loads at a time; the dependent sum below then runs from LDS)
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) spend += __shfl_xor(spend, s, 64);
    __syncthreads();
    if (lane == 0) {
        const double budget_d = (double)adc::budget_to_cents(budget_in[env]) / 100.0;     // np.round(budget, 2)
        if (budget_d - spend > 1.0e-6 * (1.0 + budget_d)) {
            double reward = 0.0;                                   // rust.sum_list(profits): left to right (gymnasium_kw_env.py:222)
            for (int k = 0; k < K; ++k) reward += s_profit[k];
            step_tail(v, env, v.tick[env], false, 0, reward);
        } else {
            v.flag_list[atomicAdd(&v.flag_count[parity], 1)] = env;          // the budget may bind: reference-order walker
        }
    }
}

// -------------------------------------------------------------------------------------------------
// k_step_float_day (K <= 256): a flagged EXPLICIT env's day, one 256-lane workgroup per env, lane = keyword for the
// whole day - the keyword's thresholds, float64 sums and counters stay in registers, LDS holds one ROW of click lists
// (20 KB: occupancy is set by registers, where the one-wavefront-per-env walker below sits at 2 waves per SIMD behind its
// 21 KB of per-env arrays).  Per sub-timestep row (bidding_simulation.py:214-233):
//   1. every lane resolves its keyword's cell and lists the clicked costs in LDS, in auction order;
//   2. wave 0 walks the row's cells that have a click in keyword order, 64 at a time from the row's click mask - the cell's
//      own lane pays its clicks while `budget >= cost` (:97-104) from the campaign's remaining budget, which then loses the
//      cell's cost (:225) and stops the campaign at <= 0 (:230-233): float64, the reference's operation order.  A cell whose
//      first click already costs more than what is left at the start of its 64 breaks at once whatever happens before it
//      (`remaining` only shrinks), so it is not visited; and while what is left exceeds the 64 cells' total by a margin no
//      rounding can bridge, every click is affordable and only the per-cell subtractions run in order;
//   3. every lane finishes its cell: the paid clicks' conversions and revenues, the phantom click of an impression-less
//      cell, and the keyword's float64 sums in the reference's order (cost click by click, profit cell by cell).
// (A cell's first four clicked impressions sit in per-cell slots, further ones in blocks of four chained from a pool the row's
// cells share: the first cell of a low-volume day holds the whole day, bidding_simulation.py:151-167.)  A cell of more than
// 255 auctions, a row that exhausts the pool, and a day that starts with a budget <= 0 send the env to
// k_step_explicit_rows (retry list).  Sets the hint k_step_explicit_fast reads (did the budget bind).
struct XDayBlock {                                  // four more clicked impressions of a cell
    float cost[4];
    unsigned char aidx[4];
    unsigned short next, pad;
};
template <int KMAX>
struct XDayShared {
    float cost[kXDayInline][KMAX];                  // the first clicked costs of the row's cell k, in auction order
    unsigned char aidx[kXDayInline][KMAX];          // the click's auction index within the cell
    unsigned short more[KMAX];                      // cell k's first overflow block
    unsigned char ccnt[KMAX];                       // the cell's clicks; after the walk: its PAID clicks
    XDayBlock pool[2 * KMAX];                       // (kXDayPool at the base width)
    unsigned long long rowmask[KMAX / kWave];       // cells of the row that have a click
    double profit[KMAX];
    int pool_used, stop_k, stopped, binding, give_up;
};

// the clicked impressions of one cell, read in order (inline slots first, then the chain of overflow blocks)
template <int KMAX>
struct XDayCursor {
    const XDayShared<KMAX> &sh;
    int k, c, blk;
    __device__ XDayCursor(const XDayShared<KMAX> &s, int kw) : sh(s), k(kw), c(0), blk(0) {}
    __device__ void next(float &cost, int &aidx)
    {
        if (c < kXDayInline) { cost = sh.cost[c][k]; aidx = sh.aidx[c][k]; }
        else {
            const int slot = (c - kXDayInline) & 3;
            if (slot == 0) blk = c == kXDayInline ? sh.more[k] : sh.pool[blk].next;
            cost = sh.pool[blk].cost[slot];
            aidx = sh.pool[blk].aidx[slot];
        }
        ++c;
    }
};

// MODEL = ADC_MODEL_EXPLICIT, or ADC_MODEL_IMPLICIT_GENERAL (the default ImplicitKeyword: the same day - float64 money, one row of
// click lists, the same walk - with its own auction in step 1 and its own conversion words in step 3; a price can be negative
// there, so `remaining` may grow: the bulk test takes the POSITIVE costs - an upper bound of every prefix - and a cell is skipped
// on its first click only against what is left PLUS what the row's negative prices could still add).
// KMAX = lanes = keywords the workgroup takes: 256 (5 workgroups per CU), 512 or 1024 (one or two per CU: what K > 256 used to
// send to the one-wavefront walkers).
template <int MODEL, int KMAX = kXDayK>
__global__ __launch_bounds__(KMAX, KMAX == kXDayK ? 5 : 4) void k_step_float_day(View v, const float *__restrict__ bids,
                                                              const float *__restrict__ budget_in, int parity)
{
    constexpr bool GENERAL = MODEL == ADC_MODEL_IMPLICIT_GENERAL;
    __shared__ XDayShared<KMAX> sh;
    [[maybe_unused]] __shared__ float s_bidder_cdf[GENERAL ? adc::kBidderTable : 1];      // GENERAL: P(bidders <= b), adc_law.h fill_bidder_cdf
    if ((int)blockIdx.x >= v.flag_count[parity]) return;
    const int env = v.flag_list[blockIdx.x];
    const int K = v.K, k = threadIdx.x, lane = k & 63, wv = k >> 6;
    const bool valid = k < K;
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    const double budget_d = (double)adc::budget_to_cents(budget_in[env]) / 100.0;
    const bool hinted = v.exact_hint[env] != 0;           // k_step_explicit_fast skipped this env: pending drift is applied here
    if (k == 0) { sh.pool_used = 0; sh.stop_k = K; sh.stopped = 0; sh.binding = 0; sh.give_up = budget_d > 0.0 ? 0 : 1; }
    if constexpr (GENERAL) { if (k == 0) { const adc::BidderLaw bl = adc::general_bidder_law(v.max_bidders, v.participation_rate); if (bl.pmf0 > 0.0f) adc::fill_bidder_cdf(s_bidder_cdf, bl); } }

    int V = 0;
    unsigned long long t_imp = 0, t_click = 0, t_conv = 0;
    float bid_d = 0.f, mu = 0.f, sd = 0.f;
    [[maybe_unused]] float g_loc = 0.f, g_scale = 0.f;             // GENERAL: the competitors' bid law
    [[maybe_unused]] double g_bid = 0.0;
    [[maybe_unused]] const int g_top = v.num_winners + 2;
    [[maybe_unused]] const uint64_t g_t_part = adc::bernoulli_threshold(v.participation_rate);
    [[maybe_unused]] const adc::BidderLaw g_bidder_law = adc::general_bidder_law(v.max_bidders, v.participation_rate);
    if (valid) {
        float vol_mean = param_at(v, ADC_P_VOL_MEAN, env, k), bctr = param_at(v, ADC_P_BCTR, env, k), sctr = param_at(v, ADC_P_SCTR, env, k);
        const float vol_std = param_at(v, ADC_P_VOL_STD, env, k);
        if (hinted && v.drift_on && v.drift_pending[env] && drift_keyword(v, env, key, tick - 1u, k, vol_mean, vol_std, bctr, sctr)) {
            param_at(v, ADC_P_VOL_MEAN, env, k) = vol_mean;
            param_at(v, ADC_P_BCTR, env, k) = bctr;
            param_at(v, ADC_P_SCTR, env, k) = sctr;
        }
        V = adc::volume_from_word(adc::volume_word(key, (uint32_t)k, tick), vol_mean, vol_std, g_norm_table);
        bid_d = (float)((double)adc::bid_to_cents(bids[(size_t)env * K + k]) / 100.0);
        if constexpr (GENERAL) {
            g_bid = (double)adc::bid_to_cents(bids[(size_t)env * K + k]) / 100.0;
            g_loc = param_at(v, ADC_P_A, env, k);
            g_scale = param_at(v, ADC_P_B, env, k);
        } else {
            t_imp = adc::bernoulli_threshold(adc::threshold_sigmoid_f32(bid_d, v.imp_thresh, param_at(v, ADC_P_A, env, k), param_at(v, ADC_P_B, env, k)));
        }
        t_click = adc::bernoulli_threshold(bctr);
        t_conv = adc::bernoulli_threshold(sctr);
        mu = param_at(v, ADC_P_REV_MEAN, env, k);
        sd = param_at(v, ADC_P_REV_STD, env, k);
    }
    double obs_cost = 0.0, profit = 0.0;
    long long rev_c = 0;
    int imps_k = 0, paid_k = 0, convs_k = 0;
    double remaining = budget_d;                          // (wave 0's copy is the live one)
    bool binding = false;
    __syncthreads();

    for (int t = 0; t < adc::kTimesteps; ++t) {
        // ---- 1. the row's cells: impressions and clicked costs
        int32_t j0, n;
        adc::cell_range(V, t, j0, n);
        int imps = 0, listed = 0, blk = 0;
        bool pool_full = false;
        auto list_click = [&](float cost, int i) {                    // the clicked cost of auction j0 + i, in auction order
            if (listed < kXDayInline) {
                sh.cost[listed][k] = cost;
                sh.aidx[listed][k] = (unsigned char)i;
            } else if (!pool_full) {
                const int slot = (listed - kXDayInline) & 3;
                if (slot == 0) {
                    const int nb = atomicAdd(&sh.pool_used, 1);
                    if (nb >= 2 * KMAX) pool_full = true;
                    else {
                        if (listed == kXDayInline) sh.more[k] = (unsigned short)nb; else sh.pool[blk].next = (unsigned short)nb;
                        blk = nb;
                    }
                }
                if (!pool_full) { sh.pool[blk].cost[slot] = cost; sh.pool[blk].aidx[slot] = (unsigned char)i; }
            }
            ++listed;
        };
        if constexpr (GENERAL) {
            // the default ImplicitKeyword's auction, as in k_step_general_fast / k_step_exact<IMPLICIT_GENERAL>
            int B = 0;
            if (n > 0 && g_bidder_law.pmf0 > 0.0f) {                      // (engine-uniform) by inversion, adc_law.h bidders_from_word
                const adc::U4 bw = adc::draw(key, (uint32_t)(t >> 2), adc::ST_GBIDDERS, (uint32_t)k, tick);
                B = adc::bidders_from_table((t & 3) == 0 ? bw.x : (t & 3) == 1 ? bw.y : (t & 3) == 2 ? bw.z : bw.w, s_bidder_cdf, g_bidder_law.n);
            } else if (n > 0)
                for (int b0 = 0; b0 < v.max_bidders; b0 += 4) {
                    const adc::U4 w = adc::draw(key, (uint32_t)(64 * t + (b0 >> 2)), adc::ST_GBIDDERS, (uint32_t)k, tick);
                    B += (int)adc::bernoulli(w.x, g_t_part);
                    if (b0 + 1 < v.max_bidders) B += (int)adc::bernoulli(w.y, g_t_part);
                    if (b0 + 2 < v.max_bidders) B += (int)adc::bernoulli(w.z, g_t_part);
                    if (b0 + 3 < v.max_bidders) B += (int)adc::bernoulli(w.w, g_t_part);
                }
            for (int i = 0; i < n && i < 255; ++i) {
                const uint32_t j = (uint32_t)(j0 + i);
                float price;
                if (!adc::clear_general_auction(adc::draw(key, j, adc::ST_GBID, (uint32_t)k, tick), B, g_top - 2, g_loc, g_scale, g_bid, price)) continue;
                ++imps;                                               // a win is an impression
                const adc::U4 w3 = adc::draw(key, j, adc::ST_GCLICK, (uint32_t)k, tick);
                if (!adc::bernoulli(w3.x, t_click)) continue;
                list_click(price, i);                                 // (a float32 bid, or the 0.0 of a missing bidder)
            }
        } else {
            for (int i = 0; i < n && i < 255; ++i) {
                const adc::U4 w = adc::draw(key, (uint32_t)(j0 + i), adc::ST_AUCTION, (uint32_t)k, tick);
                if (!adc::bernoulli(w.x, t_imp)) continue;            // Binomial(n, p) as n Bernoullis (src/lib.rs:70-76)
                ++imps;
                if (!adc::bernoulli(w.z, t_click)) continue;
                list_click(adc::explicit_cost(w.y, bid_d), i);        // cost_create, src/lib.rs:54-67
            }
        }
        sh.ccnt[k] = (unsigned char)listed;                           // (<= 255 auctions looked at)
        {
            const unsigned long long m = __builtin_amdgcn_ballot_w64(listed > 0);
            if (lane == 0) sh.rowmask[wv] = m;
        }
        if (pool_full || n > 255) sh.give_up = 1;                     // (benign race: every writer stores 1)
        __syncthreads();
        if (sh.give_up) break;                                        // (uniform)

        // ---- 2. the budget walk over the row (wave 0)
        if (wv == 0) {
            bool stop = false;
            for (int c64 = 0; c64 < KMAX / kWave && !stop; ++c64) {
                const unsigned long long has_mask = sh.rowmask[c64];
                if (has_mask == 0ull) continue;
                const int kk = c64 * kWave + lane;
                const bool has = (has_mask >> lane) & 1ull;
                const int cnt = sh.ccnt[kk];
                // bulk: every lane adds up its own cell (in click order, as the walk would); if what is left exceeds the chunk's
                // total by a margin no rounding can bridge, every `budget >= cost` of the chunk passes and the campaign's
                // remaining budget just loses the cells' sums in keyword order (:225) - no click-by-click walk
                double my_total = 0.0, my_bound = 0.0;
                [[maybe_unused]] double my_neg = 0.0;                     // GENERAL: what the cell's negative prices could ADD to `remaining`
                if (has) {
                    XDayCursor<KMAX> cur(sh, kk);
                    for (int p = 0; p < cnt; ++p) {
                        float xf; int ai;
                        cur.next(xf, ai);
                        my_total += (double)xf;
                        if (!GENERAL || xf > 0.0f) my_bound += (double)xf;   // (GENERAL: prices can be negative; bound every prefix)
                        if (GENERAL && xf < 0.0f) my_neg -= (double)xf;
                    }
                }
                double chunk_total = my_bound;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) chunk_total += __shfl_xor(chunk_total, o, 64);
                if (remaining - chunk_total > 1.0e-6 * (1.0 + remaining)) {
                    remaining = chain_subtract_wave(remaining, has ? my_total : 0.0);     // (:225, cell by cell in order: common.inc)
                    continue;
                }
                // A cell whose FIRST click costs more than what is left when its turn comes breaks at that click (:99-104) and pays
                // nothing, whatever its later clicks cost.  EXPLICIT: `remaining` only shrinks, so what is left at the start of the
                // 64 bounds it.  GENERAL (round 4): it can grow, but by no more than the negative prices of the 64 cells add up to -
                // none at all on almost every row - so the same test holds against that bound, with a margin no rounding of the
                // walk's subtractions can bridge; round 3 visited every cell with a click (7.9 / 13.6 ms at 4096 x 512 / 2048 x 1024).
                double reach = remaining;
                if constexpr (GENERAL) {
                    double neg = my_neg;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) neg += __shfl_xor(neg, o, 64);
                    reach = (remaining + neg) * (1.0 + 1.0e-9) + 1.0e-9;
                }
                const bool afford = has && reach >= (double)sh.cost[0][kk];
                unsigned long long m = __builtin_amdgcn_ballot_w64(afford);
                if (m != has_mask) binding = true;
                if (has && !afford) sh.ccnt[kk] = 0;                  // breaks at its first click: nothing paid
                double cell_cost = 0.0;
                bool broke = false;
                while (m) {
                    const int l = __ffsll((long long)m) - 1;
                    m &= m - 1ull;
                    if (lane == l) {
                        double b = remaining;
                        int p = 0;
                        XDayCursor<KMAX> cur(sh, kk);
                        for (; p < cnt; ++p) {
                            float xf; int ai;
                            cur.next(xf, ai);
                            const double x = (double)xf;
                            if (!(b >= x)) { broke = true; break; }    // :99-104: the cell's loop breaks at the first unaffordable click
                            b -= x;
                            cell_cost += x;
                        }
                        sh.ccnt[kk] = (unsigned char)p;
                    }
                    remaining -= readlane_f64(cell_cost, l);           // :225
                    if (remaining <= 0.0) {                            // :230-233: later cells are never visited
                        stop = true;
                        if (lane == 0) { sh.stop_k = c64 * kWave + l; sh.stopped = 1; }
                        break;
                    }
                }
                if (__builtin_amdgcn_ballot_w64(broke) != 0ull) binding = true;
            }
        }
        __syncthreads();

        // ---- 3. the cell's paid clicks -> conversions / revenue; phantom click; the keyword's sums in the reference's order
        const bool stopped = sh.stopped != 0;
        if (k == 0) sh.pool_used = 0;                                 // (nobody allocates before the barrier that ends the row)
        if (valid && !(stopped && k > sh.stop_k)) {
            const int paid = sh.ccnt[k];
            double cell_cost = 0.0;
            long long cell_rev_c = 0;
            XDayCursor<KMAX> cur(sh, k);
            for (int c = 0; c < paid; ++c) {
                float xf; int ai;
                cur.next(xf, ai);
                const double x = (double)xf;
                cell_cost += x;
                obs_cost += x;                                         // sum_list(costs), left to right
                const uint32_t j = (uint32_t)(j0 + ai);
                if constexpr (GENERAL) {
                    const adc::U4 w3 = adc::draw(key, j, adc::ST_GCLICK, (uint32_t)k, tick);
                    if (adc::bernoulli(w3.y, t_conv)) {
                        ++convs_k;
                        cell_rev_c += adc::revenue_cents_tab(w3.z, mu, sd, g_norm_table);
                    }
                } else {
                    const adc::U4 w = adc::draw(key, j, adc::ST_AUCTION, (uint32_t)k, tick);
                    if (adc::bernoulli(w.w, t_conv)) {
                        ++convs_k;
                        const adc::U4 w2 = adc::draw(key, j, adc::ST_XREV, (uint32_t)k, tick);
                        cell_rev_c += adc::revenue_cents(w2.x, mu, sd);
                    }
                }
            }
            paid_k += paid;
            if (!GENERAL && imps == 0) {
                // phantom zero-cost click opportunity (synthetic_kw_classes.py:514-515); the campaign is running here
                const adc::U4 w = adc::draw(key, (uint32_t)t, adc::ST_XPHANTOM, (uint32_t)k, tick);
                if (adc::bernoulli(w.x, t_click)) {
                    ++paid_k;
                    if (adc::bernoulli(w.y, t_conv)) {
                        ++convs_k;
                        cell_rev_c += adc::revenue_cents(w.z, mu, sd);
                    }
                }
            }
            imps_k += imps;
            rev_c += cell_rev_c;
            profit += (double)cell_rev_c / 100.0 - cell_cost;         // combine_outcomes: profit += profit
        }
        if (stopped) break;                                           // (uniform)
        __syncthreads();                                              // the row's lists are free again
    }
    if (sh.give_up) {
        if (k == 0) { v.retry_list[atomicAdd(&v.retry_count[parity], 1)] = env; v.exact_hint[env] = 0; }
#ifdef ADC_EXP_TIMING
        if (k == 0) atomicAdd(&g_dbg[0], 1ull);
        if (!(budget_d > 0.0) && k == 0) atomicAdd(&g_dbg[1], 1ull);
        { int32_t j0, n; adc::cell_range(V, 0, j0, n); if (n > 255) atomicAdd(&g_dbg[2], 1ull); }
#endif
        return;
    }
#ifdef ADC_EXP_TIMING
    if (k == 0) atomicAdd(&g_dbg[3], 1ull);
#endif
    if (wv == 0 && lane == 0) sh.binding = (binding || sh.stopped) ? 1 : 0;
    if (valid) {
        const size_t o = (size_t)env * K + k;
        v.imp[o] = imps_k;
        v.clk[o] = paid_k;
        v.conv[o] = convs_k;
        v.cost[o] = (float)obs_cost;
        v.rev[o] = (float)rev_c / 100.0f;
        sh.profit[k] = profit;
    }
    __syncthreads();
    if (k == 0) {
        double reward = 0.0;                       // rust.sum_list(profits): left to right (gymnasium_kw_env.py:222)
        for (int i = 0; i < K; ++i) reward += sh.profit[i];
        v.exact_hint[env] = (uint8_t)sh.binding;
        step_tail(v, env, tick, false, 0, reward);
    }
}

// -------------------------------------------------------------------------------------------------
// k_step_explicit_rows: reference-order budget walk for the EXPLICIT envs k_step_explicit_fast flagged.
// One wavefront per flagged env.  The day's cells are visited in the reference's order (sub-timestep major, keyword
// minor, bidding_simulation.py:214-233) 64 cells of a row at a time, each in three phases:
//   1. lane = cell: the cell's auctions are resolved (impression, click, cost) and the clicked costs are listed in LDS;
//   2. the budget walk proper, cell by cell in keyword order: the cell's own lane pays its clicks while
//      `budget >= cost` (:97-104) starting from the campaign's remaining budget, which then loses the cell's cost
//      (:225) and stops the campaign at <= 0 (:230-233) - all in float64, in the reference's operation order.  Cells
//      without a clicked impression cannot change the remaining budget and are skipped;
//   3. lane = cell again: conversions / revenues of the paid clicks, the phantom click of impression-less cells, and
//      the per-keyword float64 accumulators (a keyword is always handled by the same lane position, in row order).
// The click lists share kXPool LDS slots: a row whose largest cell has at most 16 / 64 / 256 auctions is processed
// 64 / 16 / 4 cells at a time, so a list can never overflow.  A row with a larger cell, and a day that starts with a
// budget <= 0, are left to the serial walker (k_step_exact<EXPLICIT>), via the xover list.
constexpr int kXPool = 1024;
constexpr int kXMaxClicks = kXPool / kWave;      // (list slots per cell at full width; sizes the LDS allocation)

__global__ __launch_bounds__(kWave) void k_step_explicit_rows(View v, const float *__restrict__ bids,
                                                              const float *__restrict__ budget_in, int parity,
                                                              const int *__restrict__ list, const int *__restrict__ list_count)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    if ((int)blockIdx.x >= list_count[parity]) return;
    const int env = list[blockIdx.x];
    const int K = v.K, lane = threadIdx.x;
    double *s_cost = reinterpret_cast<double *>(lds_raw);                        // [K] observed cost, float64
    double *s_profit = s_cost + K;                                               // [K]
    long long *s_rev = reinterpret_cast<long long *>(s_profit + K);              // [K] cents
    unsigned long long *s_timp = reinterpret_cast<unsigned long long *>(s_rev + K);      // [K] impression threshold
    double *s_list = reinterpret_cast<double *>(s_timp + K);                     // [width][cap] clicked costs of the chunk, width * cap = kXPool
    int *s_vol = reinterpret_cast<int *>(s_list + kXPool);                       // [K]
    int *s_imp = s_vol + K, *s_clk = s_imp + K, *s_conv = s_clk + K;             // [K] each
    unsigned char *s_idx = reinterpret_cast<unsigned char *>(s_conv + K);        // [width][cap] auction index within the cell

    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    const double budget_d = (double)adc::budget_to_cents(budget_in[env]) / 100.0;
    bool give_up = !(budget_d > 0.0);           // the first cell is then visited with nothing to spend: serial walker

    for (int k = lane; k < K && !give_up; k += kWave) {
        s_vol[k] = adc::volume_from_word(adc::volume_word(key, (uint32_t)k, tick), param_at(v, ADC_P_VOL_MEAN, env, k),
                                         param_at(v, ADC_P_VOL_STD, env, k), g_norm_table);
        const float bid_d = (float)((double)adc::bid_to_cents(bids[(size_t)env * K + k]) / 100.0);
        s_timp[k] = adc::bernoulli_threshold(adc::threshold_sigmoid_f32(bid_d, v.imp_thresh, param_at(v, ADC_P_A, env, k),
                                                                        param_at(v, ADC_P_B, env, k)));
        s_cost[k] = 0.0; s_profit[k] = 0.0; s_rev[k] = 0;
        s_imp[k] = s_clk[k] = s_conv[k] = 0;
    }
    __syncthreads();

    double remaining = budget_d;
    bool stop = false;
    for (int t = 0; t < adc::kTimesteps && !stop && !give_up; ++t) {
        // chunk width of this row from its largest cell
        int nmax = 0;
        for (int k = lane; k < K; k += kWave) {
            int32_t j0, n;
            adc::cell_range(s_vol[k], t, j0, n);
            nmax = max(nmax, n);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
        if (nmax > 256) { give_up = true; break; }
        const int width = nmax <= 16 ? 64 : nmax <= 64 ? 16 : 4;
        const int cap = kXPool / width;
        for (int kb = 0; kb < K && !stop && !give_up; kb += width) {
            const int k = kb + lane;
            const bool cell = lane < width && k < K;
            // ---- phase 1: resolve the cell's auctions
            int32_t j0 = 0, n = 0;
            unsigned long long t_imp = 0, t_click = 0, t_conv = 0;
            float bid_d = 0.f, mu = 0.f, sd = 0.f;
            int imps = 0, cnt = 0;
            if (cell) {
                adc::cell_range(s_vol[k], t, j0, n);
                t_imp = s_timp[k];
                t_click = adc::bernoulli_threshold(param_at(v, ADC_P_BCTR, env, k));
                t_conv = adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, k));
                mu = param_at(v, ADC_P_REV_MEAN, env, k);
                sd = param_at(v, ADC_P_REV_STD, env, k);
                bid_d = (float)((double)adc::bid_to_cents(bids[(size_t)env * K + k]) / 100.0);
                for (int i = 0; i < n; ++i) {
                    const adc::U4 w = adc::draw(key, (uint32_t)(j0 + i), adc::ST_AUCTION, (uint32_t)k, tick);
                    if (!adc::bernoulli(w.x, t_imp)) continue;
                    ++imps;
                    if (!adc::bernoulli(w.z, t_click)) continue;
                    s_list[lane * cap + cnt] = (double)adc::explicit_cost(w.y, bid_d);      // cnt < n <= cap
                    s_idx[lane * cap + cnt] = (unsigned char)i;
                    ++cnt;
                }
            }
            // ---- phase 2: the budget walk, cell by cell in keyword order (only cells that can spend)
            double cell_cost = 0.0;
            int paid = 0;
            int last_visited = width - 1;
            // (a cell whose first click already costs more than what is left breaks at once, :99-104, and `remaining` only
            // shrinks along the chunk: such cells pay nothing whatever happens before them - no need to visit them in order)
            unsigned long long m = __builtin_amdgcn_ballot_w64(cnt > 0 && remaining >= s_list[lane * cap]);
            while (m) {
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1ull;
                if (lane == l) {
                    double b = remaining, obs = s_cost[k];
                    for (int c = 0; c < cnt; ++c) {
                        const double x = s_list[lane * cap + c];
                        if (!(b >= x)) break;                               // :99-104: the cell's loop breaks at the first unaffordable click
                        b -= x;
                        cell_cost += x;
                        obs += x;                                           // sum_list(costs), left to right
                        ++paid;
                    }
                    s_cost[k] = obs;
                }
                remaining -= readlane_f64(cell_cost, l);                    // :225
                if (remaining <= 0.0) { stop = true; last_visited = l; break; }        // :230-233
            }
            // ---- phase 3: paid clicks -> conversions / revenue; phantom click; accumulators
            if (cell && lane <= last_visited) {
                long long cell_rev_c = 0;
                int convs = 0;
                for (int c = 0; c < paid; ++c) {
                    const uint32_t j = (uint32_t)(j0 + s_idx[lane * cap + c]);
                    const adc::U4 w = adc::draw(key, j, adc::ST_AUCTION, (uint32_t)k, tick);
                    if (adc::bernoulli(w.w, t_conv)) {
                        ++convs;
                        const adc::U4 w2 = adc::draw(key, j, adc::ST_XREV, (uint32_t)k, tick);
                        cell_rev_c += adc::revenue_cents(w2.x, mu, sd);
                    }
                }
                if (imps == 0) {
                    // phantom zero-cost click opportunity (synthetic_kw_classes.py:514-515); the campaign is running, so the
                    // budget it is checked against is > 0
                    const adc::U4 w = adc::draw(key, (uint32_t)t, adc::ST_XPHANTOM, (uint32_t)k, tick);
                    if (adc::bernoulli(w.x, t_click)) {
                        ++paid;
                        if (adc::bernoulli(w.y, t_conv)) {
                            ++convs;
                            cell_rev_c += adc::revenue_cents(w.z, mu, sd);
                        }
                    }
                }
                s_imp[k] += imps;
                s_clk[k] += paid;
                s_conv[k] += convs;
                s_rev[k] += cell_rev_c;
                s_profit[k] += (double)cell_rev_c / 100.0 - cell_cost;      // combine_outcomes: profit += profit
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    if (give_up) {
        if (lane == 0) v.xover_list[atomicAdd(&v.xover_count[parity], 1)] = env;
        return;
    }
    for (int k = lane; k < K; k += kWave) {
        const size_t o = (size_t)env * K + k;
        v.imp[o] = s_imp[k];
        v.clk[o] = s_clk[k];
        v.conv[o] = s_conv[k];
        v.cost[o] = (float)s_cost[k];
        v.rev[o] = (float)s_rev[k] / 100.0f;
    }
    if (lane == 0) {
        double reward = 0.0;                       // rust.sum_list(profits): left to right (gymnasium_kw_env.py:222)
        for (int k = 0; k < K; ++k) reward += s_profit[k];
        step_tail(v, env, tick, false, 0, reward);
    }
}
