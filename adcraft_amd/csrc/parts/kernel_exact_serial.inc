// kernel_exact_serial.inc - step tail + k_step_exact: serial reference-order walker (TAPE replay, EXPLICIT hand-overs, K > 2048)
// (part of the single translation unit adc_engine.hip; see that file for the overview)
// -------------------------------------------------------------------------------------------------
// EXACT PASS + STEP TAIL: one wavefront per env
// -------------------------------------------------------------------------------------------------
struct TapeView {
    const int32_t *volumes, *bid_cents, *x_impressions;
    const double *x_cost;
    const uint8_t *click, *conv;
    const int32_t *rev_cents;
    const int64_t *off_bid, *off_ximp, *off_xcost, *off_click, *off_conv, *off_rev;
    int64_t *end_bid, *end_ximp, *end_xcost, *end_click, *end_conv, *end_rev;
    int64_t len_bid, len_ximp, len_xcost, len_click, len_conv, len_rev;
    int *error;      // set to 1 by any read past the end of a tape (the read then yields 0)
    const float *drift_uniforms;     // [3][N][K] or null: update_keywords() coefficients applied at the end of the step
};

// bounds-checked tape read: a malformed tape must never become an out-of-bounds device access
template <typename T>
__device__ __forceinline__ T tape_at(const T *tape, int64_t index, int64_t len, int *error)
{
    if (index >= 0 && index < len) return tape[index];
    *error = 1;
    return T(0);
}

// Read-only REPLAY of one env-step (adc_engine_outcomes_replay / _tape): with `records` non-null the kernel walks env `env` once more
// with the stream position that step had (tick - ticks_back; or over the caller's tape) and the keyword parameters as they stand (the last step's own:
// its pending drift is applied by the NEXT step; an earlier step's only while nothing has changed them since - the caller's
// responsibility), writes nothing of the engine's state, and lists every paid click in the
// reference's order - what src/lib.rs:251-275 formats as 'costs' / 'revenues' / 'revenues_per_cost' of info["bidding_outcomes"].
struct ReplayOut {
    int4 *records;            // per paid click: {keyword, sub-timestep, revenue in cents or -1 (no conversion), 0}
    double *costs;            // its cost in dollars (IMPLICIT: cents / 100; the other models: the float64 cost itself)
    int *count;               // paid clicks of the step (records beyond `capacity` are counted, not stored)
    int *share_volume;        // [K] sum of the auctions of the cells that had an impression (combine_outcomes' impression_share denominator)
    const float *bids_env;    // [K] the step's bids for this env
    float budget;
    int capacity, env;
    unsigned int ticks_back;  // how many steps ago the replayed step was (1 = the last one)
};

// dynamic LDS layout (K entries each): cost i64|f64, rev i64, profit f64, vol i32, imp i32, clk i32, conv i32

template <int MODEL, bool TAPE>
__global__ __launch_bounds__(kWave) void k_step_exact(View v, const float *__restrict__ bids,
                                                       const float *__restrict__ budget_in, TapeView tp, int fast_ran, ReplayOut rp)
{
    const bool replay = rp.records != nullptr;          // (TAPE: adc_engine_outcomes_replay_tape)
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int K = v.K;
    long long *s_cost_i = reinterpret_cast<long long *>(lds_raw);                 // [K]
    double *s_cost_d = reinterpret_cast<double *>(lds_raw);                       // [K] (EXPLICIT view)
    long long *s_rev = s_cost_i + K;                                              // [K]
    double *s_profit = reinterpret_cast<double *>(s_rev + K);                     // [K]
    int *s_vol = reinterpret_cast<int *>(s_profit + K);                           // [K]
    int *s_imp = s_vol + K, *s_clk = s_imp + K, *s_conv = s_clk + K;

    // fast_ran: 0 = every env (TAPE replay, K beyond the row kernel); IMPLICIT 1 = re-run only envs whose fast-pass
    // spend reached the budget; EXPLICIT 1 + parity = only the envs k_step_explicit_rows handed over (xover list), 3 + parity = the envs
    // k_step_explicit_fast flagged (K too large for the row walker's LDS)
    int env = replay ? rp.env : (int)blockIdx.x;
    if (MODEL != ADC_MODEL_IMPLICIT && !TAPE && fast_ran) {
        const int par = (fast_ran - 1) & 1;
        // 1 + parity: handed over by k_step_explicit_rows (xover list); 3 + parity: straight from the fast pass (flag list);
        // 5 + parity: left by k_step_float_day (retry list)
        const int *const list = fast_ran <= 2 ? v.xover_list : fast_ran <= 4 ? v.flag_list : v.retry_list;
        const int count = fast_ran <= 2 ? v.xover_count[par] : fast_ran <= 4 ? v.flag_count[par] : v.retry_count[par];
        if ((int)blockIdx.x >= count) return;
        env = list[blockIdx.x];
    }
    const int lane = threadIdx.x;
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env] - (replay ? rp.ticks_back : 0u);
    const long long budget_c = adc::budget_to_cents(replay ? rp.budget : budget_in[env]);
    if (replay) bids = rp.bids_env - (size_t)env * K;           // (only ever indexed as bids[env K + k])
    int rec_base = 0;                                           // replay: paid clicks listed so far (wave-uniform)
    auto record = [&](bool is_paid, unsigned long long paid_mask, int k, int t, double cost_dollars, bool convd, long long rev_cents) {
        if (is_paid) {
            const int idx = rec_base + (int)__popcll(paid_mask & lanemask_lt());
            if (idx < rp.capacity) {
                rp.records[idx] = make_int4(k, t, convd ? (int)rev_cents : -1, 0);
                rp.costs[idx] = cost_dollars;
            }
        }
        rec_base += (int)__popcll(paid_mask);
    };

    bool rerun = true;
    if (MODEL == ADC_MODEL_IMPLICIT && !TAPE && fast_ran) rerun = !(v.env_cost[env] < budget_c);

    double reward_d = 0.0;
    long long profit_c = 0;

    if (rerun) {
        // without a fast pass before it, pending drift is applied here
        // (IMPLICIT_GENERAL: k_step_general_fast skips an env whose budget bound yesterday - v.exact_hint - and leaves its drift to us)
        const bool fast_skipped = MODEL == ADC_MODEL_IMPLICIT_GENERAL && !TAPE && fast_ran && v.exact_hint[env] != 0;
        if (MODEL != ADC_MODEL_IMPLICIT && !TAPE && !replay && (!fast_ran || fast_skipped) && v.drift_on && v.drift_pending[env]) {
            for (int k = lane; k < K; k += kWave) {
                drift_keyword_planes(v, env, key, tick - 1u, k);
            }
        }
        for (int k = lane; k < K; k += kWave) {
            int V;
            if (TAPE) V = tp.volumes[(size_t)env * K + k];
            else {
                V = adc::volume_from_word(adc::volume_word(key, (uint32_t)k, tick), param_at(v, ADC_P_VOL_MEAN, env, k),
                                          param_at(v, ADC_P_VOL_STD, env, k), g_norm_table);
            }
            s_vol[k] = V;
            s_imp[k] = s_clk[k] = s_conv[k] = 0;
            s_cost_i[k] = 0;   // also zeroes the double view
            s_rev[k] = 0;
            s_profit[k] = 0.0;
        }
        __syncthreads();

        double remaining_d = (double)budget_c / 100.0;          // np.round(budget, 2)
        int64_t cur_bid = 0, cur_ximp = 0, cur_xcost = 0, cur_click = 0, cur_conv = 0, cur_rev = 0;
        if (TAPE) {
            cur_bid = tp.off_bid ? tp.off_bid[env] : 0;
            cur_ximp = tp.off_ximp ? tp.off_ximp[env] : 0;
            cur_xcost = tp.off_xcost ? tp.off_xcost[env] : 0;
            cur_click = tp.off_click ? tp.off_click[env] : 0;
            cur_conv = tp.off_conv ? tp.off_conv[env] : 0;
            cur_rev = tp.off_rev ? tp.off_rev[env] : 0;
        }
        bool stop = false;
        bool budget_bound = false;                  // (IMPLICIT_GENERAL) a click was refused: tomorrow's fast pass would be wasted
        const unsigned long long lt = lanemask_lt();

        for (int t = 0; t < adc::kTimesteps && !stop; ++t) {
            for (int k = 0; k < K && !stop; ++k) {
                int32_t j0, n;
                adc::cell_range(s_vol[k], t, j0, n);
                const long long bid_c = adc::bid_to_cents(bids[(size_t)env * K + k]);
                const uint64_t t_click = adc::bernoulli_threshold(param_at(v, ADC_P_BCTR, env, k));
                const uint64_t t_conv = adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, k));
                const float mu = param_at(v, ADC_P_REV_MEAN, env, k), sd = param_at(v, ADC_P_REV_STD, env, k);

                if (MODEL == ADC_MODEL_IMPLICIT) {
                    const float loc = param_at(v, ADC_P_A, env, k), scale = param_at(v, ADC_P_B, env, k);
                    const adc::AuctionLaw law = adc::make_auction_law(param_at(v, ADC_P_BCTR, env, k));
                    int wins = 0, paid = 0, convs = 0;
                    long long cell_cost = 0, cell_rev = 0;
                    // money totals are exact cents; the budget walk runs in the reference's binary floating point
                    // (cost = cents/100 as np.around(x, 2) gives it, `budget -= cost` per paid click, the campaign's
                    // remaining loses the left-to-right sum of the cell's paid costs): an exact tie remaining == cost
                    // is decided by the float residue there, and whether the campaign then stops changes the
                    // impressions of every later cell.
                    double budget = remaining_d, cell_sum_d = 0.0;
                    bool broke = false;
                    for (int base = 0; base < n; base += kWave) {
                        const int i = base + lane;
                        const bool act = i < n;
                        bool click_bit = false;
                        long long comp = 0;
                        uint32_t word = 0u;
                        const uint32_t j = (uint32_t)(j0 + i);
                        if (act) {
                            if (TAPE) comp = tape_at(tp.bid_cents, cur_bid + i, tp.len_bid, tp.error);
                            else {
                                const adc::U4 w = adc::draw(key, j >> 2, adc::ST_AUCTION, (uint32_t)k, tick);
                                word = (j & 3u) == 0 ? w.x : (j & 3u) == 1 ? w.y : (j & 3u) == 2 ? w.z : w.w;
                                comp = adc::auction_outcome(word, law, loc, scale, g_log_table, click_bit);
                            }
                        }
                        const bool win = act && (TAPE ? bid_c > comp : adc::auction_wins(word, (int32_t)bid_c, (int32_t)comp));
                        const unsigned long long win_mask = __ballot(win);
                        bool clicked = false;
                        if (win) {
                            if (TAPE) clicked = tape_at(tp.click, cur_click + wins + __popcll(win_mask & lt), tp.len_click, tp.error) != 0;
                            else clicked = click_bit;
                        }
                        // budget walk (bidding_simulation.py:97-104), click by click in auction order
                        unsigned long long cand = __ballot(clicked);
                        unsigned long long paid_mask = 0ull;
                        while (cand && !broke) {
                            const int l = __ffsll((long long)cand) - 1;
                            cand &= cand - 1ull;
                            const double cost_d = adc::cents_to_dollars_f64(__shfl(comp, l, 64));
                            if (budget >= cost_d) { budget -= cost_d; cell_sum_d += cost_d; paid_mask |= 1ull << l; }
                            else broke = true;
                        }
                        const bool is_paid = (paid_mask >> lane) & 1ull;
                        bool convd = false;
                        long long rv = 0;
                        if (is_paid) {
                            if (TAPE) convd = tape_at(tp.conv, cur_conv + paid + __popcll(paid_mask & lt), tp.len_conv, tp.error) != 0;
                            else {
                                const adc::U4 w2 = adc::draw(key, j, adc::ST_CONV, (uint32_t)k, tick);
                                convd = adc::bernoulli(w2.x, t_conv);
                                if (convd) rv = adc::revenue_cents_tab(w2.y, mu, sd, g_norm_table);
                            }
                        }
                        const unsigned long long conv_mask = __ballot(convd);
                        if (TAPE && convd) rv = tape_at(tp.rev_cents, cur_rev + convs + __popcll(conv_mask & lt), tp.len_rev, tp.error);
                        if (replay) record(is_paid, paid_mask, k, t, adc::cents_to_dollars_f64((int)comp), convd, rv);
                        cell_cost += wave_sum_i64(is_paid ? comp : 0);
                        cell_rev += wave_sum_i64(rv);
                        wins += __popcll(win_mask);
                        paid += __popcll(paid_mask);
                        convs += __popcll(conv_mask);
                    }
                    if (TAPE) { cur_bid += n; cur_click += wins; cur_conv += paid; cur_rev += convs; }
                    if (replay && lane == 0 && wins > 0) rp.share_volume[k] += n;
                    if (lane == 0) {
                        s_imp[k] += wins;          // impressions are not budget-limited (:86-88)
                        s_clk[k] += paid;
                        s_conv[k] += convs;
                        s_cost_i[k] += cell_cost;
                        s_rev[k] += cell_rev;
                    }
                    remaining_d -= cell_sum_d;     // :225 (rust.sum_list(costs): left to right)
                    if (remaining_d <= 0.0) stop = true; // :230-233
                } else if (MODEL == ADC_MODEL_IMPLICIT_GENERAL) {
                    // the reference's default ImplicitKeyword (synthetic_kw_classes.py:610-686): B bidders for the whole call, raw
                    // Laplace bids, nth_price_auction(bid, other_bids, n = 2, num_winners) (synthetic_kw_helpers.py:116-180):
                    // the top (w + 2) competitor bids of an auction in ascending order (zero bids stand in for missing bidders),
                    // index = how many of them are below our bid, won iff index > 2, price = the one just below.  Lane = auction;
                    // the top four bids live in registers (w <= 2), kept sorted by a 3-step insertion network.  Money is float64.
                    const float loc = param_at(v, ADC_P_A, env, k), scale = param_at(v, ADC_P_B, env, k);
                    const double bid_d = (double)bid_c / 100.0;
                    const int top = v.num_winners + 2;
                    double budget = remaining_d, cell_cost = 0.0, obs_cost = s_cost_d[k];
                    long long cell_rev_c = 0;
                    int imps = 0, paid = 0, convs = 0;
                    bool broke = false;
                    int B = 0;
                    if (TAPE) {
                        B = tape_at(tp.x_impressions, cur_ximp, tp.len_ximp, tp.error);
                        if (B < 0 || B > 252 || (int64_t)B * n > tp.len_xcost) { *tp.error = 1; B = 0; }
                    } else {
                        const uint64_t t_part = adc::bernoulli_threshold(v.participation_rate);
                        const adc::BidderLaw bidder_law = adc::general_bidder_law(v.max_bidders, v.participation_rate);
                        if (bidder_law.pmf0 > 0.0f) {        // (engine-uniform) by inversion, adc_law.h bidders_from_word
                            const adc::U4 bw = adc::draw(key, (uint32_t)(t >> 2), adc::ST_GBIDDERS, (uint32_t)k, tick);
                            B = adc::bidders_from_word((t & 3) == 0 ? bw.x : (t & 3) == 1 ? bw.y : (t & 3) == 2 ? bw.z : bw.w, bidder_law);
                        } else
                        for (int b0 = 0; b0 < v.max_bidders; b0 += kWave) {
                            const int b = b0 + lane;
                            bool in = false;
                            if (b < v.max_bidders) {
                                const adc::U4 w = adc::draw(key, (uint32_t)(64 * t + (b >> 2)), adc::ST_GBIDDERS, (uint32_t)k, tick);
                                in = adc::bernoulli((b & 3) == 0 ? w.x : (b & 3) == 1 ? w.y : (b & 3) == 2 ? w.z : w.w, t_part);
                            }
                            B += (int)__popcll(__ballot(in));
                        }
                    }
                    const double kNone = -1.0e300;       // below any bid: an empty slot of the top four
                    for (int base = 0; base < n; base += kWave) {
                        const int i = base + lane;
                        const bool act = i < n;
                        const uint32_t j = (uint32_t)(j0 + i);
                        double a0 = kNone, a1 = kNone, a2 = kNone, a3 = kNone;          // ascending: a3 the highest so far
                        auto insert = [&](double x) {
                            if (x > a0) {
                                a0 = x;
                                if (a0 > a1) { const double s2 = a0; a0 = a1; a1 = s2; }
                                if (a1 > a2) { const double s2 = a1; a1 = a2; a2 = s2; }
                                if (a2 > a3) { const double s2 = a2; a2 = a3; a3 = s2; }
                            }
                        };
                        for (int z = B; z < top; ++z) insert(0.0);                       // :156-161 zero bids for missing bidders
                        if (TAPE) {                                      // every recorded bid of the call (rng.laplace(loc, scale), :681-686)
                            for (int b = 0; b < B; ++b) insert(act ? tape_at(tp.x_cost, cur_xcost + (int64_t)b * n + i, tp.len_xcost, tp.error) : 0.0);
                        } else if (B > 0 && act) {                       // the engine's stream: the top bids as order statistics (adc_law.h)
                            float xs[4];
                            const int nb = adc::top_laplace_bids(adc::draw(key, j, adc::ST_GBID, (uint32_t)k, tick), B, top, loc, scale, xs);
                            for (int h = 0; h < nb; ++h) insert((double)xs[h]);
                        }
                        // the top (w + 2) in ascending order: t0 <= t1 <= t2 (<= t3)
                        const double t0 = top == 4 ? a0 : a1, t1 = top == 4 ? a1 : a2, t2 = top == 4 ? a2 : a3, t3 = a3;
                        int index = (t0 < bid_d) + (t1 < bid_d) + (t2 < bid_d) + (top == 4 ? (t3 < bid_d) : 0);      // :167 searchsorted left
                        const bool win = act && index > 2;                                                           // :170
                        const double cost = index == 4 ? t3 : t2;                                                    // sorted[index - 1], :173-175
                        const unsigned long long win_mask = __ballot(win);
                        adc::U4 w3{0u, 0u, 0u, 0u};
                        bool clicked = false;
                        if (win) {
                            if (TAPE) clicked = tape_at(tp.click, cur_click + imps + __popcll(win_mask & lt), tp.len_click, tp.error) != 0;
                            else {
                                w3 = adc::draw(key, j, adc::ST_GCLICK, (uint32_t)k, tick);
                                clicked = adc::bernoulli(w3.x, t_click);
                            }
                        }
                        imps += __popcll(win_mask);
                        unsigned long long cand = __ballot(clicked);
                        unsigned long long paid_mask = 0ull;
                        while (cand && !broke) {                 // the click-by-click walk in f64 (:97-104): same order, same ops
                            const int l = __ffsll((long long)cand) - 1;
                            cand &= cand - 1ull;
                            const double c = __shfl(cost, l, 64);
                            if (budget >= c) { budget -= c; cell_cost += c; obs_cost += c; paid_mask |= 1ull << l; }
                            else broke = true;
                        }
                        const bool is_paid = (paid_mask >> lane) & 1ull;
                        bool convd = false;
                        if (is_paid) {
                            if (TAPE) convd = tape_at(tp.conv, cur_conv + paid + __popcll(paid_mask & lt), tp.len_conv, tp.error) != 0;
                            else convd = adc::bernoulli(w3.y, t_conv);
                        }
                        const unsigned long long conv_mask = __ballot(convd);
                        long long rv = 0;
                        if (convd) {
                            if (TAPE) rv = tape_at(tp.rev_cents, cur_rev + convs + __popcll(conv_mask & lt), tp.len_rev, tp.error);
                            else rv = adc::revenue_cents_tab(w3.z, mu, sd, g_norm_table);
                        }
                        if (replay) record(is_paid, paid_mask, k, t, cost, convd, rv);
                        cell_rev_c += wave_sum_i64(rv);
                        paid += __popcll(paid_mask);
                        convs += __popcll(conv_mask);
                    }
                    if (TAPE) { cur_ximp += 1; cur_xcost += (int64_t)B * n; cur_click += imps; cur_conv += paid; cur_rev += convs; }
                    budget_bound = budget_bound || broke;
                    if (replay && lane == 0 && imps > 0) rp.share_volume[k] += n;
                    if (lane == 0) {
                        s_imp[k] += imps;
                        s_clk[k] += paid;
                        s_conv[k] += convs;
                        s_cost_d[k] = obs_cost;
                        s_rev[k] += cell_rev_c;
                        s_profit[k] += (double)cell_rev_c / 100.0 - cell_cost;
                    }
                    remaining_d -= cell_cost;
                    if (remaining_d <= 0.0) stop = true;
                } else {
                    // EXPLICIT cell
                    const float bid_d = (float)((double)bid_c / 100.0);
                    const float p_imp = adc::threshold_sigmoid_f32(bid_d, v.imp_thresh, param_at(v, ADC_P_A, env, k),
                                                                   param_at(v, ADC_P_B, env, k));
                    const uint64_t t_imp = adc::bernoulli_threshold(p_imp);
                    double budget = remaining_d, cell_cost = 0.0;
                    double obs_cost = s_cost_d[k];           // obs cost = sum_list(costs): left to right
                    long long cell_rev_c = 0;
                    int imps = 0, paid = 0, convs = 0;
                    bool broke = false;
                    int entries = n;
                    if (TAPE) {
                        entries = tape_at(tp.x_impressions, cur_ximp, tp.len_ximp, tp.error);
                        if (entries < 0 || (int64_t)entries > tp.len_xcost) { *tp.error = 1; entries = 0; }
                    }
                    for (int base = 0; base < entries; base += kWave) {
                        const int i = base + lane;
                        const bool act = i < entries;
                        adc::U4 w{0u, 0u, 0u, 0u};
                        bool is_imp = false, clicked = false;
                        double cost = 0.0;
                        if (act) {
                            if (TAPE) {
                                is_imp = true;
                                cost = tape_at(tp.x_cost, cur_xcost + i, tp.len_xcost, tp.error);
                                clicked = tape_at(tp.click, cur_click + i, tp.len_click, tp.error) != 0;
                            } else {
                                w = adc::draw(key, (uint32_t)(j0 + i), adc::ST_AUCTION, (uint32_t)k, tick);
                                is_imp = adc::bernoulli(w.x, t_imp);          // Binomial(n,p) as n Bernoullis
                                cost = (double)adc::explicit_cost(w.y, bid_d);
                                clicked = is_imp && adc::bernoulli(w.z, t_click);
                            }
                        }
                        imps += __popcll(__ballot(is_imp));
                        // the reference walks the clicks one by one in f64 (:97-104): same order, same ops
                        unsigned long long cand = __ballot(clicked);
                        unsigned long long paid_mask = 0ull;
                        while (cand && !broke) {
                            const int l = __ffsll((long long)cand) - 1;
                            cand &= cand - 1ull;
                            const double c = __shfl(cost, l, 64);
                            if (budget >= c) { budget -= c; cell_cost += c; obs_cost += c; paid_mask |= 1ull << l; }
                            else broke = true;
                        }
                        const bool is_paid = (paid_mask >> lane) & 1ull;
                        bool convd = false;
                        if (is_paid) {
                            if (TAPE) convd = tape_at(tp.conv, cur_conv + paid + __popcll(paid_mask & lt), tp.len_conv, tp.error) != 0;
                            else convd = adc::bernoulli(w.w, t_conv);
                        }
                        const unsigned long long conv_mask = __ballot(convd);
                        long long rv = 0;
                        if (convd) {
                            if (TAPE) rv = tape_at(tp.rev_cents, cur_rev + convs + __popcll(conv_mask & lt), tp.len_rev, tp.error);
                            else {
                                const adc::U4 w2 = adc::draw(key, (uint32_t)(j0 + i), adc::ST_XREV, (uint32_t)k, tick);
                                rv = adc::revenue_cents(w2.x, mu, sd);
                            }
                        }
                        if (replay) record(is_paid, paid_mask, k, t, cost, convd, rv);
                        cell_rev_c += wave_sum_i64(rv);
                        paid += __popcll(paid_mask);
                        convs += __popcll(conv_mask);
                    }
                    if (TAPE) {
                        cur_ximp += 1;
                        cur_xcost += entries;
                        cur_click += entries;
                        cur_conv += paid;
                        cur_rev += convs;
                    }
                    if (imps == 0) {
                        // phantom zero-cost click opportunity (synthetic_kw_classes.py:514-515), once per cell
                        bool clicked, convd = false;
                        long long rv = 0;
                        adc::U4 w{0u, 0u, 0u, 0u};
                        if (TAPE) clicked = tape_at(tp.click, cur_click++, tp.len_click, tp.error) != 0;
                        else {
                            w = adc::draw(key, (uint32_t)t, adc::ST_XPHANTOM, (uint32_t)k, tick);
                            clicked = adc::bernoulli(w.x, t_click);
                        }
                        if (clicked && budget >= 0.0) {
                            ++paid;
                            if (TAPE) convd = tape_at(tp.conv, cur_conv++, tp.len_conv, tp.error) != 0;
                            else convd = adc::bernoulli(w.y, t_conv);
                            if (convd) {
                                ++convs;
                                if (TAPE) rv = tape_at(tp.rev_cents, cur_rev++, tp.len_rev, tp.error);
                                else rv = adc::revenue_cents(w.z, mu, sd);
                                cell_rev_c += rv;
                            }
                            if (replay) record(lane == 0, 1ull, k, t, 0.0, convd, rv);      // (a zero-cost click: the reference lists it)
                        }
                    }
                    if (replay && lane == 0 && imps > 0) rp.share_volume[k] += n;
                    if (lane == 0) {
                        s_imp[k] += imps;
                        s_clk[k] += paid;
                        s_conv[k] += convs;
                        s_cost_d[k] = obs_cost;
                        s_rev[k] += cell_rev_c;
                        s_profit[k] += (double)cell_rev_c / 100.0 - cell_cost;    // combine_outcomes: profit += profit
                    }
                    remaining_d -= cell_cost;
                    if (remaining_d <= 0.0) stop = true;
                }
            }
        }
        __syncthreads();
        if (replay) {                       // nothing of the engine's state is written
            if (lane == 0) *rp.count = rec_base;
            return;
        }
        if (TAPE && lane == 0) {
            if (tp.end_bid) tp.end_bid[env] = cur_bid;
            if (tp.end_ximp) tp.end_ximp[env] = cur_ximp;
            if (tp.end_xcost) tp.end_xcost[env] = cur_xcost;
            if (tp.end_click) tp.end_click[env] = cur_click;
            if (tp.end_conv) tp.end_conv[env] = cur_conv;
            if (tp.end_rev) tp.end_rev[env] = cur_rev;
        }
        // per-keyword observations of the exact pass
        long long pc = 0;
        for (int k = lane; k < K; k += kWave) {
            const size_t o = (size_t)env * K + k;
            const float fast_rev = v.rev[o], fast_cost = v.cost[o];       // what the fast pass (if any) left there
            v.imp[o] = s_imp[k];
            v.clk[o] = s_clk[k];
            v.conv[o] = s_conv[k];
            const long long r = s_rev[k];
            v.rev[o] = (float)r / 100.0f;
            if (MODEL == ADC_MODEL_IMPLICIT) {
                const long long c = s_cost_i[k];
                v.cost[o] = (float)c / 100.0f;
                pc += r - c;
                if (v.metrics_on && !TAPE && fast_ran) {
                    // K beyond the row kernel: this kernel re-ran an env the fast pass had already added to the metric sums;
                    // take that contribution back exactly (k_step_exact_rows does the same)
                    const float fr = fast_rev, fc = fast_cost;
                    long long old;
                    if (fr < 41943.0f && fc < 41943.0f) old = (long long)__builtin_rintf(fr * 100.0f) - (long long)__builtin_rintf(fc * 100.0f);
                    else {
                        unsigned int cv; unsigned long long rv, pcost;
                        walk_cell<1>(key, tick, (uint32_t)k, 0, s_vol[k], (int)adc::bid_to_cents(bids[o]), param_at(v, ADC_P_A, env, k),
                                     param_at(v, ADC_P_B, env, k), adc::make_auction_law(param_at(v, ADC_P_BCTR, env, k)),
                                     adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, k)), param_at(v, ADC_P_REV_MEAN, env, k),
                                     param_at(v, ADC_P_REV_STD, env, k), g_log_table, 0, cv, rv, pcost);
                        old = (long long)rv - (long long)pcost;
                    }
                    metric_add(v, o, (r - c) - old);
                } else if (v.metrics_on && !TAPE) metric_add(v, o, r - c);
            } else {
                v.cost[o] = (float)s_cost_d[k];
            }
        }
        profit_c = wave_sum_i64(pc);
        if (MODEL == ADC_MODEL_IMPLICIT_GENERAL && !TAPE && lane == 0) v.exact_hint[env] = (budget_bound || stop) ? 1 : 0;
        if (MODEL != ADC_MODEL_IMPLICIT) {
            // reward = rust.sum_list(profit_k): left to right (gymnasium_kw_env.py:222)
            double r = 0.0;
            for (int k = 0; k < K; ++k) r += s_profit[k];
            reward_d = r;
        }
    } else {
        profit_c = v.env_profit[env];
    }

    if (lane == 0) step_tail(v, env, tick, MODEL == ADC_MODEL_IMPLICIT, profit_c, reward_d);
    if (TAPE && v.drift_on && tp.drift_uniforms) {
        // update_keywords() with the recorded coefficient vectors (gymnasium_kw_env.py:132-158, called at :246)
        const size_t NK = (size_t)v.N * K;
        for (int k = lane; k < K; k += kWave) {
            if (!drift_selected(v, env, k)) continue;       // (the selection gates the recorded coefficients too)
            const size_t i = (size_t)env * K + k;
            float vm = param_at(v, ADC_P_VOL_MEAN, env, k), bc = param_at(v, ADC_P_BCTR, env, k), sc = param_at(v, ADC_P_SCTR, env, k);
            apply_drift_coefficients(tp.drift_uniforms[i], tp.drift_uniforms[NK + i], tp.drift_uniforms[2 * NK + i],
                                     vm, param_at(v, ADC_P_VOL_STD, env, k), bc, sc);
            param_at(v, ADC_P_VOL_MEAN, env, k) = vm;
            param_at(v, ADC_P_BCTR, env, k) = bc;
            param_at(v, ADC_P_SCTR, env, k) = sc;
        }
        if (lane == 0) v.drift_pending[env] = 0;      // (same lane as step_tail's store: program order)
    }
}

