// kernel_exact_rows.inc - k_step_exact_rows: row-parallel budget-exact pass + step tail (IMPLICIT, K <= 2048)
// (part of the single translation unit adc_engine.hip; see that file for the overview)
// -------------------------------------------------------------------------------------------------
// EXACT PASS, ROW-PARALLEL (IMPLICIT, engine stream): one 256-lane workgroup per env
// -------------------------------------------------------------------------------------------------
// The reference walks the day's 24 x K cells in order (t-major, keyword-minor) with one shared budget
// (adcraft/bidding_simulation.py:214-233).  Per sub-timestep row t:
//   pass A  every cell (t,k) of the row is evaluated in parallel (one lane per cell): wins W, clicked
//           wins NC, their total cost T, and the cost X1 of the first clicked win;
//   resolve the budget walk over the row's cells, in keyword order, as a loop of three block-wide steps:
//           (a) bulk - cells whose running total stays strictly below the remaining budget are paid in
//               full (every click affordable, remaining stays > 0);
//           (b) the first cell that does not fit is walked click by click by its lane (pay while the
//               running cost fits, :97-104); exact exhaustion (remaining == 0) stops the campaign (:230-233);
//           (c) skip - with what is left, a cell whose FIRST click is unaffordable pays nothing (the
//               reference breaks at it), so jump to the next cell with X1 <= remaining;
//   pass B  cells paid in full are re-walked with the conversion / revenue draws; the others only count
//           their impressions (impressions are not budget-limited, :86-88).
// Costs are >= 0, so remaining never increases and (a)/(c) are exact, not heuristics.
// developer instrumentation (python adcraft_amd/build.py --timing; tools/exp_rows_timing.py): per-phase wall-clock sums
#ifdef ADC_EXP_TIMING
#define DBG_T() wall_clock64()
#define DBG_ADD(i, x) dbg[i] += (x)
#else
#define DBG_T() 0ull
#define DBG_ADD(i, x) (void)0
#endif
constexpr int kRowsBlock = 256;
#ifndef ADC_ROWS_MIN_BLOCKS
#define ADC_ROWS_MIN_BLOCKS 4
#endif
constexpr int kRowsMinBlocks = ADC_ROWS_MIN_BLOCKS;      // resident workgroups per CU the register budget is set for (K > 256: LDS allows two anyway)
// K <= 256: since the lean rows moved to k_step_rest_of_day the kernel's register demand is lower and more workgroups per CU pay
// (measured on cfg2 at budget 1000: 3 per CU 0.635, 4 0.570, 5 0.557, 6 0.546, 7 0.548, 8 0.641 ms)
#ifndef ADC_ROWS_MIN_BLOCKS_ONE
#define ADC_ROWS_MIN_BLOCKS_ONE 6
#endif
constexpr int kRowsMinBlocksOne = ADC_ROWS_MIN_BLOCKS_ONE;
constexpr int kRowsMaxK = 2048;      // 73 B of LDS per keyword: 2048 keywords = 146 KB of the CU's 160 KB (one workgroup per CU)
constexpr int kRowsRing = 128;        // per-wave ring of paid clicks awaiting their conversion / revenue draw

struct CellStat {
    unsigned int wins, clicks, first;     // first = cost of the first clicked win (0xFFFFFFFF if none)
    unsigned int mask;                    // bit i = auction j0+i of the cell is a clicked win (cells of <= 32 auctions)
    unsigned long long total;             // cost of all clicked wins, cents
    double sum_d;                         // the same as the reference adds it up: ((0.0 + c1/100) + c2/100) + ...
    unsigned long long q4;                // prices of the first four clicked wins, 16 bits each (0xFFFF: more than that)
};

// mode 0: statistics only (st.sum_d = the float sum the campaign's remaining budget loses if the cell is paid in full).
// mode 1: every click is paid (adds conversions / revenue); `paid_cost` returns the cents spent.
template <int MODE>
__device__ __forceinline__ CellStat walk_cell(uint64_t key, uint32_t tick, uint32_t kw, int j0, int n, int bid_c, float loc,
                                              float scale, const adc::AuctionLaw &law, unsigned long long t_conv, float mu,
                                              float sd, const adc::LogTableEntry *logtab, long long sum_limit,
                                              unsigned int &conv_out, unsigned long long &rev_out, unsigned long long &paid_cost,
                                              adc::U4 *quad = nullptr, int *quad_index = nullptr)
{
    // quad / quad_index (optional): the last Philox call of this keyword's previous cell - consecutive cells of a keyword
    // share the call that straddles their boundary (a call serves four consecutive auctions)
    CellStat st{0u, 0u, 0xFFFFFFFFu, 0u, 0ull, 0.0, 0ull};
    conv_out = 0u;
    rev_out = 0ull;
    paid_cost = 0ull;
    const int jend = j0 + n;
    for (int q = j0 >> 2; 4 * q < jend; ++q) {
        adc::U4 w;
        if (quad && *quad_index == q) w = *quad;
        else w = adc::draw(key, (uint32_t)q, adc::ST_AUCTION, kw, tick);
        if (quad) { *quad = w; *quad_index = q; }
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int j = 4 * q + h;
            if (j < j0 || j >= jend) continue;
            bool click_bit;
            const uint32_t word = h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w;
            const int comp = adc::auction_outcome(word, law, loc, scale, logtab, click_bit);
            if (!adc::auction_wins(word, bid_c, comp)) continue;
            st.wins += 1u;
            if (!click_bit) continue;
            if (MODE == 0) {
                if (st.clicks < 4u) st.q4 |= (unsigned long long)min(comp, 0xFFFF) << (16u * st.clicks);
                st.clicks += 1u;
                st.total += (unsigned long long)comp;
                // the float sum is only read for a cell paid in full, and such a cell's running total never exceeds
                // the budget left at the start of its row
                if ((long long)st.total <= sum_limit) st.sum_d += adc::cents_to_dollars_f64(comp);
                if (st.first == 0xFFFFFFFFu) st.first = (unsigned int)comp;
                if (j - j0 < 32) st.mask |= 1u << (j - j0);
                continue;
            }
            st.clicks += 1u;
            paid_cost += (unsigned long long)comp;
            const adc::U4 w2 = adc::draw(key, (uint32_t)j, adc::ST_CONV, kw, tick);
            if (adc::bernoulli(w2.x, t_conv)) {
                conv_out += 1u;
                rev_out += (unsigned long long)adc::revenue_cents_tab(w2.y, mu, sd, g_norm_table);
            }
        }
    }
    st.total = MODE == 0 ? st.total : paid_cost;
    return st;
}

// The reference's in-cell loop (adcraft/bidding_simulation.py:86-118) for ONE cell, by a whole wavefront: lane i resolves
// auction j0+i, the clicked wins are then walked in auction order in the reference's float arithmetic (pay while
// `budget >= cost`, `budget -= cost`, :97-104), and the paid clicks draw conversion / revenue lane-parallel.
// All results are wave-uniform.
struct CellWalk {
    unsigned int wins, paid, convs;
    unsigned long long cost_c, rev_c;     // cents
    double sum_d;                         // ((0.0 + c1/100) + c2/100) + ... over the paid clicks: what `remaining` loses (:225)
};
__device__ __forceinline__ CellWalk walk_cell_wave(uint64_t key, uint32_t tick, uint32_t kw, int j0, int n, int bid_c, float loc,
                                                   float scale, const adc::AuctionLaw &law, unsigned long long t_conv, float mu,
                                                   float sd, double budget, const adc::LogTableEntry *logtab)
{
    const int lane = threadIdx.x & 63;
    CellWalk cw{0u, 0u, 0u, 0ull, 0ull, 0.0};
    bool broke = false;
    for (int base = 0; base < n; base += kWave) {
        const int i = base + lane;
        const uint32_t j = (uint32_t)(j0 + i);
        bool click_bit = false;
        int comp = 0x7FFFFFFF;
        uint32_t word = 0u;
        if (i < n) {
            const adc::U4 w = adc::draw(key, j >> 2, adc::ST_AUCTION, kw, tick);
            word = (j & 3u) == 0 ? w.x : (j & 3u) == 1 ? w.y : (j & 3u) == 2 ? w.z : w.w;
            comp = adc::auction_outcome(word, law, loc, scale, logtab, click_bit);
        }
        const bool win = i < n && adc::auction_wins(word, bid_c, comp);
        cw.wins += (unsigned int)__popcll(__ballot(win));
        unsigned long long cand = __ballot(win && click_bit);
        unsigned long long paid_mask = 0ull;
        while (cand && !broke) {
            const int l = __ffsll((long long)cand) - 1;
            cand &= cand - 1ull;
            const double cost_d = adc::cents_to_dollars_f64(__shfl(comp, l, 64));
            if (budget >= cost_d) { budget -= cost_d; cw.sum_d += cost_d; paid_mask |= 1ull << l; }
            else broke = true;
        }
        const bool is_paid = (paid_mask >> lane) & 1ull;
        bool convd = false;
        long long rv = 0;
        if (is_paid) {
            const adc::U4 w2 = adc::draw(key, j, adc::ST_CONV, kw, tick);
            convd = adc::bernoulli(w2.x, t_conv);
            if (convd) rv = adc::revenue_cents_tab(w2.y, mu, sd, g_norm_table);
        }
        cw.paid += (unsigned int)__popcll(paid_mask);
        cw.convs += (unsigned int)__popcll(__ballot(convd));
        cw.cost_c += (unsigned long long)wave_sum_i64(is_paid ? (long long)comp : 0ll);
        cw.rev_c += (unsigned long long)wave_sum_i64(rv);
    }
    return cw;
}

constexpr int kRowsMaxWaves = 16;
struct RowsShared {
    long long wave_part[kRowsMaxWaves];
    int wave_min[kRowsMaxWaves];
    long long remaining;
    double remaining_d;       // the reference's float `remaining_budget`, advanced lazily in cell order
    int chain_pos;            // cells [0, chain_pos) of the current row are already subtracted from remaining_d
    int cur;
    int stopped;
    int bound_k;
};

// One lane per env (coalesced): envs for which the fast pass was exact get their step tail here; the others -
// spend reached the budget, or the fast pass skipped them on a hint - are appended to the step's flagged list
// for k_step_exact_rows.  The list counter is double-buffered by step parity so that it can be cleared for the
// next step without a memset node: this launch clears the other parity's counter.
// plain_fast_ran: the fast pass of this step was k_step_implicit_fast in the variant WITHOUT click lists (the host had not heard
// of an env that wants them yet) - an env that wants them is told so, so that the row kernel does not conclude that lists are
// not on offer (as they are not while k_step_implicit_sparse is the fast pass)
// direct_follows: k_step_rest_of_day<true, true> (+ k_rest_walk) is launched this step - an env with hint 6 (yesterday its budget ran out
// within the first cells of the day) is parked for them here, before anything of its day has been looked at: the row kernel
// would evaluate the whole first row in full only to find that out again.
__global__ void k_tail_or_flag(View v, const float *__restrict__ budget_in, int parity, int plain_fast_ran, int direct_follows)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env == 0) {
        v.flag_count[parity ^ 1] = 0; v.flag_next[parity ^ 1] = 0; v.xover_count[parity ^ 1] = 0; v.retry_count[parity ^ 1] = 0;
        if (v.rest_state) { v.rest_count[parity ^ 1] = 0; v.rest_next[parity ^ 1] = 0; }
        if (v.direct_list) { v.direct_count[parity ^ 1] = 0; v.direct_next[parity ^ 1] = 0; }
    }
    bool flagged = false, listed = false, direct = false;
    if (env < v.N) {
        const long long budget_c = adc::budget_to_cents(budget_in[env]);
        const int hint = v.exact_hint[env];
        const uint32_t tick = v.tick[env];
        if (hint == 6) {                                // (the fast pass skipped the env)
            // (not with nothing to spend - :230-233 visits the first cell then, the row kernel's business - and not with a budget
            //  well above the one that ran out so early)
            direct = direct_follows && v.direct_list && budget_c > 0 && budget_c <= v.direct_budget[env] + (v.direct_budget[env] >> 2);
            flagged = !direct;
            if (direct) {
                RestState st;
                st.R = budget_c;
                st.r_d = (double)budget_c / 100.0;
                st.row = 0;
                st.flags = 1 | 4 | (6 << 4);
                st.pc = 0;
                v.rest_state[env] = st;
            }
        } else
        if (hint != 2 && v.env_cost[env] < budget_c) {
            if (hint == 1) {                            // it no longer binds
                v.exact_hint[env] = 0;
                if (v.click_count) { for (int t = 0; t < adc::kTimesteps; ++t) v.click_count[(size_t)env * adc::kTimesteps + t] = 0u; v.click_tick[env] = 0u; }
            }
            step_tail(v, env, tick, true, v.env_profit[env], 0.0);
        } else {
            listed = hint == 1 && v.click_count && v.click_tick[env] == tick + 1u;     // the fast pass listed this step's clicked wins
            flagged = !listed;
            if (hint == 1 && v.click_count && plain_fast_ran) v.click_tick[env] = 0xFFFFFFFFu;
        }
    }
    // one atomic per wavefront and list, not per env (same-address atomics serialise)
    const int lane = threadIdx.x & 63;
    auto append = [&](bool mine, int *list, int *count) {
        const unsigned long long m = __ballot(mine);
        if (!m) return;
        int base = 0;
        if (lane == __ffsll((long long)m) - 1) base = atomicAdd(count, (int)__popcll(m));
        base = __shfl(base, __ffsll((long long)m) - 1, 64);
        if (mine) list[base + (int)__popcll(m & ((1ull << lane) - 1ull))] = env;
    };
    append(flagged, v.flag_list, &v.flag_count[parity]);
    append(listed, v.xover_list, &v.xover_count[parity]);
    if (v.direct_list) {
        const unsigned long long m = __ballot(direct);
        if (m) {
            append(direct, v.direct_list, &v.direct_count[parity]);
            if (lane == __ffsll((long long)m) - 1) atomicAdd(v.direct_days, (unsigned long long)__popcll(m));      // (this engine's own counter: adc_debug_direct_days)
        }
    }
}

// What an IMPLICIT env's exact pass leaves for tomorrow (one lane): the scheduling hint, and the click lists' state.
// direct_budget >= 0: tomorrow k_tail_or_flag may park the env at once (hint 6) unless its budget is well above this one
__device__ __forceinline__ void exact_pass_epilogue(const View &v, int env, int hint_in, bool few_clicks, bool was_binding, int bound_row,
                                                    long long direct_budget = -1)
{
    // tomorrow: list the clicked wins for k_step_click_walk where that path exists and has not just overflowed
    // (hint_in == 1 here: the fast pass that ran does not list clicks - the sparse kernel - so do without from now on;
    //  hint_in == 1 with the marker: the fast pass that ran was the variant without lists - the host had not heard yet)
    const bool plain_ran = hint_in == 1 && v.click_count && v.click_tick[env] == 0xFFFFFFFFu;
    const bool list = was_binding && v.click_count && ((hint_in == 0 && few_clicks) || hint_in == 4 || plain_ran);
    if (list) tell_host_once(v.listing_flag, v.flags_seen + 1);
    v.exact_hint[env] = !was_binding ? 0 : list ? 1 : direct_budget >= 0 ? 6 : 2;
    if (was_binding && !list && direct_budget >= 0) { v.direct_budget[env] = direct_budget; tell_host_once(v.direct_flag, v.flags_seen + 2); }
    if (list && hint_in == 0) { v.click_row_hint[env] = adc::kTimesteps - 1; v.click_price_hint[env] = 0u; }      // the first lists are complete
    if (v.click_count) { for (int t = 0; t < adc::kTimesteps; ++t) v.click_count[(size_t)env * adc::kTimesteps + t] = 0u; v.click_tick[env] = 0u; }
}

// persistent grid: every workgroup takes the next flagged env from a ticket counter until the list is exhausted
// ONE (K <= BLOCK): a lane serves the same keyword in every row, so the keyword's constants (bid, competitor law, click
// law) and the Philox call straddling two of its cells stay in registers for the whole day.
// rest_follows: k_step_rest_of_day is launched behind this kernel (the host does that once this kernel has told it, through
// View::binding_flag, that budgets bind: until then a day is finished here, lean row by lean row)
// BLOCK: lanes per workgroup.  ONE (a lane per keyword) exists for K <= 256 only; beyond that a workgroup of 256 lanes (K <= 512) or of 512
// (K <= 2048) takes 2 - 4 cells per lane and row one after the other.  (ONE with 512 / 1024 lanes was built in round 4, lost to these
// and was removed in round 5: profiles/HISTORY.md.)
template <bool ONE, int BLOCK = kRowsBlock>
// (the second bound is wavefronts per SIMD; 512 lanes: two workgroups per CU hold the tables of 1024 keywords - four wavefronts per
//  SIMD, 128 registers and no spill)
__global__ __launch_bounds__(BLOCK, BLOCK == 512 ? 4 : ONE ? kRowsMinBlocksOne : kRowsMinBlocks) void k_step_exact_rows(View v, const float *__restrict__ bids,
                                                                const float *__restrict__ budget_in, int parity, int rest_follows)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ RowsShared rs;
    __shared__ adc::LogTableEntry s_logtab[adc::kLogTableIntervals];       // copy of g_log_table (one lookup per auction)
    static_assert(adc::kLogTableIntervals <= BLOCK && BLOCK / kWave <= kRowsMaxWaves, "a table entry per lane; RowsShared");
    if (threadIdx.x < adc::kLogTableIntervals) s_logtab[threadIdx.x] = g_log_table[threadIdx.x];
    const int K = v.K;
    // per keyword (persistent over the day)
    unsigned long long *a_cost = reinterpret_cast<unsigned long long *>(lds_raw);        // [K]
    unsigned long long *a_rev = a_cost + K;                                               // [K]
    unsigned long long *c_total = a_rev + K;          // per cell of the current row: cost of clicked wins
    double *c_sum_d = reinterpret_cast<double *>(c_total + K);       // float sum of the cell's clicked costs
    unsigned long long *c_q4 = reinterpret_cast<unsigned long long *>(c_sum_d + K);      // CellStat::q4
    int *s_vol = reinterpret_cast<int *>(c_q4 + K);
    unsigned int *a_imp = reinterpret_cast<unsigned int *>(s_vol + K);
    unsigned int *a_clk = a_imp + K, *a_conv = a_clk + K;
    unsigned int *c_wins = a_conv + K, *c_first = c_wins + K, *c_mask = c_first + K, *c_clicks = c_mask + K;
    unsigned int *rings = c_clicks + K;                                         // [BLOCK / kWave][kRowsRing]
    unsigned char *c_state = reinterpret_cast<unsigned char *>(rings + (BLOCK / kWave) * kRowsRing);
    // c_state: 0 impressions only, 1 paid in full, 2 done, 3 not visited

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    unsigned long long dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)dbg;
    const int n_flagged = v.flag_count[parity];
  // first ticket = the workgroup's own index (no atomic: with nothing flagged every workgroup leaves at once, and
  // thousands of same-address atomics would serialise at ~12 ns each); later tickets come from the shared counter
  for (int fi = blockIdx.x;;) {
    if (fi >= n_flagged) break;
    const int env = v.flag_list[fi];
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    const long long budget_c = adc::budget_to_cents(budget_in[env]);
    const int hint_in = v.exact_hint[env];
    const bool hinted = (hint_in & ~4) == 2;           // the fast pass skipped this env (6: and k_tail_or_flag did not park it today)
    // (first binding day of an env, click lists available: how many clicked wins the fast pass counted - the lists pay off
    // below a few thousand a day)
    bool few_clicks = false;
    if (hint_in == 0 && v.click_count) {
        int c = 0;
        for (int k = tid; k < K; k += BLOCK) c += v.clk[(size_t)env * K + k];
        c = wave_sum_i32(c);
        if (lane == 0) rs.wave_min[wv] = c;
        __syncthreads();
        int total = 0;
        for (int i = 0; i < BLOCK / kWave; ++i) total += rs.wave_min[i];
        few_clicks = total <= v.click_list_max;
    }
    __syncthreads();
    const bool drift = hinted && v.drift_on && v.drift_pending[env];    // the skipped fast pass would have applied it
    bool was_binding = false;
    int bound_t = adc::kTimesteps;                     // the sub-timestep in which the budget bound
    if (tid == 0) rs.bound_k = 0x7FFFFFFF;             // ... and the first cell of it that did not fit as a whole

    for (int k = tid; k < K; k += BLOCK) {
        if (drift) {
            drift_keyword_planes(v, env, key, tick - 1u, k);
        }
        s_vol[k] = adc::volume_from_word(adc::volume_word(key, (uint32_t)k, tick), param_at(v, ADC_P_VOL_MEAN, env, k),
                                         param_at(v, ADC_P_VOL_STD, env, k), g_norm_table);
    }
    for (int k = tid; k < K; k += BLOCK) {
        a_imp[k] = a_clk[k] = a_conv[k] = 0u;
        a_cost[k] = a_rev[k] = 0ull;
    }
    // (ONE) this lane's keyword for the whole day
    int my_bid_c = 0;
    float my_loc = 0.f, my_scale = 0.f;
    adc::AuctionLaw my_law{0u, 0u, 0u};
    adc::U4 my_quad{0u, 0u, 0u, 0u};
    int my_quad_index = -1;
    if (ONE && tid < K) {
        my_bid_c = (int)adc::bid_to_cents(bids[(size_t)env * K + tid]);
        my_loc = param_at(v, ADC_P_A, env, tid);
        my_scale = param_at(v, ADC_P_B, env, tid);
        my_law = adc::make_auction_law(param_at(v, ADC_P_BCTR, env, tid));
    }
    if (tid == 0) { rs.remaining = budget_c; rs.remaining_d = (double)budget_c / 100.0; rs.stopped = 0; }
    bool handed = false;                               // the rest of the day goes to k_step_rest_of_day
    __syncthreads();
    // LEAN ROWS.  After a row that did not fit the budget as a whole, what is left is smaller than a row's clicks cost and
    // stays so (costs are >= 0): in the following rows a cell only matters if its FIRST clicked win is affordable - any other
    // cell breaks at that click and only counts impressions (:97-104).  Such rows are classified instead of priced: wins and
    // the first clicked win of a cell come from the keyword's win intervals in word space (adc_law.h win_intervals, two
    // compares per auction), and only that first click is priced.  A cell with a click is given an unpayable total, so the
    // resolve below never takes it as paid in full: it is skipped (first click too dear) or walked click by click (exact for
    // any cell).  With no affordable first click in the whole row - the usual case once the budget is ground down - the row
    // is "impressions += wins" and nothing else.  (K > 256: the same record from the auction-by-auction evaluation, see below.)
    constexpr long long kUnpayable = 1ll << 55;        // > any budget in cents (budget_to_cents caps at 9e15); 64 of them fit an i64

    for (int t = 0; t < adc::kTimesteps; ++t) {
        const bool lean = was_binding;                  // (uniform)
        if (lean && v.rest_state && tid == 0) tell_host_once(v.binding_flag, v.flags_seen);
        if (lean && v.rest_state && rest_follows) {
            // THE REST OF THE DAY goes to k_step_rest_of_day (below): from here on a cell only matters if it holds a clicked win
            // that costs at most what is left, and that is decided for all remaining rows at once - in a kernel of its own,
            // because this one's register budget is spent (the pass was first written in place: 51 spilled registers, and its
            // loop waited on them).  The env's state is parked in global memory.
            // (metric mode reads the fast pass's float outputs back as cents, exact below 2^22 cents: a larger keyword-day stays here)
            bool big = false;
            if (v.metrics_on && !hinted)
                for (int k = tid; k < K; k += BLOCK) { const size_t o = (size_t)env * K + k; big = big || !(v.rev[o] < 41943.0f && v.cost[o] < 41943.0f); }
            if (!__syncthreads_or(big ? 1 : 0)) {
                // (k_rest_walk follows - View::rest_marks: what the day has so far is written out here, 256 lanes wide; the walk's one
                //  wavefront per env then only touches the keywords of the few cells that still pay)
                const bool out_here = v.rest_marks != nullptr;
                long long pc_here = 0;
                for (int k = tid; k < K; k += BLOCK) {
                    const size_t o = (size_t)env * K + k;
                    const long long c = (long long)a_cost[k], r = (long long)a_rev[k];
                    v.rest_cost[o] = c;
                    v.rest_rev[o] = r;
                    v.rest_counts[o] = make_uint4(a_imp[k], a_clk[k], a_conv[k], (unsigned int)s_vol[k]);
                    if (out_here) {
                        if (v.metrics_on) {         // (what the discarded fast pass added, if it ran: below 2^22 cents, checked above)
                            const long long old = hinted ? 0ll : (long long)__builtin_rintf(v.rev[o] * 100.0f) - (long long)__builtin_rintf(v.cost[o] * 100.0f);
                            metric_add(v, o, (r - c) - old);
                        }
                        v.clk[o] = (int)a_clk[k];
                        v.conv[o] = (int)a_conv[k];
                        v.cost[o] = adc::cents_to_dollars_f32(c);
                        v.rev[o] = adc::cents_to_dollars_f32(r);
                        pc_here += r - c;
                    }
                }
                if (out_here) {
                    pc_here = wave_sum_i64(pc_here);
                    if (lane == 0) rs.wave_part[wv] = pc_here;
                    __syncthreads();
                }
                if (tid == 0) {
                    RestState st;
                    st.R = rs.remaining;
                    st.r_d = rs.remaining_d;
                    st.row = t;
                    // (bit 3: the budget ran out within the first quarter of the day's first row - tid 0 is in wave 0)
                    st.flags = (hinted ? 1 : 0) | (hint_in << 4) | (few_clicks ? 2 : 0) | (bound_t == 0 && rs.bound_k < K / 4 + 1 ? 8 : 0);
                    st.pc = 0;
                    if (out_here) for (int i = 0; i < BLOCK / kWave; ++i) st.pc += rs.wave_part[i];
                    v.rest_state[env] = st;
                    v.retry_list[atomicAdd(&v.rest_count[parity], 1)] = env;
                }
                handed = true;
                break;                                  // (uniform)
            }
        }
        // ---- pass A: statistics of every cell of the row
        [[maybe_unused]] const unsigned long long tA = DBG_T();
        DBG_ADD(5, 1);
        const long long R_row = rs.remaining;          // (uniform; written before the barrier that ended the previous row)
        long long my_total = 0;
        unsigned int my_first = 0xFFFFFFFFu;
        if (lean) {
            // (K > 256, or K <= 256 without k_step_rest_of_day) the lean record (wins, price of the first clicked win) comes from
            // the auction-by-auction evaluation, minus all the bookkeeping of the full pass A
            bool maybe = false;
            for (int k = tid; k < K; k += BLOCK) {
                int32_t j0, n;
                adc::cell_range(s_vol[k], t, j0, n);
                const int jend = j0 + n;
                const int bid_c = (int)adc::bid_to_cents(bids[(size_t)env * K + k]);
                const float loc = param_at(v, ADC_P_A, env, k), scale = param_at(v, ADC_P_B, env, k);
                const adc::AuctionLaw law = adc::make_auction_law(param_at(v, ADC_P_BCTR, env, k));
                unsigned int wins = 0u, first = 0xFFFFFFFFu;
                for (int q = j0 >> 2; 4 * q < jend; ++q) {
                    const adc::U4 w = adc::draw(key, (uint32_t)q, adc::ST_AUCTION, (uint32_t)k, tick);
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const int j = 4 * q + h;
                        if (j < j0 || j >= jend) continue;
                        const uint32_t word = h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w;
                        bool click_bit;
                        const int comp = adc::auction_outcome(word, law, loc, scale, s_logtab, click_bit);
                        if (!adc::auction_wins(word, bid_c, comp)) continue;
                        wins += 1u;
                        if (click_bit && first == 0xFFFFFFFFu) first = (unsigned int)comp;
                    }
                }
                c_wins[k] = wins;
                c_first[k] = first;
                c_total[k] = first != 0xFFFFFFFFu ? (unsigned long long)kUnpayable : 0ull;
                maybe = maybe || (long long)first <= R_row;
                my_first = min(my_first, first);
            }
            if (!__syncthreads_or(maybe ? 1 : 0)) {         // nobody can pay anything in this row: impressions only
                for (int k = tid; k < K; k += BLOCK) a_imp[k] += c_wins[k];
                DBG_ADD(0, DBG_T() - tA);
                continue;
            }
            for (int k = tid; k < K; k += BLOCK) {
                c_sum_d[k] = 0.0;
                c_mask[k] = 0u;
                c_clicks[k] = 0u;
                c_state[k] = 1;
            }
        } else
        for (int k = tid; k < K; k += BLOCK) {
            int32_t j0, n;
            adc::cell_range(s_vol[k], t, j0, n);
            unsigned int cv; unsigned long long rv, pc;
            const CellStat st = ONE
                ? walk_cell<0>(key, tick, (uint32_t)k, j0, n, my_bid_c, my_loc, my_scale, my_law, 0ull, 0.f, 0.f, s_logtab, R_row, cv, rv, pc,
                               &my_quad, &my_quad_index)
                : walk_cell<0>(key, tick, (uint32_t)k, j0, n, (int)adc::bid_to_cents(bids[(size_t)env * K + k]),
                               param_at(v, ADC_P_A, env, k), param_at(v, ADC_P_B, env, k),
                               adc::make_auction_law(param_at(v, ADC_P_BCTR, env, k)), 0ull, 0.f, 0.f, s_logtab, R_row, cv, rv, pc);
            c_wins[k] = st.wins;
            c_first[k] = st.first;
            c_total[k] = st.total;
            c_sum_d[k] = st.sum_d;
            c_q4[k] = st.q4;
            c_mask[k] = st.mask;
            c_clicks[k] = st.clicks;
            c_state[k] = 1;
            my_total += (long long)st.total;
            my_first = min(my_first, st.first);
        }
        my_total = wave_sum_i64(my_total);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) my_first = min(my_first, (unsigned int)__shfl_xor((int)my_first, o, 64));
        if (lane == 0) { rs.wave_part[wv] = my_total; rs.wave_min[wv] = (int)my_first; }
        if (tid == 0) rs.chain_pos = 0;
        __syncthreads();
        // The reference keeps `remaining_budget` as a float and subtracts every cell's float cost sum from it in cell
        // order (:225); whether a check that is an exact tie in cents passes, and whether an exhausted budget reads
        // <= 0 (:230-233), is decided by that float residue.  advance_chain(upto) subtracts the sums of the fully paid
        // cells in [chain_pos, upto) in keyword order.  Called by all of wave 0: each lane fetches one cell's sum, and 64 of them
        // are subtracted at a time, exactly as the chain of 64 rounded subtractions would (common.inc chain_subtract_wave: an
        // integer prefix scan inside the running value's binade).
        auto advance_chain = [&](int upto) {
            double r = rs.remaining_d;
            const int from = rs.chain_pos;
            for (int base = from & ~63; base < upto; base += kWave) {
                const int kk = base + lane;
                const double x = (kk >= from && kk < upto && c_state[kk] == 1) ? c_sum_d[kk] : 0.0;
                r = chain_subtract_wave(r, x);
            }
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) { rs.remaining_d = r; rs.chain_pos = upto; }
            return r;
        };
        long long row_total = 0;
        unsigned int row_first = 0xFFFFFFFFu;           // cheapest first click of the row
#pragma unroll
        for (int i = 0; i < BLOCK / kWave; ++i) {
            row_total += rs.wave_part[i];
            row_first = min(row_first, (unsigned int)rs.wave_min[i]);
        }
        long long R = rs.remaining;
        __syncthreads();
        [[maybe_unused]] const unsigned long long tR = DBG_T();
        DBG_ADD(0, tR - tA);
        if (lean) {
            if ((long long)row_first > R) {             // (not reached: the one-barrier test above has already taken such rows)
                for (int k = tid; k < K; k += BLOCK) a_imp[k] += c_wins[k];
                continue;
            }
            row_total = kUnpayable;                     // (some cell has a click: the row does not fit as a whole)
        }

        if (!(R - row_total > 0)) {
            // ---- the row does not fit as a whole: wave 0 resolves it in keyword order with wave-level operations only
            // (the three other waves wait at one barrier; block-wide steps cost ten barriers per walked cell)
            was_binding = true;
            if (bound_t == adc::kTimesteps) bound_t = t;
            const bool visit_first = t == 0 && budget_c <= 0;     // :230-233: the first cell is visited even with nothing to spend
            if (wv == 0) {
                int cur = 0;
                bool stop = false;
                if ((long long)row_first > R && !visit_first) {
                    // nothing in this row is affordable: every cell breaks at its first click (impressions still count)
                    for (int k = lane; k < K; k += kWave) c_state[k] = 0;
                    cur = K;
                    if (lane == 0 && rs.bound_k == 0x7FFFFFFF) rs.bound_k = 0;
                }
                while (cur < K && !stop) {
                    // (a) bulk: cells whose running total from `cur` stays strictly below R are paid in full (keep state 1)
                    bool found = false;
                    for (int base = cur & ~63; base < K; base += kWave) {
                        const int kk = base + lane;
                        const bool in = kk >= cur && kk < K;
                        const long long x = in ? (long long)c_total[kk] : 0;
                        const long long incl = wave_scan_i64(x);
                        const unsigned long long nofit = __builtin_amdgcn_ballot_w64(in && !(incl < R));
                        if (nofit == 0ull) { R -= readlane_i64(incl, 63); cur = base + kWave; continue; }
                        const int l = __ffsll((long long)nofit) - 1;
                        R -= readlane_i64(incl - x, l);               // what the cells before it took
                        cur = base + l;
                        if (lane == 0 && rs.bound_k == 0x7FFFFFFF) rs.bound_k = cur;
                        found = true;
                        break;
                    }
                    if (!found) { cur = K; break; }
                    // (b) skip cells whose first click is unaffordable (they pay nothing, impressions still count)
                    found = false;
                    for (int base = cur & ~63; base < K; base += kWave) {
                        const int kk = base + lane;
                        const bool in = kk >= cur && kk < K;
                        const bool hit = in && ((long long)c_first[kk] <= R || (visit_first && kk == 0));
                        const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
                        const int l = m ? __ffsll((long long)m) - 1 : kWave;
                        if (in && lane < l) c_state[kk] = 0;
                        if (m) { cur = base + l; found = true; break; }
                    }
                    if (!found) { cur = K; break; }
                    // (c) a cell whose first click is affordable but which does not fit as a whole is walked
                    DBG_ADD(6, 1);
                    const int k = cur;
                    const double budget_d = advance_chain(k);          // the float remaining budget at this cell's start
                    int32_t j0, n;
                    adc::cell_range(s_vol[k], t, j0, n);
                    // a cell of a few clicked wins whose prices pass A kept: the reference's in-cell loop (:97-104) from those -
                    // pay while `budget >= cost` - and the cell then stands in the table as one paid in full with only its paid
                    // clicks (pass B draws their conversions); no auction is evaluated again, nothing is loaded
                    const unsigned int n_clk = lean ? 0u : c_clicks[k];
                    const unsigned long long q4 = lean ? 0ull : c_q4[k];
                    bool simple = n <= 32 && n_clk >= 1u && n_clk <= 4u;
#pragma unroll
                    for (unsigned int i = 0; i < 4u; ++i) simple = simple && (i >= n_clk || ((q4 >> (16u * i)) & 0xFFFFull) != 0xFFFFull);
                    if (simple) {
                        double budget = budget_d, sum_d = 0.0;
                        unsigned long long cost = 0ull;
                        unsigned int paid = 0u;
#pragma unroll
                        for (unsigned int i = 0; i < 4u; ++i)
                            if (i < n_clk && paid == i) {       // (the first click that does not fit ends the cell)
                                const int price = (int)((q4 >> (16u * i)) & 0xFFFFull);
                                const double cost_d = adc::cents_to_dollars_f64(price);
                                if (budget >= cost_d) { budget -= cost_d; sum_d += cost_d; cost += (unsigned long long)price; ++paid; }
                            }
                        const double left = budget_d - sum_d;           // :225
                        if (lane == 0) {
                            unsigned int m = c_mask[k], keep = 0u;
#pragma unroll
                            for (unsigned int i = 0; i < 4u; ++i)
                                if (i < paid) { const unsigned int b = m & (0u - m); keep |= b; m ^= b; }
                            c_mask[k] = keep;
                            c_clicks[k] = paid;
                            c_total[k] = cost;
                            rs.remaining_d = left;
                            rs.chain_pos = k + 1;
                        }
                        R -= (long long)cost;
                        if (left <= 0.0) {                  // :230-233
                            stop = true;
                            for (int kk = cur + 1 + lane; kk < K; kk += kWave) c_state[kk] = 3;
                            break;
                        }
                        cur += 1;
                        continue;
                    }
                    const CellWalk cw = walk_cell_wave(key, tick, (uint32_t)k, j0, n, (int)adc::bid_to_cents(bids[(size_t)env * K + k]),
                                                       param_at(v, ADC_P_A, env, k), param_at(v, ADC_P_B, env, k),
                                                       adc::make_auction_law(param_at(v, ADC_P_BCTR, env, k)),
                                                       adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, k)),
                                                       param_at(v, ADC_P_REV_MEAN, env, k), param_at(v, ADC_P_REV_STD, env, k), budget_d, s_logtab);
                    const double left = budget_d - cw.sum_d;            // :225, left-to-right sum of the cell's paid costs
                    if (lane == 0) {
                        a_imp[k] += cw.wins;
                        a_clk[k] += cw.paid;
                        a_cost[k] += cw.cost_c;
                        a_conv[k] += cw.convs;
                        a_rev[k] += cw.rev_c;
                        c_state[k] = 2;
                        rs.remaining_d = left;
                        rs.chain_pos = k + 1;
                    }
                    R -= (long long)cw.cost_c;
                    if (left <= 0.0) {                  // :230-233, decided by the float residue as in the reference
                        stop = true;                    // campaign stop: later cells are never visited
                        for (int kk = cur + 1 + lane; kk < K; kk += kWave) c_state[kk] = 3;
                        break;
                    }
                    cur += 1;
                }
                if (!stop) advance_chain(K);            // fully paid cells after the last walked one
                if (lane == 0) { rs.remaining = R; if (stop) rs.stopped = 1; }
            }
            __syncthreads();
            R = rs.remaining;
        } else {
            R -= row_total;
            if (wv == 0) advance_chain(K);
            DBG_ADD(7, 1);
#ifdef ADC_EXP_TIMING
            __syncthreads();
            DBG_ADD(2, DBG_T() - tR);
#endif
        }
        __syncthreads();
        [[maybe_unused]] const unsigned long long tB = DBG_T();
        DBG_ADD(1, tB - tR);
        if (tid == 0) rs.remaining = R;
        // ---- pass B: commit.  Cells paid in full take their statistics as they are; each of their clicked wins
        // (a bit of the cell's mask) goes through a per-wave ring so that the conversion / revenue call runs on
        // full wavefronts (as in k_step_implicit_fast).  Cells of more than 32 auctions are re-walked instead.
        {
            unsigned int *const ring = rings + wv * kRowsRing;
            unsigned int qhead = 0, qtail = 0;
            auto resolve = [&](unsigned int pos) {
                const unsigned int ent = ring[pos & (kRowsRing - 1)];
                const unsigned int kk = ent >> 20, j = ent & 0x000FFFFFu;          // 12 bits of keyword (K <= 2048), j < 2^20
                const adc::U4 w2 = adc::draw(key, j, adc::ST_CONV, kk, tick);
                if (adc::bernoulli(w2.x, adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, kk)))) {
                    const int rv = adc::revenue_cents_tab(w2.y, param_at(v, ADC_P_REV_MEAN, env, kk), param_at(v, ADC_P_REV_STD, env, kk),
                                                          g_norm_table);
                    atomicAdd(&a_conv[kk], 1u);
                    atomicAdd(&a_rev[kk], (unsigned long long)rv);
                }
            };
            for (int kb = 0; kb < K; kb += BLOCK) {             // wave-uniform trip count
                const int k = kb + tid;
                unsigned int bits = 0;
                int j0 = 0;
                if (k < K) {
                    const unsigned char stt = c_state[k];
                    int32_t n;
                    adc::cell_range(s_vol[k], t, j0, n);
                    if (stt == 0) a_imp[k] += c_wins[k];
                    else if (stt == 1 && n <= 32) {
                        a_imp[k] += c_wins[k];
                        a_clk[k] += c_clicks[k];
                        a_cost[k] += c_total[k];
                        bits = c_mask[k];
                    } else if (stt == 1) {
                        unsigned int cv; unsigned long long rv, pc;
                        const CellStat st = walk_cell<1>(key, tick, (uint32_t)k, j0, n, (int)adc::bid_to_cents(bids[(size_t)env * K + k]),
                                                         param_at(v, ADC_P_A, env, k), param_at(v, ADC_P_B, env, k),
                                                         adc::make_auction_law(param_at(v, ADC_P_BCTR, env, k)),
                                                         adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, k)),
                                                         param_at(v, ADC_P_REV_MEAN, env, k), param_at(v, ADC_P_REV_STD, env, k), s_logtab, 0, cv, rv, pc);
                        a_imp[k] += st.wins;
                        a_clk[k] += st.clicks;
                        a_cost[k] += pc;
                        atomicAdd(&a_conv[k], cv);
                        atomicAdd(&a_rev[k], rv);
                    }
                }
                while (__any(bits != 0u)) {                            // every lane pushes its lowest remaining click
                    const bool has = bits != 0u;
                    const unsigned long long m = __ballot(has);
                    const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
                    if (has) {
                        const int i = __ffs((int)bits) - 1;
                        bits &= bits - 1u;
                        ring[(qtail + rank) & (kRowsRing - 1)] = ((unsigned int)k << 20) | (unsigned int)(j0 + i);
                    }
                    qtail += __popcll(m);
                    while (qtail - qhead >= (unsigned int)kWave) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        resolve(qhead + lane);
                        qhead += kWave;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if ((unsigned int)lane < qtail - qhead) resolve(qhead + lane);
        }
        __syncthreads();
        DBG_ADD(3, DBG_T() - tB);
        if (rs.stopped) break;
    }

    // ---- observations and the step tail (unless the env's day is finished elsewhere)
    long long pc = 0;
    for (int k = tid; k < K && !handed; k += BLOCK) {
        const size_t o = (size_t)env * K + k;
        const long long c = (long long)a_cost[k], r = (long long)a_rev[k];
        if (v.metrics_on) {
            long long old = 0;          // what the (discarded) fast pass added for this keyword, if it ran
            if (!hinted) {
                // its outputs are float32 dollars = cents / 100 correctly rounded: below 2^22 cents rint(x * 100) gives the
                // cents back exactly; a larger keyword-day (> $41,943) is resolved again without the budget instead
                const float fr = v.rev[o], fc = v.cost[o];
                if (fr < 41943.0f && fc < 41943.0f) old = (long long)__builtin_rintf(fr * 100.0f) - (long long)__builtin_rintf(fc * 100.0f);
                else {
                    unsigned int cv; unsigned long long rv, pc;
                    walk_cell<1>(key, tick, (uint32_t)k, 0, s_vol[k], (int)adc::bid_to_cents(bids[o]), param_at(v, ADC_P_A, env, k),
                                 param_at(v, ADC_P_B, env, k), adc::make_auction_law(param_at(v, ADC_P_BCTR, env, k)),
                                 adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, k)), param_at(v, ADC_P_REV_MEAN, env, k),
                                 param_at(v, ADC_P_REV_STD, env, k), s_logtab, 0, cv, rv, pc);
                    old = (long long)rv - (long long)pc;
                }
            }
            metric_add(v, o, (r - c) - old);
        }
        v.imp[o] = (int)a_imp[k];
        v.clk[o] = (int)a_clk[k];
        v.conv[o] = (int)a_conv[k];
        v.cost[o] = adc::cents_to_dollars_f32(c);
        v.rev[o] = adc::cents_to_dollars_f32(r);
        pc += r - c;
    }
    pc = wave_sum_i64(pc);
    __syncthreads();
    if (lane == 0) rs.wave_part[wv] = pc;
    __syncthreads();
    if (tid == 0 && !handed) {
        long long profit_c = 0;
        for (int i = 0; i < BLOCK / kWave; ++i) profit_c += rs.wave_part[i];
        exact_pass_epilogue(v, env, hint_in, few_clicks, was_binding, bound_t);
        step_tail(v, env, tick, true, profit_c, 0.0);
    }
    __syncthreads();                                   // everybody is done with rs / LDS of this env
    if (tid == 0) rs.cur = (int)gridDim.x + atomicAdd(&v.flag_next[parity], 1);
    __syncthreads();
    fi = rs.cur;
    DBG_ADD(4, 1);
  }   // flagged envs of this workgroup
#ifdef ADC_EXP_TIMING
  if (tid == 0) for (int i = 0; i < 8; ++i) atomicAdd(&g_dbg[i], dbg[i]);
#endif
}


// -------------------------------------------------------------------------------------------------
// k_step_rest_of_day: the rest of a budget-bound day at once (IMPLICIT, K <= 1024), for the envs k_step_exact_rows parked
// -------------------------------------------------------------------------------------------------
// After the row in which the budget bound, what is left is less than that row's clicks cost and never grows: in every later
// row a cell matters only if its first clicked win is affordable (any other cell breaks at that click, :97-104); all other
// cells just count their wins, and wins do not care about rows.  One lane per keyword runs through ALL the keyword's
// remaining auctions in whole Philox calls (a row-by-row pass spends ~460 instructions per wave on ~5 auctions per lane:
// per-cell ranges, partial calls), counts the wins by the keyword's exact word intervals (adc::win_intervals), and for the
// clicked wins inside the conservative bracket of "costs at most R" (adc::win_brackets for a bid of R + 1 cents) prices the
// FIRST clicked win of a cell, if it lies inside the conservative bracket of "costs at most R" (adc::win_brackets for a bid of
// R + 1 cents), and keeps that price per cell in LDS (a cell whose first click lies outside pays nothing whatever happens before
// it).  Wave 0 then goes through the remaining 24 x K cells in the reference's order: a cell whose first click costs at most
// what is left NOW pays at least that click and is walked from its auctions, exactly as a row's walked cell is (walk_cell_wave); a campaign stop (:230-233) ends the day there, and the wins are recounted up to the stop.  Then the
// observations and the step tail, as at the end of k_step_exact_rows.
#ifdef ADC_EXP_TIMING
// developer instrumentation (python adcraft_amd/build.py --timing; tools/exp_rows_timing.py): k_step_rest_of_day's phases in
// 10 ns ticks (lane 0 of every workgroup): pass over the auctions | of which the laws | marked cells | outputs | envs | cells
// walked | of which paid
__device__ unsigned long long g_rest_phase[20];     // 16..: at-once variant: own cells | chain | commit | envs
//     // 8..: list of the marks | k_rest_walk: before the walk | chunks resolved | whole env | slowest env
#define RDBG_ADD(slot, val) do { if (tid == 0) atomicAdd(&g_rest_phase[slot], (unsigned long long)(val)); } while (0)
#define RDBG_MAX(slot, val) do { if (tid == 0) atomicMax(&g_rest_phase[slot], (unsigned long long)(val)); } while (0)
#else
#define RDBG_ADD(slot, val) (void)0
#define RDBG_MAX(slot, val) (void)0
#endif
constexpr int kRestMaxK = 1024;      // keywords k_step_rest_of_day takes (its per-cell table is 48 B of LDS per keyword)
struct RestShared {
    long long wave_part[kRowsMaxWaves];
    long long f_R;                                                      // an env parked by k_tail_or_flag: what is left after its first row
    double f_rd;
    int stop_cell;                                                      // row * K + keyword after which the campaign stopped, or -1
    int cur;
    int mark_cnt[1][kRowsMaxWaves];                                     // PASS_ONLY: marked cells per wave
};
constexpr int kRestMarks = 1024;                                        // marked cells per 256 keywords of an env handed to k_rest_walk as a list (more: the whole table)
// dynamic LDS: 76 B per keyword (K = 1024: 76 KB, two workgroups per CU; K = 256: 19 KB)
__host__ __device__ inline size_t rest_lds_bytes(int K) { return (size_t)K * (adc::kTimesteps * 2 + 2 * 8 + 3 * 4); }

// a keyword's laws for the rest of its day, from its parameters (the pass and the recount after a stop use the same recipe)
struct RestLaws { adc::WinIntervals iv, cheap; adc::AuctionLaw law; float loc, scale; int vol, j_from; };
__device__ __forceinline__ RestLaws rest_laws(const View &v, const float *__restrict__ bids, int env, int K, const RestState &st, int k)
{
    RestLaws L;
    const size_t o = (size_t)env * K + k;
    L.vol = (int)v.rest_counts[o].w;
    int32_t n_unused;
    if (st.row < adc::kTimesteps) adc::cell_range(L.vol, st.row, L.j_from, n_unused);
    else L.j_from = L.vol;                              // (nothing of the day is left)
    const int bid_c = (int)adc::bid_to_cents(bids[o]);
    L.loc = param_at(v, ADC_P_A, env, k);
    L.scale = param_at(v, ADC_P_B, env, k);
    const float bctr = param_at(v, ADC_P_BCTR, env, k);
    L.law = adc::make_auction_law(bctr);
    // (the float64 offsets: four candidate trials side by side cost k_step_rest_of_day<false> four registers and its seventh wave)
    L.iv = adc::win_intervals<false, true>(bid_c, L.loc, L.scale, adc::bernoulli_threshold(bctr), L.law, g_log_table);
    const int cheap_bid = min(bid_c, (int)(st.R < 0x3FFFFFFFll ? (st.R > 0 ? st.R : 0) : 0x3FFFFFFFll) + 1);
    L.cheap = adc::win_brackets(cheap_bid, L.loc, L.scale, adc::bernoulli_threshold_f32(bctr)).out;
    return L;
}
// wins of auctions [a, b) of keyword k; with a table ([24][K]: per cell the price of its FIRST clicked win if that lies within the
// bracket, in cents capped at 0xFFFE; 0xFFFF: no such cell - no click, or a first click that costs more than what is left and
// ends the cell (:97-104); a cell is written by the one lane that owns its keyword, and the lane meets its auctions in order)
__device__ __forceinline__ unsigned int rest_count_wins(uint64_t key, uint32_t tick, int K, int k, const RestLaws &L, int a, int b, unsigned short *table)
{
    unsigned int w_count = 0u;
    int last_cw = -1;                                   // the latest clicked win so far (one select per auction; the rest is rare)
    auto one = [&](uint32_t word, int j) {
        const bool cw = (word - L.iv.c_lo) < L.iv.c_w;
        w_count += (unsigned int)(cw | ((word - L.iv.n_lo) < L.iv.n_w));
        if (table && cw && (word - L.cheap.c_lo) < L.cheap.c_w) {
            // (adc::cell_range: cell 0 takes the remainder, the others vol / 24 auctions each)
            const int s24 = L.vol / adc::kTimesteps, first24 = L.vol - (adc::kTimesteps - 1) * s24;
            const int row = j < first24 ? 0 : min(1 + (j - first24) / max(s24, 1), adc::kTimesteps - 1);
            const int row_start = row == 0 ? 0 : first24 + (row - 1) * s24;
            if (last_cw < row_start) {                  // the cell's first clicked win
                bool click_bit;
                const int comp = adc::auction_outcome(word, L.law, L.loc, L.scale, g_log_table, click_bit);
                table[row * K + k] = (unsigned short)min(comp, 0xFFFE);
            }
        }
        last_cw = cw ? j : last_cw;
    };
    for (int q = a >> 2; 4 * q < b; ++q) {
        const adc::U4 w = adc::draw(key, (uint32_t)q, adc::ST_AUCTION, (uint32_t)k, tick);
        if (4 * q >= a && 4 * q + 4 <= b) {             // a whole call (all but the range's first and last)
            one(w.x, 4 * q); one(w.y, 4 * q + 1); one(w.z, 4 * q + 2); one(w.w, 4 * q + 3);
        } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int j = 4 * q + h;
                if (j >= a && j < b) one(h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w, j);
            }
        }
    }
    return w_count;
}

// PASS_ONLY (1024 envs or more): the pass over the auctions alone - the marked cells go to global memory as a list in the reference's
// order (View::rest_marks; more than kRestMarks of them: the whole table, View::rest_table) and k_rest_walk does the rest with
// one wavefront per env: in one kernel wave 0 walks the marked cells (half of an env's time here) while the other three
// waves hold their registers and the workgroup its LDS.
// (workgroups per CU of the pass-only variant, measured on cfg2 with every budget binding: 4: 0.540, 5: 0.530, 6: 0.520, 8: 0.525 ms)
constexpr int kRestPassBlocks = 6;
#ifndef ADC_REST_FRESH_BLOCKS
#define ADC_REST_FRESH_BLOCKS 5
#endif
constexpr int kRestFreshBlocks = ADC_REST_FRESH_BLOCKS;        // ... of the at-once variant
// FRESH (a PASS_ONLY variant of its own: the first row costs registers the plain pass does not have): the envs k_tail_or_flag
// parked at once (View::direct_list) - their first row here, then the pass over rows 1..23.
// BLOCK: 512 lanes for keyword sets beyond 512 (48 KB of LDS at 1024 keywords: three workgroups per CU - of 256 lanes that is
// twelve wavefronts per CU for a pass that lives on latency).  (The second launch bound is wavefronts per SIMD.)
template <bool PASS_ONLY, bool FRESH = false, int BLOCK = kRowsBlock>
__global__ __launch_bounds__(BLOCK, BLOCK == 512 ? 6 : FRESH ? kRestFreshBlocks : PASS_ONLY ? kRestPassBlocks : 5) void k_step_rest_of_day(View v, const float *__restrict__ bids, int parity)
{
    static_assert(PASS_ONLY || !FRESH, "the at-once variant hands its marks to k_rest_walk");
    static_assert(BLOCK == kRowsBlock || (PASS_ONLY && !FRESH), "wider workgroups: the plain pass only");
    extern __shared__ __align__(16) unsigned char rest_raw[];
    __shared__ RestShared sh;
    const int K = v.K;
    unsigned long long *const a_cost = reinterpret_cast<unsigned long long *>(rest_raw);      // [K]
    unsigned long long *const a_rev = a_cost + K;                                              // [K]
    unsigned int *const a_clk = reinterpret_cast<unsigned int *>(a_rev + K);                   // [K]
    unsigned int *const a_conv = a_clk + K;                                                    // [K]
    int *const s_vol = reinterpret_cast<int *>(a_conv + K);                                    // [K]
    unsigned short *const cheapest = reinterpret_cast<unsigned short *>(PASS_ONLY ? (void *)rest_raw : (void *)(s_vol + K));   // [24][K], see rest_count_wins
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ adc::LogTableEntry s_logtab[FRESH ? adc::kLogTableIntervals : 1];       // FRESH: copy of g_log_table (one lookup per auction of the first row)
    if (FRESH) s_logtab[threadIdx.x] = g_log_table[threadIdx.x];
    const int n_listed = FRESH ? v.direct_count[parity] : v.rest_count[parity];
  for (int fi = blockIdx.x;;) {
    if (fi >= n_listed) break;
    const int env = FRESH ? v.direct_list[fi] : v.retry_list[fi];
    RestState st = v.rest_state[env];
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    const bool hinted = (st.flags & 1) != 0, few_clicks = (st.flags & 2) != 0;
    const int hint_in = st.flags >> 4;
    [[maybe_unused]] const unsigned long long t_r0 = DBG_T();
    if (FRESH) {
        // ---- AN ENV PARKED BY k_tail_or_flag (hint 6): nothing of its day has been looked at, and yesterday its budget ran out
        // within the first cells of the day.  What k_step_exact_rows does at the start of a day (pending drift, the volumes),
        // then the day's first row the way k_rest_walk walks a chunk of marked cells: every lane resolves its own cell (wins,
        // its first clicked wins and their prices), wave 0 runs the reference's float chain over the row in keyword order -
        // only over cells whose first click costs at most what is left then (:97-104, :225, :230-233) - and the lanes draw
        // their paid clicks' conversions.  With what is left after that row the ordinary pass takes rows 1..23.
        // (LDS: the table's space, which the pass only fills afterwards)
        constexpr unsigned int kNone = 0xFFFFFFFFu, kLook = 0xFFFFFFFEu;         // no click | a cell for the whole wavefront
#ifndef ADC_FRESH_CLICKS
#define ADC_FRESH_CLICKS 4
#endif
        // (clicked wins a lane keeps: the day's first row holds vol % 24 auctions more than the others and so more clicks per cell, but
        //  eight instead of four measured slower - 272 against 252 us on cfg2: the registers cost more than the cells sent to the wave)
        constexpr int kLaneClicks = ADC_FRESH_CLICKS, kLaneAuctions = 48;
        static_assert(kLaneClicks == 4 || kLaneClicks == 8, "two words of four prices");
        unsigned long long *const f_q4 = reinterpret_cast<unsigned long long *>(rest_raw);          // [2][K] prices of the first 8 clicked wins, 16 bits each
        unsigned long long *const c_cost = f_q4 + 2 * K, *const c_rev = c_cost + K;                // [K] whole-wavefront cells: what they paid / earned
        unsigned int *const f_first = reinterpret_cast<unsigned int *>(c_rev + K);                  // [K] price of the first clicked win
        unsigned int *const f_paid = f_first + K, *const c_conv = f_paid + K, *const c_wins = c_conv + K;    // [K] clicks << 8 | paid ...
        const bool drift = v.drift_on && v.drift_pending[env];         // (the skipped fast pass would have applied it)
        [[maybe_unused]] const unsigned long long t_f0 = DBG_T();
        const int k = tid;
        const size_t o = (size_t)env * K + (k < K ? k : 0);
        int vol = 0, f_wins = 0, n_clicks = 0, bid_c = 0;
        int q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t qj[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        bool whole = false;
        if (k < K) {
            if (drift) {
                drift_keyword_planes(v, env, key, tick - 1u, k);
            }
            vol = adc::volume_from_word(adc::volume_word(key, (uint32_t)k, tick), param_at(v, ADC_P_VOL_MEAN, env, k),
                                        param_at(v, ADC_P_VOL_STD, env, k), g_norm_table);
            int32_t j0, n;
            adc::cell_range(vol, 0, j0, n);
            bid_c = (int)adc::bid_to_cents(bids[o]);
            if (n > kLaneAuctions) whole = true;
            else {
                const float loc = param_at(v, ADC_P_A, env, k), scale = param_at(v, ADC_P_B, env, k);
                const adc::AuctionLaw law = adc::make_auction_law(param_at(v, ADC_P_BCTR, env, k));
                for (int qd = j0 >> 2; 4 * qd < j0 + n; ++qd) {
                    const adc::U4 w = adc::draw(key, (uint32_t)qd, adc::ST_AUCTION, (uint32_t)k, tick);
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const int j = 4 * qd + h;
                        if (j < j0 || j >= j0 + n) continue;
                        const uint32_t word = h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w;
                        bool click_bit;
                        const int comp = adc::auction_outcome(word, law, loc, scale, s_logtab, click_bit);
                        if (!adc::auction_wins(word, bid_c, comp)) continue;
                        ++f_wins;
                        if (click_bit) {
#pragma unroll
                            for (int i = 0; i < kLaneClicks; ++i)
                                if (n_clicks == i) { q[i] = comp; qj[i] = (uint32_t)j; }
                            whole = whole || (n_clicks < kLaneClicks && comp > 0xFFFE);
                            ++n_clicks;
                        }
                    }
                }
            }
            // (more clicked wins than a lane keeps: the cell goes to the whole wavefront only if all of those get paid)
            f_q4[k] = (unsigned long long)(unsigned int)q[0] | ((unsigned long long)(unsigned int)q[1] << 16) | ((unsigned long long)(unsigned int)q[2] << 32) |
                      ((unsigned long long)(unsigned int)q[3] << 48);
            f_q4[K + k] = (unsigned long long)(unsigned int)q[4] | ((unsigned long long)(unsigned int)q[5] << 16) | ((unsigned long long)(unsigned int)q[6] << 32) |
                          ((unsigned long long)(unsigned int)q[7] << 48);
            f_first[k] = whole ? kLook : n_clicks ? (unsigned int)q[0] : kNone;
            f_paid[k] = whole ? 0u : ((unsigned int)min(n_clicks, kLaneClicks) << 8) | (n_clicks > kLaneClicks ? 0x80000000u : 0u);
            c_conv[k] = c_wins[k] = 0u;
            c_cost[k] = c_rev[k] = 0ull;
            v.rest_counts[o].w = (unsigned int)vol;     // (walk_cell_wave below and the pass read it)
        }
        __syncthreads();
        [[maybe_unused]] const unsigned long long t_f1 = DBG_T();
        RDBG_ADD(16, t_f1 - t_f0);
        if (wv == 0) {
            long long R = st.R;
            double r_d = st.r_d;
            int stop_k = -1, cells_paid = 0;
            for (int c64 = 0; c64 < K && stop_k < 0; c64 += kWave) {
                const unsigned int mine = c64 + lane < K ? f_first[c64 + lane] : kNone;
                unsigned long long done = 0ull;
                for (;;) {
                    // the next cell, in keyword order, whose first click costs at most what is left now
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(mine != kNone && ((long long)mine <= R || mine == kLook)) & ~done;
                    if (!m) break;
                    const int l = __ffsll((long long)m) - 1;
                    done |= (2ull << l) - 1ull;
                    const int kw = c64 + l;
                    bool by_wave = (unsigned int)__builtin_amdgcn_readlane((int)mine, l) == kLook;
                    if (!by_wave) {
                        const unsigned int rec = f_paid[kw];
                        const int n_l = (int)((rec >> 8) & 0xFFu);
                        double budget = r_d, sum_d = 0.0;
                        long long cost = 0;
                        int paid = 0;
                        // (the prices in dollars by as many lanes at once: a float64 division each, not several in a row)
                        const int lane_price = (int)((f_q4[(lane & 4 ? K : 0) + kw] >> (16 * (lane & 3))) & 0xFFFFull);
                        const double lane_cost_d = adc::cents_to_dollars_f64(lane_price);
#pragma unroll
                        for (int i = 0; i < kLaneClicks; ++i)
                            if (i < n_l && paid == i) {         // (the first click that does not fit ends the cell, :97-104)
                                const int price = __builtin_amdgcn_readlane(lane_price, i);
                                const double cost_d = readlane_f64(lane_cost_d, i);
                                if (budget >= cost_d) { budget -= cost_d; sum_d += cost_d; cost += price; ++paid; }
                            }
                        if (paid == kLaneClicks && (rec & 0x80000000u)) {        // all of them paid and there are more: from its auctions
                            by_wave = true;
                            if (lane == 0) { f_first[kw] = kLook; f_paid[kw] = 0u; }
                        } else {
                            if (lane == 0) f_paid[kw] = rec | (unsigned int)paid;
                            r_d -= sum_d;               // :225
                            R -= cost;
                            cells_paid += paid ? 1 : 0;
                        }
                    }
                    if (by_wave) {
                        const size_t ok = (size_t)env * K + kw;
                        int32_t j0c, n_cell;
                        adc::cell_range((int)v.rest_counts[ok].w, 0, j0c, n_cell);
                        const CellWalk cw = walk_cell_wave(key, tick, (uint32_t)kw, j0c, n_cell, (int)adc::bid_to_cents(bids[ok]),
                                                           param_at(v, ADC_P_A, env, kw), param_at(v, ADC_P_B, env, kw),
                                                           adc::make_auction_law(param_at(v, ADC_P_BCTR, env, kw)),
                                                           adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, kw)),
                                                           param_at(v, ADC_P_REV_MEAN, env, kw), param_at(v, ADC_P_REV_STD, env, kw), r_d, g_log_table);
                        if (lane == 0) { c_wins[kw] = cw.wins; f_paid[kw] = cw.paid; c_conv[kw] = cw.convs; c_cost[kw] = cw.cost_c; c_rev[kw] = cw.rev_c; }
                        r_d -= cw.sum_d;                // :225
                        R -= (long long)cw.cost_c;
                        cells_paid += cw.paid ? 1 : 0;
                    }
                    if (r_d <= 0.0) { stop_k = kw; break; }      // :230-233: the campaign stops, later cells are never visited
                }
            }
            if (lane == 0) { sh.f_R = R; sh.f_rd = r_d; sh.stop_cell = stop_k; sh.cur = cells_paid; }
        }
        __syncthreads();
        [[maybe_unused]] const unsigned long long t_f2 = DBG_T();
        RDBG_ADD(17, t_f2 - t_f1);
        const int stop_k = sh.stop_cell;
        long long pc = 0;
        if (k < K) {
            unsigned int imp, clk, convs = 0u;
            unsigned long long cost_c = 0ull, rev_c = 0ull;
            if (f_first[k] == kLook) { imp = c_wins[k]; clk = f_paid[k]; convs = c_conv[k]; cost_c = c_cost[k]; rev_c = c_rev[k]; }
            else {
                imp = stop_k >= 0 && k > stop_k ? 0u : (unsigned int)f_wins;        // (a cell after the stop is never visited)
                clk = f_paid[k] & 0xFFu;
                if (clk) {                              // the paid clicks' conversions and revenues
                    const unsigned long long t_conv = adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, k));
                    const float mu = param_at(v, ADC_P_REV_MEAN, env, k), sd = param_at(v, ADC_P_REV_STD, env, k);
#pragma unroll
                    for (int i = 0; i < kLaneClicks; ++i)
                        if ((unsigned int)i < clk) {
                            const adc::U4 w2 = adc::draw(key, qj[i], adc::ST_CONV, (uint32_t)k, tick);
                            if (adc::bernoulli(w2.x, t_conv)) {
                                ++convs;
                                rev_c += (unsigned long long)adc::revenue_cents_tab(w2.y, mu, sd, g_norm_table);
                            }
                            cost_c += (unsigned long long)q[i];
                        }
                }
            }
            v.rest_counts[o] = make_uint4(imp, clk, convs, (unsigned int)vol);
            v.rest_cost[o] = (long long)cost_c;
            v.rest_rev[o] = (long long)rev_c;
            if (v.metrics_on) metric_add(v, o, (long long)rev_c - (long long)cost_c);
            v.clk[o] = (int)clk;
            v.conv[o] = (int)convs;
            v.cost[o] = adc::cents_to_dollars_f32((long long)cost_c);
            v.rev[o] = adc::cents_to_dollars_f32((long long)rev_c);
            pc = (long long)rev_c - (long long)cost_c;
        }
        pc = wave_sum_i64(pc);
        if (lane == 0) sh.wave_part[wv] = pc;
        __syncthreads();
        st.R = sh.f_R;
        st.r_d = sh.f_rd;
        st.row = stop_k >= 0 ? adc::kTimesteps : 1;     // (a campaign that stopped: nothing of the day is left)
        st.flags = (st.flags & ~(4 | 8)) | (sh.cur <= K / 4 + 1 ? 8 : 0);          // (bit 3: at once again tomorrow - few cells paid)
        st.pc = 0;
        for (int i = 0; i < BLOCK / kWave; ++i) st.pc += sh.wave_part[i];
        if (tid == 0) v.rest_state[env] = st;
        __syncthreads();                                // (the table's space is free again)
        RDBG_ADD(18, DBG_T() - t_f2);
        RDBG_ADD(19, 1);
    }
    for (int i = tid; i < adc::kTimesteps * K; i += BLOCK) cheapest[i] = 0xFFFFu;
    if (tid == 0) sh.stop_cell = -1;
    __syncthreads();
    // ---- every keyword's remaining auctions: wins, and the cells that may hold an affordable click
    for (int k = tid; k < K; k += BLOCK) {
        const size_t o = (size_t)env * K + k;
        const uint4 c = v.rest_counts[o];
        if (!PASS_ONLY) {
            a_clk[k] = c.y;
            a_conv[k] = c.z;
            a_cost[k] = (unsigned long long)v.rest_cost[o];
            a_rev[k] = (unsigned long long)v.rest_rev[o];
        }
        [[maybe_unused]] const unsigned long long t_l0 = DBG_T();
        const RestLaws L = rest_laws(v, bids, env, K, st, k);
        RDBG_ADD(1, DBG_T() - t_l0);
        if (!PASS_ONLY) s_vol[k] = L.vol;
        // (the impressions so far + the rest of the day's wins; corrected later if the campaign stops)
        const unsigned int imp_all = c.x + rest_count_wins(key, tick, K, k, L, L.j_from, L.vol, cheapest);
        // (k_rest_walk: the observation itself; the parked count stays, for a campaign that stops early - see there)
        if (PASS_ONLY) v.imp[o] = (int)imp_all; else v.rest_counts[o].x = imp_all;
    }
    __syncthreads();
    [[maybe_unused]] const unsigned long long t_r1 = DBG_T();
    RDBG_ADD(0, t_r1 - t_r0);
    RDBG_ADD(4, 1);
    if (PASS_ONLY) {
        // the marked cells as a list in the reference's order (sub-timestep by sub-timestep, keyword by keyword): a thread takes
        // a run of consecutive cells of that order, counts its marks, and a scan over the workgroup gives it its place
        // (thread = keyword and a ballot per sub-timestep was 48 dependent LDS round trips per env)
        const int n_cells = adc::kTimesteps * K, per_thread = (n_cells + BLOCK - 1) / BLOCK;
        const int c_from = tid * per_thread, c_to = min(c_from + per_thread, n_cells);
        int mine = 0;
        for (int i = c_from; i < c_to; ++i) mine += cheapest[i] != 0xFFFFu ? 1 : 0;
        const int incl = wave_scan_i32(mine);
        if (lane == kWave - 1) sh.mark_cnt[0][wv] = incl;
        __syncthreads();
        int base = 0, pos = incl - mine;
        for (int w = 0; w < BLOCK / kWave; ++w) {
            const int n_w = sh.mark_cnt[0][w];
            pos += w < wv ? n_w : 0;
            base += n_w;
        }
        if (mine && base <= v.rest_marks_cap)
            for (int i = c_from; i < c_to; ++i) {
                const unsigned int c16 = cheapest[i];
                if (c16 != 0xFFFFu) v.rest_marks[(size_t)env * v.rest_marks_stride + pos++] = ((unsigned int)i << 16) | c16;
            }
        if (tid == 0) v.rest_nmarks[env] = base <= v.rest_marks_cap ? base : -1;
        RDBG_ADD(8, DBG_T() - t_r1);
        if (base > v.rest_marks_cap) {                         // (rare: the table itself)
            unsigned int *const out = reinterpret_cast<unsigned int *>(v.rest_table + (size_t)env * adc::kTimesteps * K);
            const unsigned int *const in = reinterpret_cast<const unsigned int *>(cheapest);
            for (int i = tid; i < adc::kTimesteps * K / 2; i += BLOCK) out[i] = in[i];
        }
    } else {
    // ---- the marked cells in the reference's order (wave 0; every lane carries the same scalars)
    if (wv == 0) {
        long long R = st.R;
        double r_d = st.r_d;
        bool stop = false;
        for (int row = st.row; row < adc::kTimesteps && !stop; ++row)
            for (int c64 = 0; c64 < K && !stop; c64 += kWave) {
                const unsigned int mine = c64 + lane < K ? (unsigned int)cheapest[row * K + c64 + lane] : 0xFFFFu;
                unsigned long long done = 0ull;             // lanes (cells) of this chunk already passed
                for (;;) {
                    // the next cell, in keyword order, whose cheapest click costs at most what is left now (a capped price: look)
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(mine != 0xFFFFu && ((long long)mine <= R || mine == 0xFFFEu)) & ~done;
                    if (!m) break;
                    const int l = __ffsll((long long)m) - 1;
                    done |= (2ull << l) - 1ull;
                    const int kw = c64 + l;
                    int32_t j0c, n_cell;
                    adc::cell_range(s_vol[kw], row, j0c, n_cell);
                    const CellWalk cw = walk_cell_wave(key, tick, (uint32_t)kw, j0c, n_cell, (int)adc::bid_to_cents(bids[(size_t)env * K + kw]),
                                                       param_at(v, ADC_P_A, env, kw), param_at(v, ADC_P_B, env, kw),
                                                       adc::make_auction_law(param_at(v, ADC_P_BCTR, env, kw)),
                                                       adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, kw)),
                                                       param_at(v, ADC_P_REV_MEAN, env, kw), param_at(v, ADC_P_REV_STD, env, kw), r_d, g_log_table);
                    RDBG_ADD(5, 1);
                    RDBG_ADD(6, cw.paid ? 1 : 0);
                    if (lane == 0) {                    // (the cell's wins are counted already)
                        a_clk[kw] += cw.paid;
                        a_cost[kw] += cw.cost_c;
                        a_conv[kw] += cw.convs;
                        a_rev[kw] += cw.rev_c;
                    }
                    r_d -= cw.sum_d;                    // :225
                    R -= (long long)cw.cost_c;
                    if (r_d <= 0.0) {                   // :230-233: the campaign stops, later cells are never visited
                        if (lane == 0) sh.stop_cell = row * K + kw;
                        stop = true;
                        break;
                    }
                }
            }
    }
    __syncthreads();
    [[maybe_unused]] const unsigned long long t_r2 = DBG_T();
    RDBG_ADD(2, t_r2 - t_r1);
    // ---- observations and the step tail (as at the end of k_step_exact_rows)
    long long pc = 0;
    const int stop_cell = sh.stop_cell;
    for (int k = tid; k < K; k += BLOCK) {
        const size_t o = (size_t)env * K + k;
        unsigned int imp = v.rest_counts[o].x;
        if (stop_cell >= 0) {                           // only the cells up to the stop count: take the later wins off again
            const int vrow = stop_cell / K + (k <= stop_cell % K ? 1 : 0);
            if (vrow < adc::kTimesteps) {
                const RestLaws L = rest_laws(v, bids, env, K, st, k);
                int32_t j_to, n_unused;
                adc::cell_range(L.vol, vrow, j_to, n_unused);
                imp -= rest_count_wins(key, tick, K, k, L, j_to, L.vol, nullptr);
            }
        }
        const long long c = (long long)a_cost[k], r = (long long)a_rev[k];
        if (v.metrics_on) {
            // what the (discarded) fast pass added for this keyword, if it ran (below 2^22 cents: checked before the hand-over)
            const long long old = hinted ? 0ll : (long long)__builtin_rintf(v.rev[o] * 100.0f) - (long long)__builtin_rintf(v.cost[o] * 100.0f);
            metric_add(v, o, (r - c) - old);
        }
        v.imp[o] = (int)imp;
        v.clk[o] = (int)a_clk[k];
        v.conv[o] = (int)a_conv[k];
        v.cost[o] = adc::cents_to_dollars_f32(c);
        v.rev[o] = adc::cents_to_dollars_f32(r);
        pc += r - c;
    }
    pc = wave_sum_i64(pc);
    if (lane == 0) sh.wave_part[wv] = pc;
    __syncthreads();
    if (tid == 0) {
        long long profit_c = 0;
        for (int i = 0; i < BLOCK / kWave; ++i) profit_c += sh.wave_part[i];
        exact_pass_epilogue(v, env, hint_in, few_clicks, true, st.row - 1);
        step_tail(v, env, tick, true, profit_c, 0.0);
    }
    RDBG_ADD(3, DBG_T() - t_r2);
    }   // !PASS_ONLY
    __syncthreads();                                   // everybody is done with this env's LDS
    if (tid == 0) sh.cur = (int)gridDim.x + atomicAdd(FRESH ? &v.direct_next[parity] : &v.rest_next[parity], 1);
    __syncthreads();
    fi = sh.cur;
  }
}

// wins of auctions [a, b) of keyword k, auction by auction (no interval records: ~65 instructions per auction against ~700 per
// keyword + ~23 per auction through rest_laws / rest_count_wins - for a few auctions)
__device__ __forceinline__ unsigned int count_wins_direct(const View &v, const float *__restrict__ bids, uint64_t key, uint32_t tick, int env, int K, int k, int a, int b)
{
    const size_t o = (size_t)env * K + k;
    const int bid_c = (int)adc::bid_to_cents(bids[o]);
    const float loc = param_at(v, ADC_P_A, env, k), scale = param_at(v, ADC_P_B, env, k);
    const adc::AuctionLaw law = adc::make_auction_law(param_at(v, ADC_P_BCTR, env, k));
    unsigned int wins = 0u;
    for (int q = a >> 2; 4 * q < b; ++q) {
        const adc::U4 w = adc::draw(key, (uint32_t)q, adc::ST_AUCTION, (uint32_t)k, tick);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int j = 4 * q + h;
            if (j < a || j >= b) continue;
            const uint32_t word = h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w;
            bool click_bit;
            const int comp = adc::auction_outcome(word, law, loc, scale, g_log_table, click_bit);
            wins += adc::auction_wins(word, bid_c, comp) ? 1u : 0u;
        }
    }
    return wins;
}

// k_rest_walk (K <= 1024): the second half of k_step_rest_of_day<true> - one wavefront per parked env, so that a CU walks dozens
// of envs' marked cells at a time instead of a workgroup's wave 0 walking one.  The day's observations so far are in place
// (k_step_exact_rows at the hand-over, the impressions by k_step_rest_of_day); the few cells that still pay add to their
// keywords' counts and parked sums by atomics (this wavefront alone touches the env), and only those keywords' cost and
// revenue observations are written again; then the step tail.
constexpr int kRestTouched = 254;
struct RestWalkShared {
    unsigned int n_touched;                             // keywords that paid (beyond kRestTouched: every keyword is written again)
    unsigned short touched[kRestTouched];
};
__global__ __launch_bounds__(kWave, 4) void k_rest_walk(View v, const float *__restrict__ bids, const float *__restrict__ budget_in, int parity, int direct_follows)
{
    __shared__ RestWalkShared ws;
    const int K = v.K;
    const int lane = threadIdx.x;
    [[maybe_unused]] const int tid = lane;
    // (the envs k_step_exact_rows parked, then those k_tail_or_flag did)
    const int n_parked = v.rest_count[parity];
    const int n_listed = n_parked + (direct_follows ? v.direct_count[parity] : 0);
  for (int fi = blockIdx.x;;) {
    if (fi >= n_listed) break;
    [[maybe_unused]] const unsigned long long t_e0 = DBG_T();
    const int env = fi < n_parked ? v.retry_list[fi] : v.direct_list[fi - n_parked];
    const RestState st = v.rest_state[env];
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    const bool few_clicks = (st.flags & 2) != 0;
    const int hint_in = st.flags >> 4;
    // ---- the marked cells in the reference's order (every lane carries the same scalars)
    [[maybe_unused]] const unsigned long long t_w0 = DBG_T();
    long long R = st.R;
    double r_d = st.r_d;
    int stop_cell = -1;
    int cells_paid = 0;                                 // cells that paid a click (what the walk of this day cost)
    long long my_pc = 0;                                // what this lane's paid clicks earned - cost, cents
    if (lane == 0) ws.n_touched = 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // a lane's cell paid: its keyword's counts (the observations themselves), parked sums and metric word, by atomics
    auto pay = [&](int kw, unsigned int paid, unsigned int convs, unsigned long long cost_c, unsigned long long rev_c) {
        const size_t o = (size_t)env * K + kw;
        atomicAdd(&v.clk[o], (int)paid);
        if (convs) atomicAdd(&v.conv[o], (int)convs);
        atomicAdd(reinterpret_cast<unsigned long long *>(&v.rest_cost[o]), cost_c);
        if (rev_c) atomicAdd(reinterpret_cast<unsigned long long *>(&v.rest_rev[o]), rev_c);
        if (v.metrics_on) atomicAdd(reinterpret_cast<unsigned long long *>(&v.metric_hi[o]), rev_c - cost_c);      // (metric_total: spill + word)
        my_pc += (long long)rev_c - (long long)cost_c;
        const unsigned int slot = atomicAdd(&ws.n_touched, 1u);
        if (slot < (unsigned int)kRestTouched) ws.touched[slot] = (unsigned short)kw;
    };
    // one cell by the whole wavefront (cells of many auctions or more than kLaneClicks clicked wins)
    auto walk_whole = [&](int the_cell) {
        const int row = the_cell / K, kw = the_cell - row * K;
        const size_t o = (size_t)env * K + kw;
        int32_t j0c, n_cell;
        adc::cell_range((int)v.rest_counts[o].w, row, j0c, n_cell);
        const CellWalk cw = walk_cell_wave(key, tick, (uint32_t)kw, j0c, n_cell, (int)adc::bid_to_cents(bids[o]),
                                           param_at(v, ADC_P_A, env, kw), param_at(v, ADC_P_B, env, kw),
                                           adc::make_auction_law(param_at(v, ADC_P_BCTR, env, kw)),
                                           adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, kw)),
                                           param_at(v, ADC_P_REV_MEAN, env, kw), param_at(v, ADC_P_REV_STD, env, kw), r_d, g_log_table);
        if (lane == 0 && cw.paid) {                     // (the cell's wins are counted already)
            pay(kw, cw.paid, cw.convs, cw.cost_c, cw.rev_c);
        }
        r_d -= cw.sum_d;                                // :225
        R -= (long long)cw.cost_c;
        cells_paid += cw.paid ? 1 : 0;
    };
    // Up to 64 marked cells in order, one per lane (c16: the cell's cheapest click, 0xFFFF: no cell).  What a cell's auctions
    // are does not depend on the money left, only which of its clicks get paid does: every lane resolves its own cell first
    // (its clicked wins in auction order), the wave then runs the reference's float chain over the cells in order from those
    // lists (:97-104, :225), and the lanes draw the paid clicks' conversions.
    constexpr int kLaneClicks = 4, kLaneAuctions = 48;
    auto walk_chunk = [&](unsigned int c16, int cell) {
        // (what is left only shrinks: a cell whose cheapest click does not fit now never will)
        const bool has = c16 != 0xFFFFu && ((long long)c16 <= R || c16 == 0xFFFEu);
        if (!__builtin_amdgcn_ballot_w64(has)) return;
        RDBG_ADD(10, 1);
        [[maybe_unused]] const unsigned long long t_c0 = DBG_T();
        int q[kLaneClicks] = {0, 0, 0, 0};              // prices of the cell's clicked wins, cents
        uint32_t qj[kLaneClicks] = {0u, 0u, 0u, 0u};    // and their auctions
        int n_clicks = 0, kw = 0;
        bool whole = false;
        size_t o = (size_t)env * K;
        if (has) {
            const int row = cell / K;
            kw = cell - row * K;
            o += kw;
            int32_t j0, n;
            adc::cell_range((int)v.rest_counts[o].w, row, j0, n);
            if (n > kLaneAuctions) whole = true;
            else {
                const int bid_c = (int)adc::bid_to_cents(bids[o]);
                const float loc = param_at(v, ADC_P_A, env, kw), scale = param_at(v, ADC_P_B, env, kw);
                const adc::AuctionLaw law = adc::make_auction_law(param_at(v, ADC_P_BCTR, env, kw));
                for (int qd = j0 >> 2; 4 * qd < j0 + n; ++qd) {
                    const adc::U4 w = adc::draw(key, (uint32_t)qd, adc::ST_AUCTION, (uint32_t)kw, tick);
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const int j = 4 * qd + h;
                        if (j < j0 || j >= j0 + n) continue;
                        const uint32_t word = h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w;
                        bool click_bit;
                        const int comp = adc::auction_outcome(word, law, loc, scale, g_log_table, click_bit);
                        if (click_bit && adc::auction_wins(word, bid_c, comp)) {
#pragma unroll
                            for (int i = 0; i < kLaneClicks; ++i)
                                if (n_clicks == i) { q[i] = comp; qj[i] = (uint32_t)j; }
                            ++n_clicks;
                        }
                    }
                }
                whole = n_clicks > kLaneClicks;
            }
        }
        int my_paid = 0;
        unsigned long long done = 0ull;                 // lanes (cells) of this chunk already passed
        [[maybe_unused]] const unsigned long long t_c1 = DBG_T();
        RDBG_ADD(13, t_c1 - t_c0);
        for (;;) {
            // the next cell whose cheapest click costs at most what is left now (a capped price: look)
            const unsigned long long m = __builtin_amdgcn_ballot_w64(has && ((long long)c16 <= R || c16 == 0xFFFEu)) & ~done;
            if (!m) break;
            const int l = __ffsll((long long)m) - 1;
            done |= (2ull << l) - 1ull;
            const int the_cell = __builtin_amdgcn_readlane(cell, l);
            if (__builtin_amdgcn_readlane((int)whole, l)) walk_whole(the_cell);
            else {
                const int n_l = __builtin_amdgcn_readlane(n_clicks, l);
                double budget = r_d, sum_d = 0.0;
                long long cost = 0;
                int paid = 0;
#pragma unroll
                for (int i = 0; i < kLaneClicks; ++i)
                    if (i < n_l && paid == i) {         // (the first click that does not fit ends the cell, :97-104)
                        const int price = __builtin_amdgcn_readlane(q[i], l);
                        const double cost_d = adc::cents_to_dollars_f64(price);
                        if (budget >= cost_d) { budget -= cost_d; sum_d += cost_d; cost += price; ++paid; }
                    }
                if (lane == l) my_paid = paid;
                r_d -= sum_d;                           // :225
                R -= cost;
                cells_paid += paid ? 1 : 0;
            }
            if (r_d <= 0.0) { stop_cell = the_cell; break; }          // :230-233: the campaign stops, later cells are never visited
        }
        [[maybe_unused]] const unsigned long long t_c2 = DBG_T();
        RDBG_ADD(14, t_c2 - t_c1);
        if (my_paid) {                                  // the paid clicks' conversions and revenues, and the cell's sums
            const unsigned long long t_conv = adc::bernoulli_threshold(param_at(v, ADC_P_SCTR, env, kw));
            const float mu = param_at(v, ADC_P_REV_MEAN, env, kw), sd = param_at(v, ADC_P_REV_STD, env, kw);
            unsigned int convs = 0u;
            unsigned long long cost_c = 0ull, rev_c = 0ull;
#pragma unroll
            for (int i = 0; i < kLaneClicks; ++i)
                if (i < my_paid) {
                    const adc::U4 w2 = adc::draw(key, qj[i], adc::ST_CONV, (uint32_t)kw, tick);
                    if (adc::bernoulli(w2.x, t_conv)) {
                        ++convs;
                        rev_c += (unsigned long long)adc::revenue_cents_tab(w2.y, mu, sd, g_norm_table);
                    }
                    cost_c += (unsigned long long)q[i];
                }
            pay(kw, (unsigned int)my_paid, convs, cost_c, rev_c);        // (two cells of a chunk can be one keyword's)
        }
        RDBG_ADD(15, DBG_T() - t_c2);
    };
    const int n_marks = v.rest_nmarks[env];
    if (n_marks >= 0) {
        unsigned int e_next = lane < n_marks ? v.rest_marks[(size_t)env * v.rest_marks_stride + lane] : 0xFFFFu;
        for (int b0 = 0; b0 < n_marks && stop_cell < 0; b0 += kWave) {
            const unsigned int e = e_next;
            e_next = b0 + kWave + lane < n_marks ? v.rest_marks[(size_t)env * v.rest_marks_stride + b0 + kWave + lane] : 0xFFFFu;
            walk_chunk(e & 0xFFFFu, (int)(e >> 16));
        }
    } else {
        // (more marks than the list holds: the table itself, 256 cells of a sub-timestep at a time - four per lane, the next
        //  stretch's loads under way - and chunk by chunk only where some cell's first click fits what is left now; this env is
        //  the step's slowest)
        const unsigned short *const tab = v.rest_table + (size_t)env * adc::kTimesteps * K;
        const int stretches = (K + 255) / 256, n_rt = adc::kTimesteps * stretches;
        auto load_stretch = [&](int rt, unsigned int (&c)[4]) {
            const int row = rt / stretches, k0 = (rt - row * stretches) * 256;
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = rt < n_rt && k0 + 4 * lane + i < K ? (unsigned int)tab[row * K + k0 + 4 * lane + i] : 0xFFFFu;
        };
        unsigned int nxt[4];
        load_stretch(st.row * stretches, nxt);
        for (int rt = st.row * stretches; rt < n_rt && stop_cell < 0; ++rt) {
            unsigned int cur4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) cur4[i] = nxt[i];
            load_stretch(rt + 1, nxt);
            bool any = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) any = any || (cur4[i] != 0xFFFFu && ((long long)cur4[i] <= R || cur4[i] == 0xFFFEu));
            if (!__builtin_amdgcn_ballot_w64(any)) continue;
            const int row = rt / stretches, k0 = (rt - row * stretches) * 256;
            for (int c64 = k0; c64 < min(k0 + 256, K) && stop_cell < 0; c64 += kWave)
                walk_chunk(c64 + lane < K ? (unsigned int)tab[row * K + c64 + lane] : 0xFFFFu, row * K + c64 + lane);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    [[maybe_unused]] const unsigned long long t_w1 = DBG_T();
    // ---- the keywords whose cells paid: their cost and revenue observations again (from the parked sums); a campaign that stopped:
    // the later wins off again; the step tail
    {
        const unsigned int n_t = ws.n_touched;
        auto refresh = [&](int k) {
            const size_t o = (size_t)env * K + k;
            v.cost[o] = adc::cents_to_dollars_f32(__hip_atomic_load(&v.rest_cost[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            v.rev[o] = adc::cents_to_dollars_f32(__hip_atomic_load(&v.rest_rev[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        };
        if (n_t <= (unsigned int)kRestTouched) { for (unsigned int i = lane; i < n_t; i += kWave) refresh((int)ws.touched[i]); }
        else for (int k = lane; k < K; k += kWave) refresh(k);
    }
    for (int k = lane; k < K && stop_cell >= 0; k += kWave) {
        const size_t o = (size_t)env * K + k;
        if (stop_cell >= 0) {
            // A campaign that stopped: only the cells up to the stop count.  Either the wins after it come off the day's total
            // again, or - a stop early in what was left of the day, the usual case with a small budget - the few cells before
            // it are added to the parked count, auction by auction: this wavefront does the env's 256 keywords alone, and the
            // step waits for the slowest env.
            const int vrow = stop_cell / K + (k <= stop_cell % K ? 1 : 0);        // this keyword's first cell that does not count
            if (vrow < adc::kTimesteps) {
                const int vol = (int)v.rest_counts[o].w;
                int32_t j_from, j_to, n_unused;
                adc::cell_range(vol, st.row, j_from, n_unused);
                adc::cell_range(vol, vrow, j_to, n_unused);
                if (65 * (j_to - j_from) <= 700 + 23 * (vol - j_to))
                    v.imp[o] = (int)(v.rest_counts[o].x + count_wins_direct(v, bids, key, tick, env, K, k, j_from, j_to));
                else {
                    const RestLaws L = rest_laws(v, bids, env, K, st, k);
                    v.imp[o] = v.imp[o] - (int)rest_count_wins(key, tick, K, k, L, j_to, L.vol, nullptr);
                }
            }
        }
    }
    const long long pc = st.pc + wave_sum_i64(my_pc);
    if (lane == 0) {
        // tomorrow at once (hint 6), without the row kernel: a day that was parked so today and paid few cells, or one whose budget
        // ran out within the first cells of its first row
        const bool direct = v.direct_list != nullptr && (st.flags & 8) != 0 && cells_paid <= 128;
        exact_pass_epilogue(v, env, hint_in, few_clicks, true, max(st.row - 1, 0), direct ? adc::budget_to_cents(budget_in[env]) : -1ll);
        step_tail(v, env, tick, true, pc, 0.0);
    }
    [[maybe_unused]] const unsigned long long t_w2 = DBG_T();
    RDBG_ADD(2, t_w1 - t_w0);       // (the timers' own atomics last: the wave waits for them at its fence otherwise)
    RDBG_ADD(3, t_w2 - t_w1);
    RDBG_ADD(6, n_marks < 0 ? 100000 : n_marks);
    RDBG_ADD(9, t_w0 - t_e0);
    RDBG_ADD(11, t_w2 - t_e0);
    RDBG_MAX(12, t_w2 - t_e0);
    fi += (int)gridDim.x;        // (no ticket counter: thousands of waves asking one word for a ticket wait ~12 ns each, in turn)
  }
}
