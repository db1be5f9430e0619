// law.inc (part of adc_shims.cpp) - the auction law in word space on the host (adc_law.h: the code the step kernels run): the win intervals and their
// brackets, the win bounds, the offsets, dead keywords; with the host's log table and the thread helper the wide twins share.
// The word-space form of the 2nd-price clearing used by k_step_implicit_fast, evaluated on the host (same code,
// adc_law.h): for a keyword (bid, competitor law, click rate) the auction word w is a clicked win iff
// (w - out[0]) < out[1] and an unclicked win iff (w - out[2]) < out[3] in unsigned 32-bit arithmetic.  Diagnostic entry
// point: lets a caller (and tests/test_abi_and_host.py) check the thresholds against auction-by-auction resolution
// (adcraft/synthetic_kw_helpers.py:116-180 on the sampled competitor bid) without a GPU.
static const adc::LogTableEntry *host_log_table()
{
    static adc::LogTableEntry table[adc::kLogTableIntervals];
    static bool ready = false;
    if (!ready) {
        for (int i = 0; i < adc::kLogTableIntervals; ++i) table[i] = adc::log_table_entry(i);
        ready = true;
    }
    return table;
}

ADC_EXPORT int adc_auction_word_intervals(float bid, float cost_loc, float cost_scale, float buyside_ctr, uint32_t *out4)
{
    if (!out4) return ADC_EINVAL;
    const adc::LogTableEntry *table = host_log_table();
    const adc::AuctionLaw law = adc::make_auction_law(buyside_ctr);
    const adc::WinIntervals r = adc::win_intervals((int32_t)adc::bid_to_cents(bid), cost_loc, cost_scale,
                                                   adc::bernoulli_threshold(buyside_ctr), law, table);
    out4[0] = r.c_lo; out4[1] = r.c_w; out4[2] = r.n_lo; out4[3] = r.n_w;
    return ADC_OK;
}

// The conservative brackets of those two intervals that k_step_implicit_sparse classifies auctions with (adc_law.h
// win_brackets): out8 = {outer c_lo, c_w, n_lo, n_w, inner c_lo, c_w, n_lo, n_w}.  Host evaluation of the same code (the
// device's exp2 / rcp differ in the last bits; both stay inside the slack - adc_engine_debug_win_brackets is the device's).
ADC_EXPORT int adc_auction_word_brackets(float bid, float cost_loc, float cost_scale, float buyside_ctr, uint32_t *out8)
{
    if (!out8) return ADC_EINVAL;
    const adc::WinBrackets b = adc::win_brackets((int32_t)adc::bid_to_cents(bid), cost_loc, cost_scale, adc::bernoulli_threshold_f32(buyside_ctr));
    out8[0] = b.out.c_lo; out8[1] = b.out.c_w; out8[2] = b.out.n_lo; out8[3] = b.out.n_w;
    out8[4] = b.in.c_lo; out8[5] = b.in.c_w; out8[6] = b.in.n_lo; out8[7] = b.in.n_w;
    return ADC_OK;
}

// [lo, lo + w) as a pair of 64-bit ends; an empty interval has w == 0
static inline bool interval_inside(uint32_t a_lo, uint32_t a_w, uint32_t b_lo, uint32_t b_w)
{
    if (a_w == 0u) return true;
    return b_w != 0u && a_lo >= b_lo && (uint64_t)a_lo + a_w <= (uint64_t)b_lo + b_w;
}

// Checks inner subset-of exact subset-of outer for n keywords; brackets8 == NULL: the host's own win_brackets, otherwise the given
// ones (8 words per keyword, e.g. computed on the device).  Returns the number of keywords that violate an inclusion
// (first_bad = index of the first, or -1); *ambiguous_words (optional) = total width of the in-between zones, the
// long-way share of the stream.
ADC_EXPORT int64_t adc_check_win_brackets(int64_t n, const float *bid, const float *cost_loc, const float *cost_scale, const float *buyside_ctr,
                                          const uint32_t *brackets8, int64_t *first_bad, double *ambiguous_words)
{
    if (n < 0 || !bid || !cost_loc || !cost_scale || !buyside_ctr) return -1;
    const adc::LogTableEntry *table = host_log_table();
    int64_t bad = 0, first = -1;
    double amb = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t bid_c = (int32_t)adc::bid_to_cents(bid[i]);
        const adc::AuctionLaw law = adc::make_auction_law(buyside_ctr[i]);
        const adc::WinIntervals x = adc::win_intervals(bid_c, cost_loc[i], cost_scale[i], adc::bernoulli_threshold(buyside_ctr[i]), law, table);
        adc::WinBrackets b;
        if (brackets8) {
            const uint32_t *p = brackets8 + 8 * i;
            b.out = adc::WinIntervals{p[0], p[1], p[2], p[3]};
            b.in = adc::WinIntervals{p[4], p[5], p[6], p[7]};
        } else {
            b = adc::win_brackets(bid_c, cost_loc[i], cost_scale[i], adc::bernoulli_threshold_f32(buyside_ctr[i]));
        }
        const bool ok = interval_inside(b.in.c_lo, b.in.c_w, x.c_lo, x.c_w) && interval_inside(x.c_lo, x.c_w, b.out.c_lo, b.out.c_w) &&
                        interval_inside(b.in.n_lo, b.in.n_w, x.n_lo, x.n_w) && interval_inside(x.n_lo, x.n_w, b.out.n_lo, b.out.n_w) &&
                        (uint64_t)b.out.c_lo + b.out.c_w <= 0xFFFFFFFFull && (uint64_t)b.out.n_lo + b.out.n_w <= 0xFFFFFFFFull;
        if (!ok) { if (first < 0) first = i; ++bad; }
        amb += ((double)b.out.c_w - (double)b.in.c_w) + ((double)b.out.n_w - (double)b.in.n_w);
    }
    if (first_bad) *first_bad = first;
    if (ambiguous_words) *ambiguous_words = amb;
    return bad;
}

// ---- the win bounds of a keyword on the host: adc_law.h lower_bound_v (window, three accepting evaluations, neighbourhood,
// bisection) next to lower_bound_v_bisect (the verified-window bisection alone: the reference), for tests/test_win_bound_host.py
// one step of a splitmix64 stream: advances s, returns its next 64 bits (the twins' random words)
static inline uint64_t shim_splitmix64(uint64_t &s)
{
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <typename F>
static void shim_parallel_for(int64_t n, F body)          // body(i0, i1) on up to 8 threads
{
    const int T = n < 4096 ? 1 : 8;
    std::vector<std::thread> threads;
    for (int t = 0; t < T; ++t) threads.emplace_back([=]() { body(n * t / T, n * (t + 1) / T); });
    for (auto &th : threads) th.join();
}

ADC_EXPORT int adc_lower_bound_v_host(int64_t n, const int32_t *target, const float *loc, const float *scale, uint32_t *v_out, uint8_t *stage_out)
{
    if (n < 0 || (n > 0 && (!target || !loc || !scale || !v_out))) return ADC_EINVAL;
    const adc::LogTableEntry *table = host_log_table();
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            int stage = 0;
            v_out[i] = adc::lower_bound_v_staged(target[i], loc[i], scale[i], table, stage);
            if (stage_out) stage_out[i] = (uint8_t)stage;
        }
    });
    return ADC_OK;
}

ADC_EXPORT int adc_lower_bound_v_bisect_host(int64_t n, const int32_t *target, const float *loc, const float *scale, uint32_t *v_out,
                                             uint8_t *whole_range_out)
{
    if (n < 0 || (n > 0 && (!target || !loc || !scale || !v_out))) return ADC_EINVAL;
    const adc::LogTableEntry *table = host_log_table();
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            bool whole = false;
            v_out[i] = adc::lower_bound_v_bisect(target[i], loc[i], scale[i], table, &whole);
            if (whole_range_out) whole_range_out[i] = whole ? 1 : 0;
        }
    });
    return ADC_OK;
}

// adc::offset_reaching for n triples (range <= 2^32 as uint64).  path_out (nullable): adc::OffsetPath, 0 = the verified float32
// candidate, 1 = the float64 routine
ADC_EXPORT int adc_offset_reaching_host(int64_t n, const uint32_t *W, const uint32_t *m, const uint64_t *range, uint64_t *d_out, uint8_t *path_out)
{
    if (n < 0 || (n > 0 && (!W || !m || !range || !d_out))) return ADC_EINVAL;
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            int path = 0;
            d_out[i] = adc::offset_reaching_staged(W[i], m[i], range[i], path);
            if (path_out) path_out[i] = (uint8_t)path;
        }
    });
    return ADC_OK;
}

// adc::offset_reaching_f64, the routine every earlier result was computed with.  path_out (nullable): 0 = W == 0, 1 = no offset can
// reach W (W > 2^24 - 1 or m == 0), 2 = the float64 quotient is at or beyond the range, 3 = the quotient settled on the products
ADC_EXPORT int adc_offset_reaching_f64_host(int64_t n, const uint32_t *W, const uint32_t *m, const uint64_t *range, uint64_t *d_out, uint8_t *path_out)
{
    if (n < 0 || (n > 0 && (!W || !m || !range || !d_out))) return ADC_EINVAL;
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            d_out[i] = adc::offset_reaching_f64(W[i], m[i], range[i]);
            if (path_out)
                path_out[i] = W[i] == 0u ? 0 : (W[i] > 0x00FFFFFFu || m[i] == 0u) ? 1
                              : !(((double)W[i] * 4294967296.0) / (double)m[i] < (double)range[i]) ? 2 : 3;
        }
    });
    return ADC_OK;
}

// adc::win_intervals for n keywords (bid in cents, as the kernels hold it) under the two exports below.  bisect: the bounds by
// lower_bound_v_bisect; offsets: 0 the intervals as the kernels form them, 1 by the verified candidate, 2 by the float64 routine alone.
// flag_out (nullable): the bounds' stage, or - offsets != 0 - the offsets' path
static int win_intervals_host_run(int64_t n, const int32_t *bid_c, const float *cost_loc, const float *cost_scale, const float *buyside_ctr, bool bisect, int offsets,
                                  uint32_t *out4, uint8_t *flag_out)
{
    if (n < 0 || (n > 0 && (!bid_c || !cost_loc || !cost_scale || !buyside_ctr || !out4))) return ADC_EINVAL;
    const adc::LogTableEntry *table = host_log_table();
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const adc::AuctionLaw law = adc::make_auction_law(buyside_ctr[i]);
            const uint64_t t_click = adc::bernoulli_threshold(buyside_ctr[i]);
            uint32_t w_lo, w_hi;
            int stage = 0, path = 0;
            if (bisect) {
                bool a = false, b = false;
                w_lo = adc::lower_bound_v_bisect(1 - bid_c[i], cost_loc[i], cost_scale[i], table, &a);
                w_hi = adc::lower_bound_v_bisect(bid_c[i], cost_loc[i], cost_scale[i], table, &b);
                stage = (a || b) ? 1 : 0;
            } else {
                adc::lower_bound_pair(bid_c[i], cost_loc[i], cost_scale[i], table, w_lo, w_hi, stage);
            }
            const adc::WinIntervals r = offsets == 0   ? adc::win_intervals_of_bounds(w_lo, w_hi, t_click, law)
                                        : offsets == 2 ? adc::win_intervals_of_bounds<true>(w_lo, w_hi, t_click, law, &path)
                                                       : adc::win_intervals_of_bounds<false>(w_lo, w_hi, t_click, law, &path);
            uint32_t *o = out4 + 4 * i;
            o[0] = r.c_lo; o[1] = r.c_w; o[2] = r.n_lo; o[3] = r.n_w;
            if (flag_out) flag_out[i] = (uint8_t)(offsets ? path : stage);
        }
    });
    return ADC_OK;
}

// bisect != 0: the same intervals from the two lower_bound_v_bisect bounds.  stage_out (nullable): the later stage of the keyword's
// two bounds (0 accepted, 1 neighbourhood, 2 bisection; with bisect != 0: 1 if either bound's window failed and the bisection ran over
// the whole range, else 0)
ADC_EXPORT int adc_win_intervals_host(int64_t n, const int32_t *bid_c, const float *cost_loc, const float *cost_scale, const float *buyside_ctr,
                                      int32_t bisect, uint32_t *out4, uint8_t *stage_out)
{
    return win_intervals_host_run(n, bid_c, cost_loc, cost_scale, buyside_ctr, bisect != 0, 0, out4, stage_out);
}

// the offsets by the verified candidate (f64 == 0; path_out: 1 if one of the keyword's four offsets took the float64 routine) or by the
// float64 routine alone (f64 != 0: the earlier form, the reference)
ADC_EXPORT int adc_win_intervals_offsets_host(int64_t n, const int32_t *bid_c, const float *cost_loc, const float *cost_scale, const float *buyside_ctr,
                                              int32_t f64, uint32_t *out4, uint8_t *path_out)
{
    return win_intervals_host_run(n, bid_c, cost_loc, cost_scale, buyside_ctr, false, f64 ? 2 : 1, out4, path_out);
}

// adc::fast_keyword_is_dead for n keywords as phase 1 of k_step_implicit_fast forms it (bid in dollars -> bid_to_cents ->
// win_intervals), next to what it claims, for tests/test_fast_dead_keywords_host.py: dead_out[i] = 1 if the dense form gives the
// keyword no work, out4 (nullable) the intervals.
// wins2 (nullable, two counts per keyword): over the words 0, T - 1, T, 2^32 - 2 (T = the click threshold, clipped to the words
// there are) and n_random words of a splitmix64 stream of (seed, i), how many win by the auction-by-auction form (adc::auction_outcome
// + adc::auction_wins: what the DIRECT form and the oracle evaluate for every auction) and how many by the two intervals.
ADC_EXPORT int adc_fast_dead_keywords_host(int64_t n, const float *bid, const float *cost_loc, const float *cost_scale, const float *buyside_ctr,
                                           int32_t n_random, uint64_t seed, uint8_t *dead_out, uint32_t *out4, int64_t *wins2)
{
    if (n < 0 || n_random < 0 || (n > 0 && (!bid || !cost_loc || !cost_scale || !buyside_ctr || !dead_out))) return ADC_EINVAL;
    const adc::LogTableEntry *table = host_log_table();
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const int32_t bid_c = (int32_t)adc::bid_to_cents(bid[i]);
            const adc::AuctionLaw law = adc::make_auction_law(buyside_ctr[i]);
            const uint64_t t_click = adc::bernoulli_threshold(buyside_ctr[i]);
            const adc::WinIntervals iv = adc::win_intervals(bid_c, cost_loc[i], cost_scale[i], t_click, law, table);
            dead_out[i] = adc::fast_keyword_is_dead(iv) ? 1 : 0;
            if (out4) { uint32_t *o = out4 + 4 * i; o[0] = iv.c_lo; o[1] = iv.c_w; o[2] = iv.n_lo; o[3] = iv.n_w; }
            if (!wins2) continue;
            int64_t by_auction = 0, by_interval = 0;
            auto word = [&](uint32_t w) {
                bool click;
                const int32_t comp = adc::auction_outcome(w, law, cost_loc[i], cost_scale[i], table, click);
                by_auction += adc::auction_wins(w, bid_c, comp) ? 1 : 0;
                by_interval += ((w - iv.c_lo) < iv.c_w || (w - iv.n_lo) < iv.n_w) ? 1 : 0;
            };
            const uint64_t top = 0xFFFFFFFEull;
            word(0u);
            word((uint32_t)(t_click == 0 ? 0ull : t_click - 1 < top ? t_click - 1 : top));
            word((uint32_t)(t_click < top ? t_click : top));
            word((uint32_t)top);
            uint64_t s = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
            for (int32_t r = 0; r < n_random; ++r) word((uint32_t)(shim_splitmix64(s) >> 32));
            wins2[2 * i] = by_auction;
            wins2[2 * i + 1] = by_interval;
        }
    });
    return ADC_OK;
}
