// adc_shims.cpp - scalar entry points that mirror the reference's pyo3 module `adcraft.rust`
// function by function (src/lib.rs).  These are the host-side FFI a maintainer binds in place of
// the Rust crate; the per-step hot path does not go through them (it is adc_engine_step*).
//
// The reference's samplers draw from an unseeded thread_rng (src/lib.rs:25,43,61,75,320), so their
// individual values are not reproducible even by the reference; these take (seed, counter) and
// draw from the engine's Philox stream with the same float32 transforms the kernels use.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/adcraft_engine.h"
#include "adc_law.h"
#include "adc_fast_schedule.h"
#include "adc_interp.h"
#include "adc_mlp.h"
#include "adc_gru.h"
#include "adc_es.h"
#include "adc_pg.h"
#include "adc_pg_kl.h"
#include "adc_pg_shuffle.h"
#include "adc_imitation.h"
#include "adc_dagger.h"
#include "adc_td3.h"
#include "adc_sac.h"
#include "adc_pbt.h"
#include "adc_norm.h"
#include "adc_rew_norm.h"
#include "adc_td3_norm.h"
#include "adc_sac_norm.h"
#include "adc_per.h"

#define ADC_EXPORT extern "C" __attribute__((visibility("default")))

// src/lib.rs:290-294
ADC_EXPORT double adc_sigmoid(double x, double s, double t) { return 1.0 / (1.0 + std::exp(-s * (x - t))); }

// src/lib.rs:296-300 (num::clamp)
ADC_EXPORT double adc_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// src/lib.rs:93-105
ADC_EXPORT double adc_threshold_sigmoid(double p, double impression_thresh, double impression_bid_intercept,
                                        double impression_slope)
{
    const double halver = 2.0 + 1e-10;
    const double thresh = adc_clamp(halver * impression_thresh, 0.0, 1.0) / halver;
    const double r = adc_sigmoid(p, impression_slope, impression_bid_intercept);
    return adc_clamp((1.0 + 2.0 * thresh) * r - thresh, 0.0, 1.0);
}

// src/lib.rs:108-116,310-312: sequential left-to-right f64 sum
ADC_EXPORT double adc_sum_f64(const double *x, int64_t n)
{
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += x[i];
    return s;
}

// src/lib.rs:119-127
ADC_EXPORT int64_t adc_count_true(const uint8_t *x, int64_t n)
{
    int64_t c = 0;
    for (int64_t i = 0; i < n; ++i) c += x[i] != 0;
    return c;
}

static inline adc::U4 shim_draw(uint64_t seed, uint64_t counter, uint32_t lane)
{
    return adc::philox4x32((uint32_t)counter, (uint32_t)(counter >> 32), lane, 0x5348494Du /* "SHIM" */,
                              (uint32_t)seed, (uint32_t)(seed >> 32));
}

// src/lib.rs:314-325: round(max(N(mean, std), 0)), f64::round = half away from zero
ADC_EXPORT uint64_t adc_nonneg_int_normal(double mean, double std, uint64_t seed, uint64_t counter)
{
    const adc::U4 w = shim_draw(seed, counter, 0);
    double x = mean + std * (double)adc::normal_from_word(w.x);
    if (!(x > 0.0)) x = 0.0;
    return (uint64_t)std::round(x);
}

// src/lib.rs:70-76: Binomial(n, p) as n Bernoulli draws
ADC_EXPORT uint64_t adc_binomial(uint64_t n, double p, uint64_t seed, uint64_t counter)
{
    const uint64_t thr = adc::bernoulli_threshold((float)p);
    uint64_t c = 0;
    for (uint64_t i = 0; i < n; i += 4) {
        const adc::U4 w = shim_draw(seed, counter, (uint32_t)(1 + i / 4));
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        for (uint64_t j = 0; j < 4 && i + j < n; ++j) c += adc::bernoulli(ws[j], thr);
    }
    return c;
}

// src/lib.rs:54-67: clamp(sqrt(x)/4 + 4.4/2 + N(0, 1e-10 + sqrt(x)/6), 0, 4.4) - note the constant 4.4
ADC_EXPORT int adc_cost_create(double x, int64_t n, uint64_t seed, uint64_t counter, double *out)
{
    if (n < 0 || (n > 0 && !out) || !(x >= 0.0)) return ADC_EINVAL;
    for (int64_t i = 0; i < n; i += 4) {
        const adc::U4 w = shim_draw(seed, counter, (uint32_t)(1 + i / 4));
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        for (int64_t j = 0; j < 4 && i + j < n; ++j) out[i + j] = (double)adc::explicit_cost(ws[j], (float)x);
    }
    return ADC_OK;
}

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

// adc::win_intervals for n keywords (bid in cents, as the kernels hold it); bisect != 0: the same intervals from the two
// lower_bound_v_bisect bounds.  stage_out (nullable): the later stage of the keyword's two bounds (0 accepted, 1 neighbourhood,
// 2 bisection; with bisect != 0: 1 if either bound's window failed and the bisection ran over the whole range, else 0)
ADC_EXPORT int adc_win_intervals_host(int64_t n, const int32_t *bid_c, const float *cost_loc, const float *cost_scale, const float *buyside_ctr,
                                      int32_t bisect, uint32_t *out4, uint8_t *stage_out)
{
    if (n < 0 || (n > 0 && (!bid_c || !cost_loc || !cost_scale || !buyside_ctr || !out4))) return ADC_EINVAL;
    const adc::LogTableEntry *table = host_log_table();
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const adc::AuctionLaw law = adc::make_auction_law(buyside_ctr[i]);
            const uint64_t t_click = adc::bernoulli_threshold(buyside_ctr[i]);
            uint32_t w_lo, w_hi;
            int stage = 0;
            if (bisect) {
                bool a = false, b = false;
                w_lo = adc::lower_bound_v_bisect(1 - bid_c[i], cost_loc[i], cost_scale[i], table, &a);
                w_hi = adc::lower_bound_v_bisect(bid_c[i], cost_loc[i], cost_scale[i], table, &b);
                stage = (a || b) ? 1 : 0;
            } else {
                adc::lower_bound_pair(bid_c[i], cost_loc[i], cost_scale[i], table, w_lo, w_hi, stage);
            }
            const adc::WinIntervals r = adc::win_intervals_of_bounds(w_lo, w_hi, t_click, law);
            uint32_t *o = out4 + 4 * i;
            o[0] = r.c_lo; o[1] = r.c_w; o[2] = r.n_lo; o[3] = r.n_w;
            if (stage_out) stage_out[i] = (uint8_t)stage;
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

// adc::win_intervals for n keywords with its offsets by the verified candidate (f64 == 0; path_out: 1 if one of the keyword's
// four offsets took the float64 routine) or by the float64 routine alone (f64 != 0: the earlier form, the reference)
ADC_EXPORT int adc_win_intervals_offsets_host(int64_t n, const int32_t *bid_c, const float *cost_loc, const float *cost_scale, const float *buyside_ctr,
                                              int32_t f64, uint32_t *out4, uint8_t *path_out)
{
    if (n < 0 || (n > 0 && (!bid_c || !cost_loc || !cost_scale || !buyside_ctr || !out4))) return ADC_EINVAL;
    const adc::LogTableEntry *table = host_log_table();
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const adc::AuctionLaw law = adc::make_auction_law(buyside_ctr[i]);
            const uint64_t t_click = adc::bernoulli_threshold(buyside_ctr[i]);
            uint32_t w_lo, w_hi;
            int stage = 0, path = 0;
            adc::lower_bound_pair(bid_c[i], cost_loc[i], cost_scale[i], table, w_lo, w_hi, stage);
            const adc::WinIntervals r = f64 ? adc::win_intervals_of_bounds<true>(w_lo, w_hi, t_click, law, &path)
                                            : adc::win_intervals_of_bounds<false>(w_lo, w_hi, t_click, law, &path);
            uint32_t *o = out4 + 4 * i;
            o[0] = r.c_lo; o[1] = r.c_w; o[2] = r.n_lo; o[3] = r.n_w;
            if (path_out) path_out[i] = (uint8_t)path;
        }
    });
    return ADC_OK;
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
            for (int32_t r = 0; r < n_random; ++r) {
                s += 0x9E3779B97F4A7C15ull;
                uint64_t z = s;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                word((uint32_t)((z ^ (z >> 31)) >> 32));
            }
            wins2[2 * i] = by_auction;
            wins2[2 * i + 1] = by_interval;
        }
    });
    return ADC_OK;
}

// ---- what the dense fast pass hoists out of its stages (adc_law.h), next to the routines it replaces there: for
// tests/test_law_hoists_host.py ----------------------------------------------------------------------------------------------
// n calls: plain4 = adc::draw, folded4 = adc::draw_folded, kw4 = adc::draw_kw_folded from the keyword's half (four words each)
ADC_EXPORT int adc_draw_folded_host(int64_t n, const uint64_t *key, const uint32_t *index, const uint32_t *stage, const uint32_t *keyword,
                                    const uint32_t *tick, uint32_t *plain4, uint32_t *folded4, uint32_t *kw4)
{
    if (n < 0 || (n > 0 && (!key || !index || !stage || !keyword || !tick || !plain4 || !folded4 || !kw4))) return ADC_EINVAL;
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const uint32_t tick_k1 = adc::philox_fold_tick(key[i], tick[i]);
            const adc::U4 a = adc::draw(key[i], index[i], stage[i], keyword[i], tick[i]);
            const adc::U4 b = adc::draw_folded(key[i], index[i], stage[i], keyword[i], tick_k1);
            const adc::U4 c = adc::draw_kw_folded(key[i], index[i], adc::philox_kw_half(stage[i], keyword[i], (uint32_t)key[i]), tick_k1);
            uint32_t *pa = plain4 + 4 * i, *pb = folded4 + 4 * i, *pc = kw4 + 4 * i;
            pa[0] = a.x; pa[1] = a.y; pa[2] = a.z; pa[3] = a.w;
            pb[0] = b.x; pb[1] = b.y; pb[2] = b.z; pb[3] = b.w;
            pc[0] = c.x; pc[1] = c.y; pc[2] = c.z; pc[3] = c.w;
        }
    });
    return ADC_OK;
}

// For n keywords (bid in cents): every v of the keyword's win range [W_lo, W_hi) (adc::lower_bound_pair, what adc::win_intervals
// is made of) if the range has at most `exhaustive_below` values, otherwise its `ends` first and last values and `samples` drawn
// ones; and through the words, as stage B of the kernel does: the first and last word of the clicked-win interval, rescaled.  At
// each, adc::competitor_cents_of_proven_win against adc::competitor_cents_from_v.  Returns the number of values that differ
// (first_bad3 = {keyword, v, 0 / 1 for the word route} of the first, or -1s); *checked = values compared.
ADC_EXPORT int64_t adc_proven_win_price_host(int64_t n, const int32_t *bid_c, const float *cost_loc, const float *cost_scale, const float *buyside_ctr,
                                             int64_t exhaustive_below, int32_t ends, int32_t samples, uint64_t seed, int64_t *checked, int64_t *first_bad3)
{
    if (n < 0 || (n > 0 && (!bid_c || !cost_loc || !cost_scale || !buyside_ctr)) || ends < 0 || samples < 0) return -1;
    const adc::LogTableEntry *table = host_log_table();
    int64_t bad = 0, count = 0, first[3] = {-1, -1, -1};
    uint64_t s = seed | 1ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int64_t i = 0; i < n; ++i) {
        const float loc = cost_loc[i], scale = cost_scale[i];
        auto check = [&](uint32_t v, int route) {
            ++count;
            if (adc::competitor_cents_of_proven_win(v, loc, scale, table) != adc::competitor_cents_from_v(v, loc, scale, table)) {
                if (first[0] < 0) { first[0] = i; first[1] = (int64_t)v; first[2] = route; }
                ++bad;
            }
        };
        uint32_t w_lo, w_hi;
        int stage = 0;
        adc::lower_bound_pair(bid_c[i], loc, scale, table, w_lo, w_hi, stage);
        if (w_lo < w_hi) {
            const uint32_t width = w_hi - w_lo;
            if ((int64_t)width <= exhaustive_below) {
                for (uint32_t v = w_lo; v < w_hi; ++v) check(v, 0);
            } else {
                for (uint32_t e = 0; e < (uint32_t)ends && e < width; ++e) { check(w_lo + e, 0); check(w_hi - 1u - e, 0); }
                for (int32_t k = 0; k < samples; ++k) check(w_lo + (uint32_t)(next() % width), 0);
            }
        }
        const adc::AuctionLaw law = adc::make_auction_law(buyside_ctr[i]);
        const adc::WinIntervals iv = adc::win_intervals_of_bounds(w_lo, w_hi, adc::bernoulli_threshold(buyside_ctr[i]), law);
        if (iv.c_w != 0u) {
            for (int e = 0; e < 2; ++e) {
                const uint32_t word = e == 0 ? iv.c_lo : iv.c_lo + iv.c_w - 1u;
                const uint32_t v = adc::mulhi32(word, law.m_click);
                check(v < 0x00FFFFFFu ? v : 0x00FFFFFFu, 1);
            }
        }
    }
    if (checked) *checked = count;
    if (first_bad3) { first_bad3[0] = first[0]; first_bad3[1] = first[1]; first_bad3[2] = first[2]; }
    return bad;
}

// ---- the packed money accumulator of k_step_implicit_fast (adc_law.h fast_money_packs), for tests/test_fast_packed_money_host.py ----
struct HostNormTables { adc::NormTableEntry entry[adc::kNormTableEntries]; float node[adc::kNormTableEntries + 1]; };
static const HostNormTables *host_norm_tables()
{
    // (a function-local static built by a lambda: initialised once, whichever thread comes first)
    static const HostNormTables t = [] {
        HostNormTables r;
        for (int i = 0; i < adc::kNormTableEntries; ++i) r.entry[i] = adc::norm_table_entry(i);
        for (int i = 0; i <= adc::kNormTableEntries; ++i) r.node[i] = adc::norm_table_node(i);
        return r;
    }();
    return &t;
}

// For n keyword-days (volume, bid in dollars, revenue law), as phase 1 of the kernel asks: packs[i] = adc::fast_money_packs;
// bid_c[i] = adc::bid_to_cents; r_max[i] = the revenue bound in cents the predicate multiplies (-1 where the bound in dollars is not
// below 1e7: NaN, infinite or too large to pack at any volume); rev[i * n_words + j] = adc::revenue_cents_tab at words[j].
// *z_max_out (nullable) = the table's largest node.
ADC_EXPORT int adc_fast_money_packs_host(int64_t n, const int32_t *volume, const float *bid, const float *rev_mean, const float *rev_std,
                                         const uint32_t *words, int32_t n_words, uint8_t *packs, int32_t *bid_c, int64_t *r_max, int32_t *rev,
                                         float *z_max_out)
{
    if (n < 0 || n_words < 0 || (n > 0 && (!volume || !bid || !rev_mean || !rev_std || !packs || !bid_c || !r_max)) || (n_words > 0 && (!words || !rev)))
        return ADC_EINVAL;
    const HostNormTables *t = host_norm_tables();
    const float z_max = t->node[0];
    if (z_max_out) *z_max_out = z_max;
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const int32_t bc = (int32_t)adc::bid_to_cents(bid[i]);
            bid_c[i] = bc;
            packs[i] = adc::fast_money_packs(volume[i], bc, rev_mean[i], rev_std[i], z_max) ? 1 : 0;
            const float r = adc::revenue_dollars_max(rev_mean[i], rev_std[i], z_max);
            r_max[i] = r < 1.0e7f ? (int64_t)adc::money_to_cents(r > 0.01f ? r : 0.01f) : -1;
            for (int32_t j = 0; j < n_words; ++j) rev[i * n_words + j] = adc::revenue_cents_tab(words[j], rev_mean[i], rev_std[i], t->entry);
        }
    });
    return ADC_OK;
}

// ---- plain keyword-days of k_step_implicit_fast (adc_law.h fast_keyword_plain), for tests/test_fast_plain_tiles_host.py -----------
// For n keyword-days (volume, bid in dollars, revenue law, conversion rate): plain[i] = adc::fast_keyword_plain; t32[i] / T[i] = the
// conversion threshold saturated to 32 bits / as it is (<= 2^32); rev_tab / rev_plain [i * n_words + j] = adc::revenue_cents_tab and
// adc::revenue_cents_unclamped at words[j], written only where the law is plain (what the unclamped form is defined for), as are
// rev_rmax2[2 i], [2 i + 1] = adc::money_to_cents and adc::money_to_cents_unclamped at the law's revenue bound in dollars;
// conv_bad[i] = over the words 0, T - 1, T, 2^32 - 2, 2^32 - 1 and n_random words drawn with `seed`, how many times
// `word < t32` differs from adc::bernoulli(word, T) (every law, plain or not).
ADC_EXPORT int adc_fast_plain_tiles_host(int64_t n, const int32_t *volume, const float *bid, const float *rev_mean, const float *rev_std,
                                         const float *sellside_ctr, const uint32_t *words, int32_t n_words, int32_t n_random, uint64_t seed,
                                         uint8_t *plain, uint32_t *t32, uint64_t *T, int32_t *rev_tab, int32_t *rev_plain, int32_t *rev_rmax2,
                                         int32_t *conv_bad)
{
    if (n < 0 || n_words < 0 || n_random < 0 || (n > 0 && (!volume || !bid || !rev_mean || !rev_std || !sellside_ctr || !plain || !t32 || !T || !rev_rmax2 || !conv_bad)) ||
        (n_words > 0 && (!words || !rev_tab || !rev_plain)))
        return ADC_EINVAL;
    const HostNormTables *t = host_norm_tables();
    const float z_max = t->node[0];
    shim_parallel_for(n, [=](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const int32_t bc = (int32_t)adc::bid_to_cents(bid[i]);
            const bool p = adc::fast_keyword_plain(volume[i], bc, rev_mean[i], rev_std[i], z_max, sellside_ctr[i]);
            plain[i] = p ? 1 : 0;
            const uint64_t Ti = adc::bernoulli_threshold(sellside_ctr[i]);
            const uint32_t ti = adc::saturate_threshold(Ti);
            T[i] = Ti;
            t32[i] = ti;
            if (p) {
                for (int32_t j = 0; j < n_words; ++j) {
                    rev_tab[i * n_words + j] = adc::revenue_cents_tab(words[j], rev_mean[i], rev_std[i], t->entry);
                    rev_plain[i * n_words + j] = adc::revenue_cents_unclamped(words[j], rev_mean[i], rev_std[i], t->entry);
                }
                const float r = adc::revenue_dollars_max(rev_mean[i], rev_std[i], z_max);
                rev_rmax2[2 * i] = adc::money_to_cents(r);
                rev_rmax2[2 * i + 1] = adc::money_to_cents_unclamped(r);
            }
            const uint32_t fixed[5] = {0u, (uint32_t)(Ti - 1ull), (uint32_t)Ti, 0xFFFFFFFEu, 0xFFFFFFFFu};
            uint64_t s = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
            int32_t bad = 0;
            for (int32_t j = 0; j < 5 + n_random; ++j) {
                uint32_t w;
                if (j < 5) w = fixed[j];
                else {                                  // splitmix64
                    s += 0x9E3779B97F4A7C15ull;
                    uint64_t z = s;
                    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                    w = (uint32_t)((z ^ (z >> 31)) >> 16);
                }
                bad += (w < ti) != adc::bernoulli(w, Ti) ? 1 : 0;
            }
            conv_bad[i] = bad;
        }
    });
    return ADC_OK;
}
// the queue tag of a clicked win (adc_law.h fast_tag) and what stage B reads back from it: out4 = {tag, accumulator byte offset,
// keyword, auction}
ADC_EXPORT int adc_fast_tag_host(uint32_t keyword_in_tile, uint32_t auction, uint32_t *out4)
{
    if (!out4 || keyword_in_tile >= (uint32_t)adc::kFastTileLanes || auction > (uint32_t)adc::kVolumeMax) return ADC_EINVAL;
    const uint32_t tag = adc::fast_tag(keyword_in_tile, auction);
    out4[0] = tag;
    out4[1] = adc::fast_tag_acc_offset(tag);
    out4[2] = adc::fast_tag_keyword(tag);
    out4[3] = adc::fast_tag_auction(tag);
    return ADC_OK;
}

// ---- the host twin of k_step_implicit_fast's phase-2 schedule (adc_fast_schedule.h: the helpers the kernel calls) ------------
// For tile number tile_index (env x tiles-per-env + tile: it only rotates which wave takes which part of the items) of tile_kw
// keywords with the given volumes: every (pass, wave, round, lane) slot the kernel issues, as rows of
// seven int32 {pass, wave, round, lane, keyword, first auction, count} (an idle slot: keyword -1, count 0); pass 0 = full items,
// 1 = the tails' whole calls, 2 = the partial calls.  Returns the number of rows (the first `cap` of them are written; slots7 may be
// NULL with cap 0), or a negative adc_status.  totals2 (nullable) = {wave-call-slots issued: Philox calls, counted once per wave
// that runs them; calls that hold at least one auction, summed over the keywords}; info2 (nullable) = {chunk_shift, dense}.
ADC_EXPORT int64_t adc_fast_schedule_host(const int32_t *vol_k, int32_t tile_kw, int32_t tile_index, int32_t *slots7, int64_t cap, int64_t *totals2,
                                          int32_t *info2)
{
    constexpr int B = adc::kFastTileLanes, WL = adc::kFastWaveLanes, NW = adc::kFastTileWaves;
    if (!vol_k || tile_kw < 1 || tile_kw > B || tile_index < 0 || cap < 0 || (cap > 0 && !slots7)) return ADC_EINVAL;
    int V[B];
    int64_t volume = 0, needed = 0;
    int live = 0;
    for (int t = 0; t < B; ++t) {
        V[t] = t < tile_kw ? vol_k[t] : 0;
        if (V[t] < 0 || V[t] > adc::kVolumeMax) return ADC_EINVAL;
        volume += V[t];
        live += V[t] > 0;
        needed += adc::fast_calls_needed(V[t]);
    }
    const int tile_volume = (int)volume;                        // (<= 256 * 2^20)
    const int chunk_shift = adc::fast_chunk_shift(tile_volume);
    // the two prefixes as the kernel forms them: one packed scan per wave of 64 keywords, the waves' totals added unpacked
    std::vector<int> off((size_t)B + 1), first_call((size_t)B);
    std::vector<unsigned char> tail_kw((size_t)(adc::kFastTailCallsMax * B));
    int total = 0, total2 = 0;
    for (int w = 0; w < NW; ++w) {
        int packed = 0;
        for (int lane = 0; lane < WL; ++lane) {
            const int t = w * WL + lane;
            const int nch = adc::fast_full_items(V[t], chunk_shift), ntc = adc::fast_tail_calls(V[t], chunk_shift);
            packed += adc::fast_pack_counts(nch, ntc);
            off[(size_t)t] = total + adc::fast_packed_items(packed) - nch;
            first_call[(size_t)t] = total2 + adc::fast_packed_calls(packed) - ntc;
            for (int c = 0; c < adc::kFastTailCallsMax; ++c)
                if (c < ntc) tail_kw[(size_t)(first_call[(size_t)t] + c)] = (unsigned char)t;
        }
        total += adc::fast_packed_items(packed);
        total2 += adc::fast_packed_calls(packed);
    }
    off[(size_t)B] = total;
    int64_t rows = 0, issued = 0;
    auto emit = [&](int pass, int w, int r, int lane, int u, int j0, int n) {
        if (rows < cap) {
            int32_t *o = slots7 + 7 * rows;
            o[0] = pass; o[1] = w; o[2] = r; o[3] = lane; o[4] = n > 0 ? u : -1; o[5] = n > 0 ? j0 : 0; o[6] = n;
        }
        rows += 1;
    };
    for (int pass = 0; pass < 2; ++pass) {
        const int shift = pass == 0 ? chunk_shift : adc::kFastCallShift;
        const int ptotal = pass == 0 ? total : total2;
        for (int w = 0; w < NW; ++w) {
            const int part = adc::fast_wave_part(w, tile_index);
            const int rounds = adc::fast_wave_rounds(ptotal, part), base = adc::fast_wave_base(ptotal, part);
            issued += (int64_t)rounds << (shift - adc::kFastCallShift);
            for (int lane = 0; lane < WL; ++lane) {
                const int first = adc::fast_lane_first(base, rounds, lane, ptotal);
                int u = 0, u_end = 0;
                if (pass == 0) {
                    for (int s = B / 2; s > 0; s >>= 1)
                        if (off[(size_t)(u + s)] <= first) u += s;
                    u_end = off[(size_t)u + 1];
                }
                for (int r = 0; r < rounds; ++r) {
                    const int item = first + r;
                    const bool has = adc::fast_item_exists(item, ptotal);
                    int j0 = 0;
                    if (pass == 0) {
                        while (has && item >= u_end) { u += 1; u_end = off[(size_t)u + 1]; }
                        if (has) j0 = (item - off[(size_t)u]) << shift;
                    } else if (has) {
                        u = tail_kw[(size_t)item];
                        j0 = adc::fast_tail_first(V[u], chunk_shift) + ((item - first_call[(size_t)u]) << shift);
                    }
                    emit(pass, w, r, lane, u, j0, has ? 1 << shift : 0);
                }
            }
        }
    }
    for (int w = 0; w < NW; ++w) {                              // (a wave none of whose keywords has a partial call issues nothing)
        bool any = false;
        for (int lane = 0; lane < WL; ++lane) any = any || adc::fast_partial_count(V[w * WL + lane]) != 0;
        if (!any) continue;
        issued += 1;
        for (int lane = 0; lane < WL; ++lane) {
            const int t = w * WL + lane;
            emit(2, w, 0, lane, t, adc::fast_partial_first(V[t]), adc::fast_partial_count(V[t]));
        }
    }
    if (totals2) { totals2[0] = issued; totals2[1] = needed; }
    if (info2) { info2[0] = chunk_shift; info2[1] = adc::fast_tile_dense(tile_volume, live) ? 1 : 0; }
    return rows;
}

// adcraft/gymnasium_kw_utils.py:113-156 (sample_random_keywords), one keyword: what k_generate_explicit_keywords writes
ADC_EXPORT int adc_sample_random_keyword(uint64_t key, uint32_t keyword, uint32_t serial, float *out8)
{
    if (!out8) return ADC_EINVAL;
    adc::generate_explicit_keyword(key, keyword, serial, out8);
    return ADC_OK;
}

// the host twin of an EXPLICIT keyword's cached bid curve (k_explicit_curves): the same n draws of the ST_METRIC stream, sorted,
// and the same adc::explicit_curve_point on their two middle normals.  cpc is bit-identical to the device's; ir uses the host's exp
// (the device's is ocml's).  z_mid2_out (nullable) receives z_lo, z_hi.
ADC_EXPORT int adc_explicit_curve_host(uint64_t key, uint32_t tick, int32_t keyword, int32_t n_samples, float impression_thresh, float a,
                                       float b, const double *bid_grid, int32_t n_bids, double *ir_out, double *cpc_out, double *z_mid2_out)
{
    if (n_samples <= 0 || n_samples > (1 << 20) || keyword < 0 || n_bids < 0 || (n_bids > 0 && (!bid_grid || !ir_out || !cpc_out)))
        return ADC_EINVAL;
    std::vector<float> z((size_t)n_samples);
    for (int32_t i = 0; i < n_samples; i += 4) {
        const adc::U4 w = adc::draw(key, (uint32_t)(i / 4), adc::ST_METRIC, (uint32_t)keyword, tick);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        for (int j = 0; j < 4 && i + j < n_samples; ++j) z[(size_t)(i + j)] = adc::normal_from_word(ws[j]);
    }
    std::sort(z.begin(), z.end());
    const float z_lo = z[(size_t)((n_samples - 1) / 2)], z_hi = z[(size_t)(n_samples / 2)];
    if (z_mid2_out) { z_mid2_out[0] = z_lo; z_mid2_out[1] = z_hi; }
    for (int32_t i = 0; i < n_bids; ++i) {
        double mu, sigma;
        adc::explicit_cost_law(bid_grid[i], mu, sigma);
        const adc::CurvePoint q = adc::explicit_curve_point(impression_thresh, a, b, z_lo, z_hi, bid_grid[i], mu, sigma);
        ir_out[i] = q.ir;
        cpc_out[i] = q.cpc;
    }
    return ADC_OK;
}

ADC_EXPORT double adc_interp_key_host(float bid) { return adc::interp_key(bid); }

ADC_EXPORT int adc_interp_act_host(float ave_rpc, int32_t n_rpc, float ave_sctr, int32_t n_sctr, double max_observed, double threshold,
                                   double bid_step, const double *grid, int32_t n_bids, int32_t n_clk, const uint16_t *clk_cent,
                                   const float *clk_ave, int32_t n_cpc, const uint16_t *cpc_cent, const double *cpc_ave, double u,
                                   double *margin_out, double *cost_out, double *bid_out, int32_t *index_out,
                                   double *mass_out)
{
    if (n_bids < 1 || n_bids > adc::kInterpMaxBids || !grid || n_clk < 0 || n_cpc < 0 || n_clk > adc::kInterpCents ||
        n_cpc > n_clk || (n_clk > 0 && (!clk_cent || !clk_ave)) || (n_cpc > 0 && (!cpc_cent || !cpc_ave)) || !bid_out || !index_out)
        return ADC_EINVAL;
    for (int i = 0; i < n_clk; ++i)
        if (clk_cent[i] < 1 || clk_cent[i] > adc::kInterpCents || (i > 0 && clk_cent[i] <= clk_cent[i - 1])) return ADC_EINVAL;
    for (int i = 0; i < n_cpc; ++i)
        if (cpc_cent[i] < 1 || cpc_cent[i] > adc::kInterpCents || (i > 0 && cpc_cent[i] <= cpc_cent[i - 1])) return ADC_EINVAL;
    const adc::InterpSeries<float> clk{clk_cent, clk_ave, 1, n_clk};
    const adc::InterpSeries<double> cpc{cpc_cent, cpc_ave, 1, n_cpc};
    double cpc_right = 0.0;
    for (int i = 0; i < n_cpc; ++i) cpc_right = (i == 0 || cpc_ave[i] > cpc_right) ? cpc_ave[i] : cpc_right;
    const double erpc = adc::interp_erpc(ave_rpc, n_rpc, ave_sctr, n_sctr);
    const double thr = adc::interp_threshold(n_rpc, n_sctr, threshold);
    const int end = adc::interp_end_index(max_observed, bid_step, n_bids);
    auto eval = [&](int j) { return adc::interp_point(clk, cpc, cpc_right, erpc, grid[j]); };
    for (int j = 0; j < n_bids; ++j) {
        const adc::InterpPoint q = eval(j);
        if (margin_out) margin_out[j] = q.margin;
        if (cost_out) cost_out[j] = q.cost;
    }
    const adc::InterpPick pk = adc::interp_pick(eval, thr, end, [&]() { return u; });
    *index_out = pk.index;
    if (mass_out) *mass_out = pk.mass;
    *bid_out = pk.index >= 0 ? grid[pk.index] : 0.01;
    return ADC_OK;
}

// ---- the MLP policy on the host (adc_mlp.h: the code parts/kernel_mlp_policy.inc runs) -------------------------------------
// the checks adc_engine_mlp_init makes on a configuration for an engine of num_keywords keywords; message (nullable) names the first failure
ADC_EXPORT int adc_mlp_config_check(const adc_mlp_config *cfg, int32_t num_keywords, const char **message)
{
    const char *msg = nullptr;
    const int A = num_keywords + 1;
    if (!cfg || cfg->struct_size != sizeof(adc_mlp_config)) msg = "adc_mlp_config: NULL or struct_size mismatch";
    else if (num_keywords < 1) msg = "num_keywords < 1";
    else if (cfg->activation != ADC_MLP_TANH && cfg->activation != ADC_MLP_RELU) msg = "unknown activation";
    else if (cfg->n_policy_layers < 1 || cfg->n_policy_layers > adc::kMlpMaxLayers) msg = "the policy network has 1 to 4 layers";
    else if (cfg->n_value_layers < 0 || cfg->n_value_layers > adc::kMlpMaxLayers) msg = "the value network has 0 to 4 layers";
    else if (cfg->clamp_log_std && !(cfg->log_std_lo <= cfg->log_std_hi)) msg = "log_std clamp: lo <= hi";
    else {
        for (int l = 0; l + 1 < cfg->n_policy_layers && !msg; ++l)
            if (cfg->policy_widths[l] < 1 || cfg->policy_widths[l] > adc::kMlpMaxWidth) msg = "hidden widths are 1 to 256";
        for (int l = 0; l + 1 < cfg->n_value_layers && !msg; ++l)
            if (cfg->value_widths[l] < 1 || cfg->value_widths[l] > adc::kMlpMaxWidth) msg = "hidden widths are 1 to 256";
        const int P = cfg->policy_widths[cfg->n_policy_layers - 1];
        if (!msg && P != A && P != 2 * A) msg = "the policy network ends in num_keywords + 1 outputs (means) or twice that (means, log-stds)";
        if (!msg && cfg->n_value_layers > 0 && cfg->value_widths[cfg->n_value_layers - 1] != 1) msg = "the value network ends in one output";
    }
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

namespace {
// one network of the law on a host input row; weights given [n_in][n_out] row-major, re-laid chain-major as the device holds them
std::vector<float> mlp_forward_host(const float *x0, int D, int layers, const int32_t *widths, const float *const *w, const float *const *b, int activation)
{
    std::vector<float> x(x0, x0 + D);
    for (int l = 0; l < layers; ++l) {
        const int n_in = (int)x.size(), n_out = widths[l];
        std::vector<float> cm(adc::mlp_weight_count(n_in, n_out), 0.0f), y((size_t)n_out);
        for (int j = 0; j < n_in; ++j)
            for (int h = 0; h < n_out; ++h) cm[adc::mlp_weight_index(j, h, n_out)] = w[l][(size_t)j * n_out + h];
        const float *xp = x.data();
        for (int h = 0; h < n_out; ++h) {
            const float v = adc::mlp_neuron(cm.data(), b[l], n_in, n_out, h, [&](int j) { return xp[j]; });
            y[(size_t)h] = l + 1 < layers ? adc::mlp_act(v, activation) : v;
        }
        x.swap(y);
    }
    return x;
}
void mlp_heads_host(const adc_mlp_config *cfg, int K, const std::vector<float> &o, float v, const float *log_std_a, const float *normals_a,
                    uint64_t agent_key, uint32_t tick, float budget_override, float *mean_a, float *log_std_out_a, float *action_a, float *logp,
                    float *value, float *bids_k, float *budget);
}  // namespace

ADC_EXPORT int adc_mlp_stack_row_host(int32_t num_keywords, int32_t frames, const float *frame0_d0, float *hist_hd0, int32_t *last, int32_t *from,
                                      int32_t day, int32_t commit, float *row_d)
{
    if (num_keywords < 1 || frames < 1 || frames > adc::kMlpMaxFrames || day < 0 || !hist_hd0 || !last || !from || !row_d) return ADC_EINVAL;
    const int D0 = 5 * num_keywords + 2, D = frames * D0;
    const int32_t fr = adc::mlp_hist_from(day, *last, *from);
    for (int i = 0; i < D; ++i) row_d[i] = i < D0 ? (frame0_d0 && day != 0 ? frame0_d0[i] : 0.0f) : adc::mlp_hist_at(i, D0, frames, hist_hd0, day, fr);
    if (commit) {
        float *slot = hist_hd0 + (size_t)adc::mlp_hist_slot(day, frames) * (size_t)D0;
        for (int j = 0; j < D0; ++j) slot[j] = row_d[j];
        *last = day;
        *from = fr;
    }
    return ADC_OK;
}

ADC_EXPORT int adc_mlp_act_host(const adc_mlp_config *cfg, int32_t num_keywords, const float *obs_d, const float *const *policy_w,
                                const float *const *policy_b, const float *const *value_w, const float *const *value_b, const float *shift_d,
                                const float *scale_d, const float *log_std_a, const float *normals_a, uint64_t agent_key, uint32_t tick,
                                float budget_override, float *mean_a, float *log_std_out_a, float *action_a, float *logp, float *value,
                                float *bids_k, float *budget)
{
    if (adc_mlp_config_check(cfg, num_keywords, nullptr) != ADC_OK) return ADC_EINVAL;
    const int K = num_keywords, A = K + 1, D = 5 * K + 2;
    const int P = cfg->policy_widths[cfg->n_policy_layers - 1];
    const bool two_heads = P == 2 * A;
    if (!policy_w || !policy_b || (cfg->n_value_layers > 0 && (!value_w || !value_b)) || (cfg->normalize && (!shift_d || !scale_d)) ||
        (!two_heads && !log_std_a))
        return ADC_EINVAL;
    const int activation = cfg->activation == ADC_MLP_TANH ? adc::kMlpTanh : adc::kMlpRelu;
    std::vector<float> x((size_t)D, 0.0f);
    for (int j = 0; j < D; ++j) {
        float xj = obs_d ? obs_d[j] : 0.0f;
        if (cfg->normalize) xj = adc::mlp_normalize(xj, shift_d[j], scale_d[j]);
        x[(size_t)j] = xj;
    }
    float v = 0.0f;
    if (cfg->n_value_layers > 0) v = mlp_forward_host(x.data(), D, cfg->n_value_layers, cfg->value_widths, value_w, value_b, activation)[0];
    const std::vector<float> o = mlp_forward_host(x.data(), D, cfg->n_policy_layers, cfg->policy_widths, policy_w, policy_b, activation);
    mlp_heads_host(cfg, K, o, v, log_std_a, normals_a, agent_key, tick, budget_override, mean_a, log_std_out_a, action_a, logp, value, bids_k, budget);
    return ADC_OK;
}

namespace {
// everything after the policy network's outputs o [P] (adc_mlp.h: heads, sample, log-probability, bids, budget); v: the value
void mlp_heads_host(const adc_mlp_config *cfg, int K, const std::vector<float> &o, float v, const float *log_std_a, const float *normals_a,
                    uint64_t agent_key, uint32_t tick, float budget_override, float *mean_a, float *log_std_out_a, float *action_a, float *logp,
                    float *value, float *bids_k, float *budget)
{
    const int A = K + 1;
    const bool two_heads = cfg->policy_widths[cfg->n_policy_layers - 1] == 2 * A;
    std::vector<float> term((size_t)A);
    for (int a = 0; a < A; ++a) {
        const float mean = o[(size_t)a];
        const float ls = adc::mlp_clamp_log_std(two_heads ? o[(size_t)(A + a)] : log_std_a[a], cfg->clamp_log_std != 0, cfg->log_std_lo, cfg->log_std_hi);
        float z = 0.0f;
        if (!cfg->deterministic) z = normals_a ? normals_a[a] : adc::mlp_normal(agent_key, tick, a);
        const float act = adc::mlp_sample(mean, ls, z, cfg->deterministic != 0);
        if (mean_a) mean_a[a] = mean;
        if (log_std_out_a) log_std_out_a[a] = ls;
        if (action_a) action_a[a] = act;
        if (a == 0) { if (budget) *budget = adc::mlp_budget(act, budget_override); }
        else if (bids_k) bids_k[a - 1] = adc::mlp_bid(act, cfg->bid_clip_hi);
        term[(size_t)a] = adc::mlp_logp_term(z, ls);
    }
    float s[adc::kMlpChains];
    for (int c = 0; c < adc::kMlpChains; ++c) {
        float acc = 0.0f;
        for (int a = c; a < A; a += adc::kMlpChains) acc = acc + term[(size_t)a];
        s[c] = acc;
    }
    if (logp) *logp = adc::mlp_logp_finish(adc::mlp_join8(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]), A);
    if (value) *value = v;
}

// one layer of the law without an activation: y = W x + b, weights [n_in][n_out] row-major
std::vector<float> mlp_linear_host(const float *x, int n_in, int n_out, const float *w, const float *b)
{
    const int32_t widths[1] = {n_out};
    const float *const ws[1] = {w}, *const bs[1] = {b};
    return mlp_forward_host(x, n_in, 1, widths, ws, bs, adc::kMlpTanh);
}
// the cell (adc_gru.h) on x [n_in] and h [G]
std::vector<float> gru_cell_host(int n_in, int G, const float *x, const float *h, const float *wi, const float *bi, const float *wh, const float *bh)
{
    const std::vector<float> gi = mlp_linear_host(x, n_in, 3 * G, wi, bi), gh = mlp_linear_host(h, G, 3 * G, wh, bh);
    std::vector<float> out((size_t)G);
    for (int g = 0; g < G; ++g)
        out[(size_t)g] = adc::gru_unit(gi[(size_t)g], gh[(size_t)g], gi[(size_t)(G + g)], gh[(size_t)(G + g)], gi[(size_t)(2 * G + g)], gh[(size_t)(2 * G + g)], h[g]);
    return out;
}
}  // namespace

// ---- the recurrent policy on the host (adc_gru.h: the code parts/kernel_mlp_gru.inc runs) ------------------------------------------
ADC_EXPORT int adc_gru_cell_host(int32_t n_in, int32_t gru_width, const float *x_in, const float *h_g, const float *wi_in_3g, const float *bi_3g,
                                 const float *wh_g_3g, const float *bh_3g, float *h_out_g)
{
    if (n_in < 1 || gru_width < 1 || gru_width > adc::kGruMaxWidth || !x_in || !h_g || !wi_in_3g || !bi_3g || !wh_g_3g || !bh_3g || !h_out_g) return ADC_EINVAL;
    const std::vector<float> out = gru_cell_host(n_in, gru_width, x_in, h_g, wi_in_3g, bi_3g, wh_g_3g, bh_3g);
    std::copy(out.begin(), out.end(), h_out_g);
    return ADC_OK;
}

ADC_EXPORT int adc_mlp_act_recurrent_host(const adc_mlp_config *cfg, int32_t num_keywords, int32_t gru_width, const float *obs_d,
                                          const float *const *policy_w, const float *const *policy_b, const float *wi_in_3g, const float *bi_3g,
                                          const float *wh_g_3g, const float *bh_3g, const float *const *value_w, const float *const *value_b,
                                          const float *shift_d, const float *scale_d, const float *log_std_a, const float *normals_a,
                                          uint64_t agent_key, uint32_t tick, float budget_override, const float *h_in_g, float *mean_a,
                                          float *log_std_out_a, float *action_a, float *logp, float *value, float *bids_k, float *budget,
                                          float *h_out_g)
{
    if (adc_mlp_config_check(cfg, num_keywords, nullptr) != ADC_OK) return ADC_EINVAL;
    const int K = num_keywords, A = K + 1, D = 5 * K + 2, G = gru_width, L = cfg->n_policy_layers;
    const int P = cfg->policy_widths[L - 1];
    if (G < 1 || G > adc::kGruMaxWidth) return ADC_EINVAL;
    if (!policy_w || !policy_b || !wi_in_3g || !bi_3g || !wh_g_3g || !bh_3g || (cfg->n_value_layers > 0 && (!value_w || !value_b)) ||
        (cfg->normalize && (!shift_d || !scale_d)) || (P != 2 * A && !log_std_a))
        return ADC_EINVAL;
    const int activation = cfg->activation == ADC_MLP_TANH ? adc::kMlpTanh : adc::kMlpRelu;
    std::vector<float> x((size_t)D, 0.0f);
    for (int j = 0; j < D; ++j) {
        float xj = obs_d ? obs_d[j] : 0.0f;
        if (cfg->normalize) xj = adc::mlp_normalize(xj, shift_d[j], scale_d[j]);
        x[(size_t)j] = xj;
    }
    float v = 0.0f;
    if (cfg->n_value_layers > 0) v = mlp_forward_host(x.data(), D, cfg->n_value_layers, cfg->value_widths, value_w, value_b, activation)[0];
    // the trunk (the activation after each of its layers), the cell, the output layer on the new state
    for (int l = 0; l + 1 < L; ++l) {
        std::vector<float> y = mlp_linear_host(x.data(), (int)x.size(), cfg->policy_widths[l], policy_w[l], policy_b[l]);
        for (float &t : y) t = adc::mlp_act(t, activation);
        x.swap(y);
    }
    const std::vector<float> h0((size_t)G, 0.0f);
    const std::vector<float> h1 = gru_cell_host((int)x.size(), G, x.data(), h_in_g ? h_in_g : h0.data(), wi_in_3g, bi_3g, wh_g_3g, bh_3g);
    if (h_out_g) std::copy(h1.begin(), h1.end(), h_out_g);
    const std::vector<float> o = mlp_linear_host(h1.data(), G, P, policy_w[L - 1], policy_b[L - 1]);
    mlp_heads_host(cfg, K, o, v, log_std_a, normals_a, agent_key, tick, budget_override, mean_a, log_std_out_a, action_a, logp, value, bids_k, budget);
    return ADC_OK;
}

ADC_EXPORT int adc_gru_state_host(int32_t gru_width, int32_t day, float *h_2g, int32_t *last, int32_t *from, float *h_in_g, const float *h_new_g)
{
    const int G = gru_width;
    if (G < 1 || G > adc::kGruMaxWidth || day < 0 || !h_2g || !last || !from || !h_in_g) return ADC_EINVAL;
    const int32_t fr = adc::mlp_hist_from(day, *last, *from);
    const bool zeros = adc::gru_starts_from_zeros(day, fr);
    for (int g = 0; g < G; ++g) h_in_g[g] = zeros ? 0.0f : h_2g[(size_t)adc::gru_read_slot(day) * (size_t)G + (size_t)g];
    if (h_new_g) {
        for (int g = 0; g < G; ++g) h_2g[(size_t)adc::gru_write_slot(day) * (size_t)G + (size_t)g] = h_new_g[g];
        *last = day;
        *from = fr;
    }
    return ADC_OK;
}

ADC_EXPORT float adc_mlp_math_host(int32_t fn, float x) { return fn == 0 ? adc::mlp_tanh(x) : adc::mlp_exp(x); }

ADC_EXPORT int adc_mlp_squash_host(int32_t count, const float *u_a, const float *lo_a, const float *hi_a, float *out_a)
{
    if (count < 0 || (count > 0 && (!u_a || !lo_a || !hi_a || !out_a))) return ADC_EINVAL;
    for (int a = 0; a < count; ++a) out_a[a] = adc::mlp_squash(u_a[a], lo_a[a], adc::mlp_squash_half(lo_a[a], hi_a[a]));
    return ADC_OK;
}

ADC_EXPORT int adc_mlp_bounded_host(int32_t count, const float *mean_a, const float *log_std_a, const float *normals_a, uint64_t agent_key, uint32_t tick,
                                    int32_t mode, const float *lo_a, const float *hi_a, float *n_a, float *env_a)
{
    if (count < 1 || !mean_a || !log_std_a || !lo_a || !hi_a || mode < 0 || mode > 2) return ADC_EINVAL;
    const int deterministic = mode == 1, explore = mode == 2 ? adc::kMlpRandom : adc::kMlpGaussian;
    for (int a = 0; a < count; ++a) {
        float z = 0.0f;
        uint32_t w = 0u;
        if (!deterministic) {
            if (explore == adc::kMlpRandom) w = adc::mlp_word(agent_key, tick, a);
            else z = normals_a ? normals_a[a] : adc::mlp_normal(agent_key, tick, a);
        }
        const float n = adc::mlp_bounded_action(mean_a[a], log_std_a[a], z, w, deterministic, explore);
        if (n_a) n_a[a] = n;
        if (env_a) env_a[a] = adc::mlp_box(n, lo_a[a], adc::mlp_squash_half(lo_a[a], hi_a[a]));
    }
    return ADC_OK;
}

ADC_EXPORT int adc_mlp_unbox_host(int32_t count, const float *e_a, const float *lo_a, const float *hi_a, float *n_a)
{
    if (count < 1 || !e_a || !lo_a || !hi_a || !n_a) return ADC_EINVAL;
    for (int a = 0; a < count; ++a) n_a[a] = adc::mlp_unbox(e_a[a], lo_a[a], adc::mlp_inv_half(adc::mlp_squash_half(lo_a[a], hi_a[a])));
    return ADC_OK;
}

ADC_EXPORT uint64_t adc_mlp_agent_key_host(uint64_t seed) { return adc::mlp_agent_key(seed); }
ADC_EXPORT uint64_t adc_mlp_default_agent_key_host(uint64_t engine_seed, uint64_t global_env_id) { return adc::mlp_default_agent_key(engine_seed, global_env_id); }

ADC_EXPORT int64_t adc_mlp_math_sweep_host(int32_t fn, float lo, float hi, double *out3, int64_t *violations4)
{
    if (!(lo <= hi) || (fn != 0 && fn != 1)) return -1;
    // floats in value order: key = bits of a positive float, or the negation of a negative one's magnitude bits
    auto key_of = [](float f) { const uint32_t u = adc::float_to_bits(f); return (u & 0x80000000u) ? -(int64_t)(u & 0x7FFFFFFFu) : (int64_t)u; };
    auto float_of = [](int64_t k) { return adc::bits_to_float(k < 0 ? (0x80000000u | (uint32_t)(-k)) : (uint32_t)k); };
    const int64_t k0 = key_of(lo), k1 = key_of(hi), total = k1 - k0 + 1;
    const int T = 8;
    struct Part { double max_abs = 0.0, max_ulp = 0.0, max_mag = 0.0; int64_t bad[4] = {0, 0, 0, 0}; };
    std::vector<Part> parts((size_t)T);
    std::vector<std::thread> threads;
    auto eval = [fn](float x) { return fn == 0 ? adc::mlp_tanh(x) : adc::mlp_exp(x); };
    for (int t = 0; t < T; ++t) {
        threads.emplace_back([&, t]() {
            Part &p = parts[(size_t)t];
            const int64_t a = k0 + total * t / T, b = k0 + total * (t + 1) / T;      // keys [a, b); the first compares with its predecessor
            float prev = a > k0 ? eval(float_of(a - 1)) : -__builtin_inff();
            for (int64_t k = a; k < b; ++k) {
                if (k == 0 && a != 0) continue;                                       // (-0 and +0 share key 0: taken once)
                const float x = float_of(k);
                const float y = eval(x);
                const double exact = fn == 0 ? std::tanh((double)x) : std::exp((double)x);
                const double err = std::fabs((double)y - exact);
                if (err > p.max_abs) p.max_abs = err;
                int ex;
                (void)std::frexp(exact, &ex);
                const double ulp = std::ldexp(1.0, std::max(ex - 24, -149));
                if (err / ulp > p.max_ulp) p.max_ulp = err / ulp;
                if (std::fabs((double)y) > p.max_mag) p.max_mag = std::fabs((double)y);
                if (fn == 0 && eval(-x) != -y) p.bad[0] += 1;
                if (y < prev) p.bad[1] += 1;
                if (fn == 0 && std::fabs(y) > 1.0f) p.bad[2] += 1;
                if (y != y) p.bad[3] += 1;
                prev = y;
            }
        });
    }
    for (auto &th : threads) th.join();
    Part all;
    for (const Part &p : parts) {
        all.max_abs = std::max(all.max_abs, p.max_abs); all.max_ulp = std::max(all.max_ulp, p.max_ulp); all.max_mag = std::max(all.max_mag, p.max_mag);
        for (int i = 0; i < 4; ++i) all.bad[i] += p.bad[i];
    }
    if (out3) { out3[0] = all.max_abs; out3[1] = all.max_ulp; out3[2] = all.max_mag; }
    if (violations4) for (int i = 0; i < 4; ++i) violations4[i] = all.bad[i];
    return total;
}

// ---- the evolution strategy on the host (adc_es.h: the code parts/kernel_es.inc runs) ----------------------------------------
ADC_EXPORT int adc_es_config_check(const adc_es_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_es_config)) msg = "adc_es_config: NULL or struct_size mismatch";
    else if (!(cfg->sigma > 0.0f) || !(cfg->sigma < __builtin_inff())) msg = "sigma must be positive and finite";
    else if (!(cfg->lr >= 0.0f)) msg = "lr >= 0";
    else if (cfg->shaping != ADC_ES_CENTERED_RANK && cfg->shaping != ADC_ES_RAW) msg = "unknown fitness shaping";
    else if (cfg->optimiser != ADC_ES_ADAM && cfg->optimiser != ADC_ES_SGD) msg = "unknown optimiser";
    else if (!(cfg->l2 >= 0.0f)) msg = "l2 >= 0";
    else if (cfg->optimiser == ADC_ES_ADAM && (!(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f) || !(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f)))
        msg = "Adam: 0 <= beta1, beta2 < 1";
    else if (cfg->optimiser == ADC_ES_ADAM && !(cfg->eps > 0.0f)) msg = "Adam: eps > 0";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_es_noise_host(uint64_t seed, uint32_t pair, uint32_t generation, int64_t p0, int64_t n, float *eps_n)
{
    if (p0 < 0 || n < 0 || p0 + n > 0x7FFFFFFFll || (n > 0 && !eps_n)) return ADC_EINVAL;
    const uint64_t key = adc::es_key(seed);
    for (int64_t q = p0 / 4; q * 4 < p0 + n; ++q) {
        float e4[4];
        adc::es_noise4(key, (uint32_t)q, pair, generation, e4);
        for (int k = 0; k < 4; ++k) {
            const int64_t p = q * 4 + k;
            if (p >= p0 && p < p0 + n) eps_n[p - p0] = e4[k];
        }
    }
    return ADC_OK;
}

ADC_EXPORT int adc_es_update_host(const adc_es_config *cfg, uint64_t seed, int32_t members, int64_t n_params, const double *fitness_m,
                                  int64_t generation, float *theta_p, float *m_p, float *v_p, float *grad_p)
{
    if (adc_es_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (members < 2 || (members & 1) || n_params < 1 || n_params > 0x7FFFFFFFll || generation < 0 || generation > 0x7FFFFFFFll || !fitness_m ||
        !theta_p || !m_p || !v_p)
        return ADC_EINVAL;
    const int M = members;
    const uint64_t key = adc::es_key(seed);
    std::vector<double> du;
    adc::es_shape(cfg->shaping == ADC_ES_RAW ? adc::kEsRaw : adc::kEsCenteredRank, fitness_m, M, du);
    adc::EsStep step{};
    step.optimiser = cfg->optimiser == ADC_ES_SGD ? adc::kEsSgd : adc::kEsAdam;
    step.lr = cfg->lr; step.beta1 = cfg->beta1; step.beta2 = cfg->beta2; step.eps = cfg->eps; step.l2 = cfg->l2;
    step.c1 = adc::es_bias_correction(step.beta1, (uint32_t)(generation + 1));
    step.c2 = adc::es_bias_correction(step.beta2, (uint32_t)(generation + 1));
    for (int64_t q = 0; q * 4 < n_params; ++q) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < M / 2; ++i) {
            float e4[4];
            adc::es_noise4(key, (uint32_t)q, (uint32_t)i, (uint32_t)generation, e4);
            for (int k = 0; k < 4; ++k) acc[k] = adc::es_grad_step(acc[k], du[(size_t)i], e4[k]);
        }
        for (int k = 0; k < 4 && q * 4 + k < n_params; ++k) {
            const int64_t p = q * 4 + k;
            const float g = adc::es_decay(adc::es_grad_finish(acc[k], M, cfg->sigma), theta_p[p], step.l2);
            theta_p[p] = adc::es_apply(step, theta_p[p], g, m_p[p], v_p[p]);
            if (grad_p) grad_p[p] = g;
        }
    }
    return ADC_OK;
}

namespace {
// the observation moments of S rows of D columns merged into the running state, column by column (adc_norm.h); raw: the rows are raw
// observations (adc_td3_norm.h)
void obs_norm_columns(const adc::NormConfig &c, bool raw, int64_t S, int32_t D, const float *x_sd, int64_t *count, double *mean_d, double *m2_d,
                      float *shift_d, float *scale_d)
{
    const int64_t count0 = *count;
    int64_t cnt = count0;
    for (int32_t j = 0; j < D; ++j) {
        const double sx = adc::pg_csum(S, [&](double part, int64_t i) { return adc::norm_chain_sum(part, x_sd[(size_t)i * (size_t)D + (size_t)j]); });
        const double qx = adc::pg_csum(S, [&](double part, int64_t i) {
            const float x = x_sd[(size_t)i * (size_t)D + (size_t)j];
            return adc::pg_chain_mac(part, x, x);
        });
        cnt = count0;
        adc::norm_finish(c, raw, sx, qx, S, cnt, mean_d[j], m2_d[j], shift_d[j], scale_d[j]);
    }
    *count = cnt;
}

// the discounted returns of `days` days of num_envs envs, their moments merged into the running state, the envs' carry advanced
// (adc_rew_norm.h)
void rew_norm_days(const adc::NormConfig &c, int32_t days, int32_t num_envs, const float *gamma_n, const float *reward_tn, const uint8_t *terminated_tn,
                   const uint8_t *truncated_tn, int64_t *count, double *mean, double *m2, float *scale, double *carry_n)
{
    const size_t N = (size_t)num_envs;
    const int64_t S = (int64_t)days * num_envs;
    std::vector<double> g((size_t)S);
    for (size_t n = 0; n < N; ++n) {
        double G = carry_n[n];
        for (int t = 0; t < days; ++t) {
            const size_t i = (size_t)t * N + n;
            g[i] = adc::rew_norm_scan_day(G, gamma_n[n], reward_tn[i], terminated_tn[i] | truncated_tn[i]);
        }
        carry_n[n] = G;
    }
    const double sx = adc::pg_csum(S, [&](double part, int64_t i) { return adc::rew_norm_chain_sum(part, g[(size_t)i]); });
    const double qx = adc::pg_csum(S, [&](double part, int64_t i) { return adc::rew_norm_chain_sq(part, g[(size_t)i]); });
    adc::rew_norm_finish(c, sx, qx, S, *count, *mean, *m2, *scale);
}
}  // namespace

// ---- the running observation normaliser on the host (adc_norm.h: the code parts/kernel_norm.inc runs) ---------------------------
ADC_EXPORT int adc_obs_norm_config_check(const adc_obs_norm_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_obs_norm_config)) msg = "adc_obs_norm_config: NULL or struct_size mismatch";
    else if (!(cfg->min_std > 0.0 && cfg->min_std < (double)__builtin_inff())) msg = "min_std must be finite and > 0";
    else if (cfg->count_cap < 0) msg = "count_cap >= 0 (0: no forgetting)";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_obs_norm_host(const adc_obs_norm_config *cfg, int64_t S, int32_t D, const float *x_sd, int64_t *count, double *mean_d, double *m2_d,
                                 float *shift_d, float *scale_d)
{
    if (adc_obs_norm_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (S < 1 || D < 1 || !x_sd || !count || !mean_d || !m2_d || !shift_d || !scale_d || *count < 0) return ADC_EINVAL;
    obs_norm_columns(adc::NormConfig{cfg->min_std, cfg->count_cap}, /* raw = */ false, S, D, x_sd, count, mean_d, m2_d, shift_d, scale_d);
    return ADC_OK;
}

// ---- policy-gradient training on the host (adc_pg.h: the code parts/kernel_pg.inc runs) ---------------------------------------
ADC_EXPORT int adc_pg_config_check(const adc_pg_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_pg_config)) msg = "adc_pg_config: NULL or struct_size mismatch";
    else if (!(cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) msg = "gamma: 0 to 1";
    else if (!(cfg->lambda >= 0.0f && cfg->lambda <= 1.0f)) msg = "lambda: 0 to 1";
    else if (!(cfg->eps_clip < 1.0f)) msg = "eps_clip < 1 (<= 0: no clip)";
    else if (!(cfg->vf_coef >= 0.0f && cfg->vf_coef < inf)) msg = "vf_coef >= 0";
    else if (!(cfg->ent_coef >= 0.0f && cfg->ent_coef < inf)) msg = "ent_coef >= 0";
    else if (!(cfg->reward_scale != 0.0f && cfg->reward_scale > -inf && cfg->reward_scale < inf)) msg = "reward_scale must be finite and not 0";
    else if (!(cfg->max_grad_norm >= 0.0f && cfg->max_grad_norm < inf)) msg = "max_grad_norm >= 0 (0: off)";
    else if (cfg->optimiser != ADC_PG_ADAM && cfg->optimiser != ADC_PG_SGD) msg = "unknown optimiser";
    else if (!(cfg->lr >= 0.0f && cfg->lr < inf)) msg = "lr >= 0";
    else if (cfg->optimiser == ADC_PG_ADAM && (!(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f) || !(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f)))
        msg = "Adam: 0 <= beta1, beta2 < 1";
    else if (cfg->optimiser == ADC_PG_ADAM && !(cfg->eps > 0.0f)) msg = "Adam: eps > 0";
    else if (cfg->minibatch_envs < 0) msg = "minibatch_envs >= 0 (0: all envs)";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

// the configurations of a learner population: `count` = 1 (shared by all members) or `members` of them
ADC_EXPORT int adc_pg_pop_config_check(const adc_pg_config *cfgs, int32_t count, int32_t num_envs, int32_t members, const char **message)
{
    const char *msg = nullptr;
    if (!cfgs) msg = "adc_pg_config array is NULL";
    else if (num_envs < 1 || members < 1 || num_envs % members != 0) msg = "members must be positive and divide num_envs";
    else if (count != 1 && count != members) msg = "count: 1 (one configuration shared by all members) or the number of members";
    else {
        const int n = num_envs / members;
        for (int i = 0; i < count && !msg; ++i) {
            if (adc_pg_config_check(cfgs + i, &msg) != ADC_OK) break;
            if (cfgs[i].minibatch_envs != cfgs[0].minibatch_envs) msg = "minibatch_envs must be equal in all members' configurations (their minibatches run in the same launches)";
        }
        if (!msg) {
            const int mb = cfgs[0].minibatch_envs == 0 ? n : cfgs[0].minibatch_envs;
            if (mb > n || n % mb != 0) msg = "minibatch_envs must divide the envs of a member (num_envs / members)";
        }
    }
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_pg_gae_host(const adc_pg_config *cfg, int32_t days, int32_t num_envs, const float *reward_tn, const uint8_t *terminated_tn,
                               const uint8_t *truncated_tn, const float *value_tn, const float *bootstrap_n, float *adv_tn, float *ret_tn)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (days < 1 || num_envs < 1 || !reward_tn || !terminated_tn || !truncated_tn || !value_tn || !bootstrap_n || !adv_tn || !ret_tn) return ADC_EINVAL;
    const size_t N = (size_t)num_envs;
    const float gl = cfg->gamma * cfg->lambda;
    for (size_t n = 0; n < N; ++n) {
        float adv = 0.0f, next = bootstrap_n[n];
        for (int t = days - 1; t >= 0; --t) {
            const size_t i = (size_t)t * N + n;
            const float v = value_tn[i];
            const float a = adc::pg_gae_day(reward_tn[i], cfg->reward_scale, terminated_tn[i] | truncated_tn[i], v, next, cfg->gamma, gl, adv);
            adv_tn[i] = a;
            ret_tn[i] = a + v;
            next = v;
        }
    }
    if (cfg->normalize_advantages) {
        const int64_t cnt = (int64_t)days * num_envs;
        const double mean = adc::pg_csum(cnt, [&](double part, int64_t i) { return part + (double)adv_tn[i]; }) / (double)cnt;
        const double var = adc::pg_csum(cnt, [&](double part, int64_t i) { return adc::pg_chain_sqdev(part, adv_tn[i], mean); }) / (double)cnt;
        const double sd = std::sqrt(var);
        for (int64_t i = 0; i < cnt; ++i) adv_tn[i] = adc::pg_normalized(adv_tn[i], mean, sd);
    }
    return ADC_OK;
}

// ---- the running reward normaliser on the host (adc_rew_norm.h: the code parts/kernel_norm.inc runs) ----------------------------
ADC_EXPORT int adc_rew_norm_config_check(const adc_rew_norm_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_rew_norm_config)) msg = "adc_rew_norm_config: NULL or struct_size mismatch";
    else if (!(cfg->min_std > 0.0 && cfg->min_std < (double)__builtin_inff())) msg = "min_std must be finite and > 0";
    else if (!(cfg->clip >= 0.0f && cfg->clip < __builtin_inff())) msg = "clip must be finite and >= 0 (0: off)";
    else if (cfg->count_cap < 0) msg = "count_cap >= 0 (0: no forgetting)";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_rew_norm_host(const adc_rew_norm_config *cfg, int32_t days, int32_t num_envs, const float *gamma_n, const float *reward_tn,
                                 const uint8_t *terminated_tn, const uint8_t *truncated_tn, int64_t *count, double *mean, double *m2, float *scale,
                                 double *carry_n)
{
    if (adc_rew_norm_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (days < 1 || num_envs < 1 || !gamma_n || !reward_tn || !terminated_tn || !truncated_tn || !count || !mean || !m2 || !scale || !carry_n || *count < 0)
        return ADC_EINVAL;
    rew_norm_days(adc::NormConfig{cfg->min_std, cfg->count_cap}, days, num_envs, gamma_n, reward_tn, terminated_tn, truncated_tn, count, mean, m2, scale, carry_n);
    return ADC_OK;
}

ADC_EXPORT int adc_pg_gae_norm_host(const adc_pg_config *cfg, int32_t days, int32_t num_envs, const float *reward_tn, const uint8_t *terminated_tn,
                                    const uint8_t *truncated_tn, const float *value_tn, const float *bootstrap_n, const float *scale_n, float clip,
                                    float *adv_tn, float *ret_tn)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (days < 1 || num_envs < 1 || !reward_tn || !terminated_tn || !truncated_tn || !value_tn || !bootstrap_n || !scale_n || !adv_tn || !ret_tn ||
        !(clip >= 0.0f))
        return ADC_EINVAL;
    const size_t N = (size_t)num_envs;
    const float gl = cfg->gamma * cfg->lambda;
    for (size_t n = 0; n < N; ++n) {
        float adv = 0.0f, next = bootstrap_n[n];
        for (int t = days - 1; t >= 0; --t) {
            const size_t i = (size_t)t * N + n;
            const float v = value_tn[i];
            const float a = adc::rew_norm_gae_day(reward_tn[i], cfg->reward_scale, scale_n[n], clip, terminated_tn[i] | truncated_tn[i], v, next, cfg->gamma,
                                                  gl, adv);
            adv_tn[i] = a;
            ret_tn[i] = a + v;
            next = v;
        }
    }
    if (cfg->normalize_advantages) {
        const int64_t cnt = (int64_t)days * num_envs;
        const double mean = adc::pg_csum(cnt, [&](double part, int64_t i) { return part + (double)adv_tn[i]; }) / (double)cnt;
        const double var = adc::pg_csum(cnt, [&](double part, int64_t i) { return adc::pg_chain_sqdev(part, adv_tn[i], mean); }) / (double)cnt;
        const double sd = std::sqrt(var);
        for (int64_t i = 0; i < cnt; ++i) adv_tn[i] = adc::pg_normalized(adv_tn[i], mean, sd);
    }
    return ADC_OK;
}

// ---- the TD3 learners' running normalisers on the host (adc_td3_norm.h: the code parts/kernel_norm.inc runs) --------------------
ADC_EXPORT int adc_td3_norm_config_check(const adc_td3_norm_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_td3_norm_config)) msg = "adc_td3_norm_config: NULL or struct_size mismatch";
    else if (!cfg->observations && !cfg->rewards) msg = "observations or rewards: at least one must be nonzero";
    else if (!(cfg->obs_min_std > 0.0 && cfg->obs_min_std < (double)__builtin_inff())) msg = "obs_min_std must be finite and > 0";
    else if (cfg->obs_count_cap < 0) msg = "obs_count_cap >= 0 (0: no forgetting)";
    else if (!(cfg->rew_min_std > 0.0 && cfg->rew_min_std < (double)__builtin_inff())) msg = "rew_min_std must be finite and > 0";
    else if (cfg->rew_count_cap < 0) msg = "rew_count_cap >= 0 (0: no forgetting)";
    else if (!(cfg->rew_clip >= 0.0f && cfg->rew_clip < __builtin_inff())) msg = "rew_clip must be finite and >= 0 (0: off)";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_td3_norm_obs_host(const adc_td3_norm_config *cfg, int64_t S, int32_t D, const float *x_sd, int64_t *count, double *mean_d, double *m2_d,
                                     float *shift_d, float *scale_d)
{
    if (adc_td3_norm_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (S < 1 || D < 1 || !x_sd || !count || !mean_d || !m2_d || !shift_d || !scale_d || *count < 0) return ADC_EINVAL;
    obs_norm_columns(adc::NormConfig{cfg->obs_min_std, cfg->obs_count_cap}, /* raw = */ true, S, D, x_sd, count, mean_d, m2_d, shift_d, scale_d);
    return ADC_OK;
}

ADC_EXPORT int adc_td3_norm_rew_host(const adc_td3_norm_config *cfg, int32_t days, int32_t num_envs, const float *gamma_n, const float *reward_tn,
                                     const uint8_t *terminated_tn, const uint8_t *truncated_tn, int64_t *count, double *mean, double *m2, float *scale,
                                     double *carry_n)
{
    if (adc_td3_norm_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (days < 1 || num_envs < 1 || !gamma_n || !reward_tn || !terminated_tn || !truncated_tn || !count || !mean || !m2 || !scale || !carry_n || *count < 0)
        return ADC_EINVAL;
    rew_norm_days(adc::NormConfig{cfg->rew_min_std, cfg->rew_count_cap}, days, num_envs, gamma_n, reward_tn, terminated_tn, truncated_tn, count, mean, m2, scale, carry_n);
    return ADC_OK;
}

// ---- prioritised replay on the host (adc_per.h: the code parts/kernel_per.inc runs) ----------------------------------------------
ADC_EXPORT int adc_replay_prio_config_check(const adc_replay_prio_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_replay_prio_config)) msg = "adc_replay_prio_config: NULL or struct_size mismatch";
    else if (!(cfg->alpha >= 0.0f && cfg->alpha <= 1.0f)) msg = "alpha must be in [0, 1]";
    else if (!(cfg->beta >= 0.0f && cfg->beta <= 1.0f)) msg = "beta must be in [0, 1]";
    else if (!(cfg->eps > 0.0f && cfg->eps < inf)) msg = "eps must be finite and > 0";
    else if (!(cfg->cap > cfg->eps && cfg->cap < inf)) msg = "cap must be finite and > eps";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

static bool per_tree_of(adc::PerTree &t, int64_t capacity, const float *leaf_c)
{
    for (int64_t i = 0; i < capacity; ++i) {
        if (!(leaf_c[i] >= 0.0f && leaf_c[i] < __builtin_inff())) return false;
        t.leaf[(size_t)i] = leaf_c[i];
    }
    t.rebuild();
    return true;
}

ADC_EXPORT int adc_per_tree_host(int64_t capacity, const float *leaf_c, double *nodes, int64_t *counts)
{
    if (capacity < 1 || capacity > (int64_t)1 << 31 || !leaf_c) return ADC_EINVAL;
    adc::PerTree t(capacity);
    if (!per_tree_of(t, capacity, leaf_c)) return ADC_EINVAL;
    if (counts)
        for (int l = 0; l <= adc::kPerMaxLevels; ++l) counts[l] = l <= t.sh.levels ? t.sh.n[l] : 0;
    if (nodes)
        for (int l = 1; l <= t.sh.levels; ++l)
            for (int64_t i = 0; i < t.sh.n[l]; ++i) *nodes++ = t.node[l][(size_t)i];
    return t.sh.levels;
}

ADC_EXPORT int adc_per_descend_host(int64_t capacity, const float *leaf_c, double m, int64_t *slot)
{
    if (capacity < 1 || capacity > (int64_t)1 << 31 || !leaf_c || !slot) return ADC_EINVAL;
    adc::PerTree t(capacity);
    if (!per_tree_of(t, capacity, leaf_c)) return ADC_EINVAL;
    *slot = t.descend(m);
    return ADC_OK;
}

ADC_EXPORT int adc_per_sample_host(const adc_replay_prio_config *cfg, int64_t capacity, int64_t size, const float *leaf_c, uint64_t seed, int64_t update,
                                   int32_t count, int32_t *idx_b, float *weight_b)
{
    if (adc_replay_prio_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (capacity < 1 || capacity > (int64_t)1 << 31 || size < 1 || size > capacity || !leaf_c || count < 1 || update < 0 || update >= 0xFFFFFFFFll)
        return ADC_EINVAL;
    adc::PerTree t(capacity);
    if (!per_tree_of(t, capacity, leaf_c)) return ADC_EINVAL;
    const uint64_t key = adc::td3_key(seed);
    std::vector<int64_t> slots((size_t)count);
    float lmin = __builtin_inff();
    for (int32_t b = 0; b < count; ++b) {
        const double m = adc::per_u53(key, (uint32_t)b, (uint32_t)update) * t.total();
        int64_t s = t.descend(m);
        if (s >= size) s = size - 1;
        slots[(size_t)b] = s;
        const float lf = t.leaf[(size_t)s];
        lmin = lf < lmin ? lf : lmin;
    }
    for (int32_t b = 0; b < count; ++b) {
        if (idx_b) idx_b[b] = (int32_t)slots[(size_t)b];
        if (weight_b) weight_b[b] = adc::per_weight(lmin, t.leaf[(size_t)slots[(size_t)b]], cfg->beta);
    }
    return ADC_OK;
}

ADC_EXPORT int adc_per_priority_host(const adc_replay_prio_config *cfg, int32_t count, const float *d1_b, const float *d2_b, float *pa_b)
{
    if (adc_replay_prio_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || !d1_b || !d2_b || !pa_b) return ADC_EINVAL;
    for (int32_t b = 0; b < count; ++b) pa_b[b] = adc::per_pa(adc::per_priority(d1_b[b], d2_b[b], cfg->eps, cfg->cap), cfg->alpha);
    return ADC_OK;
}

ADC_EXPORT int adc_per_leaf_update_host(int64_t capacity, float *leaf_c, float *top, int32_t count, const int32_t *idx_b, const float *pa_b)
{
    if (capacity < 1 || !leaf_c || !top || count < 1 || !idx_b || !pa_b) return ADC_EINVAL;
    for (int32_t b = 0; b < count; ++b)
        if (idx_b[b] < 0 || idx_b[b] >= capacity) return ADC_EINVAL;
    // (as the device: every element writes the largest pa among the elements that drew its slot)
    for (int32_t b = 0; b < count; ++b) {
        float hi = pa_b[b];
        for (int32_t o = 0; o < count; ++o)
            if (idx_b[o] == idx_b[b] && pa_b[o] > hi) hi = pa_b[o];
        leaf_c[idx_b[b]] = hi;
        *top = hi > *top ? hi : *top;
    }
    return ADC_OK;
}

ADC_EXPORT int adc_td3_y_norm_host(const adc_td3_config *td3, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, float scale, float clip,
                                   float *y_b)
{
    if (adc_td3_config_check(td3, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || !r_b || !done_b || !q_b || !y_b || !(clip >= 0.0f)) return ADC_EINVAL;
    const adc::Td3Law law = adc::td3_law_of(*td3);
    for (int32_t b = 0; b < count; ++b) y_b[b] = adc::td3_y_norm(r_b[b], done_b[b], q_b[b], law, scale, clip);
    return ADC_OK;
}

// ---- the SAC learners' running normalisers on the host (adc_sac_norm.h; the moments' twins are the TD3 normalisers' above) --------
ADC_EXPORT int adc_sac_norm_config_check(const adc_sac_norm_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_sac_norm_config)) msg = "adc_sac_norm_config: NULL or struct_size mismatch";
    else if (!cfg->observations && !cfg->rewards) msg = "observations or rewards: at least one must be nonzero";
    else if (!(cfg->obs_min_std > 0.0 && cfg->obs_min_std < (double)__builtin_inff())) msg = "obs_min_std must be finite and > 0";
    else if (cfg->obs_count_cap < 0) msg = "obs_count_cap >= 0 (0: no forgetting)";
    else if (!(cfg->rew_min_std > 0.0 && cfg->rew_min_std < (double)__builtin_inff())) msg = "rew_min_std must be finite and > 0";
    else if (cfg->rew_count_cap < 0) msg = "rew_count_cap >= 0 (0: no forgetting)";
    else if (!(cfg->rew_clip >= 0.0f && cfg->rew_clip < __builtin_inff())) msg = "rew_clip must be finite and >= 0 (0: off)";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_sac_y_norm_host(const adc_sac_config *sac, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *lp_b,
                                   float alpha, float scale, float clip, float *y_b)
{
    if (adc_sac_config_check(sac, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || !r_b || !done_b || !q_b || !lp_b || !y_b || !(clip >= 0.0f)) return ADC_EINVAL;
    // (sac_y_norm reads gamma and reward_scale of the law alone)
    const adc::SacLaw law{sac->gamma, sac->tau, sac->reward_scale, sac->eps_sq, 0.0f, 0.0f};
    for (int32_t b = 0; b < count; ++b) y_b[b] = adc::sac_y_norm(r_b[b], done_b[b], q_b[b], alpha, lp_b[b], law, scale, clip);
    return ADC_OK;
}

// ---- n-step returns on the host (adc_td3.h "n-step") ------------------------------------------------------------------------------
ADC_EXPORT int adc_replay_nstep_check(int32_t n, const char **message)
{
    const char *msg = (n < 1 || n > adc::kNstepMax) ? "n: 1 to 16 days" : nullptr;
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_replay_nstep_host(int32_t n, float gamma, int32_t T, int32_t N, int32_t t0, int32_t t1, const float *reward, const uint8_t *term,
                                     const uint8_t *trunc, float *R, uint8_t *done, float *gn, int32_t *m)
{
    if (adc_replay_nstep_check(n, nullptr) != ADC_OK) return ADC_EINVAL;
    if (T < 1 || N < 1 || t0 < 0 || t1 <= t0 || t1 > T || !reward || !term || !trunc) return ADC_EINVAL;
    for (int32_t t = t0; t < t1; ++t)
        for (int32_t e = 0; e < N; ++e) {
            const size_t row = (size_t)t * (size_t)N + (size_t)e, s = (size_t)(t - t0) * (size_t)N + (size_t)e;
            const adc::Td3Window w = adc::td3_nstep_window(reward + row, term + row, trunc + row, (size_t)N, t1 - t, n, gamma);
            if (R) R[s] = w.R;
            if (done) done[s] = (uint8_t)w.done;
            if (gn) gn[s] = w.g;
            if (m) m[s] = w.m;
        }
    return ADC_OK;
}

ADC_EXPORT int adc_td3_y_nstep_host(const adc_td3_config *td3, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *gn_b,
                                    float scale, float clip, float *y_b)
{
    if (adc_td3_config_check(td3, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || !r_b || !done_b || !q_b || !gn_b || !y_b || !(clip >= 0.0f)) return ADC_EINVAL;
    const adc::Td3Law law = adc::td3_law_of(*td3);
    for (int32_t b = 0; b < count; ++b) y_b[b] = adc::td3_y_norm_g(r_b[b], done_b[b], q_b[b], gn_b[b], law, scale, clip);
    return ADC_OK;
}

ADC_EXPORT int adc_sac_y_nstep_host(const adc_sac_config *sac, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *lp_b,
                                    const float *gn_b, float alpha, float scale, float clip, float *y_b)
{
    if (adc_sac_config_check(sac, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || !r_b || !done_b || !q_b || !lp_b || !gn_b || !y_b || !(clip >= 0.0f)) return ADC_EINVAL;
    // (sac_y_norm_g reads reward_scale of the law alone)
    const adc::SacLaw law{sac->gamma, sac->tau, sac->reward_scale, sac->eps_sq, 0.0f, 0.0f};
    for (int32_t b = 0; b < count; ++b) y_b[b] = adc::sac_y_norm_g(r_b[b], done_b[b], q_b[b], alpha, lp_b[b], gn_b[b], law, scale, clip);
    return ADC_OK;
}

ADC_EXPORT int adc_pg_param_count_host(const adc_mlp_config *mlp, int32_t num_keywords, int64_t *count)
{
    if (!count || adc_mlp_config_check(mlp, num_keywords, nullptr) != ADC_OK) return ADC_EINVAL;
    *count = adc::pg_param_count(adc::pg_shape_of(*mlp, num_keywords));
    return ADC_OK;
}

namespace {
// the gradient of `count` samples; addon_of(s): the sample's add-on (adc::PgNoAddon, or adc_pg_kl.h's)
// (`loss`: the configuration's constants - adc_pg_config's, or the imitation loss's vf_coef alone)
template <class AddonOf>
int pg_grad_host_core(const adc_mlp_config *mlp, int32_t num_keywords, const adc::PgLoss &loss, const float *theta_q, int64_t count, const float *obs_sd,
                      const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s, const float *value_old_s, float *grad_q,
                      double *sums10, adc_pg_stats *stats, AddonOf addon_of)
{
    if (adc_mlp_config_check(mlp, num_keywords, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || count > 0x7FFFFFFFll || !theta_q || !obs_sd || !action_sa || !logp_old_s || !adv_s || !ret_s || !value_old_s || !grad_q) return ADC_EINVAL;
    const adc::PgShape sh = adc::pg_shape_of(*mlp, num_keywords);
    const size_t S = (size_t)count, na = (size_t)adc::pg_acts_floats(sh), nd = (size_t)adc::pg_deltas_floats(sh), D = (size_t)sh.D, A = (size_t)sh.A;
    std::vector<float> acts(S * std::max<size_t>(na, 1)), deltas(S * nd), pieces(S * adc::kPgPieces);
    for (size_t s = 0; s < S; ++s)
        adc::pg_sample_host_with(sh, loss, theta_q, obs_sd + s * D, action_sa + s * A, logp_old_s[s], adv_s[s], ret_s[s], value_old_s[s],
                                 acts.data() + s * na, deltas.data() + s * nd, pieces.data() + s * adc::kPgPieces, addon_of(s));
    // the gradient's terms in the flat order: every layer (its bias the row j = n_in with x = 1), then log_std's row
    size_t q = 0, ao = 0, dof = 0;
    auto term = [&](const float *X, size_t ldx, int n_in, size_t d_off, int n_out) {
        for (int j = 0; j <= n_in; ++j)
            for (int h = 0; h < n_out; ++h) {
                const double total = adc::pg_csum(count, [&](double part, int64_t s) {
                    return adc::pg_chain_mac(part, j < n_in ? X[(size_t)s * ldx + (size_t)j] : 1.0f, deltas[(size_t)s * nd + d_off + (size_t)h]);
                });
                grad_q[q++] = adc::pg_grad_finish(total, count);
            }
    };
    for (int net = 0; net < 2; ++net) {
        for (int l = 0; l < sh.layers[net]; ++l) {
            const int n_in = adc::pg_n_in(sh, net, l), n_out = sh.n_out[net][l];
            if (l == 0) term(obs_sd, D, n_in, dof, n_out);
            else { term(acts.data() + ao, na, n_in, dof, n_out); ao += (size_t)n_in; }
            dof += (size_t)n_out;
        }
    }
    if (!sh.two_heads) term(nullptr, 0, 0, dof, sh.A);
    double sums[adc::kPgSums];
    for (int c = 0; c < 7; ++c) sums[c] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)pieces[(size_t)s * adc::kPgPieces + (size_t)c]; });
    for (int c = 0; c < 2; ++c)
        sums[7 + c] = adc::pg_csum(count, [&](double part, int64_t s) {
            const float x = pieces[(size_t)s * adc::kPgPieces + (size_t)(adc::kPgRet + c)];
            return adc::pg_chain_mac(part, x, x);
        });
    sums[9] = adc::pg_csum((int64_t)q, [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_q[p], grad_q[p]); });
    if (sums10) std::copy(sums, sums + adc::kPgSums, sums10);
    if (stats) {
        const adc::PgStatsOut o = adc::pg_stats_finish(sums, count);
        stats->steps = 0; stats->samples = count;
        stats->policy_loss = o.policy_loss; stats->value_loss = o.value_loss; stats->entropy = o.entropy; stats->approx_kl = o.approx_kl;
        stats->clip_fraction = o.clip_fraction; stats->grad_norm = o.grad_norm; stats->explained_variance = o.explained_variance;
    }
    return ADC_OK;
}
template <class AddonOf>
int pg_grad_host_run(const adc_mlp_config *mlp, int32_t num_keywords, const adc_pg_config *cfg, const float *theta_q, int64_t count, const float *obs_sd,
                     const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s, const float *value_old_s, float *grad_q,
                     double *sums10, adc_pg_stats *stats, AddonOf addon_of)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    return pg_grad_host_core(mlp, num_keywords, adc::PgLoss{cfg->eps_clip, cfg->vf_coef, cfg->ent_coef}, theta_q, count, obs_sd, action_sa, logp_old_s, adv_s,
                             ret_s, value_old_s, grad_q, sums10, stats, addon_of);
}
}  // namespace

ADC_EXPORT int adc_pg_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_pg_config *cfg, const float *theta_q, int64_t count,
                                const float *obs_sd, const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s,
                                const float *value_old_s, float *grad_q, double *sums10, adc_pg_stats *stats)
{
    return pg_grad_host_run(mlp, num_keywords, cfg, theta_q, count, obs_sd, action_sa, logp_old_s, adv_s, ret_s, value_old_s, grad_q, sums10, stats,
                            [](size_t) { return adc::PgNoAddon{}; });
}

// ---- imitation learning on the host (adc_imitation.h: the code parts/kernel_imitation.inc runs) -----------------------------------
ADC_EXPORT int adc_im_config_check(const adc_im_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_im_config)) msg = "adc_im_config: NULL or struct_size mismatch";
    else if (!(cfg->beta >= 0.0f && cfg->beta < inf)) msg = "beta >= 0 and finite (0: behaviour cloning)";
    else if (!(cfg->vf_coef >= 0.0f && cfg->vf_coef < inf)) msg = "vf_coef >= 0 and finite";
    else if (!(cfg->w_max >= 0.0f && cfg->w_max < inf)) msg = "w_max >= 0 and finite (0: no cap)";
    else if (!(cfg->ma_start >= 0.0 && cfg->ma_start < (double)inf)) msg = "ma_start >= 0 and finite";
    else if (!(cfg->ma_rate >= 0.0 && cfg->ma_rate <= 1.0)) msg = "ma_rate in [0, 1]";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_im_weight_host(const adc_im_config *cfg, int64_t count, const float *adv_s, double *ma, float *c, float *w_s)
{
    if (adc_im_config_check(cfg, nullptr) != ADC_OK || count < 1 || !adv_s || !ma || !c) return ADC_EINVAL;
    const double sumsq = adc::pg_csum(count, [&](double part, int64_t i) { return adc::pg_chain_mac(part, adv_s[i], adv_s[i]); });
    *ma = adc::im_ma_next(*ma, cfg->ma_rate, sumsq, count, *c);
    const adc::ImLaw law{cfg->beta, *c, cfg->w_max, cfg->train_log_std != 0 ? 1 : 0};
    if (w_s)
        for (int64_t i = 0; i < count; ++i) w_s[i] = adc::im_weight(adv_s[i], law);
    return ADC_OK;
}

ADC_EXPORT int adc_im_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_im_config *cfg, float c, const float *theta_q, int64_t count,
                                const float *obs_sd, const float *action_sa, const float *adv_s, const float *ret_s, const float *value_old_s, float *grad_q,
                                double *sums10, adc_im_stats *stats)
{
    if (adc_im_config_check(cfg, nullptr) != ADC_OK || count < 1 || count > 0x7FFFFFFFll) return ADC_EINVAL;
    const adc::ImLaw law{cfg->beta, c, cfg->w_max, cfg->train_log_std != 0 ? 1 : 0};
    const std::vector<float> zeros((size_t)count, 0.0f);        // (the record's logp of a teacher day: not read by the imitation loss)
    adc_pg_stats st{};
    const int rc = pg_grad_host_core(mlp, num_keywords, adc::PgLoss{0.0f, cfg->vf_coef, 0.0f}, theta_q, count, obs_sd, action_sa, zeros.data(), adv_s, ret_s,
                                     value_old_s, grad_q, sums10, &st, [&](size_t) { return adc::ImSampleHost{law}; });
    if (rc != ADC_OK) return rc;
    if (stats) {
        stats->steps = 0; stats->samples = count;
        stats->policy_loss = st.policy_loss; stats->value_loss = st.value_loss; stats->entropy = st.entropy; stats->logp = st.approx_kl;
        stats->weight = st.clip_fraction; stats->grad_norm = st.grad_norm; stats->explained_variance = st.explained_variance;
    }
    return ADC_OK;
}

// ---- DAgger on the host (adc_dagger.h: the code k_dagger_mix runs): 1 when the env's coin of the day picks the teacher -------------
ADC_EXPORT int adc_dagger_coin_host(uint64_t key, uint32_t tick, float beta)
{
    return adc::dagger_coin(key, tick, adc::bernoulli_threshold(beta)) ? 1 : 0;
}

// ---- the KL penalty and the value-loss clip on the host (adc_pg_kl.h: the code parts/kernel_pg_kl.inc runs) ---------------------
ADC_EXPORT int adc_pg_kl_config_check(const adc_pg_kl_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_pg_kl_config)) msg = "adc_pg_kl_config: NULL or struct_size mismatch";
    else if (!(cfg->kl_coef >= 0.0f && cfg->kl_coef < inf)) msg = "kl_coef >= 0 and finite";
    else if (cfg->adaptive && !(cfg->kl_target > 0.0f && cfg->kl_target < inf)) msg = "kl_target > 0 and finite when adaptive";
    else if (cfg->factor_up != 0.0f && !(cfg->factor_up > 1.0f && cfg->factor_up < inf)) msg = "factor_up > 1 and finite (0: 1.5)";
    else if (cfg->factor_down != 0.0f && !(cfg->factor_down > 0.0f && cfg->factor_down < 1.0f)) msg = "factor_down in (0, 1) (0: 0.5)";
    else if (!(cfg->vf_clip >= 0.0f && cfg->vf_clip < inf)) msg = "vf_clip >= 0 and finite (0: off)";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_pg_kl_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_pg_config *cfg, const float *theta_q, int64_t count,
                                   const float *obs_sd, const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s,
                                   const float *value_old_s, const adc_pg_kl_config *kl, float kl_coef, const float *mean_old_sa, const float *ls_old,
                                   int32_t ls_old_per_sample, float *grad_q, double *sums10, double *sums_kl2, adc_pg_stats *stats,
                                   adc_pg_kl_stats *kl_stats)
{
    if (adc_pg_kl_config_check(kl, nullptr) != ADC_OK || !(kl_coef >= 0.0f && kl_coef < __builtin_inff()) || !mean_old_sa || !ls_old) return ADC_EINVAL;
    if (count < 1 || count > 0x7FFFFFFFll || adc_mlp_config_check(mlp, num_keywords, nullptr) != ADC_OK) return ADC_EINVAL;
    const size_t S = (size_t)count, A = (size_t)num_keywords + 1u;
    std::vector<float> pk(S * adc::kPgKlPieces);
    const adc::PgKl law{kl_coef, kl->vf_clip};
    const int rc = pg_grad_host_run(mlp, num_keywords, cfg, theta_q, count, obs_sd, action_sa, logp_old_s, adv_s, ret_s, value_old_s, grad_q, sums10, stats,
                                    [&](size_t s) {
                                        return adc::PgKlSampleHost{law, mean_old_sa + s * A, ls_old_per_sample ? ls_old + s * A : ls_old,
                                                                   pk.data() + s * adc::kPgKlPieces};
                                    });
    if (rc != ADC_OK) return rc;
    double sums[adc::kPgKlPieces];
    for (int c = 0; c < adc::kPgKlPieces; ++c)
        sums[c] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)pk[(size_t)s * adc::kPgKlPieces + (size_t)c]; });
    if (sums_kl2) std::copy(sums, sums + adc::kPgKlPieces, sums_kl2);
    if (kl_stats) {
        kl_stats->kl = sums[adc::kPgKlKl] / (double)count;
        kl_stats->vf_clip_fraction = sums[adc::kPgKlVfClipped] / (double)count;
        kl_stats->kl_coef = kl_stats->kl_coef_next = kl_coef;
    }
    return ADC_OK;
}

ADC_EXPORT int adc_pg_kl_adapt_host(const adc_pg_kl_config *kl, float coef, double kl_mean, float *coef_next)
{
    if (adc_pg_kl_config_check(kl, nullptr) != ADC_OK || !coef_next) return ADC_EINVAL;
    *coef_next = adc::pg_kl_adapt(adc::pg_kl_adapt_of(*kl), coef, kl_mean);
    return ADC_OK;
}

// ---- shuffled sample-level minibatches and the target-KL stop on the host (adc_pg_shuffle.h: the code parts/kernel_pg_shuffle.inc runs)
ADC_EXPORT int adc_pg_shuffle_config_check(const adc_pg_shuffle_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_pg_shuffle_config)) msg = "adc_pg_shuffle_config: NULL or struct_size mismatch";
    else if (cfg->minibatch_samples < 1) msg = "minibatch_samples >= 1";
    else if (!(cfg->target_kl >= 0.0f && cfg->target_kl < __builtin_inff())) msg = "target_kl >= 0 and finite (0: never stop)";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_pg_shuffle_order_host(uint64_t seed, int64_t n_s, uint32_t tick, uint32_t *order_out)
{
    if (n_s < 1 || n_s > 0x7FFFFFFFll || !order_out) return ADC_EINVAL;
    const uint64_t key = adc::pg_shuffle_key(seed);
    const uint32_t n = (uint32_t)n_s, h = adc::pg_shuffle_half_bits(n);
    for (uint32_t i = 0; i < n; ++i) order_out[i] = adc::pg_shuffle_sample(key, i, n, h, tick);
    return ADC_OK;
}

ADC_EXPORT int adc_pg_shuffle_stop_host(double approx_kl, float target_kl, int32_t *stop)
{
    if (!stop || !(target_kl >= 0.0f && target_kl < __builtin_inff())) return ADC_EINVAL;
    *stop = adc::pg_shuffle_stop(approx_kl, target_kl) ? 1 : 0;
    return ADC_OK;
}

// the host twin of k_pg_decide (parts/kernel_pg_queued.inc): adc_pg_shuffle.h's pg_decide on a live member's minibatch
ADC_EXPORT int adc_pg_decide_host(const adc_pg_config *cfg, float target_kl, const double *sums10, int64_t count, int32_t *evaluated, int32_t *stop,
                                  int32_t *clip, float *scale)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (!sums10 || count < 1 || !(target_kl >= 0.0f && target_kl < __builtin_inff())) return ADC_EINVAL;
    const adc::PgDecision d = adc::pg_decide(cfg->max_grad_norm, target_kl, 1, sums10, count);
    if (evaluated) *evaluated = 1;
    if (stop) *stop = d.stop;
    if (clip) *clip = d.clip;
    if (scale) *scale = d.scale;
    return ADC_OK;
}

ADC_EXPORT int adc_pg_step_host(const adc_pg_config *cfg, int64_t n_params, int64_t steps_taken, const float *grad_q, float *theta_q, float *m_q,
                                float *v_q)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (n_params < 1 || n_params > 0x7FFFFFFFll || steps_taken < 0 || steps_taken >= 0x7FFFFFFFll || !grad_q || !theta_q || !m_q || !v_q) return ADC_EINVAL;
    adc::EsStep step{};
    step.optimiser = cfg->optimiser == ADC_PG_SGD ? adc::kEsSgd : adc::kEsAdam;
    step.lr = cfg->lr; step.beta1 = cfg->beta1; step.beta2 = cfg->beta2; step.eps = cfg->eps; step.l2 = 0.0f;
    step.c1 = adc::es_bias_correction(step.beta1, (uint32_t)(steps_taken + 1));
    step.c2 = adc::es_bias_correction(step.beta2, (uint32_t)(steps_taken + 1));
    const bool clip = cfg->max_grad_norm > 0.0f;
    float scale = 1.0f;
    if (clip) {
        const double sq = adc::pg_csum(n_params, [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_q[p], grad_q[p]); });
        scale = adc::pg_clip_scale(cfg->max_grad_norm, std::sqrt(sq));
    }
    for (int64_t p = 0; p < n_params; ++p) {
        const float g = clip ? grad_q[p] * scale : grad_q[p];
        theta_q[p] = adc::pg_apply(step, theta_q[p], g, m_q[p], v_q[p]);
    }
    return ADC_OK;
}

// ---- off-policy (TD3) training on the host (adc_td3.h: the code parts/kernel_td3.inc runs) --------------------------------------
ADC_EXPORT int adc_td3_config_check(const adc_td3_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_td3_config)) msg = "adc_td3_config: NULL or struct_size mismatch";
    else if (!(cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) msg = "gamma: 0 to 1";
    else if (!(cfg->tau > 0.0f && cfg->tau <= 1.0f)) msg = "tau: above 0, at most 1";
    else if (cfg->policy_delay < 1) msg = "policy_delay >= 1";
    else if (!(cfg->target_noise >= 0.0f && cfg->target_noise < inf)) msg = "target_noise >= 0";
    else if (!(cfg->target_noise_clip >= 0.0f && cfg->target_noise_clip < inf)) msg = "target_noise_clip >= 0";
    else if (cfg->action_lo != cfg->action_lo || cfg->action_hi != cfg->action_hi) msg = "action_lo / action_hi must not be NaN (hi <= lo: no clamp)";
    else if (!(cfg->reward_scale != 0.0f && cfg->reward_scale > -inf && cfg->reward_scale < inf)) msg = "reward_scale must be finite and not 0";
    else if (cfg->batch_size < 1 || cfg->batch_size > (1 << 20)) msg = "batch_size: 1 to 2^20";
    else if (cfg->capacity < 1 || cfg->capacity > (1 << 30)) msg = "capacity: 1 to 2^30";
    else if (cfg->n_critic_layers < 1 || cfg->n_critic_layers > adc::kMlpMaxLayers) msg = "n_critic_layers: 1 to 4";
    else if (cfg->critic_widths[cfg->n_critic_layers - 1] != 1) msg = "the last critic layer has one output";
    else if (!(cfg->actor_lr >= 0.0f && cfg->actor_lr < inf)) msg = "actor_lr >= 0";
    else if (!(cfg->critic_lr >= 0.0f && cfg->critic_lr < inf)) msg = "critic_lr >= 0";
    else if (cfg->optimiser != ADC_TD3_ADAM && cfg->optimiser != ADC_TD3_SGD) msg = "unknown optimiser";
    else if (cfg->optimiser == ADC_TD3_ADAM && (!(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f) || !(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f)))
        msg = "Adam: 0 <= beta1, beta2 < 1";
    else if (cfg->optimiser == ADC_TD3_ADAM && !(cfg->eps > 0.0f)) msg = "Adam: eps > 0";
    else if (!(cfg->max_grad_norm >= 0.0f && cfg->max_grad_norm < inf)) msg = "max_grad_norm >= 0 (0: off)";
    else
        for (int l = 0; l + 1 < cfg->n_critic_layers; ++l)
            if (cfg->critic_widths[l] < 1 || cfg->critic_widths[l] > adc::kMlpMaxWidth) msg = "hidden critic widths: 1 to 256";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_td3_pop_config_check(const adc_td3_config *cfgs, int32_t count, int32_t num_envs, int32_t members, const char **message)
{
    const char *msg = nullptr;
    if (!cfgs) msg = "adc_td3_config array is NULL";
    else if (num_envs < 1 || members < 1 || members > 65535 || num_envs % members != 0) msg = "members must be positive, at most 65535, and divide num_envs";
    else if (count != 1 && count != members) msg = "count: 1 (one configuration shared by all members) or the number of members";
    else
        for (int i = 0; i < count && !msg; ++i) {
            const adc_td3_config &c = cfgs[i], &c0 = cfgs[0];
            if (adc_td3_config_check(&c, &msg) != ADC_OK) break;
            if (c.batch_size != c0.batch_size) msg = "batch_size must be equal in all members' configurations (their updates run in the same launches)";
            else if (c.capacity != c0.capacity) msg = "capacity must be equal in all members' configurations (their rings move together)";
            else if (c.policy_delay != c0.policy_delay) msg = "policy_delay must be equal in all members' configurations (their actor steps run in the same launches)";
            else if (c.n_critic_layers != c0.n_critic_layers) msg = "n_critic_layers / critic_widths must be equal in all members' configurations (the critics' shape is shared)";
            else
                for (int l = 0; l < c.n_critic_layers; ++l)
                    if (c.critic_widths[l] != c0.critic_widths[l]) msg = "n_critic_layers / critic_widths must be equal in all members' configurations (the critics' shape is shared)";
        }
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

namespace {
// the shape two configurations give, or false: a bad configuration or a two-headed policy
bool td3_host_shape(const adc_mlp_config *mlp, int32_t K, const adc_td3_config *cfg, bool norm, adc::Td3Shape *sh)
{
    if (adc_mlp_config_check(mlp, K, nullptr) != ADC_OK || adc_td3_config_check(cfg, nullptr) != ADC_OK) return false;
    if (mlp->policy_widths[mlp->n_policy_layers - 1] != K + 1) return false;
    *sh = adc::td3_shape_of(*mlp, K, *cfg, norm ? 1 : 0);
    return true;
}
// one network's gradient terms in the flat order: g[flat0 ...] = float32(csum over the batch / count)
void td3_net_grad_host(const adc::Td3Net &net, int64_t count, const float *X0, size_t ldx0, const float *ys, size_t ny, size_t y_off, const float *deltas,
                       size_t nd, size_t d_off, float *g)
{
    size_t q = 0, lo = 0;
    for (int l = 0; l < net.layers; ++l) {
        const int n_in = adc::td3_n_in(net, l), n_out = net.n_out[l];
        const float *X = l == 0 ? X0 : ys + y_off + lo - (size_t)n_in;
        const size_t ldx = l == 0 ? ldx0 : ny;
        for (int j = 0; j <= n_in; ++j)
            for (int h = 0; h < n_out; ++h) {
                const double total = adc::pg_csum(count, [&](double part, int64_t s) {
                    return adc::pg_chain_mac(part, j < n_in ? X[(size_t)s * ldx + (size_t)j] : 1.0f, deltas[(size_t)s * nd + d_off + lo + (size_t)h]);
                });
                g[q++] = adc::pg_grad_finish(total, count);
            }
        lo += (size_t)n_out;
    }
}
}  // namespace

ADC_EXPORT int adc_td3_param_counts_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, int64_t *actor_p, int64_t *critic_qc)
{
    adc::Td3Shape sh;
    if (!td3_host_shape(mlp, num_keywords, cfg, false, &sh)) return ADC_EINVAL;
    if (actor_p) *actor_p = adc::td3_params(sh.pol);
    if (critic_qc) *critic_qc = adc::td3_params(sh.q);
    return ADC_OK;
}

ADC_EXPORT int adc_td3_batch_indices_host(uint64_t seed, int64_t update, int64_t size, int32_t count, int32_t *idx_b)
{
    if (update < 0 || update >= 0xFFFFFFFFll || size < 1 || size > (1ll << 30) || count < 1 || !idx_b) return ADC_EINVAL;
    const uint64_t key = adc::td3_key(seed);
    for (int32_t b = 0; b < count; ++b) idx_b[b] = (int32_t)adc::td3_batch_index(key, (uint32_t)b, (uint32_t)update, (uint32_t)size);
    return ADC_OK;
}

namespace {
// adc_td3_target_host; bounded: under adc_td3.h "bounded" (shift_a and scale_a NULL)
int td3_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, uint64_t seed, int64_t update,
                    const float *theta_target_p, const float *psi_target_q, const float *shift_a, const float *scale_a, int32_t count,
                    const float *x2_bd, const float *r_b, const uint8_t *done_b, float *y_b, bool bounded)
{
    adc::Td3Shape sh;
    if (!td3_host_shape(mlp, num_keywords, cfg, shift_a != nullptr, &sh)) return ADC_EINVAL;
    if ((shift_a == nullptr) != (scale_a == nullptr) || update < 0 || update >= 0xFFFFFFFFll || count < 1 || !theta_target_p || !psi_target_q || !x2_bd ||
        !r_b || !done_b || !y_b)
        return ADC_EINVAL;
    const adc::Td3Law law = adc::td3_law_of(*cfg);
    const uint64_t key = adc::td3_key(seed);
    const size_t D = (size_t)sh.D, A = (size_t)sh.A, Qc = (size_t)adc::td3_params(sh.q);
    std::vector<float> row(D + A), yp((size_t)adc::td3_outs(sh.pol)), yq((size_t)adc::td3_outs(sh.q));
    for (int32_t b = 0; b < count; ++b) {
        std::copy(x2_bd + (size_t)b * D, x2_bd + (size_t)(b + 1) * D, row.begin());
        adc::td3_forward_host(sh.pol, sh.activation, theta_target_p, row.data(), yp.data());
        const float *mu = yp.data() + adc::td3_hidden(sh.pol);
        for (int a = 0; a < sh.A; ++a) {
            const float n = adc::td3_noise(key, a, (uint32_t)b, (uint32_t)update);
            if (bounded) { row[D + (size_t)a] = adc::td3_target_action(adc::mlp_tanh(mu[a]), n, adc::td3_law_bounded(law)); continue; }
            const float ap = adc::td3_target_action(mu[a], n, law);
            row[D + (size_t)a] = adc::td3_action_norm(ap, shift_a, scale_a, a, sh.norm);
        }
        float q[2];
        for (int i = 0; i < 2; ++i) {
            adc::td3_forward_host(sh.q, sh.activation, psi_target_q + (size_t)i * Qc, row.data(), yq.data());
            q[i] = yq[(size_t)adc::td3_hidden(sh.q)];
        }
        y_b[b] = adc::td3_y(r_b[b], done_b[b], adc::td3_min(q[0], q[1]), law);
    }
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_td3_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, uint64_t seed, int64_t update,
                                   const float *theta_target_p, const float *psi_target_q, const float *shift_a, const float *scale_a, int32_t count,
                                   const float *x2_bd, const float *r_b, const uint8_t *done_b, float *y_b)
{
    return td3_target_host(mlp, num_keywords, cfg, seed, update, theta_target_p, psi_target_q, shift_a, scale_a, count, x2_bd, r_b, done_b, y_b, false);
}

ADC_EXPORT int adc_td3_bounded_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, uint64_t seed, int64_t update,
                                           const float *theta_target_p, const float *psi_target_q, int32_t count, const float *x2_bd, const float *r_b,
                                           const uint8_t *done_b, float *y_b)
{
    if (cfg && cfg->action_hi > cfg->action_lo) return ADC_EINVAL;          // (the box is [-1, 1])
    return td3_target_host(mlp, num_keywords, cfg, seed, update, theta_target_p, psi_target_q, nullptr, nullptr, count, x2_bd, r_b, done_b, y_b, true);
}

ADC_EXPORT int adc_td3_critic_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *psi_q,
                                        const float *shift_a, const float *scale_a, int32_t count, const float *x_bd, const float *a_ba, const float *y_b,
                                        float *grad_q, double *sums6)
{
    adc::Td3Shape sh;
    if (!td3_host_shape(mlp, num_keywords, cfg, shift_a != nullptr, &sh)) return ADC_EINVAL;
    if ((shift_a == nullptr) != (scale_a == nullptr) || count < 1 || !psi_q || !x_bd || !a_ba || !y_b || !grad_q) return ADC_EINVAL;
    const size_t S = (size_t)count, D = (size_t)sh.D, A = (size_t)sh.A, DA = D + A, Qc = (size_t)adc::td3_params(sh.q), no = (size_t)adc::td3_outs(sh.q),
                 nh = (size_t)adc::td3_hidden(sh.q);
    std::vector<float> xin(S * DA), ys(S * 2 * no), deltas(S * 2 * no), pieces(S * adc::kTd3Pieces, 0.0f);
    for (size_t s = 0; s < S; ++s) {
        float *row = xin.data() + s * DA;
        std::copy(x_bd + s * D, x_bd + (s + 1) * D, row);
        for (int a = 0; a < sh.A; ++a) row[D + (size_t)a] = adc::td3_action_norm(a_ba[s * A + (size_t)a], shift_a, scale_a, a, sh.norm);
        for (size_t i = 0; i < 2; ++i) {
            float *y = ys.data() + s * 2 * no + i * no, *d = deltas.data() + s * 2 * no + i * no;
            adc::td3_forward_host(sh.q, sh.activation, psi_q + i * Qc, row, y);
            float loss;
            d[nh] = adc::td3_critic_delta(y[nh], y_b[s], loss);
            pieces[s * adc::kTd3Pieces + adc::kTd3Loss1 + i] = loss;
            pieces[s * adc::kTd3Pieces + adc::kTd3Q1 + i] = y[nh];
            adc::td3_backward_host(sh.q, sh.activation, psi_q + i * Qc, y, d);
        }
        pieces[s * adc::kTd3Pieces + adc::kTd3Y] = y_b[s];
    }
    for (size_t i = 0; i < 2; ++i)
        td3_net_grad_host(sh.q, count, xin.data(), DA, ys.data(), 2 * no, i * no, deltas.data(), 2 * no, i * no, grad_q + i * Qc);
    if (sums6) {
        for (int c = 0; c < 5; ++c) sums6[c] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)pieces[(size_t)s * adc::kTd3Pieces + (size_t)c]; });
        sums6[5] = adc::pg_csum((int64_t)(2 * Qc), [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_q[p], grad_q[p]); });
    }
    return ADC_OK;
}

namespace {
// adc_td3_actor_grad_host; bounded: under adc_td3.h "bounded" (shift_a and scale_a NULL)
int td3_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *theta_p, const float *psi_q,
                        const float *shift_a, const float *scale_a, int32_t count, const float *x_bd, float *grad_p, double *sums2, bool bounded)
{
    adc::Td3Shape sh;
    if (!td3_host_shape(mlp, num_keywords, cfg, shift_a != nullptr, &sh)) return ADC_EINVAL;
    if ((shift_a == nullptr) != (scale_a == nullptr) || count < 1 || !theta_p || !psi_q || !x_bd || !grad_p) return ADC_EINVAL;
    const size_t S = (size_t)count, D = (size_t)sh.D, A = (size_t)sh.A, po = (size_t)adc::td3_outs(sh.pol), ph = (size_t)adc::td3_hidden(sh.pol),
                 no = (size_t)adc::td3_outs(sh.q), nh = (size_t)adc::td3_hidden(sh.q);
    std::vector<float> ys(S * po), deltas(S * po), row(D + A), yq(no), dq(no), qpi(S);
    for (size_t s = 0; s < S; ++s) {
        float *y = ys.data() + s * po, *d = deltas.data() + s * po;
        std::copy(x_bd + s * D, x_bd + (s + 1) * D, row.begin());
        adc::td3_forward_host(sh.pol, sh.activation, theta_p, row.data(), y);
        for (int a = 0; a < sh.A; ++a)
            row[D + (size_t)a] = bounded ? adc::mlp_tanh(y[ph + (size_t)a]) : adc::td3_action_norm(y[ph + (size_t)a], shift_a, scale_a, a, sh.norm);
        adc::td3_forward_host(sh.q, sh.activation, psi_q, row.data(), yq.data());
        qpi[s] = yq[nh];
        dq[nh] = 1.0f;
        adc::td3_backward_host(sh.q, sh.activation, psi_q, yq.data(), dq.data());
        adc::td3_input_delta_host(sh.q, psi_q, dq.data(), sh.D, sh.A, d + ph);
        for (int a = 0; a < sh.A; ++a)
            d[ph + (size_t)a] = bounded ? adc::td3_dmu_bounded(d[ph + (size_t)a], row[D + (size_t)a])
                                        : adc::td3_dmu(d[ph + (size_t)a], sh.norm ? scale_a[a] : 0.0f, sh.norm);
        adc::td3_backward_host(sh.pol, sh.activation, theta_p, y, d);
    }
    td3_net_grad_host(sh.pol, count, x_bd, D, ys.data(), po, 0, deltas.data(), po, 0, grad_p);
    if (sums2) {
        sums2[0] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)qpi[(size_t)s]; });
        sums2[1] = adc::pg_csum((int64_t)adc::td3_params(sh.pol), [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_p[p], grad_p[p]); });
    }
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_td3_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *theta_p,
                                       const float *psi_q, const float *shift_a, const float *scale_a, int32_t count, const float *x_bd, float *grad_p,
                                       double *sums2)
{
    return td3_actor_grad_host(mlp, num_keywords, cfg, theta_p, psi_q, shift_a, scale_a, count, x_bd, grad_p, sums2, false);
}

ADC_EXPORT int adc_td3_bounded_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *theta_p,
                                               const float *psi_q, int32_t count, const float *x_bd, float *grad_p, double *sums2)
{
    return td3_actor_grad_host(mlp, num_keywords, cfg, theta_p, psi_q, nullptr, nullptr, count, x_bd, grad_p, sums2, true);
}

ADC_EXPORT int adc_td3_polyak_host(float tau, int64_t n, const float *param_n, float *target_n)
{
    if (!(tau > 0.0f && tau <= 1.0f) || n < 1 || !param_n || !target_n) return ADC_EINVAL;
    for (int64_t p = 0; p < n; ++p) target_n[p] = adc::td3_polyak(target_n[p], param_n[p], tau);
    return ADC_OK;
}

// ---- soft actor-critic on the host (adc_sac.h: the code parts/kernel_sac.inc runs) ------------------------------------------------
ADC_EXPORT int adc_sac_config_check(const adc_sac_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_sac_config)) msg = "adc_sac_config: NULL or struct_size mismatch";
    else if (!(cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) msg = "gamma: 0 to 1";
    else if (!(cfg->tau > 0.0f && cfg->tau <= 1.0f)) msg = "tau: above 0, at most 1";
    else if (cfg->target_update_interval < 1) msg = "target_update_interval >= 1";
    else if (!(cfg->init_alpha > 0.0f && cfg->init_alpha < inf)) msg = "init_alpha: above 0, finite";
    else if (!(cfg->target_entropy > -inf && cfg->target_entropy < inf)) msg = "target_entropy must be finite";
    else if (!(cfg->alpha_lr >= 0.0f && cfg->alpha_lr < inf)) msg = "alpha_lr >= 0 (0: alpha stays)";
    else if (!(cfg->eps_sq > 0.0f && cfg->eps_sq < inf)) msg = "eps_sq: above 0, finite";
    else if (!(cfg->reward_scale != 0.0f && cfg->reward_scale > -inf && cfg->reward_scale < inf)) msg = "reward_scale must be finite and not 0";
    else if (cfg->batch_size < 1 || cfg->batch_size > (1 << 20)) msg = "batch_size: 1 to 2^20";
    else if (cfg->capacity < 1 || cfg->capacity > (1 << 30)) msg = "capacity: 1 to 2^30";
    else if (cfg->n_critic_layers < 1 || cfg->n_critic_layers > adc::kMlpMaxLayers) msg = "n_critic_layers: 1 to 4";
    else if (cfg->critic_widths[cfg->n_critic_layers - 1] != 1) msg = "the last critic layer has one output";
    else if (!(cfg->actor_lr >= 0.0f && cfg->actor_lr < inf)) msg = "actor_lr >= 0";
    else if (!(cfg->critic_lr >= 0.0f && cfg->critic_lr < inf)) msg = "critic_lr >= 0";
    else if (cfg->optimiser != ADC_TD3_ADAM && cfg->optimiser != ADC_TD3_SGD) msg = "unknown optimiser";
    else if (cfg->optimiser == ADC_TD3_ADAM && (!(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f) || !(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f)))
        msg = "Adam: 0 <= beta1, beta2 < 1";
    else if (cfg->optimiser == ADC_TD3_ADAM && !(cfg->eps > 0.0f)) msg = "Adam: eps > 0";
    else if (!(cfg->max_grad_norm >= 0.0f && cfg->max_grad_norm < inf)) msg = "max_grad_norm >= 0 (0: off)";
    else
        for (int l = 0; l + 1 < cfg->n_critic_layers; ++l)
            if (cfg->critic_widths[l] < 1 || cfg->critic_widths[l] > adc::kMlpMaxWidth) msg = "hidden critic widths: 1 to 256";
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_sac_pop_config_check(const adc_sac_config *cfgs, int32_t count, int32_t num_envs, int32_t members, const char **message)
{
    const char *msg = nullptr;
    if (!cfgs) msg = "adc_sac_config array is NULL";
    else if (num_envs < 1 || members < 1 || members > 65535 || num_envs % members != 0) msg = "members must be positive, at most 65535, and divide num_envs";
    else if (count != 1 && count != members) msg = "count: 1 (one configuration shared by all members) or the number of members";
    else
        for (int i = 0; i < count && !msg; ++i) {
            const adc_sac_config &c = cfgs[i], &c0 = cfgs[0];
            if (adc_sac_config_check(&c, &msg) != ADC_OK) break;
            if (c.batch_size != c0.batch_size) msg = "batch_size must be equal in all members' configurations (their updates run in the same launches)";
            else if (c.capacity != c0.capacity) msg = "capacity must be equal in all members' configurations (their rings move together)";
            else if (c.target_update_interval != c0.target_update_interval)
                msg = "target_update_interval must be equal in all members' configurations (their target steps run in the same launches)";
            else if (c.n_critic_layers != c0.n_critic_layers) msg = "n_critic_layers / critic_widths must be equal in all members' configurations (the critics' shape is shared)";
            else
                for (int l = 0; l < c.n_critic_layers; ++l)
                    if (c.critic_widths[l] != c0.critic_widths[l]) msg = "n_critic_layers / critic_widths must be equal in all members' configurations (the critics' shape is shared)";
        }
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

namespace {
// the shape two configurations give, or false: a bad configuration, a free-head policy or one without the clamp
bool sac_host_shape(const adc_mlp_config *mlp, int32_t K, const adc_sac_config *cfg, adc::Td3Shape *sh)
{
    if (adc_mlp_config_check(mlp, K, nullptr) != ADC_OK || adc_sac_config_check(cfg, nullptr) != ADC_OK) return false;
    if (mlp->policy_widths[mlp->n_policy_layers - 1] != 2 * (K + 1) || !mlp->clamp_log_std) return false;
    *sh = adc::sac_shape_of(*mlp, K, *cfg);
    return true;
}
adc::EsStep sac_host_step(const adc_sac_config &c, float lr, int64_t steps_taken)
{
    adc::EsStep step{};
    step.optimiser = c.optimiser == ADC_TD3_SGD ? adc::kEsSgd : adc::kEsAdam;
    step.lr = lr; step.beta1 = c.beta1; step.beta2 = c.beta2; step.eps = c.eps; step.l2 = 0.0f;
    step.c1 = adc::es_bias_correction(step.beta1, (uint32_t)(steps_taken + 1));
    step.c2 = adc::es_bias_correction(step.beta2, (uint32_t)(steps_taken + 1));
    return step;
}
}  // namespace

ADC_EXPORT int adc_sac_param_counts_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, int64_t *actor_p, int64_t *critic_qc)
{
    adc::Td3Shape sh;
    if (!sac_host_shape(mlp, num_keywords, cfg, &sh)) return ADC_EINVAL;
    if (actor_p) *actor_p = adc::td3_params(sh.pol);
    if (critic_qc) *critic_qc = adc::td3_params(sh.q);
    return ADC_OK;
}

ADC_EXPORT int adc_sac_logp_host(const adc_mlp_config *mlp, int32_t num_keywords, float eps_sq, int32_t count, const float *mean_ba, const float *raw_ba,
                                 const float *z_ba, float *u_ba, float *t_ba, float *lp_b)
{
    if (adc_mlp_config_check(mlp, num_keywords, nullptr) != ADC_OK || !mlp->clamp_log_std || !(eps_sq > 0.0f) || count < 1 || !mean_ba || !raw_ba || !z_ba ||
        !lp_b)
        return ADC_EINVAL;
    const int A = num_keywords + 1;
    const adc::SacLaw law{0.0f, 0.0f, 0.0f, eps_sq, mlp->log_std_lo, mlp->log_std_hi};
    std::vector<adc::SacHead> heads((size_t)A);
    std::vector<float> o((size_t)2 * A);
    for (int32_t b = 0; b < count; ++b) {
        std::copy(mean_ba + (size_t)b * A, mean_ba + (size_t)(b + 1) * A, o.begin());
        std::copy(raw_ba + (size_t)b * A, raw_ba + (size_t)(b + 1) * A, o.begin() + A);
        lp_b[b] = adc::sac_heads_host(o.data(), A, 0, 0, 0, 0, law, heads.data(), z_ba + (size_t)b * A);
        for (int a = 0; a < A; ++a) {
            if (u_ba) u_ba[(size_t)b * A + a] = heads[(size_t)a].u;
            if (t_ba) t_ba[(size_t)b * A + a] = heads[(size_t)a].t;
        }
    }
    return ADC_OK;
}

ADC_EXPORT int adc_sac_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, uint64_t seed, int64_t update, float alpha,
                                   const float *theta_p, const float *psi_target_q, int32_t count, const float *x2_bd, const float *r_b,
                                   const uint8_t *done_b, float *y_b, float *lp_b)
{
    adc::Td3Shape sh;
    if (!sac_host_shape(mlp, num_keywords, cfg, &sh)) return ADC_EINVAL;
    if (update < 0 || update >= 0xFFFFFFFFll || count < 1 || !theta_p || !psi_target_q || !x2_bd || !r_b || !done_b || !y_b) return ADC_EINVAL;
    const adc::SacLaw law = adc::sac_law_of(*mlp, *cfg);
    const uint64_t key = adc::td3_key(seed);
    const size_t D = (size_t)sh.D, A = (size_t)sh.A, Qc = (size_t)adc::td3_params(sh.q);
    std::vector<float> row(D + A), yp((size_t)adc::td3_outs(sh.pol)), yq((size_t)adc::td3_outs(sh.q));
    std::vector<adc::SacHead> heads(A);
    for (int32_t b = 0; b < count; ++b) {
        std::copy(x2_bd + (size_t)b * D, x2_bd + (size_t)(b + 1) * D, row.begin());
        adc::td3_forward_host(sh.pol, sh.activation, theta_p, row.data(), yp.data());
        const float lp = adc::sac_heads_host(yp.data() + adc::td3_hidden(sh.pol), sh.A, key, adc::ST_SAC_NEXT, (uint32_t)b, (uint32_t)update, law, heads.data(), nullptr);
        for (size_t a = 0; a < A; ++a) row[D + a] = heads[a].t;
        float q[2];
        for (int i = 0; i < 2; ++i) {
            adc::td3_forward_host(sh.q, sh.activation, psi_target_q + (size_t)i * Qc, row.data(), yq.data());
            q[i] = yq[(size_t)adc::td3_hidden(sh.q)];
        }
        y_b[b] = adc::sac_y(r_b[b], done_b[b], adc::td3_min(q[0], q[1]), alpha, lp, law);
        if (lp_b) lp_b[b] = lp;
    }
    return ADC_OK;
}

ADC_EXPORT int adc_sac_critic_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, const float *psi_q, int32_t count,
                                        const float *x_bd, const float *u_ba, const float *y_b, float *grad_q, double *sums6)
{
    adc::Td3Shape sh;
    if (!sac_host_shape(mlp, num_keywords, cfg, &sh)) return ADC_EINVAL;
    if (count < 1 || !psi_q || !x_bd || !u_ba || !y_b || !grad_q) return ADC_EINVAL;
    const size_t S = (size_t)count, D = (size_t)sh.D, A = (size_t)sh.A, DA = D + A, Qc = (size_t)adc::td3_params(sh.q), no = (size_t)adc::td3_outs(sh.q),
                 nh = (size_t)adc::td3_hidden(sh.q);
    std::vector<float> xin(S * DA), ys(S * 2 * no), deltas(S * 2 * no), pieces(S * adc::kTd3Pieces, 0.0f);
    for (size_t s = 0; s < S; ++s) {
        float *row = xin.data() + s * DA;
        std::copy(x_bd + s * D, x_bd + (s + 1) * D, row);
        for (size_t a = 0; a < A; ++a) row[D + a] = adc::mlp_tanh(u_ba[s * A + a]);
        for (size_t i = 0; i < 2; ++i) {
            float *y = ys.data() + s * 2 * no + i * no, *d = deltas.data() + s * 2 * no + i * no;
            adc::td3_forward_host(sh.q, sh.activation, psi_q + i * Qc, row, y);
            float loss;
            d[nh] = adc::td3_critic_delta(y[nh], y_b[s], loss);
            pieces[s * adc::kTd3Pieces + adc::kTd3Loss1 + i] = loss;
            pieces[s * adc::kTd3Pieces + adc::kTd3Q1 + i] = y[nh];
            adc::td3_backward_host(sh.q, sh.activation, psi_q + i * Qc, y, d);
        }
        pieces[s * adc::kTd3Pieces + adc::kTd3Y] = y_b[s];
    }
    for (size_t i = 0; i < 2; ++i)
        td3_net_grad_host(sh.q, count, xin.data(), DA, ys.data(), 2 * no, i * no, deltas.data(), 2 * no, i * no, grad_q + i * Qc);
    if (sums6) {
        for (int c = 0; c < 5; ++c) sums6[c] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)pieces[(size_t)s * adc::kTd3Pieces + (size_t)c]; });
        sums6[5] = adc::pg_csum((int64_t)(2 * Qc), [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_q[p], grad_q[p]); });
    }
    return ADC_OK;
}

ADC_EXPORT int adc_sac_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, uint64_t seed, int64_t update, float alpha,
                                       const float *theta_p, const float *psi_q, int32_t count, const float *x_bd, float *grad_p, float *lp_b, double *sums4)
{
    adc::Td3Shape sh;
    if (!sac_host_shape(mlp, num_keywords, cfg, &sh)) return ADC_EINVAL;
    if (update < 0 || update >= 0xFFFFFFFFll || count < 1 || !theta_p || !psi_q || !x_bd || !grad_p) return ADC_EINVAL;
    const adc::SacLaw law = adc::sac_law_of(*mlp, *cfg);
    const uint64_t key = adc::td3_key(seed);
    const size_t S = (size_t)count, D = (size_t)sh.D, A = (size_t)sh.A, po = (size_t)adc::td3_outs(sh.pol), ph = (size_t)adc::td3_hidden(sh.pol),
                 no = (size_t)adc::td3_outs(sh.q), nh = (size_t)adc::td3_hidden(sh.q), Qc = (size_t)adc::td3_params(sh.q);
    std::vector<float> ys(S * po), deltas(S * po), row(D + A), yq(2 * no), dq(no), gq(A), loss(S), lps(S);
    std::vector<adc::SacHead> heads(A);
    int64_t picked2 = 0;
    for (size_t s = 0; s < S; ++s) {
        float *y = ys.data() + s * po, *d = deltas.data() + s * po;
        std::copy(x_bd + s * D, x_bd + (s + 1) * D, row.begin());
        adc::td3_forward_host(sh.pol, sh.activation, theta_p, row.data(), y);
        const float lp = adc::sac_heads_host(y + ph, sh.A, key, adc::ST_SAC_PI, (uint32_t)s, (uint32_t)update, law, heads.data(), nullptr);
        for (size_t a = 0; a < A; ++a) row[D + a] = heads[a].t;
        for (size_t i = 0; i < 2; ++i) adc::td3_forward_host(sh.q, sh.activation, psi_q + i * Qc, row.data(), yq.data() + i * no);
        const size_t pick = (size_t)adc::sac_pick(yq[nh], yq[no + nh]);
        picked2 += (int64_t)pick;
        const float *psi = psi_q + pick * Qc, *yk = yq.data() + pick * no;
        dq[nh] = 1.0f;
        adc::td3_backward_host(sh.q, sh.activation, psi, yk, dq.data());
        adc::td3_input_delta_host(sh.q, psi, dq.data(), sh.D, sh.A, gq.data());
        for (size_t a = 0; a < A; ++a) {
            const adc::SacHead &h = heads[a];
            const float z = adc::sac_noise(key, adc::ST_SAC_PI, (int)a, (uint32_t)s, (uint32_t)update);
            const float du = adc::sac_du(h.t, h.w, gq[a], alpha, law.eps_sq);
            d[ph + a] = du;
            d[ph + A + a] = adc::sac_dls(du, h.sd, z, alpha, h.moved);
        }
        adc::td3_backward_host(sh.pol, sh.activation, theta_p, y, d);
        loss[s] = adc::sac_pi_loss(alpha, lp, yk[nh]);
        lps[s] = lp;
        if (lp_b) lp_b[s] = lp;
    }
    td3_net_grad_host(sh.pol, count, x_bd, D, ys.data(), po, 0, deltas.data(), po, 0, grad_p);
    if (sums4) {
        sums4[0] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)loss[(size_t)s]; });
        sums4[1] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)lps[(size_t)s]; });
        sums4[2] = adc::pg_csum((int64_t)adc::td3_params(sh.pol), [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_p[p], grad_p[p]); });
        sums4[3] = (double)picked2;
    }
    return ADC_OK;
}

ADC_EXPORT float adc_sac_log_alpha_init_host(float init_alpha) { return adc::sac_log_alpha_init(init_alpha); }

ADC_EXPORT int adc_sac_alpha_step_host(const adc_sac_config *cfg, int64_t steps_taken, double lp_sum, int32_t count, float *la3, float *alpha)
{
    if (adc_sac_config_check(cfg, nullptr) != ADC_OK || steps_taken < 0 || steps_taken >= 0x7FFFFFFFll || count < 1 || !la3) return ADC_EINVAL;
    float a = adc::mlp_exp(la3[0]);
    if (cfg->alpha_lr > 0.0f) {
        const adc::EsStep step = sac_host_step(*cfg, cfg->alpha_lr, steps_taken);
        la3[0] = adc::sac_alpha_step(step, la3[0], adc::sac_alpha_grad(lp_sum, count, cfg->target_entropy), la3[1], la3[2], a);
    }
    if (alpha) *alpha = a;
    return ADC_OK;
}

// ---- the scheduler of population-based training on the host (adc_pbt.h: the code adc_engine_pbt_step runs) ------------------------
ADC_EXPORT int adc_pbt_config_check(const adc_pbt_config *cfg, int32_t members, int32_t kind, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_pbt_config)) msg = "adc_pbt_config: NULL or struct_size mismatch";
    else if (kind != ADC_PBT_PG && kind != ADC_PBT_TD3 && kind != ADC_PBT_SAC) msg = "kind: ADC_PBT_PG, ADC_PBT_TD3 or ADC_PBT_SAC";
    else if (members < 2) msg = "population-based training needs at least 2 members";
    else if (cfg->replace_count < 1 || cfg->replace_count > members / 2) msg = "replace_count: 1 to members / 2";
    else if (!(cfg->fitness_ema >= 0.0f && cfg->fitness_ema < 1.0f)) msg = "fitness_ema: 0 (no smoothing) to below 1";
    else if (!(cfg->factor_lo > 0.0f && cfg->factor_lo < inf) || !(cfg->factor_hi > 0.0f && cfg->factor_hi < inf)) msg = "factor_lo, factor_hi: positive and finite";
    else if (!(cfg->log_factor_lo > -inf && cfg->log_factor_lo < inf) || !(cfg->log_factor_hi > -inf && cfg->log_factor_hi < inf))
        msg = "log_factor_lo, log_factor_hi: finite";
    else if (cfg->tuned_mask >> (kind == ADC_PBT_PG ? adc::kPbtPgIds : kind == ADC_PBT_SAC ? adc::kPbtSacIds : adc::kPbtTd3Ids)) msg = "tuned_mask names a hyperparameter id the trainer does not have";
    else if (cfg->with_ring != 0 && cfg->with_ring != 1) msg = "with_ring: 0 or 1";
    else if (kind == ADC_PBT_PG && cfg->with_ring) msg = "with_ring: a policy-gradient population has no ring";
    else
        for (int h = 0; h < adc::kPbtMaxHp && !msg; ++h) {
            if (!((cfg->tuned_mask >> h) & 1u)) continue;
            const float lo = cfg->lo[h], hi = cfg->hi[h];
            if (!(lo > -inf && hi < inf && lo <= hi)) msg = "lo, hi of a tuned hyperparameter: finite, lo <= hi";
            else if (kind == ADC_PBT_PG && h == 2) { if (!(hi < 1.0f)) msg = "eps_clip: hi below 1"; }
            else if ((kind == ADC_PBT_TD3 || kind == ADC_PBT_SAC) && h == 3) { if (!(lo > 0.0f && hi <= 1.0f)) msg = "tau: lo above 0, hi at most 1"; }
            else if (kind == ADC_PBT_TD3 && h == adc::kPbtSigma) { }
            else if (kind == ADC_PBT_SAC && (h == adc::kPbtAlpha || h == 5)) { }        // (log_alpha and target_entropy: any sign)
            else if (!(lo >= 0.0f)) msg = "lo of a learning rate, a coefficient or a noise: at least 0";
        }
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

ADC_EXPORT int adc_pbt_fitness_host(int32_t days, int32_t num_envs, int32_t members, const float *reward_tn, double *fitness_m)
{
    if (days < 1 || num_envs < 1 || members < 1 || num_envs % members != 0 || !reward_tn || !fitness_m) return ADC_EINVAL;
    const size_t N = (size_t)num_envs;
    const int n = num_envs / members;
    for (int m = 0; m < members; ++m) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const size_t env = (size_t)m * (size_t)n + (size_t)i;
            double ret = 0.0;
            for (int t = 0; t < days; ++t) ret = adc::pbt_chain(ret, (double)reward_tn[(size_t)t * N + env]);
            acc = adc::pbt_chain(acc, ret);
        }
        fitness_m[m] = adc::pbt_fitness_finish(acc, n);
    }
    return ADC_OK;
}

ADC_EXPORT int adc_pbt_plan_host(const adc_pbt_config *cfg, uint64_t seed, int32_t members, int64_t round, const double *fitness_m, double *smoothed_m,
                                 int32_t *rank_m, int32_t *src_m, uint32_t *bits_m)
{
    if (!cfg || cfg->struct_size != sizeof(adc_pbt_config) || members < 2 || cfg->replace_count < 1 || cfg->replace_count > members / 2 ||
        !(cfg->fitness_ema >= 0.0f && cfg->fitness_ema < 1.0f) || round < 0 || round >= 0xFFFFFFFFll || !fitness_m || !smoothed_m || !rank_m || !src_m)
        return ADC_EINVAL;
    for (int m = 0; m < members; ++m) smoothed_m[m] = adc::pbt_smooth(cfg->fitness_ema, smoothed_m[m], fitness_m[m], round == 0);
    adc::pbt_plan(adc::pbt_key(seed), (uint32_t)round, cfg->replace_count, smoothed_m, members, rank_m, src_m, bits_m);
    return ADC_OK;
}

ADC_EXPORT int adc_pbt_explore_host(const adc_pbt_config *cfg, int32_t kind, uint32_t bits, const float *donor_hp8, const float *own_hp8, float *out_hp8)
{
    if (!cfg || cfg->struct_size != sizeof(adc_pbt_config) || (kind != ADC_PBT_PG && kind != ADC_PBT_TD3 && kind != ADC_PBT_SAC) || !donor_hp8 || !own_hp8 || !out_hp8)
        return ADC_EINVAL;
    for (int h = 0; h < adc::kPbtMaxHp; ++h) {
        const int up = (int)((bits >> h) & 1u);
        if (!((cfg->tuned_mask >> h) & 1u)) out_hp8[h] = own_hp8[h];
        else if (kind == ADC_PBT_SAC && h == adc::kPbtAlpha) out_hp8[h] = own_hp8[h];      // (the temperature cell is the device's: k_pbt_exploit_cell)
        else if (kind == ADC_PBT_TD3 && h == adc::kPbtSigma)
            out_hp8[h] = adc::pbt_explore_log(donor_hp8[h], up ? cfg->log_factor_hi : cfg->log_factor_lo, cfg->lo[h], cfg->hi[h]);
        else out_hp8[h] = adc::pbt_explore(donor_hp8[h], up, cfg->factor_lo, cfg->factor_hi, cfg->lo[h], cfg->hi[h]);
    }
    return ADC_OK;
}
