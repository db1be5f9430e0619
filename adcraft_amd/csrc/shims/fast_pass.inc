// fast_pass.inc (part of adc_shims.cpp) - what the dense fast pass (parts/kernel_fast.inc) hoists, proves or packs, on the host next to the routines it
// replaces (adc_law.h, adc_fast_schedule.h): folded draws, proven prices, money packs, plain tiles, the queue tag, the schedule, the queue's protocol.
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
                const uint32_t w = j < 5 ? fixed[j] : (uint32_t)(shim_splitmix64(s) >> 16);
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

// ---- the host twin of k_step_implicit_fast's per-wave queue of clicked wins (parts/kernel_fast.inc: push, drain), for
// tests/test_fast_queue_order_host.py ---------------------------------------------------------------------------------------------
// One wave's queue over a sequence of pushes, push p writing the lanes of masks[p] behind the entries that wait (entry = p << 6 |
// lane; a slot no push has written holds 0xFFFFFFFF).  After every push, while 64 or more wait, a drain runs as the kernel's does, one
// LDS instruction of the wave after the other, each over all 64 lanes: read the batch [0, 64) into registers, read the slots behind
// it [64, 128), write those to [0, 64), take 64 off the fill, and only then resolve the batch from the registers.  What is left at the
// end is one partial batch, resolved by the lanes below the fill.  write_first = 1 places the write before the batch read (the order
// that is wrong: the test's counter-example).  entries (the first `cap`) = what the batches resolved, batch after batch, in lane
// order; batches2 (the first `batch_cap` rows) = {entries that waited when the batch started, entries it resolved}; info3 (nullable)
// = {batches, entries pushed, the largest fill}.  Returns the number of entries resolved, or a negative adc_status.
ADC_EXPORT int64_t adc_fast_queue_host(const uint64_t *masks, int64_t n_masks, int32_t write_first, uint32_t *entries, int64_t cap, int32_t *batches2,
                                       int64_t batch_cap, int64_t *info3)
{
    constexpr int WL = adc::kFastWaveLanes, kCap = 2 * adc::kFastWaveLanes;      // (kQueueCap of the kernel: <= 63 + 64 ever wait)
    if (n_masks < 0 || n_masks >= (1ll << 26) || (n_masks > 0 && !masks) || write_first < 0 || write_first > 1 || cap < 0 || batch_cap < 0 ||
        (cap > 0 && !entries) || (batch_cap > 0 && !batches2))
        return ADC_EINVAL;
    uint32_t q[kCap];
    for (int i = 0; i < kCap; ++i) q[i] = 0xFFFFFFFFu;
    int fill = 0, max_fill = 0;
    int64_t resolved = 0, n_batches = 0, pushed = 0;
    auto resolve = [&](const uint32_t *batch, int lanes, int waited) {        // (what resolve_click is handed: the entry, per lane)
        for (int lane = 0; lane < lanes; ++lane, ++resolved)
            if (resolved < cap) entries[resolved] = batch[lane];
        if (n_batches < batch_cap) { batches2[2 * n_batches] = waited; batches2[2 * n_batches + 1] = lanes; }
        n_batches += 1;
    };
    for (int64_t p = 0; p < n_masks; ++p) {
        const uint64_t m = masks[p];
        int rank = 0;
        for (int lane = 0; lane < WL; ++lane)
            if ((m >> lane) & 1ull) {
                if (fill + rank >= kCap) return ADC_EINVAL;          // (cannot happen: fill <= 63 before a push)
                q[fill + rank] = (uint32_t)(p << 6) | (uint32_t)lane;
                rank += 1;
            }
        fill += rank;
        pushed += rank;
        max_fill = fill > max_fill ? fill : max_fill;
        if (fill >= WL) {                                   // (checked after every push, as the kernel does: one drain brings it below 64)
            uint32_t batch[WL], behind[WL];
            const int waited = fill;
            if (!write_first) for (int lane = 0; lane < WL; ++lane) batch[lane] = q[lane];
            for (int lane = 0; lane < WL; ++lane) behind[lane] = q[WL + lane];
            for (int lane = 0; lane < WL; ++lane) q[lane] = behind[lane];
            if (write_first) for (int lane = 0; lane < WL; ++lane) batch[lane] = q[lane];
            fill -= WL;
            resolve(batch, WL, waited);
        }
    }
    if (fill > 0) resolve(q, fill, fill);
    if (info3) { info3[0] = n_batches; info3[1] = pushed; info3[2] = max_fill; }
    return resolved;
}
