// kernel_fast.inc - k_step_implicit_fast: the budget-free pass (dominant kernel), step_tail
// (part of the single translation unit adc_engine.hip; see that file for the overview)
// -------------------------------------------------------------------------------------------------
// FAST PASS (IMPLICIT, engine stream, budget ignored)
// -------------------------------------------------------------------------------------------------
// What bounds it: VALU issue (profiles/r02_issue_rates.md - compares, converts, min/max, integer multiplies, mbcnt cost
// 4 cycles per wave-instruction, add/logic/fma 2).  The design spends them where an outcome needs them:
//   * an auction is RESOLVED by comparing its word with the keyword's two word intervals (clicked win / unclicked win:
//     adc_law.h win_intervals, exact) - the competitor's bid is a monotone function of the word, so "bid > competitor"
//     is an interval test and no logarithm runs for the ~3/4 of auctions that are lost or not clicked;
//   * the competitor's bid (the 2nd price) is evaluated only for clicked wins, in stage B, on full wavefronts, together
//     with the conversion / revenue call;
//   * tiles with few auctions per keyword (sparse keyword sets) skip the intervals - finding them costs more than the
//     ~20 auctions they would serve - and resolve each auction from its sampled competitor bid (DIRECT).
// Both forms are the same law (the oracle only knows the auction-by-auction form); results are identical bit for bit.
constexpr int kQueueCap = 128;    // per-wave queue of deferred clicked wins (entries): drained whenever 64 wait, so <= 63 + 64 ever do
constexpr int kDenseVolumePerKeyword = adc::kDenseVolumePerKeyword;      // (adc_fast_schedule.h: the schedule of phase 2 and this test, shared with the host twin)
static_assert(kFastBlock == adc::kFastTileLanes && kWave == adc::kFastWaveLanes, "adc_fast_schedule.h describes this workgroup");

// per keyword, two 16-byte records in separate arrays (a wave's consecutive keywords then cover every LDS bank once per
// ds_read_b128; one 32-byte record per keyword is a built-in 2-way bank conflict).  16-byte aligned: a record that is only
// 4-byte aligned (as `win` was after off[257]) is read as two ds_read2_b32, each with its own address add.
struct alignas(16) KwLawA {
    unsigned int m_click, t_conv; // rescale multiplier of the click sub-interval; saturated conversion threshold
    float loc, scale;             // competitor-bid law
};
struct alignas(16) KwLawB {
    float mu, sd;                 // revenue law
    union {
        struct {
            unsigned int t_click; // saturated click threshold           (DIRECT stage A)
            int bid_c;            // the bid in cents                    (DIRECT stage A)
        } d;
        adc::KwHalf conv;         // interval form: the keyword's half of round 1 of its ST_CONV draws (stage B, adc::draw_kw_folded)
    };
};
union alignas(16) KwWin {                     // per keyword, 16 B
    adc::WinIntervals iv;                                   // interval form
    struct { unsigned int m_noclick, pad0, pad1, pad2; } d; // DIRECT form
};

// counts of a keyword-day packed in one 64-bit LDS accumulator: unclicked wins | clicks << 21 | conversions << 42
// (each is at most the day's volume <= 2^20 = adc::kVolumeMax)
constexpr int kClkShift = 21, kConvShift = 42;
// sh.vol[u] holds the keyword's volume in its low 21 bits and, above them, the exclusive prefix of the keywords' tail calls (at
// most 3 per keyword: 768 in a tile) - a second prefix array would take the listing variant over five workgroups' worth of LDS
constexpr int kVolBits = 21;
constexpr int kVolMask = (1 << kVolBits) - 1;
constexpr int kTailCallsMax = adc::kFastTailCallsMax * kFastBlock;
static_assert(adc::kVolumeMax <= kVolMask && kTailCallsMax < (1 << (31 - kVolBits)), "volume and tail-call prefix share a word");
static_assert(adc::kVolumeMax < (1 << kClkShift), "three counts of up to kVolumeMax must fit 21 bits each");
// a queued clicked win's tag (adc_law.h fast_tag): the keyword's accumulator offset in bits 3..10, the auction index above them
static_assert((kFastBlock - 1) * sizeof(unsigned long long) == adc::kFastTagAccMask && sizeof(unsigned long long) == 1u << adc::kFastTagKeywordShift,
              "the tag's keyword field is the byte offset of a_cnt[keyword]");
static_assert(((unsigned long long)adc::kVolumeMax << adc::kFastTagAuctionShift) <= 0xFFFFFFFFull, "every auction index of a day fits above the keyword");

// (Keyword sets with few auctions per keyword - the engine's volume hint - go to k_step_implicit_sparse, kernel_sparse.inc; this
// kernel still decides per tile: a tile that happens to be sparse is resolved auction by auction from the sampled competitor bid.)
struct FastShared {
    // (the queue first: its two arrays then sit 2048 bytes apart at a 256-byte aligned offset, and a push's pair of writes is
    // one ds_write2st64_b32 on the slot's address, with no constant to add)
    union {
        struct {                                            // phase 2: per wave, entry e = {tag[e], word[e]}
            unsigned int tag[kFastBlock / kWave][kQueueCap];    //   adc::fast_tag: auction index << 11 | keyword-in-tile << 3
            unsigned int word[kFastBlock / kWave][kQueueCap];   //   the auction word (DIRECT: the price)
        } queue;
        struct {                                            // phase 1 (before the queues are used)
            unsigned int volw[kFastBlock];                  // volume words of the tile's keywords
            int wave_tot[kFastBlock / kWave], wave_vol[kFastBlock / kWave], wave_live[kFastBlock / kWave];
            int wave_wide[kFastBlock / kWave];             // 1: a keyword of the wave needs the cost and the revenue in accumulators of their own; 2: one converts at every click
        };
    };
    KwWin win[kFastBlock];
    KwLawA law_a[kFastBlock];
    KwLawB law_b[kFastBlock];
    unsigned long long a_cnt[kFastBlock], a_cost[kFastBlock], a_rev[kFastBlock];      // (stage B reaches all three from &a_cnt[u])
    adc::LogTableEntry logtab[adc::kLogTableIntervals];     // copy of g_log_table
    float normtab[adc::kNormTableEntries + 1];              // node values of g_norm_table (+ the p = 1/2 node)
    int off[kFastBlock + 1];        // exclusive prefix of the keywords' full work items (+ the total)
    int vol[kFastBlock];            // volume | the same prefix of the keywords' tail calls << kVolBits
    unsigned char tail_kw[kTailCallsMax];       // the keyword of every tail call, in the prefix's order (what pass 1 finds its keyword by)
};
// what the listing variant keeps on top of that (envs that list their clicked wins for k_step_click_walk, see resolve_click)
template <bool LISTS>
struct FastListing {
    unsigned int row_count[adc::kTimesteps];                // clicked wins listed per sub-timestep
    int jcut[kFastBlock];                                   // the keyword's auctions below this index are listed whatever they cost,
    unsigned int price_cut;                                 // the later ones if they cost at most this (the env's hints)
};
template <>
struct FastListing<false> {};
// (LDS is handed out in blocks of 1280 bytes on gfx950 - kernel_sparse.inc: five workgroups per CU need 25 blocks = 32 000 bytes each)
static_assert(sizeof(FastShared) + sizeof(FastListing<true>) <= 25 * 1280, "the listing variant must allow 5 workgroups per CU too");
static_assert(kFastBlock == adc::kLogTableIntervals, "one table entry per lane is copied in phase 1");
static_assert(sizeof(FastShared) <= 25 * 1280, "FastShared must allow 5 workgroups per CU");

// normal_tab with the table's node values in LDS (same bits: the slope is (b - a) 2^-18)
__device__ __forceinline__ float normal_tab_nodes(uint32_t w, const float *nodes)
{
    const uint32_t t = ((w >> 7) & 0x00FFFFFEu) | 1u;
    const uint32_t bits = __float_as_uint((float)t);
    const uint32_t i = (bits >> 18) - (127u << 5);
    const float a = nodes[i], b = nodes[i + 1];
    const float z = adc::fma32((b - a) * 3.814697265625e-06f, (float)(bits & 0x0003FFFFu), a);
    return __uint_as_float(__float_as_uint(z) | (~w & 0x80000000u));
}

// tile_kw = keywords per workgroup: 256 (one per lane) when there are enough workgroups to fill the chip, fewer (a power
// of two >= 16) for a handful of envs - a single workgroup walking a whole env is latency-bound, while its auctions
// spread over several workgroups finish in a third of that.  The lanes of a narrow tile all work in phase 2 (items are
// dealt to all 256 lanes); results do not depend on the tiling.
// (NARROW = false: tile_kw is the compile-time 256 of the throughput configuration)
// what phase 1 reads from HBM for one keyword (+ the env's stream state): loaded one tile ahead of its use
struct FastRaw {
    float vol_mean, vol_std, bctr, sctr, loc, scale, mu, sd, bid;
    uint64_t key;
    uint32_t tick;
    bool drift, skip, emit;
};

// A workgroup resolves `tiles_per_wg` consecutive (env, keyword-tile) pairs.  One tile per workgroup when tiles are big
// (dense keyword sets: the hardware dispatcher then balances the chip); several when they are small (sparse sets: a tile
// is ~25k cycles, a third of it HBM latency and table copies) - the next tile's parameters are loaded before the current
// tile's auctions are resolved, and the two tables are copied to LDS once.
// (5 workgroups per CU.  cfg2's 4096 tiles over 1280 resident workgroups are 3.2 rounds; 4 per CU would be exactly 4 rounds, and
// was measured 6 % slower all the same - round 3: the kernel needs its 5 waves per SIMD more than the balanced tail)
// LISTS: the variant that can also list an env's clicked wins for k_step_click_walk (envs whose budget bound the day before);
// the host launches it once the device has reported such an env (adc_engine::h_listing) - the listing code costs the plain
// variant 5 % of its time even where nothing is listed (registers), so it is compiled out there.
template <bool NARROW, bool LISTS = false>
__global__ __launch_bounds__(kFastBlock, 5) void k_step_implicit_fast(View v, const float *__restrict__ bids, int tile_kw_arg, int tiles_per_wg)
{
    __shared__ FastShared sh;
    [[maybe_unused]] __shared__ FastListing<LISTS> ls;
    const int tile_kw = NARROW ? tile_kw_arg : kFastBlock;
    const int tiles = (v.K + tile_kw - 1) / tile_kw;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    [[maybe_unused]] unsigned long long fdbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    [[maybe_unused]] unsigned long long fslots[2] = {0, 0};      // (ADC_EXP_TIMING) calls issued by this wave | calls needed by this lane's keywords

    auto load_tile = [&](int tile_index) {
        FastRaw r{};
        const int env = tile_index / tiles;
        const int k = (tile_index - env * tiles) * tile_kw + tid;
        r.key = v.key[env];
        r.tick = v.tick[env];
        r.drift = v.drift_on && v.drift_pending[env];
        const int hint = v.exact_hint[env];   // scheduling hints only (same results): 2 = k_step_exact_rows computes this env alone,
        r.skip = (hint & ~4) == 2;            // (6: the same, parked for k_step_rest_of_day at once); 1 = also list the clicked wins for k_step_click_walk
        r.emit = LISTS && hint == 1 && v.click_rec != nullptr;
        if (tid < tile_kw && k < v.K && !r.skip) {
            r.vol_mean = param_at(v, ADC_P_VOL_MEAN, env, k);
            r.vol_std = param_at(v, ADC_P_VOL_STD, env, k);
            r.bctr = param_at(v, ADC_P_BCTR, env, k);
            r.sctr = param_at(v, ADC_P_SCTR, env, k);
            r.loc = param_at(v, ADC_P_A, env, k);
            r.scale = param_at(v, ADC_P_B, env, k);
            r.mu = param_at(v, ADC_P_REV_MEAN, env, k);
            r.sd = param_at(v, ADC_P_REV_STD, env, k);
            r.bid = bids[(size_t)env * v.K + k];
        }
        return r;
    };

    const int n_tiles = v.N * tiles;
    const int tile_first = blockIdx.x * tiles_per_wg, tile_last = min(tile_first + tiles_per_wg, n_tiles);
    sh.logtab[tid] = g_log_table[tid];
    for (int i = tid; i <= adc::kNormTableEntries; i += kFastBlock) sh.normtab[i] = g_norm_nodes[i];
    FastRaw next = load_tile(tile_first);

  for (int tile_index = tile_first; tile_index < tile_last; ++tile_index) {
    const FastRaw raw = next;
    if (tile_index + 1 < tile_last) next = load_tile(tile_index + 1);
    if (raw.skip) continue;                     // (block-uniform)
    const int env = tile_index / tiles;
    const int tile = tile_index - env * tiles;
    const int k = tile * tile_kw + tid;
    const bool valid = tid < tile_kw && k < v.K;
    // (block-uniform, and said so: the Philox round keys derived from them then stay in SGPRs - each is one operand of a v_bitop3 -
    // whatever the compiler makes of the tile loop's carried loads; as vector values they take 13 VGPRs through phase 2)
    const uint64_t key = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(raw.key >> 32)) << 32) |
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)raw.key);
    const uint32_t tick = (uint32_t)__builtin_amdgcn_readfirstlane((int)raw.tick);
    // tick ^ key_hi, all that round 1 of a Philox call reads of the two: folded here on the scalar unit, once per tile, so that the
    // call's xor has one SGPR operand (with two, hipcc stages one in a VGPR: a v_mov_b32 per call in stage A and per clicked win
    // in stage B).  Opaque, or the xor is re-associated into the three-input form again.
    uint32_t tick_k1 = adc::philox_fold_tick(key, tick);
    asm volatile("" : "+s"(tick_k1));
    const uint32_t kw_base = (uint32_t)(tile * tile_kw);
    if (LISTS && raw.emit && tid == 0) v.click_tick[env] = tick + 1u;      // (every tile of the env writes the same value)
    if constexpr (LISTS) { if (raw.emit && !NARROW && tid < adc::kTimesteps) ls.row_count[tid] = 0u; }      // (before phase 1's barriers)
    [[maybe_unused]] const unsigned long long t_start = FDBG_T();

    // ---- phase 1: one lane per keyword ---------------------------------------------------------
    // the tile's volume words: one Philox call serves four consecutive keywords, so 64 lanes draw for 256
    if (tid < (tile_kw + 3) / 4) {
        const adc::U4 w = adc::draw(key, 0u, adc::ST_VOL, (kw_base >> 2) + (uint32_t)tid, tick);
        *reinterpret_cast<uint4 *>(&sh.volw[4 * tid]) = make_uint4(w.x, w.y, w.z, w.w);
    }
    float vol_mean = raw.vol_mean, bctr = raw.bctr, sctr = raw.sctr;
    const float vol_std = raw.vol_std, loc = raw.loc, scale = raw.scale, mu = raw.mu, sd = raw.sd, bid = raw.bid;
    if (valid && raw.drift && drift_keyword(v, env, key, tick - 1u, k, vol_mean, vol_std, bctr, sctr)) {
        param_at(v, ADC_P_VOL_MEAN, env, k) = vol_mean;
        param_at(v, ADC_P_BCTR, env, k) = bctr;
        param_at(v, ADC_P_SCTR, env, k) = sctr;
    }
    sh.a_cnt[tid] = sh.a_cost[tid] = sh.a_rev[tid] = 0ull;
    __syncthreads();
    int V = 0;
    if (valid) {
        float x = adc::fma32(vol_std, normal_tab_nodes(sh.volw[tid], sh.normtab), vol_mean);      // adc::volume_from_word on the LDS nodes
        x = x > 0.0f ? x : 0.0f;
        x = x < (float)adc::kVolumeMax ? x : (float)adc::kVolumeMax;
        const float t = __builtin_truncf(x);
        V = (int)t + ((x - t) >= 0.5f ? 1 : 0);
    }
    if constexpr (LISTS) {
        if (raw.emit) {                         // (block-uniform) auctions of the sub-timesteps up to the env's row hint (adc::cell_range)
            const int rows = (int)v.click_row_hint[env], s = V / adc::kTimesteps;
            ls.jcut[tid] = rows >= adc::kTimesteps - 1 ? 0x7FFFFFFF : V - (adc::kTimesteps - 1) * s + rows * s;
            if (tid == 0) ls.price_cut = v.click_price_hint[env];
        }
    }
    // tile volume and number of keywords with auctions -> the form this tile is resolved in, and its work-item size; and whether
    // every keyword-day of the tile keeps its cost and its revenue below 2^32 cents each (adc::fast_money_packs: a bound from the
    // volume, the bid and the revenue law) - a clicked win then adds both with one atomic, the revenue in the high word of a_cost
    const int bid_c = (int)adc::bid_to_cents(bid);
    {
        const int vsum = wave_sum_i32(V);
        const int live = (int)__popcll(__builtin_amdgcn_ballot_w64(V > 0));
        const bool wide = V > 0 && !adc::fast_money_packs(V, bid_c, mu, sd, sh.normtab[0]);      // (normtab[0]: the largest node)
        // and whether every conversion test of the tile is `word < threshold` alone (adc::fast_conversion_plain: no threshold of 2^32)
        const bool always = V > 0 && !adc::fast_conversion_plain(sctr);
        const int any_wide =(__builtin_amdgcn_ballot_w64(wide) != 0ull ? 1 : 0) | (__builtin_amdgcn_ballot_w64(always) != 0ull ? 2 : 0);
        if (lane == 0) { sh.wave_vol[wv] = vsum; sh.wave_live[wv] = live; sh.wave_wide[wv] = any_wide; }
    }
    __syncthreads();
    int tile_volume = 0, tile_live = 0, tile_wide = 0;
#pragma unroll
    for (int i = 0; i < kFastBlock / kWave; ++i) { tile_volume += sh.wave_vol[i]; tile_live += sh.wave_live[i]; tile_wide |= sh.wave_wide[i]; }
    // (tile-uniform, in an SGPR: all ones where the tile packs.  One opaque word: as a known all-ones-or-zero value hipcc keeps it as
    // a lane mask in an SGPR pair and tests it through vcc)
    const int tile_flags = __builtin_amdgcn_readfirstlane(tile_wide);
    unsigned int pack_mask = (tile_flags & 1) == 0 ? 0xFFFFFFFFu : 0u;
    asm volatile("" : "+s"(pack_mask));
    // a PLAIN tile packs and holds no keyword that converts at every click (adc::fast_keyword_plain for every live keyword): stage B
    // then needs neither bernoulli32's second compare nor - like every tile that packs - the upper clamp of money_to_cents
    const bool plain = tile_flags == 0;
    const bool dense = adc::fast_tile_dense(tile_volume, tile_live);               // (block-uniform)
    // work-item size: 16 auctions when the tile has plenty of them; 8 or 4 on sparse tiles, so that the items still
    // number about two per lane.  Results do not depend on it: every draw is addressed by (auction, keyword).
    const int chunk_shift = adc::fast_chunk_shift(tile_volume);
    // the keyword's law (only keywords with auctions need one), before the items are counted: a keyword that cannot win an auction
    // (adc::fast_keyword_is_dead - a bid at or below the competitor's lowest price, as the agent's "no bid" 0 is) has a day of zeros
    // whatever its words are, and is dealt no item, tail call or partial call.  (tile_volume, tile_live, dense and chunk_shift stay
    // what the drawn volumes make them: they only choose the form and the item size.  A DIRECT tile has no intervals to ask, and
    // a bid - at least 1 cent, adc::bid_to_cents - that tells nothing alone.)
    [[maybe_unused]] const unsigned long long t_law = FDBG_T();
    bool dead = false;
    if (V > 0) {
        const uint64_t t_click = adc::bernoulli_threshold(bctr);
        const adc::AuctionLaw law = adc::make_auction_law(bctr);
        sh.law_a[tid] = KwLawA{law.m_click, adc::saturate_threshold(adc::bernoulli_threshold(sctr)), loc, scale};
        KwLawB lb;
        lb.mu = mu;
        lb.sd = sd;
        if (dense) {
            lb.conv = adc::philox_kw_half(adc::ST_CONV, kw_base + (uint32_t)tid, (uint32_t)key);
            const adc::WinIntervals iv = adc::win_intervals(bid_c, loc, scale, t_click, law, sh.logtab);
            sh.win[tid].iv = iv;
            dead = adc::fast_keyword_is_dead(iv);
        } else {
            lb.d.t_click = law.t32;
            lb.d.bid_c = bid_c;
            sh.win[tid].d.m_noclick = law.m_noclick;
        }
        sh.law_b[tid] = lb;
    }
    FDBG_ADD(1, FDBG_T() - t_law);
    const int Vw = dead ? 0 : V;                                // the auctions that are resolved one by one
    const int nch = adc::fast_full_items(Vw, chunk_shift);      // FULL items; the last Vw mod chunk auctions are the keyword's tail
    const int ntc = adc::fast_tail_calls(Vw, chunk_shift);      // the whole calls of that tail, dealt as items of one call
    // (both prefixes in one scan: adc::fast_pack_counts - a wave's full items stay below 2^23, its tail calls below 2^8)
    const int incl = wave_scan_i32(adc::fast_pack_counts(nch, ntc));
    if (lane == 63) sh.wave_tot[wv] = incl;
    FSLOT_ADD(1, (unsigned long long)adc::fast_calls_needed(Vw));
    __syncthreads();
    int wave_base = 0, total = 0, wave_base2 = 0, total2 = 0;
#pragma unroll
    for (int i = 0; i < kFastBlock / kWave; ++i) {
        const int t = sh.wave_tot[i];
        if (i < wv) { wave_base += adc::fast_packed_items(t); wave_base2 += adc::fast_packed_calls(t); }
        total += adc::fast_packed_items(t);
        total2 += adc::fast_packed_calls(t);
    }
    __syncthreads();                    // (wave_tot / volw share memory with the queues: everybody has read them)
    sh.off[tid] = wave_base + adc::fast_packed_items(incl) - nch;
    {
        const int first_call = wave_base2 + adc::fast_packed_calls(incl) - ntc;
        sh.vol[tid] = Vw | (first_call << kVolBits);         // (0 for a dead keyword: only keywords with auctions to resolve are looked up)
#pragma unroll
        for (int c = 0; c < adc::kFastTailCallsMax; ++c)
            if (c < ntc) sh.tail_kw[first_call + c] = (unsigned char)tid;
    }
    if (tid == 0) sh.off[kFastBlock] = total;
    __syncthreads();
    [[maybe_unused]] const unsigned long long t_p2 = FDBG_T();
    FDBG_ADD(0, t_p2 - t_start);

    // ---- phase 2: work items of `chunk` consecutive auctions of one keyword ------------------------
    // Full items are dealt lane-major and per wave (adc_fast_schedule.h): the tile's ceil(total / 64) wave-rounds are split
    // over the four waves, R_w each (they differ by at most one; w = the part the wave takes in this tile, rotated from
    // tile to tile), and lane l of wave w resolves the items
    // [base_w + l R_w, base_w + (l + 1) R_w), so a lane stays on one keyword for several rounds, the 64 lanes of a wave are on
    // ~64 different, consecutive keywords at any time (their LDS records and accumulators then fall on distinct banks, and the
    // same keyword is rarely hit twice by one stage-B batch), and the lane finds its next keyword by comparing with a bound it
    // holds in a register.  No wave runs a round for another wave's items: a workgroup-wide round count issued up to three
    // wave-rounds of empty slots per tile, and an empty slot costs what a full one does (below).
    // The keywords' tails (V mod chunk auctions) follow at the granularity of a Philox call: their whole calls are dealt as
    // items of four auctions by the same scheme over a second prefix (a tail call finds its keyword in tail_kw, and its place
    // in the keyword's tail by the prefix kept in the high bits of vol), and what is left - V mod 4 auctions - runs
    // last, one keyword per lane, as a single call.  (One keyword per lane for the whole tail was four calls in every wave
    // for a mean of 1.9 calls of work per lane.)
    // Control flow is wave-uniform (idle lanes carry an empty law) so that the deferred-click queue below can be maintained
    // with ballots.  Stage A (every auction): one Philox call per FOUR auctions (one word each); the word is classified
    // (lost / won / won and clicked).  Stage B (clicked wins only, ~1/4 of auctions): the (keyword, auction, word) is pushed
    // to a per-wave LDS queue; whenever 64 are waiting, all 64 lanes evaluate the price paid and draw the conversion /
    // revenue call together - full wavefronts instead of the lanes that happen to click.
    // The queue is linear, not a ring: entries sit at [0, qtail); a drain resolves [0, 64) and moves the 0..63 entries
    // behind them down to [0, qtail - 64) (one read and one write per lane, per 64 clicked wins; the move comes first and the
    // batch is resolved from registers, see drain), so that a push is
    // mbcnt_lo, mbcnt_hi and one address (qtail goes into its scalar base), plus the tag: no wrap mask, no head.
    // Tags and words are two arrays of 4-byte entries: consecutive slots, conflict-free, and no register pair to build (two
    // ds_write_b32 at an 8-byte stride are each a 2-way bank conflict - measured +19 % kernel time).
    const int wq = __builtin_amdgcn_readfirstlane(wv);                      // (wave-uniform: keep the bases scalar)
    unsigned int *const qtag = sh.queue.tag[wq];
    unsigned int *const qword = qtag + sizeof(sh.queue.tag) / sizeof(unsigned int);      // sh.queue.word[wq], off the tags' own base: a slot's two reads then stay one ds_read2st64_b32
    // the queue's fill is carried as the LDS byte address of its first free tag slot, qaddr = qbase + 4 qtail: a push forms its
    // address from it with one v_lshl_add_u32 and advances it with one scalar shift-and-add
    typedef __attribute__((address_space(3))) unsigned int LdsWord;
    const unsigned int qbase = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(size_t)(LdsWord *)qtag);
    constexpr unsigned int kBatchBytes = kWave * sizeof(unsigned int);
    static_assert(sizeof(sh.queue.tag) == 8 * 64 * sizeof(unsigned int), "a push writes the word at offset1:8 of ds_write2st64_b32");
    unsigned int qaddr = qbase;

    // the low word of a clicked win's count operand (one click), in a register of its own through phase 2: stage B sets only the
    // high word (the conversion) per batch, where the 64-bit constant was rebuilt with two v_mov_b64
    unsigned int cnt_lo = 1u << kClkShift;
    asm volatile("" : "+v"(cnt_lo));
    // ent = the lane's queue entry {tag, word}, read by the caller (a drain has moved the queue down before it resolves)
    // direct: the entry carries the price (stage A had to sample it); otherwise the auction word
    auto resolve_click = [&](bool direct, const uint2 ent) {
        // the keyword's accumulators by one byte offset, which the tag holds as it is (one full-rate v_and_b32; opaque, or hipcc forms
        // it again from the law records' address)
        unsigned int acc_off = adc::fast_tag_acc_offset(ent.x);
        asm volatile("" : "+v"(acc_off));
        [[maybe_unused]] const unsigned int uu = acc_off >> adc::kFastTagKeywordShift;
        const unsigned int ent_j = adc::fast_tag_auction(ent.x);
        unsigned long long *const acc = (unsigned long long *)((char *)sh.a_cnt + acc_off);      // a_cnt[uu]; a_cost, a_rev follow at kFastBlock strides
        // the keyword's 16-byte law records by that offset added to itself (a full-rate add; uu * 16 from the tag's byte is a second
        // half-rate shift)
        static_assert(sizeof(KwLawA) == 2 * sizeof(unsigned long long) && sizeof(KwLawB) == sizeof(KwLawA), "law records at twice the accumulators' stride");
        unsigned int law_off;
        asm volatile("v_add_u32 %0, %1, %1" : "=v"(law_off) : "v"(acc_off));      // (written as x + x, hipcc emits v_lshlrev_b32 x, 1)
        const KwLawA ka = *(const KwLawA *)((const char *)sh.law_a + law_off);
        const KwLawB kb = *(const KwLawB *)((const char *)sh.law_b + law_off);
        unsigned int price = ent.y;
        if (!direct) {
            unsigned int vv = adc::mulhi32(ent.y, ka.m_click);                        // a click: the offset is the word itself
            vv = vv < 0x00FFFFFFu ? vv : 0x00FFFFFFu;
            // (the entry is a win by the keyword's intervals: the price needs no clamp - adc_law.h)
            price = (unsigned int)adc::competitor_cents_of_proven_win(vv, ka.loc, ka.scale, sh.logtab);
        }
        // (interval form: the draw starts from the keyword's half of round 1, kept in law_b by phase 1 - the same bits)
        const adc::U4 w2 = direct ? adc::draw_folded(key, ent_j, adc::ST_CONV, kw_base + uu, tick_k1)
                                  : adc::draw_kw_folded(key, ent_j, kb.conv, tick_k1);
        // adc::bernoulli32: its second compare (the saturated threshold that stands for 2^32) behind a scalar branch that a plain tile
        // skips (the empty asm keeps it a branch: as a select it is the compare again)
        bool conv = w2.x < ka.t_conv;
        if (!plain) {
            unsigned int t = ka.t_conv;
            asm volatile("" : "+v"(t));
            conv |= t == 0xFFFFFFFFu;
        }
        unsigned int cnt_hi = 0u;
        unsigned int rev_c = 0u;
        if (conv) {
            float x = adc::fma32(kb.sd, normal_tab_nodes(w2.y, sh.normtab), kb.mu);
            x = x > 0.01f ? x : 0.01f;
            // a_rev[uu], and the upper clamp of money_to_cents: only a tile that does not pack (its a_cost then takes no revenue).  In
            // one that packs every revenue is below 1e7 dollars and the clamp is idle (adc::money_to_cents_unclamped); >= 1 cent: no
            // sign to extend
            if (pack_mask == 0u) { atomicAdd(acc + 2 * kFastBlock, (unsigned long long)(unsigned int)adc::money_to_cents(x)); x = 0.0f; }
            rev_c = (unsigned int)adc::money_to_cents_unclamped(x);
            cnt_hi = 1u << (kConvShift - 32);
        }
        // (both high words opaque: each is then written where its operand pair wants it, next to cnt_lo and to the price, with no
        // 64-bit select or OR to build the pair)
        asm volatile("" : "+v"(cnt_hi));
        atomicAdd(acc, ((unsigned long long)cnt_hi << 32) | cnt_lo);
        // a_cost[uu]: the price, and in a tile that packs the revenue above it (neither half can carry: adc::fast_money_packs)
        asm volatile("" : "+v"(rev_c));
        atomicAdd(acc + kFastBlock, (unsigned long long)price | ((unsigned long long)rev_c << 32));
        if constexpr (LISTS) { if (raw.emit) {
            // (block-uniform) the env's budget bound yesterday: list the clicked win for k_step_click_walk, by sub-timestep
            // (adc::cell_range inverted: the quotient estimated in float32 - exact operands below 2^24 - and fixed up)
            // sub-timesteps up to the row hint are listed completely (jcut), later ones only with the clicks that cost at most the
            // price hint
            const int j = (int)ent_j;
            if (j < ls.jcut[uu] || price <= ls.price_cut) {
                // the click's sub-timestep and index in its cell: adc::cell_range inverted, the quotient estimated in float32
                // (exact operands below 2^24) and fixed up
                const int V = sh.vol[uu] & kVolMask;
                const int s = V / adc::kTimesteps, first = V - (adc::kTimesteps - 1) * s;
                int row = 0, jc = j;
                if (j >= first) {
                    const int d = j - first;
                    int q = (int)((float)d * __builtin_amdgcn_rcpf((float)s));
                    q -= q * s > d ? 1 : 0;
                    q += (q + 1) * s <= d ? 1 : 0;
                    row = 1 + q;
                    jc = d - q * s;
                }
                // a dense tile is the whole env (K <= 256): its counters are the tile's; narrow tiles share the env's
                const unsigned int slot = NARROW ? atomicAdd(&v.click_count[(size_t)env * adc::kTimesteps + row], 1u) : atomicAdd(&ls.row_count[row], 1u);
                if (slot < click_seg_cap(v, row))
                    v.click_rec[click_seg_offset(v, env, row) + slot] = make_uint2(((kw_base + uu) << 20) | (unsigned int)jc, price);
            }
        } }
    };
    auto drain = [&](bool direct) {
        if (qaddr >= qbase + kBatchBytes) {                 // checked after every push: <= 63 + 64 entries wait
            [[maybe_unused]] const unsigned long long tb = FDBG_T();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // The move-down comes FIRST, the batch is resolved from registers after it: the batch [0, 64) is read, then the entries
            // behind it, which are written to [0, 64), and only then stage B runs.  A wave's LDS operations complete in order, so
            // a move-down after stage B returned its read - and let the wave go on to the next push - only once stage B's scattered
            // 64-bit atomics had gone through the LDS pipe, which nothing needs to wait for; now no wait stands between the last
            // atomic of a drain and the next push.
            // Why it is safe: a lane reads slot `lane` before it writes it (program order, and one wave's LDS operations execute
            // in order); the slots the other lanes write are not the ones this lane reads, [0, 64) having been read by all 64 lanes
            // before the first write (the write needs what the second read returns) and [64, 128) not being written at all; no
            // entry is overwritten before its lane has read it.  All 64 lanes copy, with no test of "lane < entries left": what
            // the others bring down lands in free slots [qtail, 64), which are written by a push before anything reads them (a
            // drain reads [0, 64) only once qtail >= 64, the last one only below qtail), and both slots are inside the wave's queue
            const uint2 ent = make_uint2(qtag[lane], qword[lane]);
            const unsigned int next_tag = qtag[kWave + lane], next_word = qword[kWave + lane];
            qtag[lane] = next_tag;
            qword[lane] = next_word;
            qaddr -= kBatchBytes;
            resolve_click(direct, ent);
            FDBG_ADD(4, FDBG_T() - tb);
            FDBG_ADD(7, 1);
        }
    };
    // m = the ballot of the lanes that push.  All 64 lanes are active wherever phase 2 pushes (256-lane workgroups, wave-uniform
    // control flow), so the pushing lanes are selected by writing the mask to exec around the one LDS write and all ones after it:
    // no saved mask, and no branch over the write (with ~20 of 64 lanes clicking it is never skipped)
    auto push = [&](unsigned long long m, unsigned int tagj, unsigned int payload) {
        const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
        // (the fill in the scalar addend rather than mbcnt_lo's: a VOP3 reads one SGPR, and the mask already is one)
        const unsigned int slot = rank * (unsigned int)sizeof(unsigned int) + qaddr;
        asm volatile("s_mov_b64 exec, %0\n\tds_write2st64_b32 %1, %2, %3 offset1:8\n\ts_mov_b64 exec, -1"
                     :: "s"(m), "v"(slot), "v"(tagj), "v"(payload) : "memory");
        qaddr += (unsigned int)__popcll(m) * (unsigned int)sizeof(unsigned int);
    };
    // one work item: auctions j0 .. j0 + n - 1 of keyword u (n == chunk unless TAIL)
    // (`calls4` = 4 x the Philox calls of the item: chunk for a full item, 4 for a tail call and for the partial call)
    auto run_item = [&](auto tail_tag, int u, int j0, int n, int calls4) {
        constexpr bool TAIL = decltype(tail_tag)::value;
        const uint32_t kw = kw_base + (uint32_t)u;
        const unsigned int tagj0 = adc::fast_tag((unsigned int)u, (unsigned int)j0);
        // the item's first Philox call: j0 is a multiple of 4 on all three paths (full items, tail calls, the partial call -
        // adc_fast_schedule.h), which the compiler cannot see, so the calls of the item are j0 / 4, + 1, ...: one add per call,
        // where (j0 + i) >> 2 is an add and a shift
        const uint32_t call0 = (uint32_t)j0 >> adc::kFastCallShift;
        unsigned int imp = 0;
        if (dense) {
            adc::WinIntervals iv = sh.win[u].iv;
            if (n == 0) iv.c_w = iv.n_w = 0u;                                       // a lane without an item resolves nothing
            asm volatile("" : "+v"(iv.c_w), "+v"(iv.n_w));      // (opaque: hipcc otherwise turns the zero width into `has-item && ...` on every compare)
            uint32_t call = call0;
            for (int i = 0; i < calls4; i += 4, call += 1u) {
                if (TAIL && __builtin_amdgcn_ballot_w64(i < n) == 0ull) break;
                FSLOT_ADD(0, 1ull);
                asm volatile("" : "+v"(call));      // (opaque: hipcc otherwise carries the call's 64-bit product from call to call, in two VGPRs more)
                const adc::U4 w = adc::draw_folded(key, call, adc::ST_AUCTION, kw, tick_k1);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const uint32_t word = h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w;
                    bool cw = (word - iv.c_lo) < iv.c_w;                           // clicked win
                    bool nw = (word - iv.n_lo) < iv.n_w;                           // unclicked win
                    if (TAIL) { const bool active = i + h < n; cw = cw && active; nw = nw && active; }
                    add_lane_bit(imp, __builtin_amdgcn_ballot_w64(nw));            // (the clicked wins are counted in stage B: phase 3 adds them)
                    push(__builtin_amdgcn_ballot_w64(cw), tagj0 + ((unsigned int)(i + h) << adc::kFastTagAuctionShift), word);     // (the mask itself: __ballot() goes through an int)
                    drain(false);
                }
            }
        }
        if (!dense) {
            const KwLawA ka = sh.law_a[u];
            const KwLawB kb = sh.law_b[u];
            const adc::AuctionLaw law{kb.d.t_click, ka.m_click, sh.win[u].d.m_noclick};
            const int bid_c = n > 0 ? kb.d.bid_c : 0;                               // (bid 0 never wins)
            uint32_t call = call0;
            for (int i = 0; i < calls4; i += 4, call += 1u) {
                if (TAIL && __builtin_amdgcn_ballot_w64(i < n) == 0ull) break;
                FSLOT_ADD(0, 1ull);
                asm volatile("" : "+v"(call));      // (opaque: hipcc otherwise carries the call's 64-bit product from call to call, in two VGPRs more)
                const adc::U4 w = adc::draw_folded(key, call, adc::ST_AUCTION, kw, tick_k1);
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const uint32_t word = h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w;
                    bool click_bit;
                    const int comp = adc::auction_outcome_unless_top_word(word, law, ka.loc, ka.scale, sh.logtab, click_bit);
                    bool win = adc::auction_wins(word, bid_c, comp);               // tie loses (helpers.py:167-170)
                    if (TAIL) win = win && i + h < n;
                    imp += (unsigned int)(win && !click_bit);
                    push(__builtin_amdgcn_ballot_w64(win && click_bit), tagj0 + ((unsigned int)(i + h) << adc::kFastTagAuctionShift), (unsigned int)comp);
                    drain(true);
                }
            }
        }
        if (imp) atomicAdd(&sh.a_cnt[u], (unsigned long long)imp);
    };

    // the full items (pass 0), then the tails' whole calls (pass 1): one loop, so that the item's code exists once
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
        const int shift = pass == 0 ? chunk_shift : adc::kFastCallShift;
        const int ptotal = pass == 0 ? total : total2;
        // R_w, base_w: wave-uniform.  The wave takes the part (w + tile index) mod 4, so that the waves with the shorter counts are
        // not the same wave - the same SIMD - in every workgroup of the CU (measured: that alone is worth more than the slots saved)
        const int part = adc::fast_wave_part(wq, tile_index);
        const int rounds = __builtin_amdgcn_readfirstlane(adc::fast_wave_rounds(ptotal, part));
        const int base = __builtin_amdgcn_readfirstlane(adc::fast_wave_base(ptotal, part));
        if (rounds == 0) continue;
        // this lane's items: `rounds` from `first`, as far as there are any; u = the keyword of the current one, u_end = where
        // that keyword's full items end
        const int first = adc::fast_lane_first(base, rounds, lane, ptotal);
        int u = 0, u_end = 0;
        if (pass == 0) {
#pragma unroll
            for (int s = kFastBlock / 2; s > 0; s >>= 1)
                if (sh.off[u + s] <= first) u += s;
            u_end = sh.off[u + 1];
        }
        for (int r = 0; r < rounds; ++r) {
            const int item = first + r;
            const bool has = adc::fast_item_exists(item, ptotal);
            [[maybe_unused]] const unsigned long long t_item = FDBG_T();
            int j0 = 0;
            if (pass == 0) {
                while (has && item >= u_end) { u += 1; u_end = sh.off[u + 1]; }     // (keywords without full items are skipped)
                if (has) j0 = (item - sh.off[u]) << shift;
            } else if (has) {
                u = sh.tail_kw[item];
                const int vw = sh.vol[u];
                j0 = adc::fast_tail_first(vw & kVolMask, chunk_shift) + ((item - (int)((unsigned int)vw >> kVolBits)) << shift);
            }
            FDBG_ADD(2, FDBG_T() - t_item);
            run_item(std::false_type{}, u, j0, has ? 1 << shift : 0, 1 << shift);
        }
    }
    // the partial calls: keyword `tid`, its last V mod 4 auctions
    // (the volume read back: nothing of phase 1 stays in a register over the passes above.  A wave none of whose 64 keywords has a
    // partial call skips the call: the test is the wave's own ballot - the queue is per wave - and no barrier stands here)
    {
        const int Vt = sh.vol[tid] & kVolMask;
        if (__builtin_amdgcn_ballot_w64(adc::fast_partial_count(Vt) != 0) != 0ull)
            run_item(std::true_type{}, tid, adc::fast_partial_first(Vt), adc::fast_partial_count(Vt), 1 << adc::kFastCallShift);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if ((unsigned int)lane < (qaddr - qbase) / (unsigned int)sizeof(unsigned int)) resolve_click(!dense, make_uint2(qtag[lane], qword[lane]));      // fewer than 64 left: the last batch reads its own entries
    [[maybe_unused]] const unsigned long long t_p3 = FDBG_T();
    FDBG_ADD(3, t_p3 - t_p2);
    __syncthreads();

    // ---- phase 3: outputs ---------------------------------------------------------------------
    if constexpr (LISTS) { if (raw.emit && !NARROW && tid < adc::kTimesteps) v.click_count[(size_t)env * adc::kTimesteps + tid] = ls.row_count[tid]; }
    if (valid) {
        const size_t o = (size_t)env * v.K + k;
        const unsigned long long cnt = sh.a_cnt[tid];
        // (a tile that packs: cost | revenue << 32 in a_cost, a_rev unused)
        const unsigned long long cw = sh.a_cost[tid];
        const long long my_cost = pack_mask ? (long long)(unsigned int)cw : (long long)cw;
        const long long r = pack_mask ? (long long)(cw >> 32) : (long long)sh.a_rev[tid];
        const unsigned int cnt_lo = (unsigned int)cnt, cnt_hi = (unsigned int)(cnt >> 32);      // 21-bit fields at bits 0, 21, 42
        // (stage A counts the unclicked wins only; an impression is a win, clicked or not: both counts are at most the day's
        // volume <= 2^20, and so is their sum, formed here in 32 bits outside the packed word)
        const unsigned int clicks = ((cnt_lo >> 21) | (cnt_hi << 11)) & 0x1FFFFFu;
        v.imp[o] = (int)((cnt_lo & 0x1FFFFFu) + clicks);
        v.clk[o] = (int)clicks;
        v.conv[o] = (int)(cnt_hi >> 10);
        v.cost[o] = adc::cents_to_dollars_f32(my_cost);
        v.rev[o] = adc::cents_to_dollars_f32(r);
        if (v.metrics_on) metric_add(v, o, r - my_cost);    // corrected by k_step_exact_rows if it re-runs this env
    }
    // tile cost / profit -> env totals: wave 0 alone sums the tile's LDS accumulators (they are final since the barrier
    // above; one wave's shuffles instead of four's)
    if (wv == 0) {
        long long c = 0, p = 0;
#pragma unroll
        for (int i = 0; i < kFastBlock / kWave; ++i) {
            const int u = lane + i * kWave;
            if (u < tile_kw && tile * tile_kw + u < v.K) {
                const unsigned long long cw = sh.a_cost[u];
                const long long cc = pack_mask ? (long long)(unsigned int)cw : (long long)cw;
                c += cc;
                p += (pack_mask ? (long long)(cw >> 32) : (long long)sh.a_rev[u]) - cc;
            }
        }
        c = wave_sum_i64(c);
        p = wave_sum_i64(p);
        if (lane == 0) {
            if (tiles == 1) { v.env_cost[env] = c; v.env_profit[env] = p; }
            else {
                atomicAdd((unsigned long long *)&v.env_cost[env], (unsigned long long)c);
                atomicAdd((unsigned long long *)&v.env_profit[env], (unsigned long long)p);
            }
        }
    }
    FDBG_ADD(5, FDBG_T() - t_p3);
    FDBG_ADD(6, 1);
    __syncthreads();                    // the next tile reuses the accumulators and the scratch
  }   // tiles of this workgroup
#ifdef ADC_EXP_TIMING
    // slots 8..15 (cycles of wave 0, summed over workgroups): phase 1 | law setup | item search | phase 2 | stage B | phase 3 | tiles | stage-B batches
    if (tid == 0) for (int i = 0; i < 8; ++i) atomicAdd(&g_fdbg[blockIdx.x & 255][i], fdbg[i]);
    // every wave: Philox calls it issued in phase 2 (wave-call-slots) | calls that hold an auction, summed over its keywords
    {
        const unsigned long long needed = (unsigned long long)wave_sum_i64((long long)fslots[1]);
        if (lane == 0) { atomicAdd(&g_fslots[blockIdx.x & 255][0], fslots[0]); atomicAdd(&g_fslots[blockIdx.x & 255][1], needed); }
    }
#endif
}

// step tail (gymnasium_kw_env.py:222-244), run by one lane per env
__device__ __forceinline__ void step_tail(const View &v, int env, uint32_t tick, bool implicit, long long profit_c, double reward_d)
{
    double reward, cum;
    if (implicit) {
        const long long cc = v.cum_cents[env] + profit_c;
        v.cum_cents[env] = cc;
        reward = (double)profit_c / 100.0;
        cum = (double)cc / 100.0;
    } else {
        reward = reward_d;
        cum = v.cum[env] + reward;
        v.cum[env] = cum;
    }
    const bool truncated = cum < -v.loss_threshold;                 // :225
    const int day = v.day[env] + 1;                                  // :227
    const bool terminated = day >= v.max_days;                       // :228
    v.reward[env] = reward;
    v.cum_profit[env] = cum;
    v.day_out[env] = day;
    v.term[env] = terminated;
    v.trunc[env] = truncated;
    v.day[env] = day;
    v.tick[env] = tick + 1u;
    if (v.drift_on) v.drift_pending[env] = 1;                        // :246 update_keywords()
    if (v.auto_reset && (terminated || truncated)) {
        v.day[env] = 0; v.cum_cents[env] = 0; v.cum[env] = 0.0;      // :327-328
    }
    v.env_cost[env] = 0;
    v.env_profit[env] = 0;
    if (v.metrics_on) {
        // per-env running sums (no same-address atomics: 4096 waves on one word serialise at ~12 ns each)
        const long long pc = implicit ? profit_c : (long long)__double2ll_rn(reward * 100.0);
        v.metric_env[env] += pc;
        v.metric_env[(size_t)v.NP + env] += 1;
        if (terminated || truncated) v.metric_env[2 * (size_t)v.NP + env] += 1;
        if (truncated) v.metric_env[3 * (size_t)v.NP + env] += 1;
    }
}

