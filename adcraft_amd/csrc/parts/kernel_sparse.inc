// kernel_sparse.inc - k_step_implicit_sparse: the budget-free pass for keyword sets with FEW auctions per keyword
// (part of the single translation unit adc_engine.hip; see that file for the overview)
// -------------------------------------------------------------------------------------------------
// Same law, same stream, same outputs as k_step_implicit_fast (bit for bit: the choice between the two is the host's
// scheduling hint), laid out for a day of ~10 auctions per keyword with half of the keywords empty
// (sample_implicit_keywords_from_quantile_dfs with no_vol_prob, adcraft/gymnasium_kw_utils.py:295-300), where what a
// KEYWORD costs matters as much as what an auction costs:
//   * an auction is classified by comparing its word with the keyword's win BRACKETS (adc_law.h win_brackets: float
//     estimates of the two win intervals with a guaranteed slack - ~65 instructions per keyword instead of the ~650 of the
//     exact intervals, or of ~35 per auction for sampling the competitor's bid): inside the inner pair it is a win, outside
//     the outer pair a loss; the ~2e-5 of words in between are resolved from the sampled competitor bid, as the oracle
//     resolves every auction.  Four subtract-and-compare pairs per auction, all mask logic on the scalar unit;
//   * work items (one Philox call = four auctions of one keyword) are dealt round-robin through a byte list in LDS that the
//     keywords fill themselves - no per-item binary search;
//   * the competitor's bid (the 2nd price) is evaluated only for clicked wins, in stage B, on full wavefronts, with the
//     conversion / revenue call (as in k_step_implicit_fast);
//   * the env's cost / profit totals are carried in registers across the tiles of an env and reduced once per env.
constexpr int kSparseItemCap = 1024;     // work items listed per tile (a multiple of kFastBlock); items beyond it are located by search

struct SparseShared {
    int2 offvol[kFastBlock + 1];                            // {first work item, volume} per keyword; [kFastBlock] = {total, 0}
    adc::WinIntervals win_out[kFastBlock], win_in[kFastBlock];
    KwLawA law_a[kFastBlock];                               // stage B: rescale multiplier of the click sub-interval, conversion threshold, competitor law
    float2 rev_law[kFastBlock];                             // stage B, conversions: revenue mean and deviation
    unsigned long long a_cnt[kFastBlock], a_cost[kFastBlock], a_rev[kFastBlock];
    float lognodes[adc::kLogTableIntervals + 1];            // copy of g_log_nodes (adc::LogNodes: half the bytes of g_log_table, same bits)
    float normtab[adc::kNormTableEntries + 1];              // copy of g_norm_nodes
    unsigned char items[kSparseItemCap];                    // keyword-in-tile of work item i
    uint2 queue[kFastBlock / kWave][kQueueCap];             // per-wave rings: {keyword-in-tile << 24 | auction index, word}; while a wave's
                                                            // ring is empty (between tiles) its first 256 bytes pass the volume words around
    int wave_tot[kFastBlock / kWave];
};
// (LDS is handed out in blocks of 1280 bytes on gfx950 - measured in round 5: a 32 608-byte variant of this kernel ran at FOUR workgroups
//  per CU, 0.535 ms on cfg3 against 0.47 at 31 968 bytes - so five workgroups per CU need 25 blocks = 32 000 bytes each, not 32 768)
static_assert(sizeof(SparseShared) <= 25 * 1280, "SparseShared must allow 5 workgroups per CU");
static_assert(kSparseItemCap % kFastBlock == 0, "a round of work items lies on one side of the list's end");

// sum of a 64-bit value over the wave, in every lane: three 22-bit limbs summed as 32-bit integers (64 x 2^22 < 2^32; the
// 64-bit DPP additions the compiler builds from wave_scan<long long> are ~40 instructions per sum)
__device__ __forceinline__ unsigned long long wave_sum_u64_limbs(unsigned long long x)
{
    const unsigned int lo = (unsigned int)x, hi = (unsigned int)(x >> 32);
    const unsigned long long a = (unsigned int)wave_sum_i32((int)(lo & 0x3FFFFFu));
    const unsigned long long b = (unsigned int)wave_sum_i32((int)((lo >> 22) | ((hi & 0xFFFu) << 10)));
    const unsigned long long c = (unsigned int)wave_sum_i32((int)(hi >> 12));
    return a + (b << 22) + (c << 44);
}

// Element `tid` of a wave-uniform array, addressed the way the hardware likes it: the base in scalar registers, the lane's part as
// one 32-bit byte offset (global_load / global_store "saddr" form).  The opaque statement keeps the compiler from folding
// the base into per-lane arithmetic - without it the loop-invariant halves (array base + 4 tid) of a dozen addresses are
// hoisted into 64-bit VGPR pairs that live through the whole tile loop and spill.  (The pointer is typed GLOBAL: after the
// opaque statement the address space can no longer be inferred, and a generic pointer means flat_load / flat_store.)
template <typename T>
__device__ __forceinline__ __attribute__((address_space(1))) T &lane_elem(T *uniform_base, unsigned int tid)
{
    typedef __attribute__((address_space(1))) char gchar;
    gchar *g = (gchar *)uniform_base;
    asm("" : "+s"(g));
    return *(__attribute__((address_space(1))) T *)(g + tid * (unsigned int)sizeof(T));
}

// What a lane holds of the NEXT tile while the current tile's auctions are resolved (requested when the current tile begins)
struct TileParams {
    float vol_mean, vol_std, bctr, sctr, loc, scale, mu, sd, bid;
    int metric_old;             // metric mode: the 32-bit word of the keyword's running profit sum (written back with the tile's outputs)
};
// The env's stream state and flags.  Loaded by every lane through an index the compiler cannot see through (a value it knows
// to be uniform is moved to scalar registers right behind its load - a wait for a memory round trip wherever the load
// stands) and made scalar with v_readfirstlane where the wait is affordable.
struct EnvHeaderV {
    unsigned long long key;
    uint32_t tick, drift, skip;
};
struct EnvHeader {
    uint64_t key;
    uint32_t tick;
    bool drift, skip;
};

#ifndef ADC_SPARSE_WAVES
#define ADC_SPARSE_WAVES 5
#endif
__global__ __launch_bounds__(kFastBlock, ADC_SPARSE_WAVES) void k_step_implicit_sparse(View v, const float *__restrict__ bids, int tiles_per_wg)
{
    __shared__ SparseShared sh;
    const int tiles = (v.K + kFastBlock - 1) / kFastBlock;
    const unsigned int tid = threadIdx.x;
    const unsigned int lane = tid & 63u;
    const int wv = (int)(tid >> 6);
    const size_t plane = (size_t)v.NP * v.K;
    [[maybe_unused]] unsigned long long fdbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    [[maybe_unused]] const unsigned long long t_kernel = FDBG_T();
    uint2 *const ring = sh.queue[__builtin_amdgcn_readfirstlane(wv)];      // (wave-uniform: keep the base scalar)
    int lane_zero;                             // 0, in a vector register the compiler cannot see through (see EnvHeaderV)
    asm("v_mov_b32 %0, 0" : "=v"(lane_zero));
    // The engine view's two dozen array pointers, re-read from the kernel-argument segment where they are used (scalar loads
    // from constant memory; `v` is the first argument, at offset 0): held in scalar registers for the whole tile loop they
    // do not fit, and every use of a spilled one is a v_readlane pair - vector issue slots, the resource this kernel runs out of.
    typedef const __attribute__((address_space(4))) View ArgView;
    auto args = [&]() -> ArgView * {
        ArgView *p = (ArgView *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(p));
        return p;
    };

    auto load_params = [&](int tile_index) {
        TileParams r{};
        const int env = tile_index / tiles;
        const int k0 = (tile_index - env * tiles) * kFastBlock;
        // (not conditional on the env's skip flag: an env that is skipped - rare - has its parameters read for nothing, but
        // no tile waits for its env's flags before it may ask for its parameters)
        if (k0 + (int)tid < v.K) {
            ArgView *a = args();
            const size_t o = (size_t)env * v.K + k0;
            const float *row = a->params + o;
            r.vol_mean = lane_elem(row + ADC_P_VOL_MEAN * plane, tid);
            r.vol_std = lane_elem(row + ADC_P_VOL_STD * plane, tid);
            r.bctr = lane_elem(row + ADC_P_BCTR * plane, tid);
            r.sctr = lane_elem(row + ADC_P_SCTR * plane, tid);
            r.loc = lane_elem(row + ADC_P_A * plane, tid);
            r.scale = lane_elem(row + ADC_P_B * plane, tid);
            r.mu = lane_elem(row + ADC_P_REV_MEAN * plane, tid);
            r.sd = lane_elem(row + ADC_P_REV_STD * plane, tid);
            r.bid = lane_elem(bids + o, tid);
            if (v.metrics_on) r.metric_old = lane_elem(a->metric_lo + o, tid);
        }
        return r;
    };
    // makes the loaded values of p "used" here, i.e. the wait for them is placed here (see phase 3 for why that matters)
    auto take_delivery = [](const TileParams &p) {
        asm volatile("" ::"v"(p.bctr), "v"(p.sctr), "v"(p.loc), "v"(p.scale), "v"(p.mu), "v"(p.sd), "v"(p.bid), "v"(p.metric_old), "v"(p.vol_mean), "v"(p.vol_std));
    };
    auto request_header = [&](int tile_index) {
        const int env = tile_index / tiles;
        EnvHeaderV h;
        ArgView *a = args();
        h.key = a->key[env + lane_zero];
        h.tick = a->tick[env + lane_zero];
        h.drift = v.drift_on ? a->drift_pending[env + lane_zero] : 0;
        h.skip = (a->exact_hint[env + lane_zero] & ~4) == 2;      // scheduling hint only (2, 6): the budget-exact kernels compute this env alone (same results)
        return h;
    };
    auto receive_header = [&](const EnvHeaderV &h) {
        EnvHeader r;
        r.key = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(h.key >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)h.key);
        r.tick = (uint32_t)__builtin_amdgcn_readfirstlane((int)h.tick);
        r.drift = __builtin_amdgcn_readfirstlane((int)h.drift) != 0;
        r.skip = __builtin_amdgcn_readfirstlane((int)h.skip) != 0;
        return r;
    };
    // the tile's volume (after the volume part of its pending drift).  One Philox call serves four consecutive keywords: 16
    // lanes of each wave draw for the wave's 64 (through the wave's own, momentarily idle click ring - no workgroup barrier).
    auto draw_volume = [&](int tile_index, const EnvHeader &h, TileParams &p) -> int {
        if (h.skip) return 0;
        const int env = tile_index / tiles;
        const int k0 = (tile_index - env * tiles) * kFastBlock;
        const bool valid = k0 + (int)tid < v.K;
        if (valid && h.drift && drift_selected(v, env, k0 + (int)tid)) {      // update_keywords() of the previous step, volume part (gymnasium_kw_env.py:136-141)
            const adc::U4 w = adc::draw(h.key, 0u, adc::ST_DRIFT, (uint32_t)(k0 + (int)tid), h.tick - 1u);
            float a_vol, a_ctr, a_cvr, unused_b = 0.0f, unused_s = 0.0f;
            drift_magnitudes(v, env, a_vol, a_ctr, a_cvr);
            apply_drift_coefficients(adc::drift_coeff(w.x, a_vol), 0.0f, 0.0f, p.vol_mean, p.vol_std, unused_b, unused_s);
            lane_elem(v.params + ((size_t)env * v.K + k0) + ADC_P_VOL_MEAN * plane, tid) = p.vol_mean;
        }
        unsigned int *const scratch = reinterpret_cast<unsigned int *>(ring);
        if (lane < 16u) {
            const adc::U4 w = adc::draw(h.key, 0u, adc::ST_VOL, ((uint32_t)k0 >> 2) + 16u * (uint32_t)wv + lane, h.tick);
            *reinterpret_cast<uint4 *>(&scratch[4u * lane]) = make_uint4(w.x, w.y, w.z, w.w);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t word = scratch[lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int V = 0;
        if (valid) {
            float x = adc::fma32(p.vol_std, normal_tab_nodes(word, sh.normtab), p.vol_mean);      // adc::volume_from_word
            x = x > 0.0f ? x : 0.0f;
            x = x < (float)adc::kVolumeMax ? x : (float)adc::kVolumeMax;
            const float t = __builtin_truncf(x);
            V = (int)t + ((x - t) >= 0.5f ? 1 : 0);
        }
        return V;
    };

    const int n_tiles = v.N * tiles;
    const int tile_first = blockIdx.x * tiles_per_wg, tile_last = min(tile_first + tiles_per_wg, n_tiles);
    for (unsigned int i = tid; i <= (unsigned int)adc::kLogTableIntervals; i += kFastBlock) sh.lognodes[i] = g_log_nodes[i];
    for (unsigned int i = tid; i <= (unsigned int)adc::kNormTableEntries; i += kFastBlock) sh.normtab[i] = g_norm_nodes[i];
    sh.a_cnt[tid] = sh.a_cost[tid] = sh.a_rev[tid] = 0ull;        // (afterwards every lane clears its own keyword's sums when it has read them)
    TileParams next = load_params(tile_first);
    EnvHeader next_env = receive_header(request_header(tile_first));
    __syncthreads();                                              // the tables are in place
    int next_V = draw_volume(tile_first, next_env, next);
    // (every path into the tile loop hands over DELIVERED values - see phase 3 - or the wait for them is placed at the loop's
    // head, behind the previous tile's stores)
    take_delivery(next);
    unsigned long long acc_cost = 0ull, acc_rev = 0ull;       // this lane's share of the env's spend / revenue (cents)

  for (int tile_index = tile_first; tile_index < tile_last; ++tile_index) {
    const EnvHeader head = next_env;
    TileParams raw = next;
    const int metric_old = raw.metric_old;
    const int V = next_V;
    const bool more = tile_index + 1 < tile_last;
    if (more) next = load_params(tile_index + 1);       // in flight through the whole tile
    const int env = tile_index / tiles;
    const int tile = tile_index - env * tiles;
    const int k0 = tile * kFastBlock;
    const bool valid = k0 + (int)tid < v.K;
    const uint64_t key = head.key;
    const uint32_t tick = head.tick;
    const uint32_t kw_base = (uint32_t)k0;
    [[maybe_unused]] const unsigned long long t_start = FDBG_T();
    [[maybe_unused]] unsigned long long t_p3 = t_start;

    // (one path through the loop body, whatever the env's flags: a `continue` would be a second way back to the loop's head,
    // and a path on which the next tile's loads look issued but not delivered puts the wait for them there - behind the stores)
    if (!head.skip) {                           // (block-uniform; a skipped env contributes nothing to acc_*)
    // ---- phase 1: one lane per keyword ---------------------------------------------------------
    if (valid && head.drift && drift_selected(v, env, k0 + (int)tid)) {      // update_keywords() of the previous step, the two rates (gymnasium_kw_env.py:142-158)
        const adc::U4 w = adc::draw(key, 0u, adc::ST_DRIFT, (uint32_t)(k0 + (int)tid), tick - 1u);
        float a_vol, a_ctr, a_cvr, unused_m = 0.0f;
        drift_magnitudes(v, env, a_vol, a_ctr, a_cvr);
        apply_drift_coefficients(0.0f, adc::drift_coeff(w.y, a_ctr), adc::drift_coeff(w.z, a_cvr), unused_m, 0.0f, raw.bctr, raw.sctr);
        float *row = v.params + ((size_t)env * v.K + k0);
        lane_elem(row + ADC_P_BCTR * plane, tid) = raw.bctr;
        lane_elem(row + ADC_P_SCTR * plane, tid) = raw.sctr;
    }
    // a work item = one Philox call = four consecutive auctions of one keyword (the keyword's last one partial)
    const int nch = (V + 3) >> 2;
    const int incl = wave_scan_i32(nch);
    if (lane == 63u) sh.wave_tot[wv] = incl;
    // the keyword's law and win brackets (only keywords with auctions need them)
    if (V > 0) {
        const float t_f = adc::bernoulli_threshold_f32(raw.bctr);
        const int bid_c = adc::bid_to_cents_i32(raw.bid);
        const adc::WinBrackets br = adc::win_brackets(bid_c, raw.loc, raw.scale, t_f);
        sh.win_out[tid] = br.out;
        sh.win_in[tid] = br.in;
        sh.law_a[tid] = KwLawA{adc::rescale_multiplier_f32(t_f), adc::saturate_threshold(adc::bernoulli_threshold(raw.sctr)), raw.loc, raw.scale};
        sh.rev_law[tid] = make_float2(raw.mu, raw.sd);
    }
    __syncthreads();
    int wave_base = 0, total = 0;
#pragma unroll
    for (int i = 0; i < kFastBlock / kWave; ++i) {
        const int t = sh.wave_tot[i];
        if (i < wv) wave_base += t;
        total += t;
    }
    const int off = wave_base + incl - nch;
    sh.offvol[tid] = make_int2(off, V);
    if (tid == 0u) sh.offvol[kFastBlock] = make_int2(total, 0);
    // every keyword lists its own work items, four per trip (wave-uniform trip count: the wave's largest keyword)
    {
        const int listed = min(nch, kSparseItemCap - off);      // (<= 0: this keyword's items lie beyond the list)
        unsigned char *const mine = &sh.items[min(off, kSparseItemCap)];
        for (int q = 0; __builtin_amdgcn_ballot_w64(q < listed) != 0ull; q += 4) {
            if (q < listed) mine[q] = (unsigned char)tid;
            if (q + 1 < listed) mine[q + 1] = (unsigned char)tid;
            if (q + 2 < listed) mine[q + 2] = (unsigned char)tid;
            if (q + 3 < listed) mine[q + 3] = (unsigned char)tid;
        }
    }
    __syncthreads();                    // (also: everybody has read wave_tot)
    [[maybe_unused]] const unsigned long long t_p2 = FDBG_T();
    FDBG_ADD(0, t_p2 - t_start);

    // ---- phase 2: work items dealt round-robin -----------------------------------------------------
    // A full round gives wave w, lane l item 256 r + 4 l + w (neighbouring lanes are four items apart, i.e. mostly on different
    // keywords: their LDS atomics do not collide); the last, partly filled round is dealt in order, so that it occupies only the
    // first wave(s).  Control flow is wave-uniform so that the deferred-click ring can be maintained with ballots.  Stage A
    // (every auction): classify the word.  Stage B (clicked wins only): the (keyword, auction, word) is pushed to a per-wave
    // LDS ring; whenever 64 are waiting, all 64 lanes evaluate the price paid and draw the conversion / revenue call together.
    unsigned int qhead = 0, qtail = 0;
    const adc::LogNodes logtab{sh.lognodes};

    auto resolve_click = [&](unsigned int pos) {
        const uint2 ent = ring[pos & (kQueueCap - 1)];
        const unsigned int uu = ent.x >> 24;
        const KwLawA ka = sh.law_a[uu];
        unsigned int vv = adc::mulhi32(ent.y, ka.m_click);                            // a click: the offset is the word itself
        vv = vv < 0x00FFFFFFu ? vv : 0x00FFFFFFu;
        const unsigned int price = (unsigned int)adc::competitor_cents_from_v(vv, ka.loc, ka.scale, logtab);
        const adc::U4 w2 = adc::draw(key, ent.x & 0x00FFFFFFu, adc::ST_CONV, kw_base + uu, tick);
        const bool conv = adc::bernoulli32(w2.x, ka.t_conv);
        unsigned long long cnt = 1ull << kClkShift;
        if (conv) {
            const float2 rl = sh.rev_law[uu];
            float x = adc::fma32(rl.y, normal_tab_nodes(w2.y, sh.normtab), rl.x);
            x = x > 0.01f ? x : 0.01f;
            const unsigned long long rc = (unsigned long long)adc::money_to_cents(x);
            atomicAdd(&sh.a_rev[uu], rc);
            acc_rev += rc;
            cnt |= 1ull << kConvShift;
        }
        atomicAdd(&sh.a_cnt[uu], cnt);
        atomicAdd(&sh.a_cost[uu], (unsigned long long)price);
        acc_cost += price;
    };
    auto drain = [&]() {
        while (qtail - qhead >= (unsigned int)kWave) {      // checked after every push: <= 63 + 64 entries wait (ring holds 128)
            [[maybe_unused]] const unsigned long long tb = FDBG_T();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            resolve_click(qhead + lane);
            qhead += kWave;
            FDBG_ADD(4, FDBG_T() - tb);
            FDBG_ADD(7, 1);
        }
    };
    // one work item: auctions j0 .. j0 + n - 1 of keyword u (n = 0: a lane without an item)
    auto run_item = [&](int u, int j0, int n) {
        const adc::WinIntervals wo = sh.win_out[u], wi = sh.win_in[u];
        const unsigned int tagj0 = ((unsigned int)u << 24) | (unsigned int)j0;
        unsigned int imp = 0;
        const adc::U4 w = adc::draw(key, (uint32_t)j0 >> 2, adc::ST_AUCTION, kw_base + (uint32_t)u, tick);
        // (unrolled: a rolled loop was measured 10 % slower - the words then rotate through registers and the ring push loses
        // its immediate tags)
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const uint32_t word = h == 0 ? w.x : h == 1 ? w.y : h == 2 ? w.z : w.w;
            const unsigned long long act = __builtin_amdgcn_ballot_w64(h < n);
            const unsigned long long co = __builtin_amdgcn_ballot_w64((word - wo.c_lo) < wo.c_w), ci = __builtin_amdgcn_ballot_w64((word - wi.c_lo) < wi.c_w);
            const unsigned long long no = __builtin_amdgcn_ballot_w64((word - wo.n_lo) < wo.n_w), ni = __builtin_amdgcn_ballot_w64((word - wi.n_lo) < wi.n_w);
            unsigned long long cw = co & act, nw = no & act;                      // clicked wins, unclicked wins (lane masks)
            const unsigned long long amb = ((co & ~ci) | (no & ~ni)) & act;       // between the brackets: the long way
            if (amb != 0ull) {
                bool e_cw = false, e_nw = false;
                if (__builtin_amdgcn_inverse_ballot_w64(amb)) {
                    // (rare: the click rate and the bid come from memory again - after the pending drift, which this
                    // workgroup wrote back before its barriers; an agent-scope load, not this CU's L1)
                    const size_t ou = (size_t)env * v.K + (size_t)(k0 + u);
                    const float bctr_u = __hip_atomic_load(v.params + ADC_P_BCTR * plane + ou, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const adc::AuctionLaw law = adc::make_auction_law(bctr_u);
                    const int bid_cu = adc::bid_to_cents_i32(bids[ou]);
                    const KwLawA ka = sh.law_a[u];
                    bool click;
                    const int comp = adc::auction_outcome_unless_top_word(word, law, ka.loc, ka.scale, logtab, click);
                    const bool win = adc::auction_wins(word, bid_cu, comp);       // tie loses (helpers.py:167-170)
                    e_cw = win && click;
                    e_nw = win && !click;
                }
                cw = (cw & ~amb) | __builtin_amdgcn_ballot_w64(e_cw);
                nw = (nw & ~amb) | __builtin_amdgcn_ballot_w64(e_nw);
            }
            add_lane_bit(imp, cw | nw);
            // push the clicked wins (one ds_write_b64 per entry: consecutive 8-byte slots are conflict-free)
            const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(cw >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)cw, qtail));
            if (__builtin_amdgcn_inverse_ballot_w64(cw)) ring[rank & (kQueueCap - 1)] = make_uint2(tagj0 + (unsigned int)h, word);
            qtail += __popcll(cw);
            drain();
        }
        if (imp) atomicAdd(&sh.a_cnt[u], (unsigned long long)imp);
    };
    // which keyword work item `item` belongs to, and that keyword's {first item, volume}
    auto locate = [&](int r, int item, int &u, int2 &ov) {
        if (r < kSparseItemCap / kFastBlock) u = sh.items[item];    // (an unlisted slot of the last round reads some keyword: n = 0)
        else {
            u = 0;
#pragma unroll
            for (int s = kFastBlock / 2; s > 0; s >>= 1)
                if (sh.offvol[u + s].x <= item) u += s;
        }
        const long long both = *reinterpret_cast<const long long *>(&sh.offvol[u]);      // (one ds_read_b64)
        ov = make_int2((int)(unsigned int)both, (int)(both >> 32));
    };
    auto item_of_round = [&](int r) { return r * kFastBlock + (r < (total >> 8) ? (int)(4u * lane) + wv : (int)tid); };

    const int rounds = (total + kFastBlock - 1) / kFastBlock;
    int u_cur = 0;
    int2 ov_cur = make_int2(0, 0);
    if (rounds > 0) locate(0, item_of_round(0), u_cur, ov_cur);
    for (int r = 0; r < rounds; ++r) {
        const int item = item_of_round(r);
        const bool has = item < total;
        if (__builtin_amdgcn_ballot_w64(has) == 0ull) break;        // (the last round is dealt in order: nothing left for this wave)
        [[maybe_unused]] const unsigned long long t_item = FDBG_T();
        const int u = u_cur;
        const int j0 = has ? (item - ov_cur.x) << 2 : 0;
        const int n = has ? min(4, ov_cur.y - j0) : 0;
        if (r + 1 < rounds) locate(r + 1, item_of_round(r + 1), u_cur, ov_cur);      // (the next round's look-up is in flight during this item)
        FDBG_ADD(2, FDBG_T() - t_item);
        run_item(u, j0, n);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < qtail - qhead) resolve_click(qhead + lane);      // fewer than 64 left
    t_p3 = FDBG_T();
    FDBG_ADD(3, t_p3 - t_p2);
    __syncthreads();
    }   // !head.skip

    // ---- phase 3: outputs; the next tile's env header is fetched and its volume drawn meanwhile ----------------------------
    // Memory operations retire in order: a loaded value first used after this tile's stores would wait for the stores'
    // acknowledgements as well (microseconds).  So: request the header, compute the outputs, take delivery of everything that
    // is in flight, draw the next volume - and only then store.
    EnvHeaderV hv{};
    if (more) hv = request_header(tile_index + 1);
    unsigned long long cnt = 0ull;
    long long my_cost = 0, rv = 0;
    const bool writes = valid && !head.skip;
    if (writes) {
        cnt = sh.a_cnt[tid];
        my_cost = (long long)sh.a_cost[tid];
        rv = (long long)sh.a_rev[tid];
        sh.a_cnt[tid] = sh.a_cost[tid] = sh.a_rev[tid] = 0ull;      // ready for the next tile (nobody else touches them before its barriers)
    }
    const float cost_d = adc::cents_to_dollars_f32_nonneg((unsigned long long)my_cost), rev_d = adc::cents_to_dollars_f32_nonneg((unsigned long long)rv);
    take_delivery(next);        // (unconditional: a path on which the loads look issued but not delivered puts the wait at the loop's head)
    if (more) {
        next_env = receive_header(hv);
        next_V = draw_volume(tile_index + 1, next_env, next);
    }
    if (writes) {
        ArgView *a = args();
        const size_t o = (size_t)env * v.K + k0;
        const unsigned int cnt_lo = (unsigned int)cnt, cnt_hi = (unsigned int)(cnt >> 32);      // 21-bit fields at bits 0, 21, 42
        lane_elem(a->imp + o, tid) = (int)(cnt_lo & 0x1FFFFFu);
        lane_elem(a->clk + o, tid) = (int)(((cnt_lo >> 21) | (cnt_hi << 11)) & 0x1FFFFFu);
        lane_elem(a->conv + o, tid) = (int)(cnt_hi >> 10);
        lane_elem(a->cost + o, tid) = cost_d;
        lane_elem(a->rev + o, tid) = rev_d;
        if (v.metrics_on) {         // (common.inc metric_add on the prefetched word; corrected by k_step_exact_rows if it re-runs this env)
            const long long s = (long long)metric_old + (rv - my_cost);
            if (s == (long long)(int)s) lane_elem(a->metric_lo + o, tid) = (int)s;
            else { lane_elem(a->metric_hi + o, tid) += s; lane_elem(a->metric_lo + o, tid) = 0; }
        }
    }
    // the env's totals leave the registers when the workgroup's next tile belongs to another env
    if (!more || (tile_index + 1) / tiles != env) {
        const unsigned long long c = wave_sum_u64_limbs(acc_cost), p = wave_sum_u64_limbs(acc_rev);
        if (lane == 0u && (c | p) != 0ull) {
            ArgView *a = args();
            atomicAdd((unsigned long long *)&a->env_cost[env], c);
            atomicAdd((unsigned long long *)&a->env_profit[env], p - c);
        }
        acc_cost = acc_rev = 0ull;
    }
    FDBG_ADD(5, FDBG_T() - t_p3);
    FDBG_ADD(6, 1);
  }   // tiles of this workgroup
#ifdef ADC_EXP_TIMING
    fdbg[1] = FDBG_T() - t_kernel;          // slot "law setup" of the report: the wave's whole life
    if (tid == 0u) for (int i = 0; i < 8; ++i) atomicAdd(&g_fdbg[blockIdx.x & 255][i], fdbg[i]);
#endif
}

// the brackets as the device computes them (its own exp2 / rcp), for tests: out8[i] = {outer c_lo, c_w, n_lo, n_w, inner ...}
__global__ void k_debug_win_brackets(int n, const float *bid, const float *loc, const float *scale, const float *bctr, uint32_t *out8)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const adc::WinBrackets b = adc::win_brackets(adc::bid_to_cents_i32(bid[i]), loc[i], scale[i], adc::bernoulli_threshold_f32(bctr[i]));
    uint32_t *o = out8 + 8 * (size_t)i;
    o[0] = b.out.c_lo; o[1] = b.out.c_w; o[2] = b.out.n_lo; o[3] = b.out.n_w;
    o[4] = b.in.c_lo; o[5] = b.in.c_w; o[6] = b.in.n_lo; o[7] = b.in.n_w;
}

// the stream's generator as the device runs it, for tests: out4[i] = philox(ctr4[i], key2[i])
__global__ void k_debug_philox(int n, const uint32_t *ctr4, const uint32_t *key2, uint32_t *out4)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const adc::U4 w = adc::philox4x32(ctr4[4 * i], ctr4[4 * i + 1], ctr4[4 * i + 2], ctr4[4 * i + 3], key2[2 * i], key2[2 * i + 1]);
    out4[4 * i] = w.x; out4[4 * i + 1] = w.y; out4[4 * i + 2] = w.z; out4[4 * i + 3] = w.w;
}

