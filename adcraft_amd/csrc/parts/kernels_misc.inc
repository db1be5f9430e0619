// kernels_misc.inc - drift, metrics, ideal profit, keyword generation, reset, actions, flat I/O, nth_price_auction
// (part of the single translation unit adc_engine.hip; see that file for the overview)
// -------------------------------------------------------------------------------------------------
// small kernels
// -------------------------------------------------------------------------------------------------
__global__ void k_materialize_drift(View v)
{
    const int env = blockIdx.x;
    if (!(v.drift_on && v.drift_pending[env])) return;
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    for (int k = threadIdx.x; k < v.K; k += blockDim.x) {
        drift_keyword_planes(v, env, key, tick - 1u, k);
    }
    __syncthreads();
    if (threadIdx.x == 0) v.drift_pending[env] = 0;
}

// update_keywords() called by the user: schedule one more drift now (draw keyed by the current tick)
__global__ void k_force_drift(View v)
{
    const int env = blockIdx.x;
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    for (int k = threadIdx.x; k < v.K; k += blockDim.x) {
        drift_keyword_planes(v, env, key, tick, k);
    }
    __syncthreads();
    if (threadIdx.x == 0) v.tick[env] = tick + 1u;    // the draw must not be reused by the next step
}

// metric_scalars[q] = sum over envs of metric_env[q][env], q = blockIdx.x (read-time reduction)
__global__ void k_metric_reduce(View v)
{
    __shared__ long long part[256 / kWave];
    const int q = blockIdx.x;
    long long s = 0;
    for (int e = threadIdx.x; e < v.N; e += blockDim.x) s += v.metric_env[(size_t)q * v.N + e];
    s = wave_sum_i64(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int i = 0; i < 256 / kWave; ++i) t += part[i];
        v.metric_scalars[q] = t;
    }
}

// metric mode, EXPLICIT and IMPLICIT_GENERAL only (the IMPLICIT kernels add their exact integer cents in their output phase):
// keyword profit of the step just finished -> running sums in cents.  These models' money is floating-point dollars in the
// reference (cost_create draws a continuous cost), so the cent sums are a rounding of it by definition: each keyword-step
// contributes rint(revenue * 100) - rint(cost * 100), within half a cent of the float profit (and the float32 observation
// itself carries less than a cent only below 2^22 cents = $41,943 per keyword-day).
__global__ void k_metric_accumulate(View v)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nk = (size_t)v.N * v.K;
    if (i >= nk) return;
    const long long r = (long long)__builtin_rintf(v.rev[i] * 100.0f);
    const long long c = v.model == ADC_MODEL_IMPLICIT ? (long long)__builtin_rintf(v.cost[i] * 100.0f)
                                                      : (long long)__double2ll_rn((double)v.cost[i] * 100.0);
    metric_add(v, i, r - c);
}

// metric_profit[k] += sum over a slab of envs of the keyword sums (metric_total); grid = (K tiles, env slabs); metric_profit is
// zeroed before the launch
constexpr int kColumnSlabs = 64;
__global__ void k_metric_columns(View v)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= v.K) return;
    const int per = (v.N + kColumnSlabs - 1) / kColumnSlabs;
    const int e0 = blockIdx.y * per, e1 = min(v.N, e0 + per);
    long long s = 0;
    for (int e = e0; e < e1; ++e) s += metric_total(v, (size_t)e * v.K + k);
    if (e1 > e0) atomicAdd((unsigned long long *)&v.metric_profit[k], (unsigned long long)s);
}

// ---- ideal (max expected) profit of a keyword, adcraft/experiment_utils/experiment_metrics.py:20-61 ------------
// One wavefront per keyword.  n_samples competitor bids (cents) are histogrammed in LDS; for every bid b of the
// grid (any order, duplicates allowed):  idx = #(samples <= b)  (searchsorted side="right", :30),  IR = idx / n (:32),
// idx' = min(idx, n-1) (:33),  cpc = (sum of the idx'+1 smallest samples) / (idx'+1) (:34-35) - i.e. the mean
// of the samples <= b PLUS the next larger one (the reference's off-by-one, reproduced) - and
// profit(b) = max(vol_mean * IR * bctr * (sctr * rev_mean - cpc), 0) (:51-57); ideal = max_b (:59).
// Supported: bids up to kIdealMaxCents (a bid of 0 or less takes no sample: idx 0, cpc = the smallest sample), n_samples up to
// kIdealMaxSamples.  The host refuses anything else (implicit_curve_args): a grid with a higher or non-finite bid is never clamped.
constexpr int kIdealMaxCents = 2046;  // bins 0 .. lim <= 2047 kept one by one: at most 32 per lane (a lane's 32-bit occupancy mask, below)
constexpr int kIdealMaxSamples = 1 << 20;     // the 32-bit prefix sums: n * 2047 < 2^31; the packed numerator (+ one sample <= 1e9) < 2^32
constexpr int kIdealWaves = 4;        // keywords a workgroup has in flight (one wavefront each; fewer where four wavefronts' tables pass 64 KB)
#ifndef IDEAL_MIN_BLOCKS
#define IDEAL_MIN_BLOCKS 6
#endif
// the grid's highest bid in cents, as the kernel turns a bid into a bin, + 1: the bins kept one by one (host side: the launch's LDS);
// 0 if a bid is not finite or above kIdealMaxCents
inline int ideal_bins_kept(const double *bid_grid, int n_bids)
{
    int b_hi = 0;
    for (int bi = 0; bi < n_bids; ++bi) {
        const double x = std::floor(bid_grid[bi] * 100.0 + 0.5);
        if (!std::isfinite(x) || x > (double)kIdealMaxCents) return 0;
        const int bb = x > 0.0 ? (int)x : 0;
        b_hi = bb > b_hi ? bb : b_hi;
    }
    return b_hi + 1;                    // <= kIdealMaxCents + 1
}
// LDS words (4 bytes) of one wavefront's tables for `lim` bins kept: count prefix, cent prefix, next occupied bin (16-bit)
__host__ __device__ inline int ideal_wave_words(int lim) { return 2 * (lim + 1) + (lim + 4) / 2; }
// wavefronts per workgroup: four while their tables and the log table fit in 64 KB (lim <= 1609; the notebooks' grid: lim = 300), else three
inline int ideal_waves(int lim) { return std::min(kIdealWaves, (65536 / 4 - adc::kLogTableIntervals - 4) / ideal_wave_words(lim)); }
inline unsigned ideal_grid(long long n_items, int num_cus, int waves) { return (unsigned)std::max(1LL, std::min((n_items + 8 * waves - 1) / (8 * waves), (long long)num_cus * 32)); }
inline size_t ideal_lds_bytes(int lim, int waves) { return 4 * ((size_t)adc::kLogTableIntervals + 4 + (size_t)waves * ideal_wave_words(lim)); }

// A wavefront per keyword, ideal_waves(lim) of them per workgroup, each walking keywords blockIdx.x * chunk + wave, + the wave count
// stride, ... (round 4 launched one 64-lane workgroup per keyword with 11 KB of LDS: 14 wavefronts per CU, 16.7 million workgroups on
// cfg3, half of which found a keyword without volume and left).  A sample is only ever looked at as "count and sum of the samples
// <= b" and "the next larger one" for the bids b of the grid, so the bins 0 .. lim = (the grid's highest bid in cents) + 1 are kept
// one by one and everything above is one number, its minimum: ~3 KB of LDS per wavefront for the reference's grid of 299 bids.
// Nothing is shared between the wavefronts but the log table's nodes, copied once: no workgroup barrier inside the loop.
__global__ __launch_bounds__(kWave * kIdealWaves, IDEAL_MIN_BLOCKS) void k_ideal_profit(View v, int n_samples, int n_bids, const double *__restrict__ bid_grid,
                                                                     const int32_t *tape_samples, double *ideal_out, double *ir_out, double *cpc_out,
                                                                     uint2 *packed_out, int lim, long long n_items)
{
    extern __shared__ unsigned int ideal_lds[];
    float *const lognodes = reinterpret_cast<float *>(ideal_lds);          // copy of g_log_nodes (adc::LogNodes), [kLogTableIntervals + 1]
    const int lane = threadIdx.x & (kWave - 1), wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)(blockDim.x / kWave);
    unsigned int *const cpre = ideal_lds + adc::kLogTableIntervals + 4 + (size_t)wv * ideal_wave_words(lim);     // count per cent value, then the inclusive prefix of the counts
    unsigned int *const spre = cpre + (lim + 1);                           // inclusive prefix of cents (<= 2^20 * 2047 < 2^31: kIdealMaxSamples)
    unsigned short *const nxt = reinterpret_cast<unsigned short *>(spre + (lim + 1));      // [lim + 2] smallest occupied bin >= i (kNoBin: none - the next sample is over_min)
    constexpr unsigned int kNoBin = 0xFFFFu;
    for (int i = threadIdx.x; i <= adc::kLogTableIntervals; i += (int)blockDim.x) lognodes[i] = g_log_nodes[i];
    __syncthreads();
    // (a wavefront's tables are its own: between its phases it only has to see its own LDS writes)
    auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    const int per = (lim + kWave) / kWave;         // bins per lane: lane l owns bins [l per, l per + per) up to lim; per <= 32
  // (a workgroup takes a contiguous run of keywords - neighbours of one env, whatever pattern the keyword set has - its wavefronts every
  //  n_waves-th of them; the grid is a few thousand workgroups, ideal_grid)
  const long long chunk = (n_items + gridDim.x - 1) / gridDim.x;
  const long long item_end = min(n_items, ((long long)blockIdx.x + 1) * chunk);
  for (long long item = (long long)blockIdx.x * chunk + wv; item < item_end; item += n_waves) {
    const int env = (int)(item / v.K), k = (int)(item - (long long)env * v.K);
    if (!ir_out && !cpc_out && !packed_out) {
        // only the maximum is asked for: a keyword without volume or clicks (half of a sparse keyword set), or without a
        // positive margin, has profit(b) = max(vol_mean * IR * bctr * (margin - cpc), 0) = 0 for every b (cpc >= 0) - no sampling
        const float vm = param_at(v, ADC_P_VOL_MEAN, env, k), bc = param_at(v, ADC_P_BCTR, env, k);
        const double mg = (double)param_at(v, ADC_P_SCTR, env, k) * (double)param_at(v, ADC_P_REV_MEAN, env, k);
        if (vm == 0.0f || bc == 0.0f || (vm > 0.0f && bc > 0.0f && mg <= 0.0)) {      // (wave-uniform)
            if (lane == 0 && ideal_out) ideal_out[item] = 0.0;
            continue;
        }
    }
    unsigned int *const hist = cpre;               // (the prefix is taken in place, below)
    for (int i = lane; i <= lim; i += kWave) hist[i] = 0u;
    wave_sync();
    const float loc = param_at(v, ADC_P_A, env, k), scale = param_at(v, ADC_P_B, env, k);
    const uint64_t key = v.key[env];
    const uint32_t tick = v.tick[env];
    unsigned int my_over = 0xFFFFFFFFu;            // this lane's smallest sample above lim
    auto count = [&](int c) {
        if (c <= lim) atomicAdd(&hist[c], 1u);
        my_over = min(my_over, c > lim ? (unsigned int)c : 0xFFFFFFFFu);
    };
    if (tape_samples) {
        for (int i = lane; i < n_samples; i += kWave) count(tape_samples[(size_t)item * n_samples + i]);
    } else {
        // sample i is word i % 4 of call i / 4: a lane takes whole calls.  A sampled competitor bid is the auction law's own transform of
        // the word's top 24 bits (adc::competitor_cents_from_v: the monotone layout, the table log - stream revision 5; revisions up to
        // 4 evaluated the full Cephes logarithm per sample: 38 instructions against 22)
        const adc::LogNodes logtab{lognodes};
        for (int q = lane; 4 * q < n_samples; q += kWave) {
            const adc::U4 w = adc::draw(key, (uint32_t)q, adc::ST_METRIC, (uint32_t)k, tick);
            count(adc::competitor_cents_from_v(w.x >> 8, loc, scale, logtab));
            if (4 * q + 1 < n_samples) count(adc::competitor_cents_from_v(w.y >> 8, loc, scale, logtab));
            if (4 * q + 2 < n_samples) count(adc::competitor_cents_from_v(w.z >> 8, loc, scale, logtab));
            if (4 * q + 3 < n_samples) count(adc::competitor_cents_from_v(w.w >> 8, loc, scale, logtab));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) my_over = min(my_over, (unsigned int)__shfl_xor((int)my_over, o, 64));
    const unsigned int over_min = my_over;         // the smallest sample above the bins kept one by one (every lane holds it)
    wave_sync();
    // prefix sums over the bins kept: each lane owns `per` consecutive bins, a wave scan joins them
    unsigned int lc = 0, ls = 0, occupied = 0u, first = 0xFFFFFFFFu;
    for (int i = per - 1; i >= 0; --i) {
        const int bin = lane * per + i;
        const unsigned int h = bin <= lim ? hist[bin] : 0u;
        if (h != 0u) { occupied |= 1u << i; first = (unsigned int)bin; }
        lc += h;
        ls += h * (unsigned int)bin;
    }
    const unsigned int bc = (unsigned int)wave_scan_i32((int)lc) - lc, bs = (unsigned int)wave_scan_i32((int)ls) - ls;
    lc = bc; ls = bs;
    for (int i = 0; i < per; ++i) {
        const int bin = lane * per + i;
        if (bin <= lim) {
            const unsigned int h = hist[bin];       // (this lane's own bins: read before it overwrites them)
            lc += h;
            ls += h * (unsigned int)bin;
            cpre[bin] = lc;
            spre[bin] = ls;
        }
    }
    // smallest occupied bin at or after i: backward over the lane's bins, then across lanes (a suffix minimum by six shuffles)
    unsigned int suffix = first;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const unsigned int other = (unsigned int)__shfl_down((int)suffix, o, 64);
        if (lane + o < kWave) suffix = min(suffix, other);
    }
    unsigned int after = (unsigned int)__shfl_down((int)suffix, 1, 64);     // first occupied bin in any later lane
    if (lane == kWave - 1) after = 0xFFFFFFFFu;
    {
        unsigned int run = after;
        for (int i = per - 1; i >= 0; --i) {
            const int bin = lane * per + i;
            if ((occupied >> i) & 1u) run = (unsigned int)bin;
            if (bin <= lim) nxt[bin] = (unsigned short)(run == 0xFFFFFFFFu ? kNoBin : run);
        }
    }
    wave_sync();
    const double vol_mean = param_at(v, ADC_P_VOL_MEAN, env, k), bctr = param_at(v, ADC_P_BCTR, env, k);
    const double margin = (double)param_at(v, ADC_P_SCTR, env, k) * (double)param_at(v, ADC_P_REV_MEAN, env, k);
    const bool pow2 = (n_samples & (n_samples - 1)) == 0;
    const double inv_n = 1.0 / (double)n_samples;
    double best = 0.0;
    for (int bi = lane; bi < n_bids; bi += kWave) {
        // the reference compares float dollars: sample c/100.0 <= bid, with bid from np.arange (so e.g. its
        // "0.10" is 0.09999999999999999 and excludes 10-cent samples).  b = largest cent value that passes.
        const double bid = bid_grid[bi];
        // (a bid at or below -0.015 - or not finite - is bin -1: idx 0, and nxt[0] = the smallest sample, searchsorted's 0 and sorted[0];
        //  the host has refused bids above the bins kept, the upper clamp only keeps nxt[b + 1] inside this wave's table)
        double x = __builtin_floor(bid * 100.0 + 0.5);
        x = x > -1.0 ? x : -1.0;
        x = x < (double)(lim - 1) ? x : (double)(lim - 1);
        int b = (int)x;
        if (b >= 0 && !(adc::cents_to_dollars_f64(b) <= bid)) b -= 1;       // ((double)b / 100.0, the IEEE quotient, without the division sequence)
        const unsigned long long idx = b >= 0 ? cpre[b] : 0u;          // searchsorted side="right" (:30)
        const unsigned long long sum = b >= 0 ? spre[b] : 0u;
        // (:32; a power-of-two sample count - the reference's 2048 - divides exactly by a multiplication: same bits, no division sequence)
        const double ir = pow2 ? (double)idx * inv_n : (double)idx / (double)n_samples;
        // cpc = (numerator cents / 100) / denominator: numerator = the idx'+1 smallest samples, idx' = min(idx, n-1)
        unsigned long long numer_c;
        double den;
        const bool full = idx >= (unsigned long long)n_samples;
        if (full) { numer_c = sum; den = (double)n_samples; }                                  // idx' = n-1
        else {
            const unsigned int nb = nxt[b + 1];                         // sorted[idx]: the smallest sample above the bid (b + 1 <= lim)
            numer_c = sum + (nb != kNoBin ? nb : over_min);
            den = (double)(idx + 1);                                    // :33-35 inclusive running mean
        }
        // (cents / 100.0 without the division sequence where adc::cents_to_dollars_f64 is proven equal to the IEEE quotient)
        const double cpc = (numer_c < 0x80000000ull ? adc::cents_to_dollars_f64((int)numer_c) : (double)numer_c / 100.0) / den;
        // the curve point in 8 bytes: k_ideal_from_curves recomputes ir and cpc from it with the very same operations
        if (packed_out) packed_out[(size_t)item * n_bids + bi] = make_uint2((unsigned int)numer_c, (unsigned int)idx | (full ? 0x80000000u : 0u));
        if (ir_out) ir_out[(size_t)item * n_bids + bi] = ir;
        if (cpc_out) cpc_out[(size_t)item * n_bids + bi] = cpc;
        double p = vol_mean * ir * bctr * (margin - cpc);               // :51-57
        p = p > 0.0 ? p : 0.0;
        best = p > best ? p : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if (lane == 0 && ideal_out) ideal_out[item] = best;                 // :59
    wave_sync();                                   // (the next keyword's zeroing comes after this one's last read)
  }
}

// one wavefront busy for `ticks` of the 100 MHz wall clock (pick_group_streams: do two streams overlap?)
__global__ __launch_bounds__(kWave) void k_spin_ticks(long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

struct KeygenTables { adc::QuantileTable t[7]; };

__global__ void k_generate_keywords(View v, KeygenTables tabs, float no_vol_prob, uint32_t serial, const uint8_t *mask)
{
    const int env = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= v.K || (mask && !mask[env])) return;
    float out[8];
    adc::generate_implicit_keyword(v.key[env], (uint32_t)k, serial, tabs.t, no_vol_prob, out);
#pragma unroll
    for (int p = 0; p < ADC_P_COUNT; ++p) param_at(v, p, env, k) = out[p];
    if (k == 0) v.drift_pending[env] = 0;
}

// the EXPLICIT (default-constructor) keyword set of every (masked) env: sample_random_keywords' law, adc::generate_explicit_keyword
__global__ void k_generate_explicit_keywords(View v, uint32_t serial, const uint8_t *mask)
{
    const int env = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= v.K || (mask && !mask[env])) return;
    float out[8];
    adc::generate_explicit_keyword(v.key[env], (uint32_t)k, serial, out);
#pragma unroll
    for (int p = 0; p < ADC_P_COUNT; ++p) param_at(v, p, env, k) = out[p];
    if (k == 0) v.drift_pending[env] = 0;
}

// chain_subtract_wave as the device runs it, for tests: out[0] = (((r0 - x[0]) - x[1]) - ...) by the integer scans, out[1] = the same by the
// plain chain of rounded subtractions (one lane)
__global__ __launch_bounds__(kWave) void k_debug_chain(double r0, int n, const double *__restrict__ x, double *out)
{
    const int lane = threadIdx.x;
    double r = r0;
    for (int base = 0; base < n; base += kWave) r = chain_subtract_wave(r, base + lane < n ? x[base + lane] : 0.0);
    if (lane == 0) {
        double p = r0;
        for (int i = 0; i < n; ++i) p -= x[i];
        out[0] = r;
        out[1] = p;
    }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void k_reset(View v, const uint8_t *mask, const uint64_t *seeds)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= v.N) return;
    if (mask && !mask[env]) return;
    v.day[env] = 0;
    v.cum_cents[env] = 0;
    v.cum[env] = 0.0;
    if (seeds) {
        v.key[env] = splitmix64(seeds[env]);
        v.tick[env] = 0u;
        v.drift_pending[env] = 0;       // keywords are resampled with a seed (gymnasium_kw_env.py:303)
    }
}

// the observation of reset() is all zeros (gymnasium_kw_env.py:329-344)
__global__ void k_clear_obs(View v, const uint8_t *mask)
{
    const int env = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= v.K || (mask && !mask[env])) return;
    const size_t o = (size_t)env * v.K + k;
    v.imp[o] = 0; v.clk[o] = 0; v.conv[o] = 0;
    v.cost[o] = 0.0f; v.rev[o] = 0.0f;
}

__global__ void k_init_keys(View v, uint64_t seed, int64_t env_id_base)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= v.N) return;
    v.key[env] = splitmix64(seed ^ splitmix64((uint64_t)(env_id_base + env) + 0x5851F42D4C957F2Dull));
}

__global__ void k_sample_actions(View v, float lo, float hi, float budget, float *bids, float *budgets)
{
    const int env = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < v.K) {
        const adc::U4 w = adc::draw(v.key[env], 0u, adc::ST_ACTION, (uint32_t)k, v.tick[env]);
        bids[(size_t)env * v.K + k] = adc::synthetic_bid(w.x, lo, hi);
    }
    if (k == 0) budgets[env] = budget;
}

// flat observation row = sorted-key concatenation of the obs dict (adcraft/gymnasium_kw_utils.py:383-390,
// adcraft/wrappers/flat_array.py:74-80): buyside_clicks[K] | cost[K] | cumulative_profit | days_passed |
// impressions[K] | revenue[K] | sellside_conversions[K], all float32
__global__ void k_flatten_obs(View v)
{
    const int env = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int K = v.K;
    float *row = v.flat_obs + (size_t)env * (5 * K + 2);
    if (k < K) {
        const size_t o = (size_t)env * K + k;
        row[k] = (float)v.clk[o];
        row[K + k] = v.cost[o];
        row[2 * K + 2 + k] = (float)v.imp[o];
        row[3 * K + 2 + k] = v.rev[o];
        row[4 * K + 2 + k] = (float)v.conv[o];
    }
    if (k == 0) {
        row[2 * K] = (float)v.cum_profit[env];
        row[2 * K + 1] = (float)v.day_out[env];
    }
}

__global__ void k_unflatten_actions(View v, const float *flat, float *bids, float *budgets)
{
    // FlatArrayWrapper action = [budget, keyword_bids...] (sorted keys, adcraft/wrappers/flat_array.py:52,76)
    const int env = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const float *row = flat + (size_t)env * (v.K + 1);
    if (k < v.K) bids[(size_t)env * v.K + k] = row[1 + k];
    if (k == 0) budgets[env] = row[0];
}

// nth_price_auction (adcraft/synthetic_kw_helpers.py:116-180): one lane per auction, the top (w+n)
// competitor bids kept sorted ascending in registers.
constexpr int kTopMax = 32;
__global__ void k_nth_price(double bid, const double *__restrict__ other, int n_auctions, int n_bidders, int n,
                            int num_winners, int *__restrict__ won, int *__restrict__ placement, double *__restrict__ cost)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_auctions) return;
    const int top = num_winners + n;
    double best[kTopMax];                            // kept ascending; best[0] = smallest of the top
    int have = 0;
    const double *row = other + (size_t)a * n_bidders;
    const int pad = n_bidders < top ? top - n_bidders : 0;   // not enough bidders: zero bids (:156-161)
    for (int b = -pad; b < n_bidders; ++b) {
        const double x = b < 0 ? 0.0 : row[b];
        if (have < top) {
            int j = have++;
            best[j] = x;
            for (; j > 0 && best[j] < best[j - 1]; --j) { const double t = best[j]; best[j] = best[j - 1]; best[j - 1] = t; }
        } else if (x > best[0]) {
            int j = 0;
            best[0] = x;
            for (; j + 1 < top && best[j] > best[j + 1]; ++j) { const double t = best[j]; best[j] = best[j + 1]; best[j + 1] = t; }
        }
    }
    int index = 0;                                   // searchsorted(auction, bid) side="left" (:167)
    while (index < top && best[index] < bid) ++index;
    const bool w = index > n;                        // :170
    won[a] = w;
    if (w) {
        placement[a] = top - index;                  // :172
        int ci = index - (n - 1);
        if (ci < 0) ci = 0;
        cost[a] = n > 1 ? best[ci] : bid;            // :173-177
    }
}


// sum of one parameter plane into *out (double atomics; a scheduling hint, not a result)
__global__ void k_sum_plane(const float *__restrict__ plane, size_t n, double *out)
{
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc += (double)plane[i];
    // wave sum by shuffles is fine here (runs once per parameter upload)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

// the three count outputs as saturated uint16 [N][3][K] (adc_step_out.counts_u16; K even); *overflow = 1 if any was clipped
__global__ void k_pack_counts(View v, unsigned short *out, int *overflow)
{
    const int half_k = v.K >> 1;
    const size_t pair = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= (size_t)v.N * half_k) return;
    const size_t env = pair / half_k;
    const int k = (int)(pair - env * half_k) * 2;
    const int32_t *src[3] = {v.imp, v.clk, v.conv};
    bool clipped = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int2 x = *reinterpret_cast<const int2 *>(src[a] + env * v.K + k);
        clipped |= x.x > 65535 || x.y > 65535;
        *reinterpret_cast<unsigned int *>(out + (env * 3 + a) * v.K + k) = (unsigned int)min(x.x, 65535) | ((unsigned int)min(x.y, 65535) << 16);
    }
    if (clipped) *overflow = 1;
}

// ---- step outputs written straight into page-locked host memory (one launch instead of up to eleven transfers)
// A host step of 4096 x 256 is bound by the 20 B per keyword that go back over PCIe.  Split over a few engines, each part's
// outputs are rows of the caller's [N, K] arrays - five strided pieces per part for a DMA engine, but one coalesced pass
// for a kernel: every lane moves 16 B per array (or packs the three counts to 3 x 8 B), a wavefront writes 1 KB runs.
struct HostOut {
    int32_t *imp, *clk, *conv;          // [n][K] each, or all null when counts_u16 is given
    unsigned short *counts_u16;         // [n][3][K] or null
    float *cost, *rev;                  // [n][K]
    double *reward, *cum;               // [n]
    int32_t *days;
    unsigned char *term, *trunc;
    int32_t *overflow;                  // nullable
};

__global__ void __launch_bounds__(256) k_outputs_to_host(View v, HostOut h)
{
    const int quads_per_row = v.K >> 2;                         // K % 4 == 0 (checked by the host)
    const size_t quads = (size_t)v.N * quads_per_row;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
        const size_t i = q * 4;
        const int4 imp = *reinterpret_cast<const int4 *>(v.imp + i), clk = *reinterpret_cast<const int4 *>(v.clk + i),
                   conv = *reinterpret_cast<const int4 *>(v.conv + i);
        if (h.counts_u16) {
            const size_t env = q / quads_per_row;
            const int k = (int)(q - env * quads_per_row) * 4;
            const int4 *src[3] = {&imp, &clk, &conv};
            bool clipped = false;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int4 x = *src[a];
                clipped |= (x.x | x.y | x.z | x.w) > 65535;       // counts are non-negative
                uint2 pk;
                pk.x = (unsigned int)min(x.x, 65535) | ((unsigned int)min(x.y, 65535) << 16);
                pk.y = (unsigned int)min(x.z, 65535) | ((unsigned int)min(x.w, 65535) << 16);
                *reinterpret_cast<uint2 *>(h.counts_u16 + (env * 3 + a) * v.K + k) = pk;
            }
            if (clipped && h.overflow) *h.overflow = 1;
        } else {
            if (h.imp) *reinterpret_cast<int4 *>(h.imp + i) = imp;
            if (h.clk) *reinterpret_cast<int4 *>(h.clk + i) = clk;
            if (h.conv) *reinterpret_cast<int4 *>(h.conv + i) = conv;
        }
        if (h.cost) *reinterpret_cast<float4 *>(h.cost + i) = *reinterpret_cast<const float4 *>(v.cost + i);
        if (h.rev) *reinterpret_cast<float4 *>(h.rev + i) = *reinterpret_cast<const float4 *>(v.rev + i);
    }
    if (blockIdx.x == 0)
        for (int env = threadIdx.x; env < v.N; env += blockDim.x) {
            if (h.reward) h.reward[env] = v.reward[env];
            if (h.cum) h.cum[env] = v.cum_profit[env];
            if (h.days) h.days[env] = v.day_out[env];
            if (h.term) h.term[env] = v.term[env];
            if (h.trunc) h.trunc[env] = v.trunc[env];
        }
}
