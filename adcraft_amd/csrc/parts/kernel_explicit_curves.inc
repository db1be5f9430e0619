// kernel_explicit_curves.inc - bid curves and ideal profit of EXPLICIT keywords (get_explicit_kw_bid_cpc_impressions,
// adcraft/experiment_utils/experiment_metrics.py:10-17, and get_max_expected_bid_profits, :40-61).  (part of adc_engine.hip)
//
// The reference's curve point at bid b: ir(b) = impression_rate(b) (threshold_sigmoid), cpc(b) = np.median(cost_create(b, n)).
// The engine draws the n standard normals of a keyword ONCE per build, from the stream the IMPLICIT estimator uses (sample i =
// word i % 4 of draw(key, i / 4, ST_METRIC, k, tick), through adc::normal_from_word, the EXPLICIT step's normal), and keeps
// their two middle order statistics: for a fixed b the cost is non-decreasing in z, so the median of the n costs is exactly
// the mean of the costs of z_((n-1)/2) and z_(n/2) (adc_law.h explicit_curve_point).  Each bid's cpc thus has the reference's
// distribution; unlike the reference, the bids of the grid share one set of draws (their medians are comonotone).  Fresh
// draws per bid would be n_bids x n normals per keyword (~6e11 at 4096 envs x 256 keywords).
//
// A wavefront per keyword, kIdealWaves of them per workgroup, the keywords dealt as k_ideal_profit deals them.  The two order
// statistics by a radix select on float_order_key(z): four passes of 8 bits, each a 256-bin LDS histogram per rank (one while
// both ranks share their prefix), the bin that holds the rank found by a wave scan.  Up to kCachedSamples samples the keys
// stay in registers (32 per lane); beyond, every pass redraws them from their counters (n <= 2^20).
// Outputs, by the pointers given: ideal_out = the ideal profit (keywords without volume, clicks or margin skip the grid:
// 0, as for IMPLICIT); curve_out = {z_lo, z_hi, impression intercept, impression slope}, the cached curve (16 bytes per keyword).
// Every later reader evaluates a point through ExplicitCurve::at (kernels_policy.inc), i.e. the same adc::explicit_curve_point.
constexpr int kCachedSamples = 32 * kWave;
constexpr int kSelectBins = 256;

template <bool kCached>
__global__ __launch_bounds__(kWave * kIdealWaves) void k_explicit_curves(View v, int n_samples, int n_bids, const double *__restrict__ bid_grid,
                                                                         const double *__restrict__ grid_mu, const double *__restrict__ grid_sigma,
                                                                         double *ideal_out, float4 *curve_out, long long n_items)
{
    __shared__ __align__(16) unsigned int hist_lds[kIdealWaves][2][kSelectBins];
    const int lane = threadIdx.x & (kWave - 1), wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned int *const h0 = hist_lds[wv][0], *const h1 = hist_lds[wv][1];
    auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    const int r_lo = (n_samples - 1) / 2, r_hi = n_samples / 2;        // 0-based ranks of the middle pair (one rank if n is odd)
    const long long chunk = (n_items + gridDim.x - 1) / gridDim.x;
    const long long item_end = min(n_items, ((long long)blockIdx.x + 1) * chunk);
    for (long long item = (long long)blockIdx.x * chunk + wv; item < item_end; item += kIdealWaves) {
        const int env = (int)(item / v.K), k = (int)(item - (long long)env * v.K);
        const float vm = param_at(v, ADC_P_VOL_MEAN, env, k), bcf = param_at(v, ADC_P_BCTR, env, k);
        const double mg = (double)param_at(v, ADC_P_SCTR, env, k) * (double)param_at(v, ADC_P_REV_MEAN, env, k);
        if (!curve_out && (vm == 0.0f || bcf == 0.0f || (vm > 0.0f && bcf > 0.0f && mg <= 0.0))) {     // (wave-uniform) profit 0 everywhere
            if (lane == 0 && ideal_out) ideal_out[item] = 0.0;
            continue;
        }
        const float a = param_at(v, ADC_P_A, env, k), b = param_at(v, ADC_P_B, env, k);
        const uint64_t key = v.key[env];
        const uint32_t tick = v.tick[env];
        // the keys of this lane's samples: call q = lane + 64 t holds samples 4 q .. 4 q + 3 (0xFFFFFFFF: none - never a normal's key)
        uint32_t keys[kCached ? 32 : 1];
        if constexpr (kCached) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int q = lane + kWave * t;
                adc::U4 w{0u, 0u, 0u, 0u};
                if (4 * q < n_samples) w = adc::draw(key, (uint32_t)q, adc::ST_METRIC, (uint32_t)k, tick);
                keys[4 * t + 0] = 4 * q + 0 < n_samples ? adc::float_order_key(adc::normal_from_word(w.x)) : 0xFFFFFFFFu;
                keys[4 * t + 1] = 4 * q + 1 < n_samples ? adc::float_order_key(adc::normal_from_word(w.y)) : 0xFFFFFFFFu;
                keys[4 * t + 2] = 4 * q + 2 < n_samples ? adc::float_order_key(adc::normal_from_word(w.z)) : 0xFFFFFFFFu;
                keys[4 * t + 3] = 4 * q + 3 < n_samples ? adc::float_order_key(adc::normal_from_word(w.w)) : 0xFFFFFFFFu;
            }
        }
        auto for_each_key = [&](auto &&f) {
            if constexpr (kCached) {
#pragma unroll
                for (int i = 0; i < 32; ++i) if (keys[i] != 0xFFFFFFFFu) f(keys[i]);
            } else {
                for (int q = lane; 4 * q < n_samples; q += kWave) {
                    const adc::U4 w = adc::draw(key, (uint32_t)q, adc::ST_METRIC, (uint32_t)k, tick);
                    f(adc::float_order_key(adc::normal_from_word(w.x)));
                    if (4 * q + 1 < n_samples) f(adc::float_order_key(adc::normal_from_word(w.y)));
                    if (4 * q + 2 < n_samples) f(adc::float_order_key(adc::normal_from_word(w.z)));
                    if (4 * q + 3 < n_samples) f(adc::float_order_key(adc::normal_from_word(w.w)));
                }
            }
        };
        // the bin of `hist` that holds rank `rank` of the counted keys: lane l owns bins 4l .. 4l + 3; returns the bin, `rank` becomes the
        // rank within it
        auto find_bin = [&](const unsigned int *hist, int &rank) -> unsigned int {
            const uint4 hb = reinterpret_cast<const uint4 *>(hist)[lane];
            const int s = (int)(hb.x + hb.y + hb.z + hb.w);
            const int incl = wave_scan_i32(s), excl = incl - s;
            const bool mine = excl <= rank && rank < incl;
            unsigned int bin = 0u;
            int below = excl;
            if (mine) {
                const int r = rank - excl;
                if (r < (int)hb.x) bin = 0u;
                else if (r < (int)(hb.x + hb.y)) { bin = 1u; below += (int)hb.x; }
                else if (r < (int)(hb.x + hb.y + hb.z)) { bin = 2u; below += (int)(hb.x + hb.y); }
                else { bin = 3u; below += (int)(hb.x + hb.y + hb.z); }
                bin += 4u * (unsigned int)lane;
            }
            const int src = (int)__builtin_ctzll(__ballot(mine));
            rank -= __shfl(below, src, kWave);
            return (unsigned int)__shfl((int)bin, src, kWave);
        };
        uint32_t pre_lo = 0u, pre_hi = 0u;
        int rk_lo = r_lo, rk_hi = r_hi;
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t hmask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
            const bool same = pre_lo == pre_hi;                        // (wave-uniform: both ranks still in one bin)
            reinterpret_cast<uint4 *>(h0)[lane] = make_uint4(0u, 0u, 0u, 0u);
            reinterpret_cast<uint4 *>(h1)[lane] = make_uint4(0u, 0u, 0u, 0u);
            wave_sync();
            for_each_key([&](uint32_t x) {
                const uint32_t top = x & hmask, d = (x >> shift) & (kSelectBins - 1);
                if (top == pre_lo) atomicAdd(&h0[d], 1u);
                if (!same && top == pre_hi) atomicAdd(&h1[d], 1u);
            });
            wave_sync();
            pre_lo |= find_bin(h0, rk_lo) << shift;
            pre_hi |= find_bin(same ? h0 : h1, rk_hi) << shift;
            wave_sync();                                               // (the next pass clears the bins after every lane read them)
        }
        const float z_lo = adc::float_from_order_key(pre_lo), z_hi = adc::float_from_order_key(pre_hi);
        if (curve_out && lane == 0) curve_out[item] = make_float4(z_lo, z_hi, a, b);
        if (ideal_out) {
            const double vol_mean = vm, bctr = bcf;
            const ExplicitCurve cv{v.imp_thresh, a, b, z_lo, z_hi, bid_grid, grid_mu, grid_sigma};
            double best = 0.0;
            for (int bi = lane; bi < n_bids; bi += kWave) {
                const CurveLine l = cv.at(bi);
                double pr = vol_mean * l.s * bctr * (mg - l.c);            // the operation order of k_ideal_from_curves / the reference
                pr = pr > 0.0 ? pr : 0.0;
                best = pr > best ? pr : best;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double other = __shfl_xor(best, o, 64);
                best = other > best ? other : best;
            }
            if (lane == 0) ideal_out[item] = best;
        }
    }
}

// the points of the cached EXPLICIT curves, [N*K][n_bids] (adc_engine_bid_curves_fetch): the doubles every ideal kernel evaluates
__global__ __launch_bounds__(256) void k_explicit_curve_points(View v, PolicyView p, double *__restrict__ ir_out, double *__restrict__ cpc_out)
{
    const size_t n = (size_t)v.N * v.K * p.n_bids;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t o = i / (size_t)p.n_bids;
        const int bi = (int)(i - o * (size_t)p.n_bids);
        const CurveLine l = explicit_curve(v, p, o).at(bi);
        ir_out[i] = l.s;
        cpc_out[i] = l.c;
    }
}
