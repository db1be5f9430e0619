// selftest_api.inc - the device self-tests (include/adcraft_engine.h): entry points that take a device id and no engine, run one
// small kernel on the null stream over blocking copies and hand its result back - the curve estimator, the win brackets, Philox,
// the float chain, nth_price_auction - and the debug readers of an engine's counters.  After parts/curves_api.inc, whose estimator
// checks and launch the first of them shares.
// (part of the single translation unit adc_engine.hip)

// the estimator alone, on caller-supplied samples (cents, >= 0) of ONE keyword and any bid grid the estimator takes (pins the kernel
// against the reference's get_implicit_kw_bid_cpc_impressions).  Arguments are checked before any HIP call
ADC_EXPORT int adc_bid_curves_from_samples(int device_id, const int32_t *samples_cents, int32_t n_samples, const double *bid_grid,
                                           int32_t n_bids, double *impression_rate_out, double *cpc_out)
{
    if (!samples_cents || n_samples <= 0 || n_bids <= 0 || !bid_grid || !impression_rate_out || !cpc_out)
        return fail(ADC_EINVAL, "bad arguments");
    int lim = 0;
    if (int rc = implicit_curve_args(n_samples, bid_grid, n_bids, &lim)) return rc;
    for (int32_t i = 0; i < n_samples; ++i)
        if (samples_cents[i] < 0) return fail(ADC_EINVAL, "a negative sample (cents)");
    HIP_TRY(hipSetDevice(device_id));
    int32_t *d_s = nullptr;
    double *d_ir = nullptr, *d_cpc = nullptr, *d_grid = nullptr;
    float *d_p = nullptr;
    uint64_t *d_key = nullptr;
    uint32_t *d_tick = nullptr;
    DevTemps tmp(nullptr);              // (the null stream, as the copies and the launch below)
    if (tmp.get(&d_s, (size_t)n_samples * 4) != hipSuccess || tmp.get(&d_ir, (size_t)n_bids * 8) != hipSuccess ||
        tmp.get(&d_cpc, (size_t)n_bids * 8) != hipSuccess || tmp.get(&d_p, ADC_P_COUNT * 4) != hipSuccess ||
        tmp.get(&d_key, 8) != hipSuccess || tmp.get(&d_tick, 4) != hipSuccess || tmp.get(&d_grid, (size_t)n_bids * 8) != hipSuccess)
        return fail(ADC_ENOMEM, "hipMalloc failed");
    if (hipMemcpy(d_grid, bid_grid, (size_t)n_bids * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(ADC_EHIP, "upload failed");
    if (hipMemcpy(d_s, samples_cents, (size_t)n_samples * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_p, 0, ADC_P_COUNT * 4) != hipSuccess ||
        hipMemset(d_key, 0, 8) != hipSuccess || hipMemset(d_tick, 0, 4) != hipSuccess)
        return fail(ADC_EHIP, "upload failed");
    View v;
    std::memset(&v, 0, sizeof(v));
    v.N = 1; v.K = 1; v.params = d_p; v.key = d_key; v.tick = d_tick;
    v.NP = 1;
    launch_ideal_profit(v, 0, 1, n_samples, n_bids, d_grid, d_s, (double *)nullptr, d_ir, d_cpc, (uint2 *)nullptr, lim, 1LL);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(ADC_EHIP, "k_ideal_profit failed");
    if (hipMemcpy(impression_rate_out, d_ir, (size_t)n_bids * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cpc_out, d_cpc, (size_t)n_bids * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(ADC_EHIP, "download failed");
    tmp.release();
    return ADC_OK;
}

// adc_law.h win_brackets evaluated by the device (k_debug_win_brackets), 8 words per keyword: tests check them against the
// exact intervals on the host (adc_check_win_brackets)
ADC_EXPORT int adc_debug_win_brackets_device(int device_id, int64_t n, const float *bid, const float *cost_loc, const float *cost_scale,
                                             const float *buyside_ctr, uint32_t *out8)
{
    if (n < 0 || n > (1 << 26)) return fail(ADC_EINVAL, "n out of range");
    if (n == 0) return ADC_OK;
    if (!bid || !cost_loc || !cost_scale || !buyside_ctr || !out8) return fail(ADC_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(device_id));
    float *d_in = nullptr;
    uint32_t *d_out = nullptr;
    DevTemps tmp(nullptr);
    const size_t m = (size_t)n;
    if (tmp.get(&d_in, 4 * m * 4) != hipSuccess || tmp.get(&d_out, 8 * m * 4) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
    const float *src[4] = {bid, cost_loc, cost_scale, buyside_ctr};
    for (int i = 0; i < 4; ++i)
        if (hipMemcpy(d_in + i * m, src[i], m * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(ADC_EHIP, "upload failed");
    hipLaunchKernelGGL(k_debug_win_brackets, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, (int)n, d_in, d_in + m, d_in + 2 * m, d_in + 3 * m, d_out);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(ADC_EHIP, "k_debug_win_brackets failed");
    if (hipMemcpy(out8, d_out, 8 * m * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ADC_EHIP, "download failed");
    tmp.release();
    return ADC_OK;
}

ADC_EXPORT int adc_debug_walk_stats(adc_engine *e, int64_t stats[4], int reset)
{
    ENGINE_GUARD(e);
    if (!stats) return fail(ADC_EINVAL, "stats is NULL");
    HIP_TRY(hipStreamSynchronize(e->stream));
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_walk_stats), sizeof(h)));
    for (int i = 0; i < 4; ++i) stats[i] = (int64_t)h[i];
#ifdef ADC_EXP_TIMING
    {   // timing build: the phase sums go to stderr (setup | sort | walk | commit | gather | second part | groups | candidates)
        unsigned long long ph[20];
        HIP_TRY(hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_walk_phase), 8 * sizeof(ph[0])));
        std::fprintf(stderr, "walk phases:");
        for (int i = 0; i < 8; ++i) std::fprintf(stderr, " %llu", ph[i]);
        std::fprintf(stderr, "\n");
        HIP_TRY(hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_rest_phase), sizeof(ph)));
        std::fprintf(stderr, "rest-of-day phases (10 ns ticks: pass over the auctions | of which laws | marked cells | outputs | envs | cells walked | of which paid / marks | - | "
                             "list of the marks | k_rest_walk: before the walk | chunks resolved | whole env | slowest env | chunk: cells | chain | paid | at-once variant: own cells | chain | commit | envs):");
        for (int i = 0; i < 20; ++i) std::fprintf(stderr, " %llu", ph[i]);
        std::fprintf(stderr, "\n");
        if (reset) {
            const unsigned long long z8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_walk_phase), z8, sizeof(z8)));
            const unsigned long long z16[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_rest_phase), z16, sizeof(z16)));
        }
    }
#endif
    if (reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_walk_stats), z, sizeof(z)));
    }
    return ADC_OK;
}

ADC_EXPORT int adc_debug_direct_days(adc_engine *e, int64_t *env_days, int reset)
{
    ENGINE_GUARD(e);
    if (!env_days) return fail(ADC_EINVAL, "env_days is NULL");
    HIP_TRY(hipStreamSynchronize(e->stream));
    unsigned long long h = 0;
    if (e->v.direct_days) {             // (null: this engine never parks an env at once - K > 256, fewer than 1024 envs, another model)
        HIP_TRY(hipMemcpy(&h, e->v.direct_days, sizeof(h), hipMemcpyDeviceToHost));
        if (reset) HIP_TRY(hipMemset(e->v.direct_days, 0, sizeof(h)));
    }
    *env_days = (int64_t)h;
    return ADC_OK;
}

// Philox4x32 (the stream's round count) evaluated by the device for n (counter, key) pairs - the GPU side of the stream battery
ADC_EXPORT int adc_debug_philox_device(int device_id, int64_t n, const uint32_t *ctr4, const uint32_t *key2, uint32_t *out4)
{
    if (n < 0 || n > (1 << 26)) return fail(ADC_EINVAL, "n out of range");
    if (n == 0) return ADC_OK;
    if (!ctr4 || !key2 || !out4) return fail(ADC_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(device_id));
    uint32_t *d = nullptr;
    const size_t m = (size_t)n;
    DevTemps tmp(nullptr);
    if (tmp.get(&d, 10 * m * 4) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
    if (hipMemcpy(d, ctr4, 4 * m * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + 4 * m, key2, 2 * m * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(ADC_EHIP, "upload failed");
    hipLaunchKernelGGL(k_debug_philox, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, (int)n, d, d + 4 * m, d + 6 * m);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(ADC_EHIP, "k_debug_philox failed");
    if (hipMemcpy(out4, d + 6 * m, 4 * m * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ADC_EHIP, "download failed");
    tmp.release();
    return ADC_OK;
}

ADC_EXPORT int adc_debug_chain_device(int device_id, double r0, int64_t n, const double *x, double *out2)
{
    if (n < 0 || n > (1 << 24)) return fail(ADC_EINVAL, "n out of range");
    if ((n > 0 && !x) || !out2) return fail(ADC_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(device_id));
    double *d = nullptr;
    DevTemps tmp(nullptr);
    if (tmp.get(&d, ((size_t)n + 2) * 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
    if (n > 0 && hipMemcpy(d + 2, x, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(ADC_EHIP, "upload failed");
    hipLaunchKernelGGL(k_debug_chain, dim3(1), dim3(kWave), 0, 0, r0, (int)n, d + 2, d);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(ADC_EHIP, "k_debug_chain failed");
    if (hipMemcpy(out2, d, 16, hipMemcpyDeviceToHost) != hipSuccess) return fail(ADC_EHIP, "download failed");
    tmp.release();
    return ADC_OK;
}

ADC_EXPORT int adc_nth_price_auction(int device_id, double bid, const double *other_bids, int32_t n_auctions, int32_t n_bidders,
                                     int32_t n, int32_t num_winners, int32_t *impressions, int32_t *placements, double *costs)
{
    if (!impressions) return fail(ADC_EINVAL, "impressions is NULL");
    *impressions = 0;
    if (n < 1 || num_winners < 1 || n + num_winners > kTopMax) return fail(ADC_EINVAL, "need n >= 1, num_winners >= 1, n + num_winners <= 32");
    if (n_auctions < 0 || n_bidders < 0) return fail(ADC_EINVAL, "negative shape");
    if (n_auctions == 0) return ADC_OK;
    if (n_bidders > 0 && !other_bids) return fail(ADC_EINVAL, "other_bids is NULL");
    HIP_TRY(hipSetDevice(device_id));
    double *d_other = nullptr, *d_cost = nullptr;
    int *d_won = nullptr, *d_place = nullptr;
    const size_t na = n_auctions, nb = n_bidders;
    DevTemps tmp(nullptr);
    if (tmp.get(&d_other, (na * nb ? na * nb : 1) * 8) != hipSuccess || tmp.get(&d_cost, na * 8) != hipSuccess ||
        tmp.get(&d_won, na * 4) != hipSuccess || tmp.get(&d_place, na * 4) != hipSuccess)
        return fail(ADC_ENOMEM, "hipMalloc failed");
    if (na * nb && hipMemcpy(d_other, other_bids, na * nb * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(ADC_EHIP, "upload failed");
    hipLaunchKernelGGL(k_nth_price, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, 0, bid, d_other, n_auctions, n_bidders, n, num_winners, d_won, d_place, d_cost);
    if (hipGetLastError() != hipSuccess) return fail(ADC_EHIP, "k_nth_price launch failed");
    std::vector<int> won(na), place(na);
    std::vector<double> cost(na);
    if (hipMemcpy(won.data(), d_won, na * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(place.data(), d_place, na * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(cost.data(), d_cost, na * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(ADC_EHIP, "download failed");
    int32_t m = 0;
    for (size_t a = 0; a < na; ++a)
        if (won[a]) {
            if (placements) placements[m] = place[a];
            if (costs) costs[m] = cost[a];
            ++m;
        }
    *impressions = m;
    tmp.release();                      // (the blocking downloads have waited for the kernel)
    return ADC_OK;
}

#ifdef ADC_EXP_TIMING
extern "C" __attribute__((visibility("default"))) int adc_debug_read(unsigned long long *out, int reset)
{
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg), sizeof(unsigned long long) * 16);
    // slots 8..15: k_step_implicit_fast (wave 0 of every workgroup), summed over the 256 rows of g_fdbg
    static unsigned long long rows[256][8];
    hipMemcpyFromSymbol(rows, HIP_SYMBOL(g_fdbg), sizeof(rows));
    for (int i = 0; i < 8; ++i) { out[8 + i] = 0; for (int r = 0; r < 256; ++r) out[8 + i] += rows[r][i]; }
    if (reset) {
        unsigned long long z[16] = {0};
        hipMemcpyToSymbol(HIP_SYMBOL(g_dbg), z, sizeof(z));
        std::memset(rows, 0, sizeof(rows));
        hipMemcpyToSymbol(HIP_SYMBOL(g_fdbg), rows, sizeof(rows));
    }
    return 0;
}

// k_step_implicit_fast, all waves since the last reset: out2 = {Philox calls issued in phase 2 (wave-call-slots), calls that hold at
// least one auction (lane-calls: 64 of them fill a slot)}
extern "C" __attribute__((visibility("default"))) int adc_debug_read_fast_slots(unsigned long long *out2, int reset)
{
    hipDeviceSynchronize();
    static unsigned long long rows[256][2];
    hipMemcpyFromSymbol(rows, HIP_SYMBOL(g_fslots), sizeof(rows));
    out2[0] = out2[1] = 0;
    for (int r = 0; r < 256; ++r) { out2[0] += rows[r][0]; out2[1] += rows[r][1]; }
    if (reset) {
        std::memset(rows, 0, sizeof(rows));
        hipMemcpyToSymbol(HIP_SYMBOL(g_fslots), rows, sizeof(rows));
    }
    return 0;
}
#endif
