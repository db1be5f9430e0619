// curves_api.inc - the extern "C" entry points of the episode metrics, the ideal profit and the bid curves (include/adcraft_engine.h;
// the kernels are parts/kernels_misc.inc, parts/kernels_policy.inc and parts/kernel_explicit_curves.inc), over parts/host_api.inc: the
// metric sums and their readers, the ideal profit on fresh samples, the cached curves with their contender lists, the per-step ideal
// and the oracle bidder on them (device-resident, chain-compatible), per-env AKNCP / NCP.
// (part of the single translation unit adc_engine.hip)

ADC_EXPORT int adc_engine_metrics_enable(adc_engine *e, int enabled)
{
    ENGINE_GUARD(e);
    e->v.metrics_on = enabled ? 1 : 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_metrics_reset(adc_engine *e)
{
    ENGINE_GUARD(e);
    HIP_TRY(hipMemsetAsync(e->v.metric_profit, 0, (size_t)e->v.K * 8, e->stream));
    HIP_TRY(hipMemsetAsync(e->v.metric_scalars, 0, 64, e->stream));
    HIP_TRY(hipMemsetAsync(e->v.metric_env, 0, (size_t)e->v.N * 32, e->stream));
    HIP_TRY(hipMemsetAsync(e->v.metric_lo, 0, (size_t)e->v.N * e->v.K * 4, e->stream));
    HIP_TRY(hipMemsetAsync(e->v.metric_hi, 0, (size_t)e->v.N * e->v.K * 8, e->stream));
    if (e->have_ideal) {
        HIP_TRY(hipMemsetAsync(e->pol.sum_ideal, 0, (size_t)e->v.N * e->v.K * 8, e->stream));
        HIP_TRY(hipMemsetAsync(e->pol.sum_ideal_pos, 0, (size_t)e->v.N * e->v.K * 8, e->stream));
    }
    return ADC_OK;
}

ADC_EXPORT int adc_engine_metrics_read(adc_engine *e, int64_t *keyword_profit_cents_k, int64_t *scalars8)
{
    ENGINE_GUARD(e);
    if (keyword_profit_cents_k) {
        HIP_TRY(hipMemsetAsync(e->v.metric_profit, 0, (size_t)e->v.K * 8, e->stream));
        hipLaunchKernelGGL(k_metric_columns, dim3((unsigned)((e->v.K + 255) / 256), kColumnSlabs), dim3(256), 0, e->stream, e->v);
        HIP_TRY(hipGetLastError());
    }
    if (keyword_profit_cents_k) HIP_TRY(hipMemcpyAsync(keyword_profit_cents_k, e->v.metric_profit, (size_t)e->v.K * 8, hipMemcpyDeviceToHost, e->stream));
    if (scalars8) {
        hipLaunchKernelGGL(k_metric_reduce, dim3(4), dim3(256), 0, e->stream, e->v);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(scalars8, e->v.metric_scalars, 64, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

namespace {
// the bid curves exist for the two single-competitor models; the reference's estimator on the default ImplicitKeyword's bidder pool
// sorts s x n bids and divides by n (an impression rate above 1), and no notebook uses it that way
int curves_model_check(const adc_engine *e, const char *what)
{
    if (e->v.model == ADC_MODEL_IMPLICIT || e->v.model == ADC_MODEL_EXPLICIT) return ADC_OK;
    return fail(ADC_EINVAL, std::string(what) + " is defined for IMPLICIT and EXPLICIT keywords (IMPLICIT_GENERAL: the reference's estimator "
                                                "on a bidder pool gives impression rates above 1)");
}
// EXPLICIT: the grid and its cost law, [3][n_bids] = bid, mu_b, sigma_b (adc::explicit_cost_law, float64 on the host)
std::vector<double> explicit_grid3(const double *bid_grid, int n_bids)
{
    std::vector<double> g(3 * (size_t)n_bids);
    for (int i = 0; i < n_bids; ++i) {
        g[i] = bid_grid[i];
        adc::explicit_cost_law(bid_grid[i], g[n_bids + i], g[2 * (size_t)n_bids + i]);
    }
    return g;
}
void launch_explicit_curves(const adc_engine *e, int n_samples, const double *d_grid3, int n_bids, double *ideal_out, float4 *curve_out)
{
    const size_t nk = (size_t)e->v.N * e->v.K;
    const dim3 grid(ideal_grid((long long)nk, e->num_cus, kIdealWaves)), block(kWave * kIdealWaves);
    if (n_samples <= kCachedSamples)
        hipLaunchKernelGGL(k_explicit_curves<true>, grid, block, 0, e->stream, e->v, n_samples, n_bids, d_grid3, d_grid3 + n_bids,
                           d_grid3 + 2 * (size_t)n_bids, ideal_out, curve_out, (long long)nk);
    else
        hipLaunchKernelGGL(k_explicit_curves<false>, grid, block, 0, e->stream, e->v, n_samples, n_bids, d_grid3, d_grid3 + n_bids,
                           d_grid3 + 2 * (size_t)n_bids, ideal_out, curve_out, (long long)nk);
}
// the per-step ideal on the cached curves: contender lists or (ADCRAFT_IDEAL_FULL_SCAN) the whole grid, for the engine's model
void launch_ideal_step(const View &v, const PolicyView &p, hipStream_t st, bool full_scan)
{
    const size_t nk = (size_t)v.N * v.K;
    if (v.model == ADC_MODEL_EXPLICIT) {
        if (full_scan) hipLaunchKernelGGL(k_ideal_from_curves<ADC_MODEL_EXPLICIT>, dim3((unsigned)((nk + 3) / 4)), dim3(256), 0, st, v, p, v.metrics_on);
        else hipLaunchKernelGGL(k_ideal_from_contenders<ADC_MODEL_EXPLICIT>, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, v, p, v.metrics_on);
    } else {
        if (full_scan) hipLaunchKernelGGL(k_ideal_from_curves<ADC_MODEL_IMPLICIT>, dim3((unsigned)((nk + 3) / 4)), dim3(256), 0, st, v, p, v.metrics_on);
        else hipLaunchKernelGGL(k_ideal_from_contenders<ADC_MODEL_IMPLICIT>, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, v, p, v.metrics_on);
    }
}
// the IMPLICIT estimator's limits (k_ideal_profit): 0, or ADC_EINVAL naming the one passed; *lim = the bins the grid keeps
int implicit_curve_args(int n_samples, const double *bid_grid, int n_bids, int *lim)
{
    if (n_samples > kIdealMaxSamples) return fail(ADC_EINVAL, "n_samples > 2^20 is not supported for IMPLICIT keywords (the estimator's 32-bit sums)");
    *lim = ideal_bins_kept(bid_grid, n_bids);
    if (*lim == 0) return fail(ADC_EINVAL, "bid grid: every bid must be finite and at most $20.46 (2046 cents) for IMPLICIT keywords");
    return 0;
}
void launch_ideal_profit(const View &v, hipStream_t st, int num_cus, int n_samples, int n_bids, const double *d_grid, const int32_t *tape,
                         double *ideal, double *ir, double *cpc, uint2 *packed, int lim, long long n_items)
{
    const int waves = ideal_waves(lim);
    hipLaunchKernelGGL(k_ideal_profit, dim3(ideal_grid(n_items, num_cus, waves)), dim3(kWave * waves), ideal_lds_bytes(lim, waves), st, v, n_samples,
                       n_bids, d_grid, tape, ideal, ir, cpc, packed, lim, n_items);
}
}  // namespace

ADC_EXPORT int adc_engine_ideal_profit(adc_engine *e, int n_samples, const double *bid_grid, int n_bids, double *host_nk)
{
    ENGINE_GUARD(e);
    if (int rc = curves_model_check(e, "ideal profit")) return rc;
    if (n_samples <= 0 || !host_nk || !bid_grid || n_bids <= 0) return fail(ADC_EINVAL, "bad arguments");
    const size_t nk = (size_t)e->v.N * e->v.K;
    if (e->v.model == ADC_MODEL_EXPLICIT) {
        if (n_samples > (1 << 20)) return fail(ADC_EINVAL, "n_samples > 2^20 is not supported for EXPLICIT keywords");
        if (e->v.drift_on) { materialize_drift(e); HIP_TRY(hipGetLastError()); }
        const std::vector<double> g3 = explicit_grid3(bid_grid, n_bids);
        DevTemps tmp(e->stream);
        double *d_out = nullptr, *d_grid = nullptr;
        HIP_TRY(tmp.get(&d_out, nk * 8));
        hipError_t err = tmp.up(&d_grid, g3.data(), g3.size() * 8);
        if (err == hipSuccess) {
            launch_explicit_curves(e, n_samples, d_grid, n_bids, d_out, (float4 *)nullptr);
            err = hipGetLastError();
        }
        if (err == hipSuccess) err = hipMemcpyAsync(host_nk, d_out, nk * 8, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        HIP_TRY(err);
        tmp.release();
        return ADC_OK;
    }
    int lim = 0;
    if (int rc = implicit_curve_args(n_samples, bid_grid, n_bids, &lim)) return rc;
    if (e->v.drift_on) { materialize_drift(e); HIP_TRY(hipGetLastError()); }
    DevTemps tmp(e->stream);
    double *d_out = nullptr, *d_grid = nullptr;
    HIP_TRY(tmp.get(&d_out, nk * 8));
    hipError_t err = tmp.up(&d_grid, bid_grid, (size_t)n_bids * 8);
    if (err == hipSuccess) {
        launch_ideal_profit(e->v, e->stream, e->num_cus, n_samples, n_bids, d_grid, (const int32_t *)nullptr, d_out, (double *)nullptr, (double *)nullptr,
                            (uint2 *)nullptr, lim, (long long)nk);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpyAsync(host_nk, d_out, nk * 8, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    HIP_TRY(err);
    tmp.release();
    return ADC_OK;
}

namespace {
int ensure_ideal_buffers(adc_engine *e)
{
    if (e->have_ideal) return ADC_OK;
    const size_t nk = (size_t)e->v.N * e->v.K;
    int rc;
    if ((rc = dev_alloc(e, &e->pol.ideal, nk))) return rc;
    if ((rc = dev_alloc(e, &e->pol.best, nk))) return rc;
    if ((rc = dev_alloc(e, &e->pol.sum_ideal, nk))) return rc;
    if ((rc = dev_alloc(e, &e->pol.sum_ideal_pos, nk))) return rc;
    e->have_ideal = true;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_bid_curves_build(adc_engine *e, int n_samples, const double *bid_grid, int n_bids)
{
    ENGINE_GUARD(e);
    if (int rc = curves_model_check(e, "bid curves")) return rc;
    if (n_samples <= 0 || !bid_grid || n_bids <= 0) return fail(ADC_EINVAL, "bad arguments");
    const bool xp = e->v.model == ADC_MODEL_EXPLICIT;
    int lim = 0;
    if (!xp) if (int rc = implicit_curve_args(n_samples, bid_grid, n_bids, &lim)) return rc;      // (before the cached curves are touched)
    const size_t nk = (size_t)e->v.N * e->v.K;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (n_samples > (1 << 20)) return fail(ADC_EINVAL, "n_samples > 2^20 is not supported for cached curves");
    if (!e->have_curves || e->pol.n_bids != n_bids) {
        for (void *p : e->curve_allocs) (void)hipFree(p);
        e->curve_allocs.clear();
        e->have_curves = false;
        void *curve = nullptr, *grid = nullptr, *cont = nullptr, *ncont = nullptr, *cpos = nullptr;
        // contender lists: 24 bytes per distinct grid point that can be the argmax (typically half of the grid); curves with more
        // points than a list holds are evaluated on the whole grid
        const int cap = std::min(n_bids, 256);
        // (EXPLICIT: 16 bytes per keyword instead of 8 per grid point, and the grid's cost law beside the grid)
        const size_t curve_bytes = xp ? nk * sizeof(float4) : nk * n_bids * sizeof(uint2);
        if (hipMalloc(&curve, curve_bytes) != hipSuccess || hipMalloc(&grid, (size_t)n_bids * 8 * (xp ? 3 : 1)) != hipSuccess ||
            hipMalloc(&cont, nk * cap * sizeof(ContenderEntry)) != hipSuccess ||
            hipMalloc(&ncont, nk * sizeof(uint16_t)) != hipSuccess || hipMalloc(&cpos, nk * sizeof(uint16_t)) != hipSuccess) {
            (void)hipFree(curve); (void)hipFree(grid); (void)hipFree(cont); (void)hipFree(ncont); (void)hipFree(cpos);
            return fail(ADC_ENOMEM, "bid curves need ~30 bytes x num_envs x num_keywords x n_bids of device memory");
        }
        e->curve_allocs = {curve, grid, cont, ncont, cpos};
        if (xp) {
            e->pol.xcurve = (float4 *)curve;
            e->pol.grid_mu = (double *)grid + n_bids;
            e->pol.grid_sigma = (double *)grid + 2 * (size_t)n_bids;
        } else {
            e->pol.curve = (uint2 *)curve;
        }
        e->pol.grid = (double *)grid; e->pol.n_bids = n_bids;
        e->pol.contender = (ContenderEntry *)cont; e->pol.n_contenders = (uint16_t *)ncont;
        e->pol.cont_pos = (uint16_t *)cpos; e->pol.cont_cap = cap;
        e->have_curves = true;
    }
    e->pol.n_samples = n_samples;
    int rc = ensure_ideal_buffers(e);
    if (rc) return rc;
    if (xp) {
        const std::vector<double> g3 = explicit_grid3(bid_grid, n_bids);
        HIP_TRY(hipMemcpyAsync(e->pol.grid, g3.data(), g3.size() * 8, hipMemcpyHostToDevice, e->stream));
        launch_explicit_curves(e, n_samples, e->pol.grid, n_bids, (double *)nullptr, e->pol.xcurve);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(e->stream));       // (g3 is a host temporary)
    } else {
    HIP_TRY(hipMemcpyAsync(e->pol.grid, bid_grid, (size_t)n_bids * 8, hipMemcpyHostToDevice, e->stream));
    launch_ideal_profit(e->v, e->stream, e->num_cus, n_samples, n_bids, e->pol.grid, (const int32_t *)nullptr, (double *)nullptr, (double *)nullptr,
                        (double *)nullptr, e->pol.curve, lim, (long long)nk);
    HIP_TRY(hipGetLastError());
    }
    // which grid points can be the argmax at all (k_curve_contenders): the per-step ideal then evaluates only those
    HIP_TRY(hipMemsetAsync(e->pol.cont_pos, 0, nk * sizeof(uint16_t), e->stream));
    if (n_bids <= kContenderLines) {
        if (xp) hipLaunchKernelGGL(k_curve_contenders<ADC_MODEL_EXPLICIT>, dim3((unsigned)nk), dim3(kWave), sizeof(ContenderScratch), e->stream, e->v, e->pol);
        else hipLaunchKernelGGL(k_curve_contenders<ADC_MODEL_IMPLICIT>, dim3((unsigned)nk), dim3(kWave), sizeof(ContenderScratch), e->stream, e->v, e->pol);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(e->pol.n_contenders, 0xFF, nk * sizeof(uint16_t), e->stream));       // kContenderAll: the whole grid
    }
    HIP_TRY(hipStreamSynchronize(e->stream));      // (bid_grid is only borrowed)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_bid_curves_fetch(adc_engine *e, double *impression_rate_host, double *cpc_host)
{
    ENGINE_GUARD(e);
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    const size_t n = (size_t)e->v.N * e->v.K * e->pol.n_bids;
    if (e->v.model == ADC_MODEL_EXPLICIT) {          // the points evaluated on the device, by the function every ideal kernel calls
        DevTemps tmp(e->stream);
        double *d = nullptr;
        if (tmp.get(&d, 2 * n * 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
        const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)e->num_cus * 64));
        hipLaunchKernelGGL(k_explicit_curve_points, dim3(blocks), dim3(256), 0, e->stream, e->v, e->pol, d, d + n);
        hipError_t err = hipGetLastError();
        if (err == hipSuccess && impression_rate_host) err = hipMemcpyAsync(impression_rate_host, d, n * 8, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess && cpc_host) err = hipMemcpyAsync(cpc_host, d + n, n * 8, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        HIP_TRY(err);
        tmp.release();
        return ADC_OK;
    }
    std::vector<uint2> packed(n);
    HIP_TRY(hipMemcpyAsync(packed.data(), e->pol.curve, n * sizeof(uint2), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const double ns = (double)e->pol.n_samples;
    for (size_t i = 0; i < n; ++i) {            // the same IEEE operations k_ideal_from_curves applies
        const unsigned int idx = packed[i].y & 0x7FFFFFFFu;
        if (impression_rate_host) impression_rate_host[i] = (double)idx / ns;
        if (cpc_host) cpc_host[i] = ((double)packed[i].x / 100.0) / ((packed[i].y >> 31) ? ns : (double)(idx + 1u));
    }
    return ADC_OK;
}

// the contender lists of the cached curves (k_curve_contenders): n_nk[N*K] (0xFFFF = "the whole grid"), per entry 6 words
// {margin interval lo, hi (float32 bits), curve point x, y, grid index, 0}
ADC_EXPORT int adc_engine_bid_curves_contenders(adc_engine *e, uint16_t *n_nk, uint32_t *entries_nkc6, int32_t *cap)
{
    ENGINE_GUARD(e);
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    const size_t nk = (size_t)e->v.N * e->v.K;
    if (cap) *cap = e->pol.cont_cap;
    if (n_nk) HIP_TRY(hipMemcpyAsync(n_nk, e->pol.n_contenders, nk * 2, hipMemcpyDeviceToHost, e->stream));
    if (entries_nkc6) HIP_TRY(hipMemcpyAsync(entries_nkc6, e->pol.contender, nk * e->pol.cont_cap * sizeof(ContenderEntry), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

namespace {
// the per-step ideal of every keyword into the device-side arrays and running sums (nothing to the host): chain-compatible
int ideal_step_chained(adc_engine *e)
{
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    const bool full_scan = e->ideal_full_scan;
    const int rc = launch_chained(e, [&](const View &v, const PolicyView &p, hipStream_t st, float *, float *) {
        // the reference evaluates env.keyword_params as they stand before the step, i.e. with the last update_keywords applied
        if (v.drift_on) hipLaunchKernelGGL(k_materialize_drift, dim3(v.N), dim3(256), 0, st, v);
        launch_ideal_step(v, p, st, full_scan);
    });
    if (!rc && e->v.drift_on) e->drift_applied = true;
    return rc;
}
int policy_oracle_chained(adc_engine *e, float budget)
{
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build / adc_engine_ideal_step have not been called");
    return launch_chained(e, [&](const View &v, const PolicyView &p, hipStream_t st, float *d_bids, float *d_budget) {
        hipLaunchKernelGGL(k_policy_oracle, dim3((unsigned)((v.K + 255) / 256), (unsigned)v.N), dim3(256), 0, st, v, p, budget, d_bids, d_budget);
    });
}
}  // namespace

ADC_EXPORT int adc_engine_ideal_step(adc_engine *e, double *ideal_host_nk, int32_t *best_index_host_nk)
{
    if (e && !ideal_host_nk && !best_index_host_nk) {
        ENGINE_GUARD_STEP(e);
        return ideal_step_chained(e);
    }
    ENGINE_GUARD(e);
    if (!e->have_curves) return fail(ADC_ESTATE, "adc_engine_bid_curves_build has not been called");
    const size_t nk = (size_t)e->v.N * e->v.K;
    // the reference evaluates env.keyword_params as they stand before the step, i.e. with the last update_keywords applied
    if (e->v.drift_on) { materialize_drift(e); HIP_TRY(hipGetLastError()); }
    launch_ideal_step(e->v, e->pol, e->stream, e->ideal_full_scan);
    HIP_TRY(hipGetLastError());
    if (ideal_host_nk) HIP_TRY(hipMemcpyAsync(ideal_host_nk, e->pol.ideal, nk * 8, hipMemcpyDeviceToHost, e->stream));
    if (best_index_host_nk) HIP_TRY(hipMemcpyAsync(best_index_host_nk, e->pol.best, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (ideal_host_nk || best_index_host_nk) HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_policy_oracle(adc_engine *e, float budget)
{
    ENGINE_GUARD_STEP(e);
    return policy_oracle_chained(e, budget);
}

ADC_EXPORT int adc_engine_metrics_read_nk(adc_engine *e, int64_t *profit_cents_nk, double *ideal_sum_nk, double *ideal_pos_sum_nk)
{
    ENGINE_GUARD(e);
    const size_t nk = (size_t)e->v.N * e->v.K;
    if ((ideal_sum_nk || ideal_pos_sum_nk) && !e->have_ideal) return fail(ADC_ESTATE, "no ideal profit has been accumulated (adc_engine_ideal_step)");
    std::vector<int32_t> lo;
    if (profit_cents_nk) {          // the 64-bit spill into the caller's array, the 32-bit words beside it: added below
        lo.resize(nk);
        HIP_TRY(hipMemcpyAsync(profit_cents_nk, e->v.metric_hi, nk * 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(lo.data(), e->v.metric_lo, nk * 4, hipMemcpyDeviceToHost, e->stream));
    }
    if (ideal_sum_nk) HIP_TRY(hipMemcpyAsync(ideal_sum_nk, e->pol.sum_ideal, nk * 8, hipMemcpyDeviceToHost, e->stream));
    if (ideal_pos_sum_nk) HIP_TRY(hipMemcpyAsync(ideal_pos_sum_nk, e->pol.sum_ideal_pos, nk * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < lo.size(); ++i) profit_cents_nk[i] += lo[i];
    return ADC_OK;
}

// per-env AKNCP and NCP of the running episode, reduced on the device (k_akncp_ncp)
ADC_EXPORT int adc_engine_metrics_akncp_ncp(adc_engine *e, double days, double *akncp_n, double *ncp_n)
{
    ENGINE_GUARD(e);
    if (!akncp_n || !ncp_n) return fail(ADC_EINVAL, "NULL output");
    if (!e->have_ideal) return fail(ADC_ESTATE, "no ideal profit has been accumulated (adc_engine_ideal_step)");
    if (!e->v.metrics_on) return fail(ADC_ESTATE, "metric mode is off (adc_engine_metrics_enable)");
    if (e->v.K > kMedianMaxK) return fail(ADC_EINVAL, "num_keywords beyond the device-side median (4096): reduce adc_engine_metrics_read_nk on the host");
    const size_t n = (size_t)e->v.N;
    DevTemps tmp(e->stream);
    double *d = nullptr;
    if (tmp.get(&d, 2 * n * 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
    int P = 1;
    while (P < e->v.K) P <<= 1;
    hipLaunchKernelGGL(k_akncp_ncp, dim3((unsigned)n), dim3(kMedianBlock), (size_t)P * 8, e->stream, e->v, e->pol, days, d, d + n);
    if (hipGetLastError() != hipSuccess) return fail(ADC_EHIP, "k_akncp_ncp launch failed");
    if (hipMemcpyAsync(akncp_n, d, n * 8, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipMemcpyAsync(ncp_n, d + n, n * 8, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return fail(ADC_EHIP, "download failed");
    tmp.release();
    return ADC_OK;
}
