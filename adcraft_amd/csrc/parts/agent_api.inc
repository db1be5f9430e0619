// agent_api.inc - the extern "C" entry points of the two hand-written agents, one per env and device-resident (include/adcraft_engine.h),
// over parts/host_api.inc: the zero-margin agent (k_agent_step of parts/kernels_policy.inc), adc_engine_get_actions, and the
// interpolation agent, NaiveInterpolationStrategy (parts/kernel_interp_agent.inc; the per-keyword act is csrc/adc_interp.h).
// (part of the single translation unit adc_engine.hip)

namespace {
// how agent_launch and interp_launch end: wait for the stream where the site says so, free what was staged, and report the
// launch's error first, the wait's second
int staged_launch_done(DevTemps &tmp, bool wait, hipError_t err)
{
    const hipError_t e2 = wait ? hipStreamSynchronize(tmp.stream) : hipSuccess;
    tmp.release();
    if (err != hipSuccess) return fail(ADC_EHIP, hipGetErrorString(err));
    if (e2 != hipSuccess) return fail(ADC_EHIP, hipGetErrorString(e2));
    return ADC_OK;
}
}  // namespace

// ---- the zero-margin agent (kernels_policy.inc) -----------------------------------------------------------------------------
ADC_EXPORT int adc_engine_agent_init(adc_engine *e, float default_rpc, const uint64_t *seeds_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N, nk = N * e->v.K;
    if (!e->have_agent) {
        int rc;
        if ((rc = dev_alloc(e, &e->pol.ave_rpc, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.n_rpc, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.ave_sctr, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.n_sctr, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.max_bid, nk))) return rc;
        if ((rc = dev_alloc(e, &e->pol.key, N))) return rc;
        if ((rc = dev_alloc(e, &e->pol.tick, N))) return rc;
        e->have_agent = true;
    }
    e->pol.default_rpc = default_rpc;
    DevTemps tmp(e->stream);
    uint64_t *d_seeds = nullptr;
    if (seeds_n) HIP_TRY(tmp.up(&d_seeds, seeds_n, N * 8));
    hipLaunchKernelGGL(k_agent_init, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, e->v, e->pol, d_seeds,
                       e->cfg.seed, e->cfg.env_id_base);
    hipError_t err = hipGetLastError();
    hipError_t err2 = hipStreamSynchronize(e->stream);
    HIP_TRY(err);
    HIP_TRY(err2);
    tmp.release();
    return ADC_OK;
}

namespace {
// update and/or act; host observation arrays (all three or none) are staged through temporaries
int agent_launch(adc_engine *e, const int32_t *clicks_nk, const int32_t *conv_nk, const float *rev_nk, int do_update, int do_act,
                 const double *replay_u_nk, float budget_override)
{
    if (!e->have_agent) return fail(ADC_ESTATE, "adc_engine_agent_init has not been called");
    const int given = (clicks_nk != nullptr) + (conv_nk != nullptr) + (rev_nk != nullptr);
    if (given != 0 && given != 3) return fail(ADC_EINVAL, "pass all of clicks/conversions/revenue, or none (= the engine's last observation)");
    const size_t nk = (size_t)e->v.N * e->v.K;
    DevTemps tmp(e->stream);
    int32_t *d_clk = nullptr, *d_conv = nullptr;
    float *d_rev = nullptr;
    double *d_u = nullptr;
    hipError_t err = hipSuccess;
    if (given == 3 && do_update) {      // the observation arrays, all or none
        if (tmp.get(&d_clk, nk * 4) != hipSuccess || tmp.get(&d_conv, nk * 4) != hipSuccess || tmp.get(&d_rev, nk * 4) != hipSuccess)
            return fail(ADC_ENOMEM, "hipMalloc failed");
        err = hipMemcpyAsync(d_clk, clicks_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_conv, conv_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_rev, rev_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess && replay_u_nk && do_act) {       // then the optional replay uniforms
        if (tmp.get(&d_u, nk * 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
        err = hipMemcpyAsync(d_u, replay_u_nk, nk * 8, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_agent_step, dim3((unsigned)e->v.N), dim3(256), 0, e->stream, e->v, e->pol,
                           d_clk ? d_clk : e->v.clk, d_conv ? d_conv : e->v.conv, d_rev ? d_rev : e->v.rev, do_update, do_act,
                           (const double *)d_u, budget_override, e->d_bids, e->d_budget);
        err = hipGetLastError();
    }
    return staged_launch_done(tmp, d_clk || d_u, err);      // (nothing staged: nothing to wait for)
}
}  // namespace

namespace {
// update + act on the engine's last observation (no host arrays): chain-compatible
int agent_step_chained(adc_engine *e, float budget_override)
{
    if (!e->have_agent) return fail(ADC_ESTATE, "adc_engine_agent_init has not been called");
    return launch_chained(e, [&](const View &v, const PolicyView &p, hipStream_t st, float *d_bids, float *d_budget) {
        hipLaunchKernelGGL(k_agent_step, dim3((unsigned)v.N), dim3(256), 0, st, v, p, v.clk, v.conv, v.rev, 1, 1, (const double *)nullptr, budget_override, d_bids, d_budget);
    });
}
}  // namespace

ADC_EXPORT int adc_engine_agent_update(adc_engine *e, const int32_t *clicks_nk, const int32_t *conversions_nk, const float *revenue_nk)
{
    ENGINE_GUARD(e);
    return agent_launch(e, clicks_nk, conversions_nk, revenue_nk, 1, 0, nullptr, 0.0f);
}

ADC_EXPORT int adc_engine_agent_act(adc_engine *e, float budget_override, const double *replay_uniforms_nk)
{
    ENGINE_GUARD(e);
    return agent_launch(e, nullptr, nullptr, nullptr, 0, 1, replay_uniforms_nk, budget_override);
}

ADC_EXPORT int adc_engine_agent_step(adc_engine *e, float budget_override)
{
    ENGINE_GUARD_STEP(e);
    return agent_step_chained(e, budget_override);
}

ADC_EXPORT int adc_engine_agent_state(adc_engine *e, float *ave_rpc_nk, int32_t *num_rpc_obs_nk, float *ave_sctr_nk,
                                      int32_t *num_sctr_obs_nk, double *max_bids_nk)
{
    ENGINE_GUARD(e);
    if (!e->have_agent) return fail(ADC_ESTATE, "adc_engine_agent_init has not been called");
    const size_t nk = (size_t)e->v.N * e->v.K;
    if (ave_rpc_nk) HIP_TRY(hipMemcpyAsync(ave_rpc_nk, e->pol.ave_rpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (num_rpc_obs_nk) HIP_TRY(hipMemcpyAsync(num_rpc_obs_nk, e->pol.n_rpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (ave_sctr_nk) HIP_TRY(hipMemcpyAsync(ave_sctr_nk, e->pol.ave_sctr, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (num_sctr_obs_nk) HIP_TRY(hipMemcpyAsync(num_sctr_obs_nk, e->pol.n_sctr, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (max_bids_nk) HIP_TRY(hipMemcpyAsync(max_bids_nk, e->pol.max_bid, nk * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_get_actions(adc_engine *e, float *bids_nk, float *budget_n)
{
    ENGINE_GUARD(e);
    if (bids_nk) HIP_TRY(hipMemcpyAsync(bids_nk, e->d_bids, (size_t)e->v.N * e->v.K * 4, hipMemcpyDeviceToHost, e->stream));
    if (budget_n) HIP_TRY(hipMemcpyAsync(budget_n, e->d_budget, (size_t)e->v.N * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

// ---- NaiveInterpolationStrategy, one agent per env (parts/kernel_interp_agent.inc) ---------------------------------------
namespace {
// the agent's view of the env group that starts at env e0: every per-keyword and per-env array moves to that env; the
// slot-major lists keep the engine's stride
inline InterpView interp_view_from(const adc_engine *e, size_t e0)
{
    InterpView p = e->ip;
    const size_t o = e0, ok = o * (size_t)e->v.K;
    auto at = [](auto *&ptr, size_t off) { if (ptr) ptr += off; };
    at(p.ave_rpc, ok); at(p.n_rpc, ok); at(p.ave_sctr, ok); at(p.n_sctr, ok); at(p.max_obs, ok); at(p.last_bid, ok); at(p.last_index, ok);
    at(p.n_clk, ok); at(p.n_cpc, ok); at(p.clk_cent, ok); at(p.clk_ave, ok); at(p.clk_cnt, ok);
    at(p.cpc_cent, ok); at(p.cpc_ave, ok); at(p.cpc_cnt, ok); at(p.kw_cost, ok); at(p.kw_profit, ok);
    at(p.budget, o); at(p.profit, o); at(p.cost, o); at(p.key, o); at(p.tick, o);
    return p;
}
// `more` further updates fit the lists (a capacity of 300 holds every cent)
inline bool interp_room(const adc_engine *e, long long more)
{
    return e->ip.cap >= adc::kInterpCents || e->interp_updates + more <= (long long)e->ip.cap;
}
inline int interp_grid_check(const double *bids, int n)
{
    if (!bids || n < 1 || n > adc::kInterpMaxBids) return fail(ADC_EINVAL, "allowed_bids must hold 1 to 2048 values");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(bids[i])) return fail(ADC_EINVAL, "allowed_bids must be finite");
    return ADC_OK;
}
int interp_step_chained(adc_engine *e, float budget_override)
{
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    // counted before anything is enqueued, so that a launch failing partway leaves the count high, never low (a captured day
    // is counted where its graph is launched)
    if (!e->in_capture) e->interp_updates += 1;
    return launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *d_bids, float *d_budget) {
        const InterpView p = interp_view_from(e, (size_t)(d_budget - e->d_budget));      // (the group's first env)
        hipLaunchKernelGGL(k_interp_step, dim3((unsigned)v.N), dim3(256), 0, st, v, p, (const float *)nullptr, v.clk, v.cost,
                           v.conv, v.rev, 1, 1, (const double *)nullptr, budget_override, d_bids, d_budget);
    });
}
}  // namespace

ADC_EXPORT int adc_engine_interp_init(adc_engine *e, double threshold, double bid_step, const double *allowed_bids, int32_t n_bids,
                                      int32_t capacity, const uint64_t *seeds_n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!std::isfinite(threshold) || !std::isfinite(bid_step)) return fail(ADC_EINVAL, "threshold and bid_step must be finite");
    if (int rc = interp_grid_check(allowed_bids, n_bids)) return rc;
    if (capacity < 0 || capacity > adc::kInterpCents) return fail(ADC_EINVAL, "capacity must be 0 (default) to 300");
    ENGINE_GUARD(e);
    const int cap = capacity > 0 ? capacity : std::min(adc::kInterpCents, std::max(1, e->v.max_days + 1));
    const size_t N = e->v.N, nk = N * e->v.K;
    if (e->have_interp && cap != e->ip.cap) return fail(ADC_EINVAL, "the capacity is fixed by the first adc_engine_interp_init");
    if (!e->have_interp) {
        InterpView &p = e->ip;
        const size_t slots = nk * (size_t)cap;
        int rc;
        if ((rc = dev_alloc(e, &p.ave_rpc, nk)) || (rc = dev_alloc(e, &p.n_rpc, nk)) || (rc = dev_alloc(e, &p.ave_sctr, nk)) ||
            (rc = dev_alloc(e, &p.n_sctr, nk)) || (rc = dev_alloc(e, &p.max_obs, nk)) || (rc = dev_alloc(e, &p.last_bid, nk)) ||
            (rc = dev_alloc(e, &p.last_index, nk)) ||
            (rc = dev_alloc(e, &p.n_clk, nk)) || (rc = dev_alloc(e, &p.n_cpc, nk)) || (rc = dev_alloc(e, &p.clk_cent, slots)) ||
            (rc = dev_alloc(e, &p.clk_ave, slots)) || (rc = dev_alloc(e, &p.clk_cnt, slots)) || (rc = dev_alloc(e, &p.cpc_cent, slots)) ||
            (rc = dev_alloc(e, &p.cpc_ave, slots)) || (rc = dev_alloc(e, &p.cpc_cnt, slots)) || (rc = dev_alloc(e, &p.kw_cost, nk)) ||
            (rc = dev_alloc(e, &p.kw_profit, nk)) || (rc = dev_alloc(e, &p.budget, N)) || (rc = dev_alloc(e, &p.profit, N)) ||
            (rc = dev_alloc(e, &p.cost, N)) || (rc = dev_alloc(e, &p.key, N)) || (rc = dev_alloc(e, &p.tick, N)))
            return rc;
        double *grid = nullptr;
        if ((rc = dev_alloc(e, &grid, (size_t)adc::kInterpMaxBids))) return rc;
        p.grid = grid;
        p.cap = cap;
        p.slot_stride = nk;
        e->have_interp = true;
    }
    e->ip.threshold = threshold;
    e->ip.bid_step = bid_step;
    e->ip.n_bids = n_bids;
    HIP_TRY(hipMemcpyAsync(const_cast<double *>(e->ip.grid), allowed_bids, (size_t)n_bids * 8, hipMemcpyHostToDevice, e->stream));
    e->interp_updates = 0;
    DevTemps tmp(e->stream);
    uint64_t *d_seeds = nullptr;
    if (seeds_n) HIP_TRY(tmp.up(&d_seeds, seeds_n, N * 8));
    hipLaunchKernelGGL(k_interp_init, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, e->ip, e->v.K,
                       d_seeds, e->cfg.seed, e->cfg.env_id_base);
    hipError_t err = hipGetLastError();
    hipError_t err2 = hipStreamSynchronize(e->stream);
    HIP_TRY(err);
    HIP_TRY(err2);
    tmp.release();
    return ADC_OK;
}

ADC_EXPORT int adc_engine_interp_set_allowed_bids(adc_engine *e, const double *bids, int32_t n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = interp_grid_check(bids, n)) return rc;
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(const_cast<double *>(e->ip.grid), bids, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->ip.n_bids = n;
    return ADC_OK;
}

namespace {
// update (host arrays: all five or none) and/or act on the engine's stream; host inputs are staged through temporaries
int interp_launch(adc_engine *e, const double *prev_bids_nk, const int32_t *clicks_nk, const float *cost_nk, const int32_t *conv_nk,
                  const float *rev_nk, int do_update, int do_act, const double *replay_u_nk, float budget_override)
{
    const size_t nk = (size_t)e->v.N * e->v.K;
    std::vector<float> bids32;
    if (do_update && prev_bids_nk) {
        bids32.resize(nk);
        for (size_t i = 0; i < nk; ++i) bids32[i] = (float)prev_bids_nk[i];       // torch.Tensor([prev_bid])
    }
    DevTemps tmp(e->stream);
    float *d_bid = nullptr, *d_cost = nullptr, *d_rev = nullptr;
    int32_t *d_clk = nullptr, *d_conv = nullptr;
    double *d_u = nullptr;
    hipError_t err = hipSuccess;
    if (do_update && prev_bids_nk) {    // the observation arrays, all or none
        if (tmp.get(&d_bid, nk * 4) != hipSuccess || tmp.get(&d_clk, nk * 4) != hipSuccess || tmp.get(&d_cost, nk * 4) != hipSuccess ||
            tmp.get(&d_conv, nk * 4) != hipSuccess || tmp.get(&d_rev, nk * 4) != hipSuccess)
            return fail(ADC_ENOMEM, "hipMalloc failed");
        err = hipMemcpyAsync(d_bid, bids32.data(), nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_clk, clicks_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_cost, cost_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_conv, conv_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(d_rev, rev_nk, nk * 4, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess && replay_u_nk && do_act) {       // then the optional replay uniforms
        if (tmp.get(&d_u, nk * 8) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc failed");
        err = hipMemcpyAsync(d_u, replay_u_nk, nk * 8, hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess) {
        if (do_update) e->interp_updates += 1;       // (before the launch: a failure leaves the count high, never low)
        hipLaunchKernelGGL(k_interp_step, dim3((unsigned)e->v.N), dim3(256), 0, e->stream, e->v, e->ip, (const float *)d_bid,
                           d_clk ? d_clk : e->v.clk, d_cost ? d_cost : e->v.cost, d_conv ? d_conv : e->v.conv, d_rev ? d_rev : e->v.rev,
                           do_update, do_act, (const double *)d_u, budget_override, e->d_bids, e->d_budget);
        err = hipGetLastError();
    }
    return staged_launch_done(tmp, true, err);
}
}  // namespace

ADC_EXPORT int adc_engine_interp_update(adc_engine *e, const double *prev_bids_nk, const int32_t *clicks_nk, const float *cost_nk,
                                        const int32_t *conversions_nk, const float *revenue_nk)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const int given = (prev_bids_nk != nullptr) + (clicks_nk != nullptr) + (cost_nk != nullptr) + (conversions_nk != nullptr) +
                      (revenue_nk != nullptr);
    if (given != 0 && given != 5) return fail(ADC_EINVAL, "pass all of prev_bids/clicks/cost/conversions/revenue, or none");
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    if (prev_bids_nk) {
        const size_t nk = (size_t)e->v.N * e->v.K;
        for (size_t i = 0; i < nk; ++i)
            if (!std::isfinite(prev_bids_nk[i])) return fail(ADC_EINVAL, "previous bids must be finite");
    }
    if (!interp_room(e, 1)) return fail(ADC_EINVAL, "the interpolation agent's capacity is full: one more update could overflow it");
    ENGINE_GUARD(e);
    return interp_launch(e, prev_bids_nk, clicks_nk, cost_nk, conversions_nk, revenue_nk, 1, 0, nullptr, 0.0f);
}

ADC_EXPORT int adc_engine_interp_act(adc_engine *e, float budget_override, const double *replay_uniforms_nk)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    ENGINE_GUARD(e);
    return interp_launch(e, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, replay_uniforms_nk, budget_override);
}

ADC_EXPORT int adc_engine_interp_step(adc_engine *e, float budget_override)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    if (!interp_room(e, 1)) return fail(ADC_EINVAL, "the interpolation agent's capacity is full: one more update could overflow it");
    ENGINE_GUARD_STEP(e);
    return interp_step_chained(e, budget_override);
}

ADC_EXPORT int adc_engine_interp_state(adc_engine *e, float *ave_rpc_nk, int32_t *num_rpc_obs_nk, float *ave_sctr_nk,
                                       int32_t *num_sctr_obs_nk, double *max_observed_nk, int32_t *bid_index_nk, double *budget_n, double *profit_beliefs_n,
                                       double *cost_beliefs_n)
{
    ENGINE_GUARD(e);
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    const size_t n = (size_t)e->v.N, nk = n * e->v.K;
    const InterpView &p = e->ip;
    if (ave_rpc_nk) HIP_TRY(hipMemcpyAsync(ave_rpc_nk, p.ave_rpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (num_rpc_obs_nk) HIP_TRY(hipMemcpyAsync(num_rpc_obs_nk, p.n_rpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (ave_sctr_nk) HIP_TRY(hipMemcpyAsync(ave_sctr_nk, p.ave_sctr, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (num_sctr_obs_nk) HIP_TRY(hipMemcpyAsync(num_sctr_obs_nk, p.n_sctr, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (max_observed_nk) HIP_TRY(hipMemcpyAsync(max_observed_nk, p.max_obs, nk * 8, hipMemcpyDeviceToHost, e->stream));
    if (bid_index_nk) HIP_TRY(hipMemcpyAsync(bid_index_nk, p.last_index, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (budget_n) HIP_TRY(hipMemcpyAsync(budget_n, p.budget, n * 8, hipMemcpyDeviceToHost, e->stream));
    if (profit_beliefs_n) HIP_TRY(hipMemcpyAsync(profit_beliefs_n, p.profit, n * 8, hipMemcpyDeviceToHost, e->stream));
    if (cost_beliefs_n) HIP_TRY(hipMemcpyAsync(cost_beliefs_n, p.cost, n * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_interp_entries(adc_engine *e, int32_t *capacity, int32_t *n_clicks_nk, uint16_t *clicks_cent_cnk,
                                         float *ave_clicks_cnk, int32_t *clicks_count_cnk, int32_t *n_cpc_nk, uint16_t *cpc_cent_cnk,
                                         double *ave_cpc_cnk, int32_t *cpc_count_cnk)
{
    ENGINE_GUARD(e);
    if (!e->have_interp) return fail(ADC_ESTATE, "adc_engine_interp_init has not been called");
    const InterpView &p = e->ip;
    const size_t nk = (size_t)e->v.N * e->v.K, slots = nk * (size_t)p.cap;
    if (capacity) *capacity = p.cap;
    if (n_clicks_nk) HIP_TRY(hipMemcpyAsync(n_clicks_nk, p.n_clk, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (clicks_cent_cnk) HIP_TRY(hipMemcpyAsync(clicks_cent_cnk, p.clk_cent, slots * 2, hipMemcpyDeviceToHost, e->stream));
    if (ave_clicks_cnk) HIP_TRY(hipMemcpyAsync(ave_clicks_cnk, p.clk_ave, slots * 4, hipMemcpyDeviceToHost, e->stream));
    if (clicks_count_cnk) HIP_TRY(hipMemcpyAsync(clicks_count_cnk, p.clk_cnt, slots * 4, hipMemcpyDeviceToHost, e->stream));
    if (n_cpc_nk) HIP_TRY(hipMemcpyAsync(n_cpc_nk, p.n_cpc, nk * 4, hipMemcpyDeviceToHost, e->stream));
    if (cpc_cent_cnk) HIP_TRY(hipMemcpyAsync(cpc_cent_cnk, p.cpc_cent, slots * 2, hipMemcpyDeviceToHost, e->stream));
    if (ave_cpc_cnk) HIP_TRY(hipMemcpyAsync(ave_cpc_cnk, p.cpc_ave, slots * 8, hipMemcpyDeviceToHost, e->stream));
    if (cpc_count_cnk) HIP_TRY(hipMemcpyAsync(cpc_count_cnk, p.cpc_cnt, slots * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
