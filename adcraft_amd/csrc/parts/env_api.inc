// env_api.inc - the extern "C" entry points that set or read the envs (include/adcraft_engine.h), over parts/host_api.inc: keyword
// parameters and both keyword generators, reset, limits, the general model, the drift setters (and the settle they share), RNG and
// episode state, update_keywords; page-locked host memory, the device buffers, env groups, the stream; the action sampler, flat
// actions and observations, the profile and the timed region, the step kernel's name.
// (part of the single translation unit adc_engine.hip)

ADC_EXPORT int adc_engine_set_params(adc_engine *e, int param_id, const float *host_nk)
{
    ENGINE_GUARD(e);
    if (param_id < 0 || param_id >= ADC_P_COUNT || !host_nk) return fail(ADC_EINVAL, "bad param_id or NULL buffer");
    const size_t NK = (size_t)e->v.N * e->v.K;
    HIP_TRY(hipMemcpyAsync(e->v.params + (size_t)param_id * NK, host_nk, NK * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (param_id == ADC_P_VOL_MEAN) e->volume_hint_dirty = true;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_get_params(adc_engine *e, int param_id, float *host_nk)
{
    ENGINE_GUARD(e);
    if (param_id < 0 || param_id >= ADC_P_COUNT || !host_nk) return fail(ADC_EINVAL, "bad param_id or NULL buffer");
    const size_t NK = (size_t)e->v.N * e->v.K;
    if (e->v.drift_on) {
        materialize_drift(e);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(host_nk, e->v.params + (size_t)param_id * NK, NK * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_env_params(adc_engine *e, int env, const float *host_8k)
{
    ENGINE_GUARD(e);
    if (env < 0 || env >= e->v.N || !host_8k) return fail(ADC_EINVAL, "env out of range or NULL buffer");
    const size_t K = e->v.K, NK = (size_t)e->v.N * K;
    for (int p = 0; p < ADC_P_COUNT; ++p)
        HIP_TRY(hipMemcpyAsync(e->v.params + p * NK + env * K, host_8k + p * K, K * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->volume_hint_dirty = true;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_generate_keywords(adc_engine *e, const adc_quantiles *q, float no_vol_prob, uint32_t serial,
                                            const uint8_t *env_mask)
{
    ENGINE_GUARD(e);
    if (e->v.model != ADC_MODEL_IMPLICIT) return fail(ADC_EINVAL, "device keyword generation is provided for IMPLICIT keywords");
    if (!q) return fail(ADC_EINVAL, "quantile tables are NULL");
    DevTemps tmp(e->stream);
    KeygenTables tabs;
    for (int i = 0; i < 7; ++i) {
        const int B = q->buckets[i];
        if (B <= 0 || !q->mins[i] || !q->medians[i] || !q->maxs[i]) return fail(ADC_EINVAL, "every quantity needs at least one bucket");
        float *d = nullptr;
        if (tmp.get(&d, (size_t)B * 12) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc (quantiles) failed");
        if (hipMemcpyAsync(d, q->mins[i], (size_t)B * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
            hipMemcpyAsync(d + B, q->medians[i], (size_t)B * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
            hipMemcpyAsync(d + 2 * B, q->maxs[i], (size_t)B * 4, hipMemcpyHostToDevice, e->stream) != hipSuccess) return fail(ADC_EHIP, "quantile upload failed");
        tabs.t[i] = adc::QuantileTable{d, d + B, d + 2 * B, B};
    }
    uint8_t *d_mask = nullptr;
    if (env_mask) {
        if (tmp.get(&d_mask, (size_t)e->v.N) != hipSuccess) return fail(ADC_ENOMEM, "hipMalloc (mask) failed");
        if (hipMemcpyAsync(d_mask, env_mask, (size_t)e->v.N, hipMemcpyHostToDevice, e->stream) != hipSuccess) return fail(ADC_EHIP, "mask upload failed");
    }
    hipLaunchKernelGGL(k_generate_keywords, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)e->v.N), dim3(256), 0, e->stream, e->v, tabs,
                       no_vol_prob, serial, d_mask);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    HIP_TRY(err);
    tmp.release();
    e->volume_hint_dirty = true;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_generate_explicit_keywords(adc_engine *e, uint32_t serial, const uint8_t *env_mask)
{
    ENGINE_GUARD(e);
    if (e->v.model != ADC_MODEL_EXPLICIT) return fail(ADC_EINVAL, "sample_random_keywords' law is the EXPLICIT model's (IMPLICIT keywords: adc_engine_generate_keywords)");
    DevTemps tmp(e->stream);
    uint8_t *d_mask = nullptr;
    if (env_mask) {
        if (tmp.get(&d_mask, (size_t)e->v.N) != hipSuccess) { (void)hipGetLastError(); return fail(ADC_ENOMEM, "hipMalloc (mask) failed"); }
        if (hipMemcpyAsync(d_mask, env_mask, (size_t)e->v.N, hipMemcpyHostToDevice, e->stream) != hipSuccess) return fail(ADC_EHIP, "mask upload failed");
    }
    hipLaunchKernelGGL(k_generate_explicit_keywords, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)e->v.N), dim3(256), 0, e->stream, e->v, serial, d_mask);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    HIP_TRY(err);
    tmp.release();
    e->volume_hint_dirty = true;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_reset(adc_engine *e, const uint8_t *env_mask, const uint64_t *seeds)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    uint8_t *d_mask = nullptr;
    uint64_t *d_seeds = nullptr;
    DevTemps tmp(e->stream);
    if (env_mask) HIP_TRY(tmp.up(&d_mask, env_mask, N));
    if (seeds) HIP_TRY(tmp.up(&d_seeds, seeds, N * 8));
    hipLaunchKernelGGL(k_reset, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, e->v, d_mask, d_seeds);
    hipError_t err = hipGetLastError();
    // the observation reset() returns is all zeros (gymnasium_kw_env.py:329-344): device-resident callers read it
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_clear_obs, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)N), dim3(256), 0, e->stream, e->v, d_mask);
        err = hipGetLastError();
    }
    // (a reset env's running discounted return ends with its episode, the PPO / A2C learners', the TD3 learners' and the SAC
    //  learners'; nothing is enqueued without a reward normaliser)
    for (const NormSet *s : {&e->rn, &e->tn, &e->sn}) {
        if (err != hipSuccess || !s->rew.G) continue;
        hipLaunchKernelGGL(k_rew_norm_carry_reset, dim3((unsigned)((N + kRewNormBlock - 1) / kRewNormBlock)), dim3(kRewNormBlock), 0, e->stream, (int)N, d_mask,
                           s->rew.G);
        err = hipGetLastError();
    }
    // (... and so does its observation history; nothing is enqueued without one)
    if (err == hipSuccess && e->have_mlp && e->mp.hist) {
        hipLaunchKernelGGL(k_mlp_hist_forget, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, (int)N, d_mask, e->mp.last);
        err = hipGetLastError();
    }
    // (... and so does the state of a recurrent policy's cell)
    if (err == hipSuccess && e->have_mlp && e->gv.G) {
        hipLaunchKernelGGL(k_mlp_hist_forget, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, e->stream, (int)N, d_mask, e->gv.last);
        err = hipGetLastError();
    }
    hipError_t err2 = hipStreamSynchronize(e->stream);
    HIP_TRY(err);
    HIP_TRY(err2);
    tmp.release();
    e->have_reset = true;
    e->last_step = 0;
    e->stream_steps = 0;
    e->env_moves += 1;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_limits(adc_engine *e, int32_t max_days, double loss_threshold)
{
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.max_days = max_days;
    e->v.loss_threshold = loss_threshold;
    e->cfg.max_days = max_days;
    e->cfg.loss_threshold = loss_threshold;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_drift(adc_engine *e, int32_t enabled, float drift_vol, float drift_ctr, float drift_cvr)
{
    ENGINE_GUARD(e);
    if (!enabled && e->v.drift_on) {      // apply what is pending under the old setting, then switch off
        materialize_drift(e);
        HIP_TRY(hipGetLastError());
        forget_replayable_steps(e);       // (the parameters have moved, and with drift off nothing would say so any more)
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.drift_on = enabled ? 1 : 0;
    e->v.drift_vol = drift_vol; e->v.drift_ctr = drift_ctr; e->v.drift_cvr = drift_cvr;
    if (!enabled) HIP_TRY(hipMemsetAsync(e->v.drift_pending, 0, (size_t)e->v.N, e->stream));
    return ADC_OK;
}

namespace {
// what adc_engine_set_drift_mask / adc_engine_set_env_drift do before they swap: the pending update_keywords() of every env is
// the one the previous step scheduled, so it moves the planes under the selection and magnitudes in force when it was
// scheduled; then nothing in flight reads the old device copy when it is overwritten
int settle_pending_drift(adc_engine *e)
{
    if (e->v.drift_on) {
        materialize_drift(e);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_set_drift_mask(adc_engine *e, const uint8_t *mask_nk)
{
    ENGINE_GUARD(e);
    { const int rc = settle_pending_drift(e); if (rc) return rc; }
    if (!mask_nk) { e->v.drift_bits = nullptr; return ADC_OK; }
    const size_t N = (size_t)e->v.N, K = (size_t)e->v.K, W = (K + 31) / 32;
    std::vector<uint32_t> bits(N * W, 0u);
    for (size_t n = 0; n < N; ++n)
        for (size_t k = 0; k < K; ++k)
            if (mask_nk[n * K + k]) bits[n * W + k / 32] |= 1u << (k % 32);
    if (!e->d_drift_bits) { const int rc = dev_alloc(e, &e->d_drift_bits, N * W); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(e->d_drift_bits, bits.data(), N * W * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.drift_bits = e->d_drift_bits;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_env_drift(adc_engine *e, const float *rates_n3)
{
    ENGINE_GUARD(e);
    { const int rc = settle_pending_drift(e); if (rc) return rc; }
    if (!rates_n3) { e->v.drift_rate = nullptr; return ADC_OK; }
    const size_t N = (size_t)e->v.N;
    if (!e->d_drift_rate) { const int rc = dev_alloc(e, &e->d_drift_rate, N * 3); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(e->d_drift_rate, rates_n3, N * 3 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.drift_rate = e->d_drift_rate;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_get_rng_state(adc_engine *e, uint64_t *keys_n, uint32_t *ticks_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    if (keys_n) HIP_TRY(hipMemcpyAsync(keys_n, e->v.key, N * 8, hipMemcpyDeviceToHost, e->stream));
    if (ticks_n) HIP_TRY(hipMemcpyAsync(ticks_n, e->v.tick, N * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_rng_state(adc_engine *e, const uint64_t *keys_n, const uint32_t *ticks_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    if (keys_n) HIP_TRY(hipMemcpyAsync(e->v.key, keys_n, N * 8, hipMemcpyHostToDevice, e->stream));
    if (ticks_n) HIP_TRY(hipMemcpyAsync(e->v.tick, ticks_n, N * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_get_episode_state(adc_engine *e, int32_t *day_n, double *cum_profit_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    if (day_n) HIP_TRY(hipMemcpyAsync(day_n, e->v.day, N * 4, hipMemcpyDeviceToHost, e->stream));
    if (cum_profit_n) {
        if (e->v.model == ADC_MODEL_IMPLICIT) {
            std::vector<int64_t> c(N);
            HIP_TRY(hipMemcpyAsync(c.data(), e->v.cum_cents, N * 8, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            for (size_t i = 0; i < N; ++i) cum_profit_n[i] = (double)c[i] / 100.0;
        } else {
            HIP_TRY(hipMemcpyAsync(cum_profit_n, e->v.cum, N * 8, hipMemcpyDeviceToHost, e->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_episode_state(adc_engine *e, const int32_t *day_n, const double *cum_profit_n)
{
    ENGINE_GUARD(e);
    const size_t N = e->v.N;
    if (day_n) HIP_TRY(hipMemcpyAsync(e->v.day, day_n, N * 4, hipMemcpyHostToDevice, e->stream));
    if (cum_profit_n) {
        std::vector<int64_t> c(N);
        for (size_t i = 0; i < N; ++i) c[i] = (int64_t)std::llrint(cum_profit_n[i] * 100.0);
        HIP_TRY(hipMemcpyAsync(e->v.cum_cents, c.data(), N * 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->v.cum, cum_profit_n, N * 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_reset = true;
    e->last_step = 0;
    e->stream_steps = 0;
    e->env_moves += 1;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_general_model(adc_engine *e, int32_t max_bidders, float participation_rate, int32_t num_winners)
{
    ENGINE_GUARD(e);
    if (max_bidders < 0 || max_bidders > 252 || (num_winners != 1 && num_winners != 2)) return fail(ADC_EINVAL, "max_bidders must be in [0, 252] and num_winners 1 or 2");
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->v.max_bidders = max_bidders;
    e->v.participation_rate = participation_rate;
    e->v.num_winners = num_winners;
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_update_keywords(adc_engine *e)
{
    ENGINE_GUARD(e);
    if (!e->v.drift_on) return ADC_OK;        // updater_mask is None: no-op (gymnasium_kw_env.py:125-126)
    materialize_drift(e);
    hipLaunchKernelGGL(k_force_drift, dim3(e->v.N), dim3(256), 0, e->stream, e->v);     // (advances every env's tick)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    forget_replayable_steps(e);
    return ADC_OK;
}

ADC_EXPORT int adc_host_alloc(size_t bytes, void **out)
{
    if (!out) return fail(ADC_EINVAL, "out is NULL");
    *out = nullptr;
    void *p = nullptr;
    hipError_t err = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (err != hipSuccess) return fail(ADC_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(err));
    *out = p;
    return ADC_OK;
}

ADC_EXPORT void adc_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

ADC_EXPORT int adc_engine_device_buffer(adc_engine *e, int buffer_id, void **dptr, size_t *bytes)
{
    ENGINE_GUARD(e);
    if (!dptr) return fail(ADC_EINVAL, "dptr is NULL");
    const View &v = e->v;
    const size_t N = v.N, K = v.K, NK = N * K;
    void *p = nullptr;
    size_t b = 0;
    switch (buffer_id) {
    case ADC_BUF_PARAMS: p = v.params; b = ADC_P_COUNT * NK * 4; break;
    case ADC_BUF_BIDS: p = e->d_bids; b = NK * 4; break;
    case ADC_BUF_BUDGET: p = e->d_budget; b = N * 4; break;
    case ADC_BUF_IMPRESSIONS: p = v.imp; b = NK * 4; break;
    case ADC_BUF_CLICKS: p = v.clk; b = NK * 4; break;
    case ADC_BUF_CONVERSIONS: p = v.conv; b = NK * 4; break;
    case ADC_BUF_COST: p = v.cost; b = NK * 4; break;
    case ADC_BUF_REVENUE: p = v.rev; b = NK * 4; break;
    case ADC_BUF_REWARD: p = v.reward; b = N * 8; break;
    case ADC_BUF_CUM_PROFIT: p = v.cum_profit; b = N * 8; break;
    case ADC_BUF_DAYS: p = v.day_out; b = N * 4; break;
    case ADC_BUF_TERMINATED: p = v.term; b = N; break;
    case ADC_BUF_TRUNCATED: p = v.trunc; b = N; break;
    case ADC_BUF_METRIC_PROFIT: p = v.metric_profit; b = K * 8; break;
    case ADC_BUF_METRIC_SCALARS: p = v.metric_scalars; b = 8 * 8; break;
    case ADC_BUF_FLAT_OBS:
        if (!v.flat_obs) return fail(ADC_ESTATE, "flat observations are not enabled (adc_engine_flat_obs_enable)");
        p = v.flat_obs; b = N * (5 * K + 2) * 4; break;
    case ADC_BUF_ROLLOUT_ACTION: case ADC_BUF_ROLLOUT_LOGP: case ADC_BUF_ROLLOUT_VALUE: case ADC_BUF_ROLLOUT_REWARD:
    case ADC_BUF_ROLLOUT_TERMINATED: case ADC_BUF_ROLLOUT_TRUNCATED: case ADC_BUF_ROLLOUT_OBS: {
        if (e->ro_T == 0) return fail(ADC_ESTATE, "the rollout record is not enabled (adc_engine_rollout_enable)");
        const size_t tn = (size_t)e->ro_T * N;
        if (buffer_id == ADC_BUF_ROLLOUT_ACTION) { p = e->ro_action; b = tn * (size_t)e->mp.A * 4; }
        else if (buffer_id == ADC_BUF_ROLLOUT_LOGP) { p = e->ro_logp; b = tn * 4; }
        else if (buffer_id == ADC_BUF_ROLLOUT_VALUE) { p = e->ro_value; b = tn * 4; }
        else if (buffer_id == ADC_BUF_ROLLOUT_REWARD) { p = e->ro_reward; b = tn * 4; }
        else if (buffer_id == ADC_BUF_ROLLOUT_TERMINATED) { p = e->ro_term; b = tn; }
        else if (buffer_id == ADC_BUF_ROLLOUT_TRUNCATED) { p = e->ro_trunc; b = tn; }
        else {
            if (!e->ro_obs) return fail(ADC_ESTATE, "the record was enabled without ADC_ROLLOUT_OBS");
            p = e->ro_obs; b = tn * (size_t)e->mp.D * 4;
        }
        break;
    }
    default: return fail(ADC_EINVAL, "unknown buffer id");
    }
    *dptr = p;
    if (bytes) *bytes = b;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_set_env_groups(adc_engine *e, int32_t groups)
{
    ENGINE_GUARD(e);
    if (groups < 0 || groups > kMaxGroups) return fail(ADC_EINVAL, "env groups: 0 (the engine chooses) or 1..4");
    e->groups_override = groups;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_env_groups(adc_engine *e, int32_t *groups)
{
    ENGINE_GUARD(e);
    if (!groups) return fail(ADC_EINVAL, "groups is NULL");
    *groups = e->last_groups;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_stream(adc_engine *e, void **hip_stream)
{
    ENGINE_GUARD(e);
    if (!hip_stream) return fail(ADC_EINVAL, "hip_stream is NULL");
    *hip_stream = (void *)e->stream;
    e->stream_exposed = true;           // (from now on the caller may enqueue on it without telling: launch_step)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sample_actions(adc_engine *e, float bid_lo, float bid_hi, float budget)
{
    ENGINE_GUARD_STEP(e);
    return launch_chained(e, [&](const View &v, const PolicyView &, hipStream_t st, float *d_bids, float *d_budget) {
        hipLaunchKernelGGL(k_sample_actions, dim3((unsigned)((v.K + 255) / 256), (unsigned)v.N), dim3(256), 0, st, v, bid_lo, bid_hi, budget, d_bids, d_budget);
    });
}

ADC_EXPORT int adc_engine_set_flat_actions_device(adc_engine *e, const float *d_flat)
{
    ENGINE_GUARD(e);
    if (!d_flat) return fail(ADC_EINVAL, "flat action pointer is NULL");
    hipLaunchKernelGGL(k_unflatten_actions, dim3((unsigned)((e->v.K + 255) / 256), (unsigned)e->v.N), dim3(256), 0, e->stream, e->v,
                       d_flat, e->d_bids, e->d_budget);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

ADC_EXPORT int adc_engine_flat_obs_enable(adc_engine *e, int enabled)
{
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (enabled && !e->d_flat_obs) {
        int rc = dev_alloc(e, &e->d_flat_obs, (size_t)e->v.N * (5 * (size_t)e->v.K + 2));
        if (rc) return rc;
    }
    e->v.flat_obs = enabled ? e->d_flat_obs : nullptr;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_profile_enable(adc_engine *e, int enabled)
{
    ENGINE_GUARD(e);
    if (enabled && e->ev.empty()) {
        e->ev.resize((size_t)kProfileRing * kProfileMarks);
        for (auto &ev : e->ev) HIP_TRY(hipEventCreate(&ev));
    }
    e->profiling = enabled != 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_profile_sample_every(adc_engine *e, int32_t every)
{
    ENGINE_GUARD(e);
    if (every < 1) return fail(ADC_EINVAL, "profile sampling interval must be >= 1");
    e->profile_every = every;
    e->profile_tick = 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_profile_read(adc_engine *e, double *kernel_ms_total, int64_t *launches)
{
    ENGINE_GUARD(e);
    int rc = flush_profile(e);
    if (rc) return rc;
    if (kernel_ms_total) for (int j = 0; j < 3; ++j) kernel_ms_total[j] = e->prof_ms[j];
    if (launches) *launches = e->prof_launches;
    e->prof_ms[0] = e->prof_ms[1] = e->prof_ms[2] = 0.0;
    e->prof_launches = 0;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_profile_records(adc_engine *e, int64_t *event_records)
{
    ENGINE_GUARD(e);
    if (!event_records) return fail(ADC_EINVAL, "event_records is NULL");
    *event_records = e->event_records;
    return ADC_OK;
}

// GPU time of a whole region of the engine's stream with ONE event pair (nothing per step): begin records an event, end records
// another, waits for it and returns the milliseconds in between - what a caller timing K steps on the host clock can check its
// figure against (the difference is launch latency and host overhead, not kernel time)
ADC_EXPORT int adc_engine_region_begin(adc_engine *e)
{
    ENGINE_GUARD(e);
    if (!e->region_ev[0]) for (hipEvent_t &ev : e->region_ev) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipEventRecord(e->region_ev[0], e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_region_end(adc_engine *e, double *gpu_ms)
{
    ENGINE_GUARD(e);
    if (!gpu_ms) return fail(ADC_EINVAL, "gpu_ms is NULL");
    if (!e->region_ev[0]) return fail(ADC_ESTATE, "adc_engine_region_begin has not been called");
    HIP_TRY(hipEventRecord(e->region_ev[1], e->stream));
    HIP_TRY(hipEventSynchronize(e->region_ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->region_ev[0], e->region_ev[1]));
    *gpu_ms = ms;
    return ADC_OK;
}

ADC_EXPORT const char *adc_engine_step_kernel_name(adc_engine *e)
{
    if (!e) return "";
    return e->step_kernel;
}
