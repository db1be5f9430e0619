// rew_norm_api.inc - the extern "C" entry points of the running reward normaliser (include/adcraft_engine.h; the kernels are
// parts/kernel_rew_norm.inc, the law csrc/adc_rew_norm.h).  Everything here runs on the engine's own stream behind ENGINE_GUARD,
// that is after the env groups - whose streams write the record - have joined, as adc_engine_pg_advantages does.
// (part of the single translation unit adc_engine.hip)
namespace {
int rn_ready(const adc_engine *e)
{
    if (!e->have_rn)
        return fail(ADC_ESTATE, "adc_engine_rew_norm_init has not been called (or the trainer, the policy, the learners or the record were re-initialised since)");
    return ADC_OK;
}
int rn_member_check(const adc_engine *e, int32_t member)
{
    if (member < 0 || member >= e->rn_M) return fail(ADC_EINVAL, "no such normaliser: 0 for the shared one, a member with per-member normalisers");
    return ADC_OK;
}
inline unsigned rn_blocks(long long lanes) { return (unsigned)((lanes + kRewNormBlock - 1) / kRewNormBlock); }
}  // namespace

ADC_EXPORT int adc_engine_rew_norm_init(adc_engine *e, const adc_rew_norm_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_rew_norm_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (e->have_td3 || e->have_td3_pop)
        return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: its reward enters at the TD3 target, not through GAE");
    if (!e->have_pg && !e->have_pg_pop)
        return fail(ADC_ESTATE, "the reward normaliser discounts by a PPO / A2C trainer's gamma: adc_engine_pg_init or adc_engine_pg_pop_init first");
    const bool per_member = cfg->per_member != 0;
    if (per_member && !e->have_pg_pop) return fail(ADC_ESTATE, "per-member normalisers need a learner population (adc_engine_pg_pop_init)");
    const size_t N = (size_t)e->v.N, Mn = per_member ? (size_t)e->lrn_M : 1u, n = N / Mn;
    const size_t chunks = (size_t)pg_chunks((long long)e->ro_T * (long long)n);
    ENGINE_GUARD(e);
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    RewNormView p{};
    double *g = nullptr, *part = nullptr;
    int32_t *src = nullptr;
    int rc;
    if ((rc = mlp_alloc(e, fresh, &p.count, Mn)) || (rc = mlp_alloc(e, fresh, &p.mean, Mn)) || (rc = mlp_alloc(e, fresh, &p.m2, Mn)) ||
        (rc = mlp_alloc(e, fresh, &p.scale, Mn)) || (rc = mlp_alloc(e, fresh, &p.G, N)) || (rc = mlp_alloc(e, fresh, &g, (size_t)e->ro_T * N)) ||
        (rc = mlp_alloc(e, fresh, &part, Mn * chunks * 2u)) || (rc = mlp_alloc(e, fresh, &src, Mn))) {
        mlp_free(e, fresh);
        return rc;
    }
    const std::vector<float> ones(Mn, 1.0f);
    HIP_TRY(hipMemcpyAsync(p.scale, ones.data(), Mn * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    rew_norm_drop(e);
    e->rn_allocs.swap(fresh);
    e->rn_view = p;
    e->rn_g = g; e->rn_part = part; e->rn_src = src;
    e->rn_cfg = *cfg;
    e->rn_M = (int)Mn;
    e->rn_t0 = 0;                       // (a normaliser set up over a record already begun consumes it from its first day)
    e->have_rn = true;
    e->pg_adv_ready = false;            // (advantages computed without the multiplier are stale)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_update(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = rn_ready(e)) return rc;
    if (e->ro_T == 0) return fail(ADC_ESTATE, "the reward normaliser is fed from the rollout record (adc_engine_rollout_enable)");
    if (e->ro_t <= e->rn_t0) return fail(ADC_ESTATE, "no day has been recorded since the last update or adc_engine_rollout_reset");
    const int N = e->v.N, Mn = e->rn_M, n = N / Mn, t0 = e->rn_t0, T = e->ro_t;
    const long long S = (long long)(T - t0) * n;
    const int chunks = (int)pg_chunks(S);
    ENGINE_GUARD(e);
    const bool pop = e->have_pg_pop;
    hipLaunchKernelGGL(k_rew_norm_scan, dim3(rn_blocks(N)), dim3(kRewNormBlock), 0, e->stream, N, n, t0, T, e->ro_reward, e->ro_term, e->ro_trunc,
                       pop ? 0.0f : e->pg_cfg.gamma, pop ? e->pgp_dmem : nullptr, pop ? e->lrn_n : N, e->rn_view.G, e->rn_g);
    hipLaunchKernelGGL(k_rew_norm_chunk_sums, dim3(rn_blocks(chunks), (unsigned)Mn), dim3(kRewNormBlock), 0, e->stream, e->rn_g, S, chunks, e->rn_part);
    hipLaunchKernelGGL(k_rew_norm_finish, dim3(rn_blocks(Mn)), dim3(kRewNormBlock), 0, e->stream, e->rn_view, Mn,
                       adc::NormConfig{e->rn_cfg.min_std, e->rn_cfg.count_cap}, e->rn_part, chunks, S);
    HIP_TRY(hipGetLastError());
    e->rn_t0 = T;
    e->pg_adv_ready = false;            // (advantages computed under the old multiplier are stale)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_state_get(adc_engine *e, int32_t member, int64_t *count, double *mean, double *m2, float *scale)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = rn_ready(e)) || (rc = rn_member_check(e, member))) return rc;
    ENGINE_GUARD(e);
    const RewNormView &p = e->rn_view;
    if (count) HIP_TRY(hipMemcpyAsync(count, p.count + member, 8, hipMemcpyDeviceToHost, e->stream));
    if (mean) HIP_TRY(hipMemcpyAsync(mean, p.mean + member, 8, hipMemcpyDeviceToHost, e->stream));
    if (m2) HIP_TRY(hipMemcpyAsync(m2, p.m2 + member, 8, hipMemcpyDeviceToHost, e->stream));
    if (scale) HIP_TRY(hipMemcpyAsync(scale, p.scale + member, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_state_set(adc_engine *e, int32_t member, int64_t count, double mean, double m2, float scale)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = rn_ready(e)) || (rc = rn_member_check(e, member))) return rc;
    if (count < 0) return fail(ADC_EINVAL, "count >= 0");
    if (!(scale > 0.0f && scale < __builtin_inff())) return fail(ADC_EINVAL, "scale must be finite and > 0");
    ENGINE_GUARD(e);
    const RewNormView &p = e->rn_view;
    HIP_TRY(hipMemcpyAsync(p.count + member, &count, 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.mean + member, &mean, 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.m2 + member, &m2, 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.scale + member, &scale, 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));       // (the arguments are this frame's until here)
    e->pg_adv_ready = false;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_returns_get(adc_engine *e, double *g_n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = rn_ready(e)) return rc;
    if (!g_n) return fail(ADC_EINVAL, "g_n is NULL");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(g_n, e->rn_view.G, (size_t)e->v.N * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_returns_set(adc_engine *e, const double *g_n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = rn_ready(e)) return rc;
    if (!g_n) return fail(ADC_EINVAL, "g_n is NULL");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(e->rn_view.G, g_n, (size_t)e->v.N * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_copy(adc_engine *e, const int32_t *src_of_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = rn_ready(e)) return rc;
    if (!e->rn_cfg.per_member) return fail(ADC_ESTATE, "the normaliser is shared by all envs: there are no members to copy between");
    if (!src_of_m) return fail(ADC_EINVAL, "src_of_m is NULL");
    const int M = e->rn_M;
    for (int m = 0; m < M; ++m)
        if (src_of_m[m] < -1 || src_of_m[m] >= M) return fail(ADC_EINVAL, "src_of_m: a member, or the member itself / -1 to keep it");
    for (int m = 0; m < M; ++m) {
        const int s = src_of_m[m];
        if (s == -1 || s == m) continue;
        if (src_of_m[s] != -1 && src_of_m[s] != s) return fail(ADC_EINVAL, "a destination is also a source: the copies of a round may not chain");
    }
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(e->rn_src, src_of_m, (size_t)M * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_rew_norm_copy, dim3(rn_blocks(M)), dim3(kRewNormBlock), 0, e->stream, e->rn_view, M, e->rn_src);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));       // (src_of_m is the caller's until here)
    e->pg_adv_ready = false;
    return ADC_OK;
}
