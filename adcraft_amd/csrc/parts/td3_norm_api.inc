// td3_norm_api.inc - the extern "C" entry points of the TD3 learners' running observation and reward normalisers
// (include/adcraft_engine.h; the kernels are parts/kernel_td3_norm.inc and the chunked sums of kernel_obs_norm.inc /
// kernel_rew_norm.inc, the law csrc/adc_td3_norm.h).  Everything here runs on the engine's own stream behind ENGINE_GUARD, that is
// after the env groups - whose streams write the record - have joined, as adc_engine_td3_store does.
// (part of the single translation unit adc_engine.hip)
namespace {
int tn_ready(const adc_engine *e)
{
    if (!e->have_tn)
        return fail(ADC_ESTATE, "adc_engine_td3_norm_init has not been called (or the TD3 trainer, the policy, the learners or the record were re-initialised since)");
    return ADC_OK;
}
int tn_member_check(const adc_engine *e, int32_t member)
{
    if (member < 0 || member >= e->tn_M) return fail(ADC_EINVAL, "no such normaliser: 0 for the shared one, a member with per-member normalisers");
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_td3_norm_init(adc_engine *e, const adc_td3_norm_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_td3_norm_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (!e->have_td3 && !e->have_td3_pop)
        return fail(ADC_ESTATE, "the TD3 normalisers belong to an off-policy trainer: adc_engine_td3_init or adc_engine_td3_pop_init first");
    const bool pop = e->have_td3_pop, per_member = cfg->per_member != 0, obs = cfg->observations != 0, rew = cfg->rewards != 0;
    if (int rc = pop ? tp_state_check(e) : td3_state_check(e)) return rc;
    if (per_member && !pop) return fail(ADC_EINVAL, "per-member normalisers need a TD3 learner population (adc_engine_td3_pop_init)");
    if (obs && !(e->have_tn ? (e->tn_shared_shift ? e->tn_shared_shift : e->mp.shift) : e->mp.shift))
        return fail(ADC_EINVAL, "the policy was initialised without normalisation");
    if (e->ro_t != 0 || e->td3_written != 0)
        return fail(ADC_ESTATE, "the record and the replay ring must be empty: their rows were written as network inputs (adc_engine_rollout_reset, and "
                                "adc_engine_td3_norm_init before the first store)");
    const size_t N = (size_t)e->v.N, D = (size_t)e->mp.D, Mn = per_member ? (size_t)e->lrn_M : 1u, n = N / Mn;
    const size_t chunks = (size_t)pg_chunks((long long)e->ro_T * (long long)n);
    if (chunks > 65535) return fail(ADC_EINVAL, "days x envs of a normaliser: at most 65535 x 1024 samples in an update");
    ENGINE_GUARD(e);
    td3_norm_drop(e);                   // (a second init starts over from the policy's own vectors)
    std::vector<void *> fresh;
    ObsNormView on{};
    RewNormView rn{};
    double *on_part = nullptr, *g = nullptr, *rn_part = nullptr;
    int32_t *src = nullptr;
    int rc = mlp_alloc(e, fresh, &src, Mn);
    if (!rc && obs) {
        on.D = (int)D;
        if ((rc = mlp_alloc(e, fresh, &on.count, Mn * D)) || (rc = mlp_alloc(e, fresh, &on.mean, Mn * D)) || (rc = mlp_alloc(e, fresh, &on.m2, Mn * D)) ||
            (rc = mlp_alloc(e, fresh, &on_part, Mn * chunks * 2u * D)) ||
            (per_member && ((rc = mlp_alloc(e, fresh, &on.shift, Mn * D)) || (rc = mlp_alloc(e, fresh, &on.scale, Mn * D))))) {}
    }
    if (!rc && rew) {
        if ((rc = mlp_alloc(e, fresh, &rn.count, Mn)) || (rc = mlp_alloc(e, fresh, &rn.mean, Mn)) || (rc = mlp_alloc(e, fresh, &rn.m2, Mn)) ||
            (rc = mlp_alloc(e, fresh, &rn.scale, Mn)) || (rc = mlp_alloc(e, fresh, &rn.G, N)) || (rc = mlp_alloc(e, fresh, &g, (size_t)e->ro_T * N)) ||
            (rc = mlp_alloc(e, fresh, &rn_part, Mn * chunks * 2u))) {}
    }
    if (rc) { mlp_free(e, fresh); return rc; }
    hipError_t err = hipSuccess;
    if (rew) {
        const std::vector<float> ones(Mn, 1.0f);
        err = hipMemcpyAsync(rn.scale, ones.data(), Mn * 4, hipMemcpyHostToDevice, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    }
    if (err == hipSuccess && obs && per_member) {
        // every member's vectors start as the shared ones
        for (size_t m = 0; m < Mn && err == hipSuccess; ++m) {
            err = hipMemcpyAsync(on.shift + m * D, e->mp.shift, D * 4, hipMemcpyDeviceToDevice, e->stream);
            if (err == hipSuccess) err = hipMemcpyAsync(on.scale + m * D, e->mp.scale, D * 4, hipMemcpyDeviceToDevice, e->stream);
        }
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    }
    if (err != hipSuccess) { mlp_free(e, fresh); HIP_TRY(err); }
    e->tn_allocs.swap(fresh);
    if (obs && per_member) {
        // (the learned agent's days are launched kernel by kernel, never from a captured graph, so the next act reads the view below)
        e->tn_shared_shift = e->mp.shift; e->tn_shared_scale = e->mp.scale;
        e->mp.shift = on.shift; e->mp.scale = on.scale; e->mp.norm_stride = D;
    } else if (obs) {
        on.shift = const_cast<float *>(e->mp.shift);
        on.scale = const_cast<float *>(e->mp.scale);
    }
    e->tn_on = on; e->tn_rn = rn;
    e->tn_on_part = on_part; e->tn_g = g; e->tn_rn_part = rn_part; e->tn_src = src;
    e->tn_cfg = *cfg;
    e->tn_M = (int)Mn;
    e->tn_t0 = 0;
    e->tn_raw = obs;
    e->have_tn = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_norm_update(adc_engine *e, int64_t *samples)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = tn_ready(e)) return rc;
    if (e->ro_t <= e->tn_t0) return fail(ADC_ESTATE, "no day has been recorded since the last update or adc_engine_rollout_reset");
    const int N = e->v.N, Mn = e->tn_M, n = N / Mn, D = e->mp.D, t0 = e->tn_t0, T = e->ro_t;
    const long long S = (long long)(T - t0) * n;
    const int chunks = (int)pg_chunks(S);
    ENGINE_GUARD(e);
    if (e->tn_on.count) {
        const unsigned tiles = (unsigned)((D + kObsNormBlock - 1) / kObsNormBlock);
        hipLaunchKernelGGL(k_obs_norm_chunk_sums, dim3(tiles, (unsigned)chunks, (unsigned)Mn), dim3(kObsNormBlock), 0, e->stream, e->ro_obs, D, N, n, t0, S,
                           e->tn_on_part);
        hipLaunchKernelGGL(k_td3_norm_obs_finish, dim3(tiles, (unsigned)Mn), dim3(kObsNormBlock), 0, e->stream, e->tn_on,
                           adc::NormConfig{e->tn_cfg.obs_min_std, e->tn_cfg.obs_count_cap}, e->tn_on_part, chunks, S);
        HIP_TRY(hipGetLastError());
    }
    if (e->tn_rn.count) {
        const bool pop = e->have_td3_pop;
        const unsigned blocks = (unsigned)((N + kRewNormBlock - 1) / kRewNormBlock);
        hipLaunchKernelGGL(k_td3_norm_scan, dim3(blocks), dim3(kRewNormBlock), 0, e->stream, N, n, t0, T, e->ro_reward, e->ro_term, e->ro_trunc,
                           pop ? 0.0f : e->td3_cfg.gamma, pop ? e->tp_dmem : nullptr, pop ? e->lrn_n : N, e->tn_rn.G, e->tn_g);
        hipLaunchKernelGGL(k_rew_norm_chunk_sums, dim3((unsigned)((chunks + kRewNormBlock - 1) / kRewNormBlock), (unsigned)Mn), dim3(kRewNormBlock), 0, e->stream,
                           e->tn_g, S, chunks, e->tn_rn_part);
        hipLaunchKernelGGL(k_rew_norm_finish, dim3((unsigned)((Mn + kRewNormBlock - 1) / kRewNormBlock)), dim3(kRewNormBlock), 0, e->stream, e->tn_rn, Mn,
                           adc::NormConfig{e->tn_cfg.rew_min_std, e->tn_cfg.rew_count_cap}, e->tn_rn_part, chunks, S);
    }
    HIP_TRY(hipGetLastError());
    e->tn_t0 = T;
    if (samples) *samples = S;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_norm_state_get(adc_engine *e, int32_t member, int64_t *obs_count, double *obs_mean_d, double *obs_m2_d, float *shift_d,
                                             float *scale_d, int64_t *rew_count, double *rew_mean, double *rew_m2, float *rew_scale)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tn_ready(e)) || (rc = tn_member_check(e, member))) return rc;
    if (!e->tn_on.count && (obs_count || obs_mean_d || obs_m2_d || shift_d || scale_d))
        return fail(ADC_ESTATE, "the normaliser was initialised without observations");
    if (!e->tn_rn.count && (rew_count || rew_mean || rew_m2 || rew_scale)) return fail(ADC_ESTATE, "the normaliser was initialised without rewards");
    ENGINE_GUARD(e);
    const ObsNormView &p = e->tn_on;
    const RewNormView &r = e->tn_rn;
    const size_t D = (size_t)e->mp.D, at = (size_t)member * D;
    if (obs_count) HIP_TRY(hipMemcpyAsync(obs_count, p.count + at, 8, hipMemcpyDeviceToHost, e->stream));
    if (obs_mean_d) HIP_TRY(hipMemcpyAsync(obs_mean_d, p.mean + at, D * 8, hipMemcpyDeviceToHost, e->stream));
    if (obs_m2_d) HIP_TRY(hipMemcpyAsync(obs_m2_d, p.m2 + at, D * 8, hipMemcpyDeviceToHost, e->stream));
    if (shift_d) HIP_TRY(hipMemcpyAsync(shift_d, p.shift + at, D * 4, hipMemcpyDeviceToHost, e->stream));
    if (scale_d) HIP_TRY(hipMemcpyAsync(scale_d, p.scale + at, D * 4, hipMemcpyDeviceToHost, e->stream));
    if (rew_count) HIP_TRY(hipMemcpyAsync(rew_count, r.count + member, 8, hipMemcpyDeviceToHost, e->stream));
    if (rew_mean) HIP_TRY(hipMemcpyAsync(rew_mean, r.mean + member, 8, hipMemcpyDeviceToHost, e->stream));
    if (rew_m2) HIP_TRY(hipMemcpyAsync(rew_m2, r.m2 + member, 8, hipMemcpyDeviceToHost, e->stream));
    if (rew_scale) HIP_TRY(hipMemcpyAsync(rew_scale, r.scale + member, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_norm_state_set(adc_engine *e, int32_t member, int64_t obs_count, const double *obs_mean_d, const double *obs_m2_d,
                                             const float *shift_d, const float *scale_d, int64_t rew_count, double rew_mean, double rew_m2, float rew_scale)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tn_ready(e)) || (rc = tn_member_check(e, member))) return rc;
    const ObsNormView &p = e->tn_on;
    const RewNormView &r = e->tn_rn;
    const size_t D = (size_t)e->mp.D, at = (size_t)member * D;
    if (p.count) {
        if (!obs_mean_d || !obs_m2_d || !shift_d || !scale_d) return fail(ADC_EINVAL, "mean, M2, shift or scale is NULL");
        if (obs_count < 0) return fail(ADC_EINVAL, "count >= 0");
        const double inf = (double)__builtin_inff();
        for (size_t j = 0; j < D; ++j) {
            if (!(scale_d[j] > 0.0f && scale_d[j] < __builtin_inff())) return fail(ADC_EINVAL, "scale must be finite and > 0");
            if (!(shift_d[j] > -__builtin_inff() && shift_d[j] < __builtin_inff()) || !(obs_mean_d[j] > -inf && obs_mean_d[j] < inf))
                return fail(ADC_EINVAL, "shift and mean must be finite");
            if (!(obs_m2_d[j] >= 0.0 && obs_m2_d[j] < inf)) return fail(ADC_EINVAL, "M2 must be finite and >= 0");
        }
    }
    if (r.count) {
        if (rew_count < 0) return fail(ADC_EINVAL, "count >= 0");
        if (!(rew_scale > 0.0f && rew_scale < __builtin_inff())) return fail(ADC_EINVAL, "scale must be finite and > 0");
        const double inf = (double)__builtin_inff();
        if (!(rew_mean > -inf && rew_mean < inf)) return fail(ADC_EINVAL, "shift and mean must be finite");
        if (!(rew_m2 >= 0.0 && rew_m2 < inf)) return fail(ADC_EINVAL, "M2 must be finite and >= 0");
    }
    ENGINE_GUARD(e);
    const std::vector<int64_t> counts(D, obs_count);
    if (p.count) {
        HIP_TRY(hipMemcpyAsync(p.count + at, counts.data(), D * 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(p.mean + at, obs_mean_d, D * 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(p.m2 + at, obs_m2_d, D * 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(p.shift + at, shift_d, D * 4, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(p.scale + at, scale_d, D * 4, hipMemcpyHostToDevice, e->stream));
    }
    if (r.count) {
        HIP_TRY(hipMemcpyAsync(r.count + member, &rew_count, 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(r.mean + member, &rew_mean, 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(r.m2 + member, &rew_m2, 8, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(r.scale + member, &rew_scale, 4, hipMemcpyHostToDevice, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));       // (the arguments are this frame's until here)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_norm_returns_get(adc_engine *e, double *g_n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = tn_ready(e)) return rc;
    if (!e->tn_rn.G) return fail(ADC_ESTATE, "the normaliser was initialised without rewards");
    if (!g_n) return fail(ADC_EINVAL, "g_n is NULL");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(g_n, e->tn_rn.G, (size_t)e->v.N * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_norm_returns_set(adc_engine *e, const double *g_n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = tn_ready(e)) return rc;
    if (!e->tn_rn.G) return fail(ADC_ESTATE, "the normaliser was initialised without rewards");
    if (!g_n) return fail(ADC_EINVAL, "g_n is NULL");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(e->tn_rn.G, g_n, (size_t)e->v.N * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_norm_copy(adc_engine *e, const int32_t *src_of_member_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = tn_ready(e)) return rc;
    if (!e->tn_cfg.per_member) return fail(ADC_ESTATE, "the normaliser is shared by all envs: there are no members to copy between");
    if (!src_of_member_m) return fail(ADC_EINVAL, "src_of_member_m is NULL");
    const int M = e->tn_M;
    for (int m = 0; m < M; ++m)
        if (src_of_member_m[m] < -1 || src_of_member_m[m] >= M) return fail(ADC_EINVAL, "src_of_member_m: a member, or the member itself / -1 to keep it");
    for (int m = 0; m < M; ++m) {
        const int s = src_of_member_m[m];
        if (s == -1 || s == m) continue;
        if (src_of_member_m[s] != -1 && src_of_member_m[s] != s) return fail(ADC_EINVAL, "a destination is also a source: the copies of a round may not chain");
    }
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(e->tn_src, src_of_member_m, (size_t)M * 4, hipMemcpyHostToDevice, e->stream));
    const int cols = e->tn_on.count ? e->tn_on.D : 1;
    hipLaunchKernelGGL(k_td3_norm_copy, dim3((unsigned)((cols + kObsNormBlock - 1) / kObsNormBlock), (unsigned)M), dim3(kObsNormBlock), 0, e->stream, e->tn_on,
                       e->tn_rn, e->tn_src);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));       // (src_of_member_m is the caller's until here)
    return ADC_OK;
}
