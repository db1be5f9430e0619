// obs_norm_api.inc - the extern "C" entry points of the running observation normaliser (include/adcraft_engine.h; the kernels
// are parts/kernel_obs_norm.inc, the law csrc/adc_norm.h).  Everything here runs on the engine's own stream behind ENGINE_GUARD,
// that is after the env groups - whose streams write the record - have joined, as adc_engine_pg_advantages does.
// (part of the single translation unit adc_engine.hip)
namespace {
int on_ready(const adc_engine *e)
{
    if (!e->have_on)
        return fail(ADC_ESTATE, "adc_engine_obs_norm_init has not been called (or the policy, the learners or the record were re-initialised since)");
    return ADC_OK;
}
int on_member_check(const adc_engine *e, int32_t member)
{
    if (member < 0 || member >= e->on_M) return fail(ADC_EINVAL, "no such normaliser: 0 for the shared one, a member with per-member normalisers");
    return ADC_OK;
}
inline unsigned on_tiles(int D) { return (unsigned)((D + kObsNormBlock - 1) / kObsNormBlock); }
}  // namespace

ADC_EXPORT int adc_engine_obs_norm_init(adc_engine *e, const adc_obs_norm_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_obs_norm_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (int rc = mlp_ready(e)) return rc;
    if (!e->mp.shift) return fail(ADC_EINVAL, "the policy was initialised without normalisation");
    const bool per_member = cfg->per_member != 0;
    if (per_member && e->lrn_M == 0) return fail(ADC_ESTATE, "per-member normalisers need learners (adc_engine_mlp_learners)");
    if (e->have_td3 || e->have_td3_pop)
        return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: its ring holds inputs normalised by older vectors");
    ENGINE_GUARD(e);
    // (a second init starts over from the policy's own vectors; the days its predecessor consumed were collected under other
    //  vectors than those and are not consumed again)
    const int t0 = e->have_on ? e->ro_t : 0;
    obs_norm_drop(e);
    const size_t D = (size_t)e->mp.D, Mn = per_member ? (size_t)e->lrn_M : 1u;
    // the vectors in force: they must be usable as a scale (the law divides by them)
    std::vector<float> shift(D), scale(D);
    HIP_TRY(hipMemcpyAsync(shift.data(), e->mp.shift, D * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(scale.data(), e->mp.scale, D * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t j = 0; j < D; ++j)
        if (!(scale[j] > 0.0f && scale[j] < __builtin_inff()))
            return fail(ADC_EINVAL, "the current scale vector holds a value that is not finite or not > 0 (adc_engine_mlp_set_norm)");
    std::vector<void *> fresh;
    ObsNormView p{};
    p.D = (int)D;
    int32_t *src = nullptr;
    int rc;
    if ((rc = mlp_alloc(e, fresh, &p.count, Mn * D)) || (rc = mlp_alloc(e, fresh, &p.mean, Mn * D)) || (rc = mlp_alloc(e, fresh, &p.m2, Mn * D)) ||
        (rc = mlp_alloc(e, fresh, &src, Mn)) ||
        (per_member && ((rc = mlp_alloc(e, fresh, &p.shift, Mn * D)) || (rc = mlp_alloc(e, fresh, &p.scale, Mn * D))))) {
        mlp_free(e, fresh);
        return rc;
    }
    if (per_member) {
        // every member's vectors start as the shared ones
        for (size_t m = 0; m < Mn; ++m) {
            HIP_TRY(hipMemcpyAsync(p.shift + m * D, shift.data(), D * 4, hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipMemcpyAsync(p.scale + m * D, scale.data(), D * 4, hipMemcpyHostToDevice, e->stream));
        }
        HIP_TRY(hipStreamSynchronize(e->stream));
    } else {
        p.shift = const_cast<float *>(e->mp.shift);
        p.scale = const_cast<float *>(e->mp.scale);
    }
    e->on_allocs.swap(fresh);
    e->on_shared_shift = e->mp.shift; e->on_shared_scale = e->mp.scale;
    // (the learned agent's days are launched kernel by kernel, never from a captured graph - adc_engine_run_days - so no graph
    //  holds the old kernel arguments: the next act reads the view below)
    if (per_member) { e->mp.shift = p.shift; e->mp.scale = p.scale; e->mp.norm_stride = D; }
    e->on_view = p;
    e->on_src = src;
    e->on_cfg = *cfg;
    e->on_M = (int)Mn;
    e->on_t0 = t0;
    e->have_on = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_obs_norm_update(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = on_ready(e)) return rc;
    if (e->ro_T == 0) return fail(ADC_ESTATE, "the observation normaliser is fed from the rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "the observation normaliser needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    if (e->ro_t <= e->on_t0) return fail(ADC_ESTATE, "no day has been recorded since the last update or adc_engine_rollout_reset");
    const int N = e->v.N, Mn = e->on_M, n = N / Mn, D = e->mp.D;
    const long long S = (long long)(e->ro_t - e->on_t0) * n, chunks = pg_chunks(S);
    if (chunks > 65535) return fail(ADC_EINVAL, "days x envs of a normaliser: at most 65535 x 1024 samples in an update");
    ENGINE_GUARD(e);
    const size_t need = (size_t)Mn * (size_t)chunks * 2u * (size_t)D;
    if (need > e->on_part_doubles) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->on_part) { (void)hipFree(e->on_part); e->on_part = nullptr; e->on_part_doubles = 0; }
        void *q = nullptr;
        if (hipMalloc(&q, need * 8) != hipSuccess) { (void)hipGetLastError(); return fail(ADC_ENOMEM, "hipMalloc failed (observation normaliser)"); }
        e->on_part = static_cast<double *>(q);
        e->on_part_doubles = need;
    }
    hipLaunchKernelGGL(k_obs_norm_chunk_sums, dim3(on_tiles(D), (unsigned)chunks, (unsigned)Mn), dim3(kObsNormBlock), 0, e->stream, e->ro_obs, D, N, n, e->on_t0, S,
                       e->on_part);
    hipLaunchKernelGGL(k_obs_norm_finish, dim3(on_tiles(D), (unsigned)Mn), dim3(kObsNormBlock), 0, e->stream, e->on_view,
                       adc::NormConfig{e->on_cfg.min_std, e->on_cfg.count_cap}, e->on_part, (int)chunks, S);
    HIP_TRY(hipGetLastError());
    e->on_t0 = e->ro_t;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_obs_norm_state_get(adc_engine *e, int32_t member, int64_t *count, double *mean_d, double *m2_d, float *shift_d, float *scale_d)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = on_ready(e)) || (rc = on_member_check(e, member))) return rc;
    ENGINE_GUARD(e);
    const ObsNormView &p = e->on_view;
    const size_t D = (size_t)p.D, at = (size_t)member * D;
    if (count) HIP_TRY(hipMemcpyAsync(count, p.count + at, 8, hipMemcpyDeviceToHost, e->stream));
    if (mean_d) HIP_TRY(hipMemcpyAsync(mean_d, p.mean + at, D * 8, hipMemcpyDeviceToHost, e->stream));
    if (m2_d) HIP_TRY(hipMemcpyAsync(m2_d, p.m2 + at, D * 8, hipMemcpyDeviceToHost, e->stream));
    if (shift_d) HIP_TRY(hipMemcpyAsync(shift_d, p.shift + at, D * 4, hipMemcpyDeviceToHost, e->stream));
    if (scale_d) HIP_TRY(hipMemcpyAsync(scale_d, p.scale + at, D * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_obs_norm_state_set(adc_engine *e, int32_t member, int64_t count, const double *mean_d, const double *m2_d, const float *shift_d,
                                             const float *scale_d)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = on_ready(e)) || (rc = on_member_check(e, member))) return rc;
    if (!mean_d || !m2_d || !shift_d || !scale_d) return fail(ADC_EINVAL, "mean, M2, shift or scale is NULL");
    if (count < 0) return fail(ADC_EINVAL, "count >= 0");
    const ObsNormView &p = e->on_view;
    const size_t D = (size_t)p.D, at = (size_t)member * D;
    for (size_t j = 0; j < D; ++j)
        if (!(scale_d[j] > 0.0f && scale_d[j] < __builtin_inff())) return fail(ADC_EINVAL, "scale must be finite and > 0");
    ENGINE_GUARD(e);
    const std::vector<int64_t> counts(D, count);
    HIP_TRY(hipMemcpyAsync(p.count + at, counts.data(), D * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.mean + at, mean_d, D * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.m2 + at, m2_d, D * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.shift + at, shift_d, D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.scale + at, scale_d, D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_obs_norm_copy(adc_engine *e, const int32_t *src_of_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = on_ready(e)) return rc;
    if (!e->on_cfg.per_member) return fail(ADC_ESTATE, "the normaliser is shared by all envs: there are no members to copy between");
    if (!src_of_m) return fail(ADC_EINVAL, "src_of_m is NULL");
    const int M = e->on_M;
    for (int m = 0; m < M; ++m)
        if (src_of_m[m] < -1 || src_of_m[m] >= M) return fail(ADC_EINVAL, "src_of_m: a member, or the member itself / -1 to keep it");
    for (int m = 0; m < M; ++m) {
        const int s = src_of_m[m];
        if (s == -1 || s == m) continue;
        if (src_of_m[s] != -1 && src_of_m[s] != s) return fail(ADC_EINVAL, "a destination is also a source: the copies of a round may not chain");
    }
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(e->on_src, src_of_m, (size_t)M * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_obs_norm_copy, dim3(on_tiles(e->on_view.D), (unsigned)M), dim3(kObsNormBlock), 0, e->stream, e->on_view, e->on_src);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));       // (src_of_m is the caller's until here)
    return ADC_OK;
}
