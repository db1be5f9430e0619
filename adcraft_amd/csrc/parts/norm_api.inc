// norm_api.inc - the extern "C" entry points of the running normalisers (include/adcraft_engine.h): the observation normaliser and
// the reward normaliser of the PPO / A2C learners, each a thin front end with its own preconditions and config, and the normalisers of
// the TD3 learners and of the SAC learners, two families of a third; all over one set of helpers that work on a NormSet (host_api.inc).  The kernels are
// parts/kernel_norm.inc, the laws csrc/adc_norm.h, adc_rew_norm.h, adc_td3_norm.h and adc_sac_norm.h.  Everything here runs on the engine's own stream behind ENGINE_GUARD,
// that is after the env groups - whose streams write the record - have joined, as adc_engine_pg_advantages and adc_engine_td3_store do.
// (part of the single translation unit adc_engine.hip)
namespace {
int norm_ready(const NormSet &s, const char *why_not)
{
    if (!s.live) return fail(ADC_ESTATE, why_not);
    return ADC_OK;
}
int norm_member_check(const NormSet &s, int32_t member)
{
    if (member < 0 || member >= s.M) return fail(ADC_EINVAL, "no such normaliser: 0 for the shared one, a member with per-member normalisers");
    return ADC_OK;
}
inline unsigned norm_blocks(long long lanes, int block) { return (unsigned)((lanes + block - 1) / block); }

// the observation part of s.M normalisers: the running moments, and - per_member - a row of vectors per member
int norm_alloc_obs(adc_engine *e, NormSet &s, bool per_member)
{
    const size_t D = (size_t)e->mp.D, MD = (size_t)s.M * D;
    s.obs.D = (int)D;
    int rc;
    if ((rc = mlp_alloc(e, s.allocs, &s.obs.count, MD)) || (rc = mlp_alloc(e, s.allocs, &s.obs.mean, MD)) || (rc = mlp_alloc(e, s.allocs, &s.obs.m2, MD)) ||
        (per_member && ((rc = mlp_alloc(e, s.allocs, &s.obs.shift, MD)) || (rc = mlp_alloc(e, s.allocs, &s.obs.scale, MD)))))
        return rc;
    return ADC_OK;
}
// the reward part of s.M normalisers: the running moments, the multiplier (it starts at 1), the envs' carry, and the scratch of an
// update over at most the whole record
int norm_alloc_rew(adc_engine *e, NormSet &s)
{
    const size_t N = (size_t)e->v.N, Mn = (size_t)s.M, chunks = (size_t)pg_chunks((long long)e->ro_T * (long long)(N / Mn));
    int rc;
    if ((rc = mlp_alloc(e, s.allocs, &s.rew.count, Mn)) || (rc = mlp_alloc(e, s.allocs, &s.rew.mean, Mn)) || (rc = mlp_alloc(e, s.allocs, &s.rew.m2, Mn)) ||
        (rc = mlp_alloc(e, s.allocs, &s.rew.scale, Mn)) || (rc = mlp_alloc(e, s.allocs, &s.rew.G, N)) || (rc = mlp_alloc(e, s.allocs, &s.g, (size_t)e->ro_T * N)) ||
        (rc = mlp_alloc(e, s.allocs, &s.rew_part, Mn * chunks * 2u)))
        return rc;
    const std::vector<float> ones(Mn, 1.0f);
    HIP_TRY(hipMemcpyAsync(s.rew.scale, ones.data(), Mn * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
// the vectors the observation part writes: the policy's own, or - per_member - every member's row, which starts as the policy's and is
// installed where the policy kernel reads.  The last step of an init: nothing fails after the engine has changed
int norm_install_vectors(adc_engine *e, NormSet &s, bool per_member)
{
    if (!per_member) {
        s.obs.shift = const_cast<float *>(e->mp.shift);
        s.obs.scale = const_cast<float *>(e->mp.scale);
        return ADC_OK;
    }
    const size_t D = (size_t)s.obs.D;
    for (size_t m = 0; m < (size_t)s.M; ++m) {
        HIP_TRY(hipMemcpyAsync(s.obs.shift + m * D, e->mp.shift, D * 4, hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(s.obs.scale + m * D, e->mp.scale, D * 4, hipMemcpyDeviceToDevice, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    // (the learned agent's days are launched kernel by kernel, never from a captured graph - adc_engine_run_days - so no graph
    //  holds the old kernel arguments: the next act reads the view below)
    s.shared_shift = e->mp.shift; s.shared_scale = e->mp.scale;
    e->mp.shift = s.obs.shift; e->mp.scale = s.obs.scale; e->mp.norm_stride = D;
    return ADC_OK;
}

// the recorded days [s.t0, ro_t) not yet consumed: n envs and S samples per normaliser, in `chunks` chunks
struct NormBatch {
    int N, n, t0, T;
    long long S, chunks;
};
NormBatch norm_batch(const adc_engine *e, const NormSet &s)
{
    NormBatch b;
    b.N = e->v.N; b.n = b.N / s.M; b.t0 = s.t0; b.T = e->ro_t;
    b.S = (long long)(b.T - b.t0) * b.n;
    b.chunks = pg_chunks(b.S);
    return b;
}
// the observation part's update: the record's batch moments into s.obs_part, the merge, the new vectors; raw: the record holds raw rows
int norm_update_obs(adc_engine *e, const NormSet &s, const NormBatch &b, const adc::NormConfig &c, bool raw)
{
    const int D = e->mp.D;
    const unsigned tiles = norm_blocks(D, kObsNormBlock);
    hipLaunchKernelGGL(k_obs_norm_chunk_sums, dim3(tiles, (unsigned)b.chunks, (unsigned)s.M), dim3(kObsNormBlock), 0, e->stream, e->ro_obs, D, b.N, b.n, b.t0, b.S,
                       s.obs_part);
    hipLaunchKernelGGL(raw ? k_obs_norm_finish<true> : k_obs_norm_finish<false>, dim3(tiles, (unsigned)s.M), dim3(kObsNormBlock), 0, e->stream, s.obs, c,
                       s.obs_part, (int)b.chunks, b.S);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}
// the reward part's update: the scan under `gamma`, or - mem != null - under every env's member's own, the returns' moments, the merge,
// the new multiplier
template <typename Member>
int norm_update_rew(adc_engine *e, const NormSet &s, const NormBatch &b, const adc::NormConfig &c, float gamma, const Member *mem)
{
    const int chunks = (int)b.chunks;
    hipLaunchKernelGGL(k_rew_norm_scan<Member>, dim3(norm_blocks(b.N, kRewNormBlock)), dim3(kRewNormBlock), 0, e->stream, b.N, b.n, b.t0, b.T, e->ro_reward,
                       e->ro_term, e->ro_trunc, gamma, mem, mem ? e->lrn_n : b.N, s.rew.G, s.g);
    hipLaunchKernelGGL(k_rew_norm_chunk_sums, dim3(norm_blocks(chunks, kRewNormBlock), (unsigned)s.M), dim3(kRewNormBlock), 0, e->stream, s.g, b.S, chunks,
                       s.rew_part);
    hipLaunchKernelGGL(k_rew_norm_finish, dim3(norm_blocks(s.M, kRewNormBlock)), dim3(kRewNormBlock), 0, e->stream, s.rew, s.M, c, s.rew_part, chunks, b.S);
    HIP_TRY(hipGetLastError());
    return ADC_OK;
}

// a normaliser's state, part by part.  The gets enqueue the copies that were asked for; the caller synchronises
int norm_obs_get(adc_engine *e, const ObsNormView &p, int32_t member, int64_t *count, double *mean_d, double *m2_d, float *shift_d, float *scale_d)
{
    const size_t D = (size_t)p.D, at = (size_t)member * D;
    if (count) HIP_TRY(hipMemcpyAsync(count, p.count + at, 8, hipMemcpyDeviceToHost, e->stream));
    if (mean_d) HIP_TRY(hipMemcpyAsync(mean_d, p.mean + at, D * 8, hipMemcpyDeviceToHost, e->stream));
    if (m2_d) HIP_TRY(hipMemcpyAsync(m2_d, p.m2 + at, D * 8, hipMemcpyDeviceToHost, e->stream));
    if (shift_d) HIP_TRY(hipMemcpyAsync(shift_d, p.shift + at, D * 4, hipMemcpyDeviceToHost, e->stream));
    if (scale_d) HIP_TRY(hipMemcpyAsync(scale_d, p.scale + at, D * 4, hipMemcpyDeviceToHost, e->stream));
    return ADC_OK;
}
int norm_rew_get(adc_engine *e, const RewNormView &r, int32_t member, int64_t *count, double *mean, double *m2, float *scale)
{
    if (count) HIP_TRY(hipMemcpyAsync(count, r.count + member, 8, hipMemcpyDeviceToHost, e->stream));
    if (mean) HIP_TRY(hipMemcpyAsync(mean, r.mean + member, 8, hipMemcpyDeviceToHost, e->stream));
    if (m2) HIP_TRY(hipMemcpyAsync(m2, r.m2 + member, 8, hipMemcpyDeviceToHost, e->stream));
    if (scale) HIP_TRY(hipMemcpyAsync(scale, r.scale + member, 4, hipMemcpyDeviceToHost, e->stream));
    return ADC_OK;
}
// what a set may write; strict: the moments (and the shift) must be finite as well
int norm_obs_check(const ObsNormView &p, bool strict, int64_t count, const double *mean_d, const double *m2_d, const float *shift_d, const float *scale_d)
{
    if (!mean_d || !m2_d || !shift_d || !scale_d) return fail(ADC_EINVAL, "mean, M2, shift or scale is NULL");
    if (count < 0) return fail(ADC_EINVAL, "count >= 0");
    const double inf = (double)__builtin_inff();
    for (size_t j = 0; j < (size_t)p.D; ++j) {
        if (!(scale_d[j] > 0.0f && scale_d[j] < __builtin_inff())) return fail(ADC_EINVAL, "scale must be finite and > 0");
        if (!strict) continue;
        if (!(shift_d[j] > -__builtin_inff() && shift_d[j] < __builtin_inff()) || !(mean_d[j] > -inf && mean_d[j] < inf))
            return fail(ADC_EINVAL, "shift and mean must be finite");
        if (!(m2_d[j] >= 0.0 && m2_d[j] < inf)) return fail(ADC_EINVAL, "M2 must be finite and >= 0");
    }
    return ADC_OK;
}
int norm_rew_check(bool strict, int64_t count, double mean, double m2, float scale)
{
    if (count < 0) return fail(ADC_EINVAL, "count >= 0");
    if (!(scale > 0.0f && scale < __builtin_inff())) return fail(ADC_EINVAL, "scale must be finite and > 0");
    if (!strict) return ADC_OK;
    const double inf = (double)__builtin_inff();
    if (!(mean > -inf && mean < inf)) return fail(ADC_EINVAL, "shift and mean must be finite");
    if (!(m2 >= 0.0 && m2 < inf)) return fail(ADC_EINVAL, "M2 must be finite and >= 0");
    return ADC_OK;
}
// the sets return once the copies have landed (their arguments are the caller's frame's until then)
int norm_obs_put(adc_engine *e, const ObsNormView &p, int32_t member, int64_t count, const double *mean_d, const double *m2_d, const float *shift_d,
                 const float *scale_d)
{
    const size_t D = (size_t)p.D, at = (size_t)member * D;
    const std::vector<int64_t> counts(D, count);
    HIP_TRY(hipMemcpyAsync(p.count + at, counts.data(), D * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.mean + at, mean_d, D * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.m2 + at, m2_d, D * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.shift + at, shift_d, D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(p.scale + at, scale_d, D * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}
int norm_rew_put(adc_engine *e, const RewNormView &r, int32_t member, int64_t count, double mean, double m2, float scale)
{
    HIP_TRY(hipMemcpyAsync(r.count + member, &count, 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(r.mean + member, &mean, 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(r.m2 + member, &m2, 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(r.scale + member, &scale, 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

// the envs' carry G [N], fetched into g_n or - set - replaced by it
int norm_returns(adc_engine *e, const NormSet &s, double *g_n, bool set)
{
    if (!s.rew.G) return fail(ADC_ESTATE, "the normaliser was initialised without rewards");
    if (!g_n) return fail(ADC_EINVAL, "g_n is NULL");
    ENGINE_GUARD(e);
    const size_t bytes = (size_t)e->v.N * 8;
    HIP_TRY(set ? hipMemcpyAsync(s.rew.G, g_n, bytes, hipMemcpyHostToDevice, e->stream) : hipMemcpyAsync(g_n, s.rew.G, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

// every replaced member's normalisers become its donor's: the donor plan `src` (the argument `name` of the entry point) is checked -
// a member, or the member itself / -1 to keep it; no destination is also a source - and handed to one launch
int norm_copy(adc_engine *e, const NormSet &s, bool per_member, const int32_t *src, const char *name)
{
    if (!per_member) return fail(ADC_ESTATE, "the normaliser is shared by all envs: there are no members to copy between");
    if (!src) return fail(ADC_EINVAL, std::string(name) + " is NULL");
    const int M = s.M;
    for (int m = 0; m < M; ++m)
        if (src[m] < -1 || src[m] >= M) return fail(ADC_EINVAL, std::string(name) + ": a member, or the member itself / -1 to keep it");
    for (int m = 0; m < M; ++m) {
        const int d = src[m];
        if (d == -1 || d == m) continue;
        if (src[d] != -1 && src[d] != d) return fail(ADC_EINVAL, "a destination is also a source: the copies of a round may not chain");
    }
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(s.src, src, (size_t)M * 4, hipMemcpyHostToDevice, e->stream));
    const int cols = s.obs.count ? s.obs.D : 1;
    hipLaunchKernelGGL(k_norm_copy, dim3(norm_blocks(cols, kObsNormBlock), (unsigned)M), dim3(kObsNormBlock), 0, e->stream, s.obs, s.rew, s.src);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));       // (src is the caller's until here)
    return ADC_OK;
}

constexpr const char *kOnNotReady =
    "adc_engine_obs_norm_init has not been called (or the policy, the learners or the record were re-initialised since)";
constexpr const char *kRnNotReady =
    "adc_engine_rew_norm_init has not been called (or the trainer, the policy, the learners or the record were re-initialised since)";
constexpr const char *kNoNewDay = "no day has been recorded since the last update or adc_engine_rollout_reset";
}  // namespace

// ---- the running observation normaliser of the PPO / A2C learners (the law is csrc/adc_norm.h) ---------------------------------
ADC_EXPORT int adc_engine_obs_norm_init(adc_engine *e, const adc_obs_norm_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_obs_norm_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (int rc = mlp_ready(e)) return rc;
    if (!e->mp.shift) return fail(ADC_EINVAL, "the policy was initialised without normalisation");
    if (e->have_im) return fail(ADC_ESTATE, "imitation is alive on this trainer (adc_engine_im_init): teacher days are recorded under the static normalisation");
    const bool per_member = cfg->per_member != 0;
    if (per_member && e->lrn_M == 0) return fail(ADC_ESTATE, "per-member normalisers need learners (adc_engine_mlp_learners)");
    if (e->have_td3 || e->have_td3_pop)
        return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: its ring holds inputs normalised by older vectors");
    if (e->have_sac || e->have_sac_pop) return fail(ADC_ESTATE, "a soft actor-critic trainer is alive on this engine: its ring holds inputs normalised by older vectors");
    ENGINE_GUARD(e);
    // (a second init starts over from the policy's own vectors; the days its predecessor consumed were collected under other
    //  vectors than those and are not consumed again)
    NormSet s;
    s.t0 = e->on.live ? e->ro_t : 0;
    s.M = per_member ? e->lrn_M : 1;
    norm_set_drop(e, e->on);
    // the vectors in force: they must be usable as a scale (the law divides by them)
    std::vector<float> scale((size_t)e->mp.D);
    HIP_TRY(hipMemcpyAsync(scale.data(), e->mp.scale, scale.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (const float sc : scale)
        if (!(sc > 0.0f && sc < __builtin_inff()))
            return fail(ADC_EINVAL, "the current scale vector holds a value that is not finite or not > 0 (adc_engine_mlp_set_norm)");
    // (the chunk partials are grown by the updates: the record may not exist yet)
    int rc;
    if ((rc = norm_alloc_obs(e, s, per_member)) || (rc = mlp_alloc(e, s.allocs, &s.src, (size_t)s.M)) || (rc = norm_install_vectors(e, s, per_member))) {
        norm_set_drop(e, s);
        return rc;
    }
    s.live = true;
    e->on = std::move(s);
    e->on_cfg = *cfg;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_obs_norm_update(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    NormSet &s = e->on;
    if (int rc = norm_ready(s, kOnNotReady)) return rc;
    if (e->ro_T == 0) return fail(ADC_ESTATE, "the observation normaliser is fed from the rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "the observation normaliser needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    if (e->ro_t <= s.t0) return fail(ADC_ESTATE, kNoNewDay);
    const NormBatch b = norm_batch(e, s);
    if (b.chunks > 65535) return fail(ADC_EINVAL, "days x envs of a normaliser: at most 65535 x 1024 samples in an update");
    ENGINE_GUARD(e);
    const size_t need = (size_t)s.M * (size_t)b.chunks * 2u * (size_t)e->mp.D;
    if (need > s.obs_part_grown) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (s.obs_part) { (void)hipFree(s.obs_part); s.obs_part = nullptr; s.obs_part_grown = 0; }
        void *q = nullptr;
        if (hipMalloc(&q, need * 8) != hipSuccess) { (void)hipGetLastError(); return fail(ADC_ENOMEM, "hipMalloc failed (observation normaliser)"); }
        s.obs_part = static_cast<double *>(q);
        s.obs_part_grown = need;
    }
    if (int rc = norm_update_obs(e, s, b, adc::NormConfig{e->on_cfg.min_std, e->on_cfg.count_cap}, /* raw = */ false)) return rc;
    s.t0 = b.T;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_obs_norm_state_get(adc_engine *e, int32_t member, int64_t *count, double *mean_d, double *m2_d, float *shift_d, float *scale_d)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = norm_ready(e->on, kOnNotReady)) || (rc = norm_member_check(e->on, member))) return rc;
    ENGINE_GUARD(e);
    if ((rc = norm_obs_get(e, e->on.obs, member, count, mean_d, m2_d, shift_d, scale_d))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_obs_norm_state_set(adc_engine *e, int32_t member, int64_t count, const double *mean_d, const double *m2_d, const float *shift_d,
                                             const float *scale_d)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = norm_ready(e->on, kOnNotReady)) || (rc = norm_member_check(e->on, member)) ||
        (rc = norm_obs_check(e->on.obs, /* strict = */ false, count, mean_d, m2_d, shift_d, scale_d)))
        return rc;
    ENGINE_GUARD(e);
    return norm_obs_put(e, e->on.obs, member, count, mean_d, m2_d, shift_d, scale_d);
}

ADC_EXPORT int adc_engine_obs_norm_copy(adc_engine *e, const int32_t *src_of_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = norm_ready(e->on, kOnNotReady)) return rc;
    return norm_copy(e, e->on, e->on_cfg.per_member != 0, src_of_m, "src_of_m");
}

// ---- the running reward normaliser of the PPO / A2C learners (the law is csrc/adc_rew_norm.h) ----------------------------------
ADC_EXPORT int adc_engine_rew_norm_init(adc_engine *e, const adc_rew_norm_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_rew_norm_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (e->have_td3 || e->have_td3_pop)
        return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: its reward enters at the TD3 target, not through GAE");
    if (!e->have_pg && !e->have_pg_pop)
        return fail(ADC_ESTATE, "the reward normaliser discounts by a PPO / A2C trainer's gamma: adc_engine_pg_init or adc_engine_pg_pop_init first");
    if (e->have_im) return fail(ADC_ESTATE, "imitation is alive on this trainer (adc_engine_im_init): the teacher's returns are not normalised");
    const bool per_member = cfg->per_member != 0;
    if (per_member && !e->have_pg_pop) return fail(ADC_ESTATE, "per-member normalisers need a learner population (adc_engine_pg_pop_init)");
    ENGINE_GUARD(e);
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was.  A normaliser set up over a record
    //  already begun consumes it from its first day: t0 = 0)
    NormSet s;
    s.M = per_member ? e->lrn_M : 1;
    int rc;
    if ((rc = norm_alloc_rew(e, s)) || (rc = mlp_alloc(e, s.allocs, &s.src, (size_t)s.M))) {
        norm_set_drop(e, s);
        return rc;
    }
    s.live = true;
    norm_set_drop(e, e->rn);
    e->rn = std::move(s);
    e->rn_cfg = *cfg;
    e->pg_adv_ready = false;            // (advantages computed without the multiplier are stale)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_update(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    NormSet &s = e->rn;
    if (int rc = norm_ready(s, kRnNotReady)) return rc;
    if (e->ro_T == 0) return fail(ADC_ESTATE, "the reward normaliser is fed from the rollout record (adc_engine_rollout_enable)");
    if (e->ro_t <= s.t0) return fail(ADC_ESTATE, kNoNewDay);
    const NormBatch b = norm_batch(e, s);
    ENGINE_GUARD(e);
    const bool pop = e->have_pg_pop;
    if (int rc = norm_update_rew(e, s, b, adc::NormConfig{e->rn_cfg.min_std, e->rn_cfg.count_cap}, pop ? 0.0f : e->pgp_cfg[0].gamma,
                                 pop ? e->pgp_dmem : (const PgMember *)nullptr))
        return rc;
    s.t0 = b.T;
    e->pg_adv_ready = false;            // (advantages computed under the old multiplier are stale)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_state_get(adc_engine *e, int32_t member, int64_t *count, double *mean, double *m2, float *scale)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = norm_ready(e->rn, kRnNotReady)) || (rc = norm_member_check(e->rn, member))) return rc;
    ENGINE_GUARD(e);
    if ((rc = norm_rew_get(e, e->rn.rew, member, count, mean, m2, scale))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_state_set(adc_engine *e, int32_t member, int64_t count, double mean, double m2, float scale)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = norm_ready(e->rn, kRnNotReady)) || (rc = norm_member_check(e->rn, member)) || (rc = norm_rew_check(/* strict = */ false, count, mean, m2, scale)))
        return rc;
    ENGINE_GUARD(e);
    if ((rc = norm_rew_put(e, e->rn.rew, member, count, mean, m2, scale))) return rc;
    e->pg_adv_ready = false;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_rew_norm_returns_get(adc_engine *e, double *g_n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = norm_ready(e->rn, kRnNotReady)) return rc;
    return norm_returns(e, e->rn, g_n, /* set = */ false);
}

ADC_EXPORT int adc_engine_rew_norm_returns_set(adc_engine *e, const double *g_n)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = norm_ready(e->rn, kRnNotReady)) return rc;
    return norm_returns(e, e->rn, const_cast<double *>(g_n), /* set = */ true);
}

ADC_EXPORT int adc_engine_rew_norm_copy(adc_engine *e, const int32_t *src_of_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = norm_ready(e->rn, kRnNotReady)) || (rc = norm_copy(e, e->rn, e->rn_cfg.per_member != 0, src_of_m, "src_of_m"))) return rc;
    e->pg_adv_ready = false;
    return ADC_OK;
}

// ---- the running normalisers of the TD3 learners and of the SAC learners (the laws are csrc/adc_td3_norm.h, adc_sac_norm.h) ---------
// Two families of one front end: each has its own NormSet, config and trainer, its entry points do not see the other's normaliser, and
// the sentences name their own calls.  A family is described once (Td3NormFamily, SacNormFamily); ring_norm_* are the entry points over it.
namespace {
struct Td3NormFamily {
    using Config = adc_td3_norm_config;
    static NormSet &set(adc_engine *e) { return e->tn; }
    static Config &cfg(adc_engine *e) { return e->tn_cfg; }
    static int config_check(const Config *c, const char **why) { return adc_td3_norm_config_check(c, why); }
    static bool solo(const adc_engine *e) { return e->have_td3; }
    static bool pop(const adc_engine *e) { return e->have_td3_pop; }
    static int state_check(const adc_engine *e) { return e->have_td3_pop ? tp_state_check(e) : td3_state_check(e); }
    static float gamma(const adc_engine *e) { return e->td3_cfg.gamma; }
    static constexpr const char *kNotReady =
        "adc_engine_td3_norm_init has not been called (or the TD3 trainer, the policy, the learners or the record were re-initialised since)";
    static constexpr const char *kNoTrainer = "the TD3 normalisers belong to an off-policy trainer: adc_engine_td3_init or adc_engine_td3_pop_init first";
    static constexpr const char *kPerMember = "per-member normalisers need a TD3 learner population (adc_engine_td3_pop_init)";
    static constexpr const char *kNotEmpty = "the record and the replay ring must be empty: their rows were written as network inputs (adc_engine_rollout_reset, and "
                                             "adc_engine_td3_norm_init before the first store)";
};
struct SacNormFamily {
    using Config = adc_sac_norm_config;
    static NormSet &set(adc_engine *e) { return e->sn; }
    static Config &cfg(adc_engine *e) { return e->sn_cfg; }
    static int config_check(const Config *c, const char **why) { return adc_sac_norm_config_check(c, why); }
    static bool solo(const adc_engine *e) { return e->have_sac; }
    static bool pop(const adc_engine *e) { return e->have_sac_pop; }
    static int state_check(const adc_engine *e) { return e->have_sac_pop ? sp_state_check(e) : sac_state_check(e); }
    static float gamma(const adc_engine *e) { return e->sac_cfg.gamma; }
    static constexpr const char *kNotReady =
        "adc_engine_sac_norm_init has not been called over a live adc_engine_sac_init / adc_engine_sac_pop_init trainer (or the trainer, the policy, the "
        "learners or the record were re-initialised since)";
    static constexpr const char *kNoTrainer = "the SAC normalisers belong to a soft actor-critic trainer: adc_engine_sac_init or adc_engine_sac_pop_init first";
    static constexpr const char *kPerMember = "per-member normalisers need a SAC learner population (adc_engine_sac_pop_init)";
    static constexpr const char *kNotEmpty = "the record and the replay ring must be empty: their rows were written as network inputs (adc_engine_rollout_reset, and "
                                             "adc_engine_sac_norm_init before the first store)";
};

template <class Family>
int ring_norm_init(adc_engine *e, const typename Family::Config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (Family::config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (!Family::solo(e) && !Family::pop(e)) return fail(ADC_ESTATE, Family::kNoTrainer);
    const bool pop = Family::pop(e), per_member = cfg->per_member != 0, obs = cfg->observations != 0, rew = cfg->rewards != 0;
    if (int rc = Family::state_check(e)) return rc;
    if (per_member && !pop) return fail(ADC_EINVAL, Family::kPerMember);
    if (obs && !e->mp.shift) return fail(ADC_EINVAL, "the policy was initialised without normalisation");
    if (e->ro_t != 0 || e->td3_written != 0) return fail(ADC_ESTATE, Family::kNotEmpty);
    NormSet s;
    s.M = per_member ? e->lrn_M : 1;
    const size_t chunks = (size_t)pg_chunks((long long)e->ro_T * (long long)(e->v.N / s.M));
    if (chunks > 65535) return fail(ADC_EINVAL, "days x envs of a normaliser: at most 65535 x 1024 samples in an update");
    ENGINE_GUARD(e);
    norm_set_drop(e, Family::set(e));            // (a second init starts over from the policy's own vectors)
    // (the chunk partials are sized for the whole record, as the reward part's scratch is)
    int rc = mlp_alloc(e, s.allocs, &s.src, (size_t)s.M);
    if (!rc && obs && !(rc = norm_alloc_obs(e, s, per_member))) rc = mlp_alloc(e, s.allocs, &s.obs_part, (size_t)s.M * chunks * 2u * (size_t)e->mp.D);
    if (!rc && rew) rc = norm_alloc_rew(e, s);
    if (!rc && obs) rc = norm_install_vectors(e, s, per_member);
    if (rc) {
        norm_set_drop(e, s);
        return rc;
    }
    s.live = true;
    Family::set(e) = std::move(s);
    Family::cfg(e) = *cfg;
    return ADC_OK;
}

template <class Family>
int ring_norm_update(adc_engine *e, int64_t *samples)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    NormSet &s = Family::set(e);
    const typename Family::Config &c = Family::cfg(e);
    if (int rc = norm_ready(s, Family::kNotReady)) return rc;
    if (e->ro_t <= s.t0) return fail(ADC_ESTATE, kNoNewDay);
    const NormBatch b = norm_batch(e, s);
    ENGINE_GUARD(e);
    int rc;
    if (s.obs.count && (rc = norm_update_obs(e, s, b, adc::NormConfig{c.obs_min_std, c.obs_count_cap}, /* raw = */ true))) return rc;
    // (the members of either family's population keep their discount in the TD3 population's table: Td3Member::law.gamma, sp_member_fill)
    const bool pop = Family::pop(e);
    if (s.rew.count && (rc = norm_update_rew(e, s, b, adc::NormConfig{c.rew_min_std, c.rew_count_cap}, pop ? 0.0f : Family::gamma(e),
                                             pop ? e->tp_dmem : (const Td3Member *)nullptr)))
        return rc;
    s.t0 = b.T;
    if (samples) *samples = b.S;
    return ADC_OK;
}

template <class Family>
int ring_norm_state_get(adc_engine *e, int32_t member, int64_t *obs_count, double *obs_mean_d, double *obs_m2_d, float *shift_d, float *scale_d,
                        int64_t *rew_count, double *rew_mean, double *rew_m2, float *rew_scale)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const NormSet &s = Family::set(e);
    int rc;
    if ((rc = norm_ready(s, Family::kNotReady)) || (rc = norm_member_check(s, member))) return rc;
    if (!s.obs.count && (obs_count || obs_mean_d || obs_m2_d || shift_d || scale_d))
        return fail(ADC_ESTATE, "the normaliser was initialised without observations");
    if (!s.rew.count && (rew_count || rew_mean || rew_m2 || rew_scale)) return fail(ADC_ESTATE, "the normaliser was initialised without rewards");
    ENGINE_GUARD(e);
    if ((rc = norm_obs_get(e, s.obs, member, obs_count, obs_mean_d, obs_m2_d, shift_d, scale_d)) ||
        (rc = norm_rew_get(e, s.rew, member, rew_count, rew_mean, rew_m2, rew_scale)))
        return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

template <class Family>
int ring_norm_state_set(adc_engine *e, int32_t member, int64_t obs_count, const double *obs_mean_d, const double *obs_m2_d, const float *shift_d,
                        const float *scale_d, int64_t rew_count, double rew_mean, double rew_m2, float rew_scale)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const NormSet &s = Family::set(e);
    int rc;
    if ((rc = norm_ready(s, Family::kNotReady)) || (rc = norm_member_check(s, member))) return rc;
    // (both parts are checked before either is written)
    if (s.obs.count && (rc = norm_obs_check(s.obs, /* strict = */ true, obs_count, obs_mean_d, obs_m2_d, shift_d, scale_d))) return rc;
    if (s.rew.count && (rc = norm_rew_check(/* strict = */ true, rew_count, rew_mean, rew_m2, rew_scale))) return rc;
    ENGINE_GUARD(e);
    if (s.obs.count && (rc = norm_obs_put(e, s.obs, member, obs_count, obs_mean_d, obs_m2_d, shift_d, scale_d))) return rc;
    if (s.rew.count && (rc = norm_rew_put(e, s.rew, member, rew_count, rew_mean, rew_m2, rew_scale))) return rc;
    return ADC_OK;
}

template <class Family>
int ring_norm_returns(adc_engine *e, double *g_n, bool set)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = norm_ready(Family::set(e), Family::kNotReady)) return rc;
    return norm_returns(e, Family::set(e), g_n, set);
}

template <class Family>
int ring_norm_copy(adc_engine *e, const int32_t *src_of_member_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = norm_ready(Family::set(e), Family::kNotReady)) return rc;
    return norm_copy(e, Family::set(e), Family::cfg(e).per_member != 0, src_of_member_m, "src_of_member_m");
}
}  // namespace

ADC_EXPORT int adc_engine_td3_norm_init(adc_engine *e, const adc_td3_norm_config *cfg) { return ring_norm_init<Td3NormFamily>(e, cfg); }
ADC_EXPORT int adc_engine_td3_norm_update(adc_engine *e, int64_t *samples) { return ring_norm_update<Td3NormFamily>(e, samples); }
ADC_EXPORT int adc_engine_td3_norm_state_get(adc_engine *e, int32_t member, int64_t *obs_count, double *obs_mean_d, double *obs_m2_d, float *shift_d,
                                             float *scale_d, int64_t *rew_count, double *rew_mean, double *rew_m2, float *rew_scale)
{
    return ring_norm_state_get<Td3NormFamily>(e, member, obs_count, obs_mean_d, obs_m2_d, shift_d, scale_d, rew_count, rew_mean, rew_m2, rew_scale);
}
ADC_EXPORT int adc_engine_td3_norm_state_set(adc_engine *e, int32_t member, int64_t obs_count, const double *obs_mean_d, const double *obs_m2_d,
                                             const float *shift_d, const float *scale_d, int64_t rew_count, double rew_mean, double rew_m2, float rew_scale)
{
    return ring_norm_state_set<Td3NormFamily>(e, member, obs_count, obs_mean_d, obs_m2_d, shift_d, scale_d, rew_count, rew_mean, rew_m2, rew_scale);
}
ADC_EXPORT int adc_engine_td3_norm_returns_get(adc_engine *e, double *g_n) { return ring_norm_returns<Td3NormFamily>(e, g_n, /* set = */ false); }
ADC_EXPORT int adc_engine_td3_norm_returns_set(adc_engine *e, const double *g_n) { return ring_norm_returns<Td3NormFamily>(e, const_cast<double *>(g_n), /* set = */ true); }
ADC_EXPORT int adc_engine_td3_norm_copy(adc_engine *e, const int32_t *src_of_member_m) { return ring_norm_copy<Td3NormFamily>(e, src_of_member_m); }

ADC_EXPORT int adc_engine_sac_norm_init(adc_engine *e, const adc_sac_norm_config *cfg) { return ring_norm_init<SacNormFamily>(e, cfg); }
ADC_EXPORT int adc_engine_sac_norm_update(adc_engine *e, int64_t *samples) { return ring_norm_update<SacNormFamily>(e, samples); }
ADC_EXPORT int adc_engine_sac_norm_state_get(adc_engine *e, int32_t member, int64_t *obs_count, double *obs_mean_d, double *obs_m2_d, float *shift_d,
                                             float *scale_d, int64_t *rew_count, double *rew_mean, double *rew_m2, float *rew_scale)
{
    return ring_norm_state_get<SacNormFamily>(e, member, obs_count, obs_mean_d, obs_m2_d, shift_d, scale_d, rew_count, rew_mean, rew_m2, rew_scale);
}
ADC_EXPORT int adc_engine_sac_norm_state_set(adc_engine *e, int32_t member, int64_t obs_count, const double *obs_mean_d, const double *obs_m2_d,
                                             const float *shift_d, const float *scale_d, int64_t rew_count, double rew_mean, double rew_m2, float rew_scale)
{
    return ring_norm_state_set<SacNormFamily>(e, member, obs_count, obs_mean_d, obs_m2_d, shift_d, scale_d, rew_count, rew_mean, rew_m2, rew_scale);
}
ADC_EXPORT int adc_engine_sac_norm_returns_get(adc_engine *e, double *g_n) { return ring_norm_returns<SacNormFamily>(e, g_n, /* set = */ false); }
ADC_EXPORT int adc_engine_sac_norm_returns_set(adc_engine *e, const double *g_n) { return ring_norm_returns<SacNormFamily>(e, const_cast<double *>(g_n), /* set = */ true); }
ADC_EXPORT int adc_engine_sac_norm_copy(adc_engine *e, const int32_t *src_of_member_m) { return ring_norm_copy<SacNormFamily>(e, src_of_member_m); }
