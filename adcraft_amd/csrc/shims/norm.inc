// norm.inc (part of adc_shims.cpp) - the running normalisers on the host (adc_norm.h, adc_rew_norm.h, adc_td3_norm.h, adc_sac_norm.h: the code
// parts/kernel_norm.inc runs): the observation moments and the discounted returns' moments once, under the configuration checks
// and the exports of the four front ends, and the ring families' targets under a multiplier (their n-step exports are shims/replay.inc's).
namespace {
// the observation moments of S rows of D columns merged into the running state, column by column (adc_norm.h); raw: the rows are raw
// observations (adc_td3_norm.h).  Both front ends' arguments are checked here
int obs_norm_columns(const adc::NormConfig &c, bool raw, int64_t S, int32_t D, const float *x_sd, int64_t *count, double *mean_d, double *m2_d,
                     float *shift_d, float *scale_d)
{
    if (S < 1 || D < 1 || !x_sd || !count || !mean_d || !m2_d || !shift_d || !scale_d || *count < 0) return ADC_EINVAL;
    const int64_t count0 = *count;
    int64_t cnt = count0;
    for (int32_t j = 0; j < D; ++j) {
        const double sx = adc::pg_csum(S, [&](double part, int64_t i) { return adc::norm_chain_sum(part, x_sd[(size_t)i * (size_t)D + (size_t)j]); });
        const double qx = adc::pg_csum(S, [&](double part, int64_t i) {
            const float x = x_sd[(size_t)i * (size_t)D + (size_t)j];
            return adc::pg_chain_mac(part, x, x);
        });
        cnt = count0;
        adc::norm_finish(c, raw, sx, qx, S, cnt, mean_d[j], m2_d[j], shift_d[j], scale_d[j]);
    }
    *count = cnt;
    return ADC_OK;
}

// the discounted returns of `days` days of num_envs envs, their moments merged into the running state, the envs' carry advanced
// (adc_rew_norm.h).  Both front ends' arguments are checked here
int rew_norm_days(const adc::NormConfig &c, int32_t days, int32_t num_envs, const float *gamma_n, const float *reward_tn, const uint8_t *terminated_tn,
                  const uint8_t *truncated_tn, int64_t *count, double *mean, double *m2, float *scale, double *carry_n)
{
    if (days < 1 || num_envs < 1 || !gamma_n || !reward_tn || !terminated_tn || !truncated_tn || !count || !mean || !m2 || !scale || !carry_n || *count < 0)
        return ADC_EINVAL;
    const size_t N = (size_t)num_envs;
    const int64_t S = (int64_t)days * num_envs;
    std::vector<double> g((size_t)S);
    for (size_t n = 0; n < N; ++n) {
        double G = carry_n[n];
        for (int t = 0; t < days; ++t) {
            const size_t i = (size_t)t * N + n;
            g[i] = adc::rew_norm_scan_day(G, gamma_n[n], reward_tn[i], terminated_tn[i] | truncated_tn[i]);
        }
        carry_n[n] = G;
    }
    const double sx = adc::pg_csum(S, [&](double part, int64_t i) { return adc::rew_norm_chain_sum(part, g[(size_t)i]); });
    const double qx = adc::pg_csum(S, [&](double part, int64_t i) { return adc::rew_norm_chain_sq(part, g[(size_t)i]); });
    adc::rew_norm_finish(c, sx, qx, S, *count, *mean, *m2, *scale);
    return ADC_OK;
}
}  // namespace

// ---- the running observation normaliser on the host (adc_norm.h: the code parts/kernel_norm.inc runs) ---------------------------
ADC_EXPORT int adc_obs_norm_config_check(const adc_obs_norm_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_obs_norm_config)) msg = "adc_obs_norm_config: NULL or struct_size mismatch";
    else if (!(cfg->min_std > 0.0 && cfg->min_std < (double)__builtin_inff())) msg = "min_std must be finite and > 0";
    else if (cfg->count_cap < 0) msg = "count_cap >= 0 (0: no forgetting)";
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_obs_norm_host(const adc_obs_norm_config *cfg, int64_t S, int32_t D, const float *x_sd, int64_t *count, double *mean_d, double *m2_d,
                                 float *shift_d, float *scale_d)
{
    if (adc_obs_norm_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    return obs_norm_columns(adc::NormConfig{cfg->min_std, cfg->count_cap}, /* raw = */ false, S, D, x_sd, count, mean_d, m2_d, shift_d, scale_d);
}

// ---- the running reward normaliser on the host (adc_rew_norm.h: the code parts/kernel_norm.inc runs) ----------------------------
ADC_EXPORT int adc_rew_norm_config_check(const adc_rew_norm_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_rew_norm_config)) msg = "adc_rew_norm_config: NULL or struct_size mismatch";
    else if (!(cfg->min_std > 0.0 && cfg->min_std < (double)__builtin_inff())) msg = "min_std must be finite and > 0";
    else if (!(cfg->clip >= 0.0f && cfg->clip < __builtin_inff())) msg = "clip must be finite and >= 0 (0: off)";
    else if (cfg->count_cap < 0) msg = "count_cap >= 0 (0: no forgetting)";
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_rew_norm_host(const adc_rew_norm_config *cfg, int32_t days, int32_t num_envs, const float *gamma_n, const float *reward_tn,
                                 const uint8_t *terminated_tn, const uint8_t *truncated_tn, int64_t *count, double *mean, double *m2, float *scale,
                                 double *carry_n)
{
    if (adc_rew_norm_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    return rew_norm_days(adc::NormConfig{cfg->min_std, cfg->count_cap}, days, num_envs, gamma_n, reward_tn, terminated_tn, truncated_tn, count, mean, m2, scale, carry_n);
}

// ---- the TD3 and the SAC learners' running normalisers on the host (adc_td3_norm.h, adc_sac_norm.h; the moments' twins below serve
// both families, the law being the same) ---------------------------------------------------------------------------------------------
// adc_td3_norm_config and adc_sac_norm_config are two types of one layout; the struct's name in the first sentence is the difference
template <class Config>
static int ring_norm_config_check(const Config *cfg, const char *null_sentence, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(Config)) msg = null_sentence;
    else if (!cfg->observations && !cfg->rewards) msg = "observations or rewards: at least one must be nonzero";
    else if (!(cfg->obs_min_std > 0.0 && cfg->obs_min_std < (double)__builtin_inff())) msg = "obs_min_std must be finite and > 0";
    else if (cfg->obs_count_cap < 0) msg = "obs_count_cap >= 0 (0: no forgetting)";
    else if (!(cfg->rew_min_std > 0.0 && cfg->rew_min_std < (double)__builtin_inff())) msg = "rew_min_std must be finite and > 0";
    else if (cfg->rew_count_cap < 0) msg = "rew_count_cap >= 0 (0: no forgetting)";
    else if (!(cfg->rew_clip >= 0.0f && cfg->rew_clip < __builtin_inff())) msg = "rew_clip must be finite and >= 0 (0: off)";
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_td3_norm_config_check(const adc_td3_norm_config *cfg, const char **message)
{
    return ring_norm_config_check(cfg, "adc_td3_norm_config: NULL or struct_size mismatch", message);
}

ADC_EXPORT int adc_sac_norm_config_check(const adc_sac_norm_config *cfg, const char **message)
{
    return ring_norm_config_check(cfg, "adc_sac_norm_config: NULL or struct_size mismatch", message);
}

ADC_EXPORT int adc_td3_norm_obs_host(const adc_td3_norm_config *cfg, int64_t S, int32_t D, const float *x_sd, int64_t *count, double *mean_d, double *m2_d,
                                     float *shift_d, float *scale_d)
{
    if (adc_td3_norm_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    return obs_norm_columns(adc::NormConfig{cfg->obs_min_std, cfg->obs_count_cap}, /* raw = */ true, S, D, x_sd, count, mean_d, m2_d, shift_d, scale_d);
}

ADC_EXPORT int adc_td3_norm_rew_host(const adc_td3_norm_config *cfg, int32_t days, int32_t num_envs, const float *gamma_n, const float *reward_tn,
                                     const uint8_t *terminated_tn, const uint8_t *truncated_tn, int64_t *count, double *mean, double *m2, float *scale,
                                     double *carry_n)
{
    if (adc_td3_norm_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    return rew_norm_days(adc::NormConfig{cfg->rew_min_std, cfg->rew_count_cap}, days, num_envs, gamma_n, reward_tn, terminated_tn, truncated_tn, count, mean, m2, scale, carry_n);
}

// ---- the targets under a reward normaliser's multiplier and clip (adc_td3_norm.h, adc_sac_norm.h) -----------------------------------
// One loop per family under its y_norm export here and its y_nstep export (replay.inc): the discount of element b is gn_b[b], or - not
// nstep - the law's gamma (td3_y_norm is td3_y_norm_g at gamma, sac_y_norm is sac_y_norm_g at gamma).  The configuration checks are
// td3.inc's and sac.inc's, declared by the public header.
static int td3_y_host(const adc_td3_config *td3, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, bool nstep, const float *gn_b,
                      float scale, float clip, float *y_b)
{
    if (adc_td3_config_check(td3, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || !r_b || !done_b || !q_b || (nstep && !gn_b) || !y_b || !(clip >= 0.0f)) return ADC_EINVAL;
    const adc::Td3Law law = adc::td3_law_of(*td3);
    for (int32_t b = 0; b < count; ++b) y_b[b] = adc::td3_y_norm_g(r_b[b], done_b[b], q_b[b], nstep ? gn_b[b] : law.gamma, law, scale, clip);
    return ADC_OK;
}

static int sac_y_host(const adc_sac_config *sac, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *lp_b, bool nstep,
                      const float *gn_b, float alpha, float scale, float clip, float *y_b)
{
    if (adc_sac_config_check(sac, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || !r_b || !done_b || !q_b || !lp_b || (nstep && !gn_b) || !y_b || !(clip >= 0.0f)) return ADC_EINVAL;
    // (sac_y_norm_g reads reward_scale of the law alone)
    const adc::SacLaw law{sac->gamma, sac->tau, sac->reward_scale, sac->eps_sq, 0.0f, 0.0f};
    for (int32_t b = 0; b < count; ++b) y_b[b] = adc::sac_y_norm_g(r_b[b], done_b[b], q_b[b], alpha, lp_b[b], nstep ? gn_b[b] : law.gamma, law, scale, clip);
    return ADC_OK;
}

ADC_EXPORT int adc_td3_y_norm_host(const adc_td3_config *td3, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, float scale, float clip,
                                   float *y_b)
{
    return td3_y_host(td3, count, r_b, done_b, q_b, /* nstep = */ false, nullptr, scale, clip, y_b);
}

ADC_EXPORT int adc_sac_y_norm_host(const adc_sac_config *sac, int32_t count, const float *r_b, const uint8_t *done_b, const float *q_b, const float *lp_b,
                                   float alpha, float scale, float clip, float *y_b)
{
    return sac_y_host(sac, count, r_b, done_b, q_b, lp_b, /* nstep = */ false, nullptr, alpha, scale, clip, y_b);
}
