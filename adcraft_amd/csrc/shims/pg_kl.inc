// pg_kl.inc (part of adc_shims.cpp) - the KL penalty and the value-loss clip on the host (adc_pg_kl.h: the code parts/kernel_pg_kl.inc runs)
ADC_EXPORT int adc_pg_kl_config_check(const adc_pg_kl_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_pg_kl_config)) msg = "adc_pg_kl_config: NULL or struct_size mismatch";
    else if (!(cfg->kl_coef >= 0.0f && cfg->kl_coef < inf)) msg = "kl_coef >= 0 and finite";
    else if (cfg->adaptive && !(cfg->kl_target > 0.0f && cfg->kl_target < inf)) msg = "kl_target > 0 and finite when adaptive";
    else if (cfg->factor_up != 0.0f && !(cfg->factor_up > 1.0f && cfg->factor_up < inf)) msg = "factor_up > 1 and finite (0: 1.5)";
    else if (cfg->factor_down != 0.0f && !(cfg->factor_down > 0.0f && cfg->factor_down < 1.0f)) msg = "factor_down in (0, 1) (0: 0.5)";
    else if (!(cfg->vf_clip >= 0.0f && cfg->vf_clip < inf)) msg = "vf_clip >= 0 and finite (0: off)";
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_pg_kl_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_pg_config *cfg, const float *theta_q, int64_t count,
                                   const float *obs_sd, const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s,
                                   const float *value_old_s, const adc_pg_kl_config *kl, float kl_coef, const float *mean_old_sa, const float *ls_old,
                                   int32_t ls_old_per_sample, float *grad_q, double *sums10, double *sums_kl2, adc_pg_stats *stats,
                                   adc_pg_kl_stats *kl_stats)
{
    if (adc_pg_kl_config_check(kl, nullptr) != ADC_OK || !(kl_coef >= 0.0f && kl_coef < __builtin_inff()) || !mean_old_sa || !ls_old) return ADC_EINVAL;
    if (count < 1 || count > 0x7FFFFFFFll || adc_mlp_config_check(mlp, num_keywords, nullptr) != ADC_OK) return ADC_EINVAL;
    const size_t S = (size_t)count, A = (size_t)num_keywords + 1u;
    std::vector<float> pk(S * adc::kPgKlPieces);
    const adc::PgKl law{kl_coef, kl->vf_clip};
    const int rc = pg_grad_host_run(mlp, num_keywords, cfg, theta_q, count, obs_sd, action_sa, logp_old_s, adv_s, ret_s, value_old_s, grad_q, sums10, stats,
                                    [&](size_t s) {
                                        return adc::PgKlSampleHost{law, mean_old_sa + s * A, ls_old_per_sample ? ls_old + s * A : ls_old,
                                                                   pk.data() + s * adc::kPgKlPieces};
                                    });
    if (rc != ADC_OK) return rc;
    double sums[adc::kPgKlPieces];
    for (int c = 0; c < adc::kPgKlPieces; ++c)
        sums[c] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)pk[(size_t)s * adc::kPgKlPieces + (size_t)c]; });
    if (sums_kl2) std::copy(sums, sums + adc::kPgKlPieces, sums_kl2);
    if (kl_stats) {
        kl_stats->kl = sums[adc::kPgKlKl] / (double)count;
        kl_stats->vf_clip_fraction = sums[adc::kPgKlVfClipped] / (double)count;
        kl_stats->kl_coef = kl_stats->kl_coef_next = kl_coef;
    }
    return ADC_OK;
}

ADC_EXPORT int adc_pg_kl_adapt_host(const adc_pg_kl_config *kl, float coef, double kl_mean, float *coef_next)
{
    if (adc_pg_kl_config_check(kl, nullptr) != ADC_OK || !coef_next) return ADC_EINVAL;
    *coef_next = adc::pg_kl_adapt(adc::pg_kl_adapt_of(*kl), coef, kl_mean);
    return ADC_OK;
}
