// imitation.inc (part of adc_shims.cpp) - imitation learning on the host (adc_imitation.h: the code parts/kernel_imitation.inc runs), and the DAgger coin
ADC_EXPORT int adc_im_config_check(const adc_im_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_im_config)) msg = "adc_im_config: NULL or struct_size mismatch";
    else if (!(cfg->beta >= 0.0f && cfg->beta < inf)) msg = "beta >= 0 and finite (0: behaviour cloning)";
    else if (!(cfg->vf_coef >= 0.0f && cfg->vf_coef < inf)) msg = "vf_coef >= 0 and finite";
    else if (!(cfg->w_max >= 0.0f && cfg->w_max < inf)) msg = "w_max >= 0 and finite (0: no cap)";
    else if (!(cfg->ma_start >= 0.0 && cfg->ma_start < (double)inf)) msg = "ma_start >= 0 and finite";
    else if (!(cfg->ma_rate >= 0.0 && cfg->ma_rate <= 1.0)) msg = "ma_rate in [0, 1]";
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_im_weight_host(const adc_im_config *cfg, int64_t count, const float *adv_s, double *ma, float *c, float *w_s)
{
    if (adc_im_config_check(cfg, nullptr) != ADC_OK || count < 1 || !adv_s || !ma || !c) return ADC_EINVAL;
    const double sumsq = adc::pg_csum(count, [&](double part, int64_t i) { return adc::pg_chain_mac(part, adv_s[i], adv_s[i]); });
    *ma = adc::im_ma_next(*ma, cfg->ma_rate, sumsq, count, *c);
    const adc::ImLaw law{cfg->beta, *c, cfg->w_max, cfg->train_log_std != 0 ? 1 : 0};
    if (w_s)
        for (int64_t i = 0; i < count; ++i) w_s[i] = adc::im_weight(adv_s[i], law);
    return ADC_OK;
}

ADC_EXPORT int adc_im_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_im_config *cfg, float c, const float *theta_q, int64_t count,
                                const float *obs_sd, const float *action_sa, const float *adv_s, const float *ret_s, const float *value_old_s, float *grad_q,
                                double *sums10, adc_im_stats *stats)
{
    if (adc_im_config_check(cfg, nullptr) != ADC_OK || count < 1 || count > 0x7FFFFFFFll) return ADC_EINVAL;
    const adc::ImLaw law{cfg->beta, c, cfg->w_max, cfg->train_log_std != 0 ? 1 : 0};
    const std::vector<float> zeros((size_t)count, 0.0f);        // (the record's logp of a teacher day: not read by the imitation loss)
    adc_pg_stats st{};
    const int rc = pg_grad_host_core(mlp, num_keywords, adc::PgLoss{0.0f, cfg->vf_coef, 0.0f}, theta_q, count, obs_sd, action_sa, zeros.data(), adv_s, ret_s,
                                     value_old_s, grad_q, sums10, &st, [&](size_t) { return adc::ImSampleHost{law}; });
    if (rc != ADC_OK) return rc;
    if (stats) {
        stats->steps = 0; stats->samples = count;
        stats->policy_loss = st.policy_loss; stats->value_loss = st.value_loss; stats->entropy = st.entropy; stats->logp = st.approx_kl;
        stats->weight = st.clip_fraction; stats->grad_norm = st.grad_norm; stats->explained_variance = st.explained_variance;
    }
    return ADC_OK;
}

// ---- DAgger on the host (adc_dagger.h: the code k_dagger_mix runs): 1 when the env's coin of the day picks the teacher -------------
ADC_EXPORT int adc_dagger_coin_host(uint64_t key, uint32_t tick, float beta)
{
    return adc::dagger_coin(key, tick, adc::bernoulli_threshold(beta)) ? 1 : 0;
}
