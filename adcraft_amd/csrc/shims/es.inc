// es.inc (part of adc_shims.cpp) - the evolution strategy on the host (adc_es.h: the code parts/kernel_es.inc runs)
ADC_EXPORT int adc_es_config_check(const adc_es_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_es_config)) msg = "adc_es_config: NULL or struct_size mismatch";
    else if (!(cfg->sigma > 0.0f) || !(cfg->sigma < __builtin_inff())) msg = "sigma must be positive and finite";
    else if (!(cfg->lr >= 0.0f)) msg = "lr >= 0";
    else if (cfg->shaping != ADC_ES_CENTERED_RANK && cfg->shaping != ADC_ES_RAW) msg = "unknown fitness shaping";
    else if (cfg->optimiser != ADC_ES_ADAM && cfg->optimiser != ADC_ES_SGD) msg = "unknown optimiser";
    else if (!(cfg->l2 >= 0.0f)) msg = "l2 >= 0";
    else if (cfg->optimiser == ADC_ES_ADAM && (!(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f) || !(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f)))
        msg = "Adam: 0 <= beta1, beta2 < 1";
    else if (cfg->optimiser == ADC_ES_ADAM && !(cfg->eps > 0.0f)) msg = "Adam: eps > 0";
    return config_verdict(msg, message);
}

// the step record of the law's optimiser after steps_taken steps (adc_es.h EsStep: the PG and the SAC twins step by it too)
static adc::EsStep shim_opt_step(bool sgd, float lr, float beta1, float beta2, float eps, float l2, int64_t steps_taken)
{
    adc::EsStep step{};
    step.optimiser = sgd ? adc::kEsSgd : adc::kEsAdam;
    step.lr = lr; step.beta1 = beta1; step.beta2 = beta2; step.eps = eps; step.l2 = l2;
    step.c1 = adc::es_bias_correction(step.beta1, (uint32_t)(steps_taken + 1));
    step.c2 = adc::es_bias_correction(step.beta2, (uint32_t)(steps_taken + 1));
    return step;
}

ADC_EXPORT int adc_es_noise_host(uint64_t seed, uint32_t pair, uint32_t generation, int64_t p0, int64_t n, float *eps_n)
{
    if (p0 < 0 || n < 0 || p0 + n > 0x7FFFFFFFll || (n > 0 && !eps_n)) return ADC_EINVAL;
    const uint64_t key = adc::es_key(seed);
    for (int64_t q = p0 / 4; q * 4 < p0 + n; ++q) {
        float e4[4];
        adc::es_noise4(key, (uint32_t)q, pair, generation, e4);
        for (int k = 0; k < 4; ++k) {
            const int64_t p = q * 4 + k;
            if (p >= p0 && p < p0 + n) eps_n[p - p0] = e4[k];
        }
    }
    return ADC_OK;
}

ADC_EXPORT int adc_es_update_host(const adc_es_config *cfg, uint64_t seed, int32_t members, int64_t n_params, const double *fitness_m,
                                  int64_t generation, float *theta_p, float *m_p, float *v_p, float *grad_p)
{
    if (adc_es_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (members < 2 || (members & 1) || n_params < 1 || n_params > 0x7FFFFFFFll || generation < 0 || generation > 0x7FFFFFFFll || !fitness_m ||
        !theta_p || !m_p || !v_p)
        return ADC_EINVAL;
    const int M = members;
    const uint64_t key = adc::es_key(seed);
    std::vector<double> du;
    adc::es_shape(cfg->shaping == ADC_ES_RAW ? adc::kEsRaw : adc::kEsCenteredRank, fitness_m, M, du);
    const adc::EsStep step = shim_opt_step(cfg->optimiser == ADC_ES_SGD, cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->l2, generation);
    for (int64_t q = 0; q * 4 < n_params; ++q) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < M / 2; ++i) {
            float e4[4];
            adc::es_noise4(key, (uint32_t)q, (uint32_t)i, (uint32_t)generation, e4);
            for (int k = 0; k < 4; ++k) acc[k] = adc::es_grad_step(acc[k], du[(size_t)i], e4[k]);
        }
        for (int k = 0; k < 4 && q * 4 + k < n_params; ++k) {
            const int64_t p = q * 4 + k;
            const float g = adc::es_decay(adc::es_grad_finish(acc[k], M, cfg->sigma), theta_p[p], step.l2);
            theta_p[p] = adc::es_apply(step, theta_p[p], g, m_p[p], v_p[p]);
            if (grad_p) grad_p[p] = g;
        }
    }
    return ADC_OK;
}
