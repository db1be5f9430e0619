// pg_shuffle.inc (part of adc_shims.cpp) - shuffled sample-level minibatches and the target-KL stop on the host (adc_pg_shuffle.h: the code
// parts/kernel_pg_shuffle.inc runs)
ADC_EXPORT int adc_pg_shuffle_config_check(const adc_pg_shuffle_config *cfg, const char **message)
{
    const char *msg = nullptr;
    if (!cfg || cfg->struct_size != sizeof(adc_pg_shuffle_config)) msg = "adc_pg_shuffle_config: NULL or struct_size mismatch";
    else if (cfg->minibatch_samples < 1) msg = "minibatch_samples >= 1";
    else if (!(cfg->target_kl >= 0.0f && cfg->target_kl < __builtin_inff())) msg = "target_kl >= 0 and finite (0: never stop)";
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_pg_shuffle_order_host(uint64_t seed, int64_t n_s, uint32_t tick, uint32_t *order_out)
{
    if (n_s < 1 || n_s > 0x7FFFFFFFll || !order_out) return ADC_EINVAL;
    const uint64_t key = adc::pg_shuffle_key(seed);
    const uint32_t n = (uint32_t)n_s, h = adc::pg_shuffle_half_bits(n);
    for (uint32_t i = 0; i < n; ++i) order_out[i] = adc::pg_shuffle_sample(key, i, n, h, tick);
    return ADC_OK;
}

ADC_EXPORT int adc_pg_shuffle_stop_host(double approx_kl, float target_kl, int32_t *stop)
{
    if (!stop || !(target_kl >= 0.0f && target_kl < __builtin_inff())) return ADC_EINVAL;
    *stop = adc::pg_shuffle_stop(approx_kl, target_kl) ? 1 : 0;
    return ADC_OK;
}
