// pbt.inc (part of adc_shims.cpp) - the scheduler of population-based training on the host (adc_pbt.h: the code adc_engine_pbt_step runs)
ADC_EXPORT int adc_pbt_config_check(const adc_pbt_config *cfg, int32_t members, int32_t kind, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_pbt_config)) msg = "adc_pbt_config: NULL or struct_size mismatch";
    else if (kind != ADC_PBT_PG && kind != ADC_PBT_TD3 && kind != ADC_PBT_SAC) msg = "kind: ADC_PBT_PG, ADC_PBT_TD3 or ADC_PBT_SAC";
    else if (members < 2) msg = "population-based training needs at least 2 members";
    else if (cfg->replace_count < 1 || cfg->replace_count > members / 2) msg = "replace_count: 1 to members / 2";
    else if (!(cfg->fitness_ema >= 0.0f && cfg->fitness_ema < 1.0f)) msg = "fitness_ema: 0 (no smoothing) to below 1";
    else if (!(cfg->factor_lo > 0.0f && cfg->factor_lo < inf) || !(cfg->factor_hi > 0.0f && cfg->factor_hi < inf)) msg = "factor_lo, factor_hi: positive and finite";
    else if (!(cfg->log_factor_lo > -inf && cfg->log_factor_lo < inf) || !(cfg->log_factor_hi > -inf && cfg->log_factor_hi < inf))
        msg = "log_factor_lo, log_factor_hi: finite";
    else if (cfg->tuned_mask >> (kind == ADC_PBT_PG ? adc::kPbtPgIds : kind == ADC_PBT_SAC ? adc::kPbtSacIds : adc::kPbtTd3Ids)) msg = "tuned_mask names a hyperparameter id the trainer does not have";
    else if (cfg->with_ring != 0 && cfg->with_ring != 1) msg = "with_ring: 0 or 1";
    else if (kind == ADC_PBT_PG && cfg->with_ring) msg = "with_ring: a policy-gradient population has no ring";
    else
        for (int h = 0; h < adc::kPbtMaxHp && !msg; ++h) {
            if (!((cfg->tuned_mask >> h) & 1u)) continue;
            const float lo = cfg->lo[h], hi = cfg->hi[h];
            if (!(lo > -inf && hi < inf && lo <= hi)) msg = "lo, hi of a tuned hyperparameter: finite, lo <= hi";
            else if (kind == ADC_PBT_PG && h == 2) { if (!(hi < 1.0f)) msg = "eps_clip: hi below 1"; }
            else if ((kind == ADC_PBT_TD3 || kind == ADC_PBT_SAC) && h == 3) { if (!(lo > 0.0f && hi <= 1.0f)) msg = "tau: lo above 0, hi at most 1"; }
            else if (kind == ADC_PBT_TD3 && h == adc::kPbtSigma) { }
            else if (kind == ADC_PBT_SAC && (h == adc::kPbtAlpha || h == 5)) { }        // (log_alpha and target_entropy: any sign)
            else if (!(lo >= 0.0f)) msg = "lo of a learning rate, a coefficient or a noise: at least 0";
        }
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_pbt_fitness_host(int32_t days, int32_t num_envs, int32_t members, const float *reward_tn, double *fitness_m)
{
    if (days < 1 || num_envs < 1 || members < 1 || num_envs % members != 0 || !reward_tn || !fitness_m) return ADC_EINVAL;
    const size_t N = (size_t)num_envs;
    const int n = num_envs / members;
    for (int m = 0; m < members; ++m) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const size_t env = (size_t)m * (size_t)n + (size_t)i;
            double ret = 0.0;
            for (int t = 0; t < days; ++t) ret = adc::pbt_chain(ret, (double)reward_tn[(size_t)t * N + env]);
            acc = adc::pbt_chain(acc, ret);
        }
        fitness_m[m] = adc::pbt_fitness_finish(acc, n);
    }
    return ADC_OK;
}

ADC_EXPORT int adc_pbt_plan_host(const adc_pbt_config *cfg, uint64_t seed, int32_t members, int64_t round, const double *fitness_m, double *smoothed_m,
                                 int32_t *rank_m, int32_t *src_m, uint32_t *bits_m)
{
    if (!cfg || cfg->struct_size != sizeof(adc_pbt_config) || members < 2 || cfg->replace_count < 1 || cfg->replace_count > members / 2 ||
        !(cfg->fitness_ema >= 0.0f && cfg->fitness_ema < 1.0f) || round < 0 || round >= 0xFFFFFFFFll || !fitness_m || !smoothed_m || !rank_m || !src_m)
        return ADC_EINVAL;
    for (int m = 0; m < members; ++m) smoothed_m[m] = adc::pbt_smooth(cfg->fitness_ema, smoothed_m[m], fitness_m[m], round == 0);
    adc::pbt_plan(adc::pbt_key(seed), (uint32_t)round, cfg->replace_count, smoothed_m, members, rank_m, src_m, bits_m);
    return ADC_OK;
}

ADC_EXPORT int adc_pbt_explore_host(const adc_pbt_config *cfg, int32_t kind, uint32_t bits, const float *donor_hp8, const float *own_hp8, float *out_hp8)
{
    if (!cfg || cfg->struct_size != sizeof(adc_pbt_config) || (kind != ADC_PBT_PG && kind != ADC_PBT_TD3 && kind != ADC_PBT_SAC) || !donor_hp8 || !own_hp8 || !out_hp8)
        return ADC_EINVAL;
    for (int h = 0; h < adc::kPbtMaxHp; ++h) {
        const int up = (int)((bits >> h) & 1u);
        if (!((cfg->tuned_mask >> h) & 1u)) out_hp8[h] = own_hp8[h];
        else if (kind == ADC_PBT_SAC && h == adc::kPbtAlpha) out_hp8[h] = own_hp8[h];      // (the temperature cell is the device's: k_pbt_exploit_cell)
        else if (kind == ADC_PBT_TD3 && h == adc::kPbtSigma)
            out_hp8[h] = adc::pbt_explore_log(donor_hp8[h], up ? cfg->log_factor_hi : cfg->log_factor_lo, cfg->lo[h], cfg->hi[h]);
        else out_hp8[h] = adc::pbt_explore(donor_hp8[h], up, cfg->factor_lo, cfg->factor_hi, cfg->lo[h], cfg->hi[h]);
    }
    return ADC_OK;
}
