// sac.inc (part of adc_shims.cpp) - soft actor-critic on the host (adc_sac.h: the code parts/kernel_sac.inc runs), over shims/offpolicy.inc
ADC_EXPORT int adc_sac_config_check(const adc_sac_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_sac_config)) msg = "adc_sac_config: NULL or struct_size mismatch";
    else if ((msg = offpolicy_discount_clause(*cfg))) { }
    else if (cfg->target_update_interval < 1) msg = "target_update_interval >= 1";
    else if (!(cfg->init_alpha > 0.0f && cfg->init_alpha < inf)) msg = "init_alpha: above 0, finite";
    else if (!(cfg->target_entropy > -inf && cfg->target_entropy < inf)) msg = "target_entropy must be finite";
    else if (!(cfg->alpha_lr >= 0.0f && cfg->alpha_lr < inf)) msg = "alpha_lr >= 0 (0: alpha stays)";
    else if (!(cfg->eps_sq > 0.0f && cfg->eps_sq < inf)) msg = "eps_sq: above 0, finite";
    else msg = offpolicy_training_clause(*cfg);
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_sac_pop_config_check(const adc_sac_config *cfgs, int32_t count, int32_t num_envs, int32_t members, const char **message)
{
    const char *msg = pop_config_clause(
        cfgs, count, members, num_envs >= 1 && members >= 1 && members <= 65535 && num_envs % members == 0, "adc_sac_config array is NULL",
        "members must be positive, at most 65535, and divide num_envs", adc_sac_config_check, [](const adc_sac_config &c, const adc_sac_config &c0) {
            return offpolicy_unequal(c, c0, c.target_update_interval == c0.target_update_interval,
                                     "target_update_interval must be equal in all members' configurations (their target steps run in the same launches)");
        });
    return config_verdict(msg, message);
}

namespace {
// the shape two configurations give, or false: a bad configuration, a free-head policy or one without the clamp
bool sac_host_shape(const adc_mlp_config *mlp, int32_t K, const adc_sac_config *cfg, adc::Td3Shape *sh)
{
    if (adc_mlp_config_check(mlp, K, nullptr) != ADC_OK || adc_sac_config_check(cfg, nullptr) != ADC_OK) return false;
    if (mlp->policy_widths[mlp->n_policy_layers - 1] != 2 * (K + 1) || !mlp->clamp_log_std) return false;
    *sh = adc::sac_shape_of(*mlp, K, *cfg);
    return true;
}
}  // namespace

ADC_EXPORT int adc_sac_param_counts_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, int64_t *actor_p, int64_t *critic_qc)
{
    adc::Td3Shape sh;
    if (!sac_host_shape(mlp, num_keywords, cfg, &sh)) return ADC_EINVAL;
    if (actor_p) *actor_p = adc::td3_params(sh.pol);
    if (critic_qc) *critic_qc = adc::td3_params(sh.q);
    return ADC_OK;
}

ADC_EXPORT int adc_sac_logp_host(const adc_mlp_config *mlp, int32_t num_keywords, float eps_sq, int32_t count, const float *mean_ba, const float *raw_ba,
                                 const float *z_ba, float *u_ba, float *t_ba, float *lp_b)
{
    if (adc_mlp_config_check(mlp, num_keywords, nullptr) != ADC_OK || !mlp->clamp_log_std || !(eps_sq > 0.0f) || count < 1 || !mean_ba || !raw_ba || !z_ba ||
        !lp_b)
        return ADC_EINVAL;
    const int A = num_keywords + 1;
    const adc::SacLaw law{0.0f, 0.0f, 0.0f, eps_sq, mlp->log_std_lo, mlp->log_std_hi};
    std::vector<adc::SacHead> heads((size_t)A);
    std::vector<float> o((size_t)2 * A);
    for (int32_t b = 0; b < count; ++b) {
        std::copy(mean_ba + (size_t)b * A, mean_ba + (size_t)(b + 1) * A, o.begin());
        std::copy(raw_ba + (size_t)b * A, raw_ba + (size_t)(b + 1) * A, o.begin() + A);
        lp_b[b] = adc::sac_heads_host(o.data(), A, 0, 0, 0, 0, law, heads.data(), z_ba + (size_t)b * A);
        for (int a = 0; a < A; ++a) {
            if (u_ba) u_ba[(size_t)b * A + a] = heads[(size_t)a].u;
            if (t_ba) t_ba[(size_t)b * A + a] = heads[(size_t)a].t;
        }
    }
    return ADC_OK;
}

ADC_EXPORT int adc_sac_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, uint64_t seed, int64_t update, float alpha,
                                   const float *theta_p, const float *psi_target_q, int32_t count, const float *x2_bd, const float *r_b,
                                   const uint8_t *done_b, float *y_b, float *lp_b)
{
    adc::Td3Shape sh;
    if (!sac_host_shape(mlp, num_keywords, cfg, &sh)) return ADC_EINVAL;
    if (update < 0 || update >= 0xFFFFFFFFll || count < 1 || !theta_p || !psi_target_q || !x2_bd || !r_b || !done_b || !y_b) return ADC_EINVAL;
    const adc::SacLaw law = adc::sac_law_of(*mlp, *cfg);
    const uint64_t key = adc::td3_key(seed);
    const size_t D = (size_t)sh.D, A = (size_t)sh.A;
    std::vector<float> row(D + A), yp((size_t)adc::td3_outs(sh.pol)), yq((size_t)adc::td3_outs(sh.q));
    std::vector<adc::SacHead> heads(A);
    for (int32_t b = 0; b < count; ++b) {
        std::copy(x2_bd + (size_t)b * D, x2_bd + (size_t)(b + 1) * D, row.begin());
        adc::td3_forward_host(sh.pol, sh.activation, theta_p, row.data(), yp.data());
        const float lp = adc::sac_heads_host(yp.data() + adc::td3_hidden(sh.pol), sh.A, key, adc::ST_SAC_NEXT, (uint32_t)b, (uint32_t)update, law, heads.data(), nullptr);
        for (size_t a = 0; a < A; ++a) row[D + a] = heads[a].t;
        y_b[b] = adc::sac_y(r_b[b], done_b[b], offpolicy_min_q_host(sh, psi_target_q, row.data(), yq), alpha, lp, law);
        if (lp_b) lp_b[b] = lp;
    }
    return ADC_OK;
}

ADC_EXPORT int adc_sac_critic_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, const float *psi_q, int32_t count,
                                        const float *x_bd, const float *u_ba, const float *y_b, float *grad_q, double *sums6)
{
    adc::Td3Shape sh;
    if (!sac_host_shape(mlp, num_keywords, cfg, &sh)) return ADC_EINVAL;
    if (count < 1 || !psi_q || !x_bd || !u_ba || !y_b || !grad_q) return ADC_EINVAL;
    const size_t A = (size_t)sh.A;
    offpolicy_critic_grad_host(sh, psi_q, count, x_bd, y_b, grad_q, sums6, [&](size_t s, size_t a) { return adc::mlp_tanh(u_ba[s * A + a]); });
    return ADC_OK;
}

ADC_EXPORT int adc_sac_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_sac_config *cfg, uint64_t seed, int64_t update, float alpha,
                                       const float *theta_p, const float *psi_q, int32_t count, const float *x_bd, float *grad_p, float *lp_b, double *sums4)
{
    adc::Td3Shape sh;
    if (!sac_host_shape(mlp, num_keywords, cfg, &sh)) return ADC_EINVAL;
    if (update < 0 || update >= 0xFFFFFFFFll || count < 1 || !theta_p || !psi_q || !x_bd || !grad_p) return ADC_EINVAL;
    const adc::SacLaw law = adc::sac_law_of(*mlp, *cfg);
    const uint64_t key = adc::td3_key(seed);
    const size_t S = (size_t)count, D = (size_t)sh.D, A = (size_t)sh.A, po = (size_t)adc::td3_outs(sh.pol), ph = (size_t)adc::td3_hidden(sh.pol),
                 no = (size_t)adc::td3_outs(sh.q), nh = (size_t)adc::td3_hidden(sh.q), Qc = (size_t)adc::td3_params(sh.q);
    std::vector<float> ys(S * po), deltas(S * po), row(D + A), yq(2 * no), dq(no), gq(A), loss(S), lps(S);
    std::vector<adc::SacHead> heads(A);
    int64_t picked2 = 0;
    for (size_t s = 0; s < S; ++s) {
        float *y = ys.data() + s * po, *d = deltas.data() + s * po;
        std::copy(x_bd + s * D, x_bd + (s + 1) * D, row.begin());
        adc::td3_forward_host(sh.pol, sh.activation, theta_p, row.data(), y);
        const float lp = adc::sac_heads_host(y + ph, sh.A, key, adc::ST_SAC_PI, (uint32_t)s, (uint32_t)update, law, heads.data(), nullptr);
        for (size_t a = 0; a < A; ++a) row[D + a] = heads[a].t;
        for (size_t i = 0; i < 2; ++i) adc::td3_forward_host(sh.q, sh.activation, psi_q + i * Qc, row.data(), yq.data() + i * no);
        const size_t pick = (size_t)adc::sac_pick(yq[nh], yq[no + nh]);
        picked2 += (int64_t)pick;
        const float *psi = psi_q + pick * Qc, *yk = yq.data() + pick * no;
        dq[nh] = 1.0f;
        adc::td3_backward_host(sh.q, sh.activation, psi, yk, dq.data());
        adc::td3_input_delta_host(sh.q, psi, dq.data(), sh.D, sh.A, gq.data());
        for (size_t a = 0; a < A; ++a) {
            const adc::SacHead &h = heads[a];
            const float z = adc::sac_noise(key, adc::ST_SAC_PI, (int)a, (uint32_t)s, (uint32_t)update);
            const float du = adc::sac_du(h.t, h.w, gq[a], alpha, law.eps_sq);
            d[ph + a] = du;
            d[ph + A + a] = adc::sac_dls(du, h.sd, z, alpha, h.moved);
        }
        adc::td3_backward_host(sh.pol, sh.activation, theta_p, y, d);
        loss[s] = adc::sac_pi_loss(alpha, lp, yk[nh]);
        lps[s] = lp;
        if (lp_b) lp_b[s] = lp;
    }
    td3_net_grad_host(sh.pol, count, x_bd, D, ys.data(), po, 0, deltas.data(), po, 0, grad_p);
    if (sums4) {
        sums4[0] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)loss[(size_t)s]; });
        sums4[1] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)lps[(size_t)s]; });
        sums4[2] = adc::pg_csum((int64_t)adc::td3_params(sh.pol), [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_p[p], grad_p[p]); });
        sums4[3] = (double)picked2;
    }
    return ADC_OK;
}

ADC_EXPORT float adc_sac_log_alpha_init_host(float init_alpha) { return adc::sac_log_alpha_init(init_alpha); }

ADC_EXPORT int adc_sac_alpha_step_host(const adc_sac_config *cfg, int64_t steps_taken, double lp_sum, int32_t count, float *la3, float *alpha)
{
    if (adc_sac_config_check(cfg, nullptr) != ADC_OK || steps_taken < 0 || steps_taken >= 0x7FFFFFFFll || count < 1 || !la3) return ADC_EINVAL;
    float a = adc::mlp_exp(la3[0]);
    if (cfg->alpha_lr > 0.0f) {
        const adc::EsStep step = shim_opt_step(cfg->optimiser == ADC_TD3_SGD, cfg->alpha_lr, cfg->beta1, cfg->beta2, cfg->eps, 0.0f, steps_taken);
        la3[0] = adc::sac_alpha_step(step, la3[0], adc::sac_alpha_grad(lp_sum, count, cfg->target_entropy), la3[1], la3[2], a);
    }
    if (alpha) *alpha = a;
    return ADC_OK;
}
