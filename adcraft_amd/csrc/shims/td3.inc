// td3.inc (part of adc_shims.cpp) - off-policy (TD3) training on the host (adc_td3.h: the code parts/kernel_td3.inc runs), over shims/offpolicy.inc
ADC_EXPORT int adc_td3_config_check(const adc_td3_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_td3_config)) msg = "adc_td3_config: NULL or struct_size mismatch";
    else if ((msg = offpolicy_discount_clause(*cfg))) { }
    else if (cfg->policy_delay < 1) msg = "policy_delay >= 1";
    else if (!(cfg->target_noise >= 0.0f && cfg->target_noise < inf)) msg = "target_noise >= 0";
    else if (!(cfg->target_noise_clip >= 0.0f && cfg->target_noise_clip < inf)) msg = "target_noise_clip >= 0";
    else if (cfg->action_lo != cfg->action_lo || cfg->action_hi != cfg->action_hi) msg = "action_lo / action_hi must not be NaN (hi <= lo: no clamp)";
    else msg = offpolicy_training_clause(*cfg);
    return config_verdict(msg, message);
}

ADC_EXPORT int adc_td3_pop_config_check(const adc_td3_config *cfgs, int32_t count, int32_t num_envs, int32_t members, const char **message)
{
    const char *msg = pop_config_clause(
        cfgs, count, members, num_envs >= 1 && members >= 1 && members <= 65535 && num_envs % members == 0, "adc_td3_config array is NULL",
        "members must be positive, at most 65535, and divide num_envs", adc_td3_config_check, [](const adc_td3_config &c, const adc_td3_config &c0) {
            return offpolicy_unequal(c, c0, c.policy_delay == c0.policy_delay,
                                     "policy_delay must be equal in all members' configurations (their actor steps run in the same launches)");
        });
    return config_verdict(msg, message);
}

namespace {
// the shape two configurations give, or false: a bad configuration or a two-headed policy
bool td3_host_shape(const adc_mlp_config *mlp, int32_t K, const adc_td3_config *cfg, bool norm, adc::Td3Shape *sh)
{
    if (adc_mlp_config_check(mlp, K, nullptr) != ADC_OK || adc_td3_config_check(cfg, nullptr) != ADC_OK) return false;
    if (mlp->policy_widths[mlp->n_policy_layers - 1] != K + 1) return false;
    *sh = adc::td3_shape_of(*mlp, K, *cfg, norm ? 1 : 0);
    return true;
}
}  // namespace

ADC_EXPORT int adc_td3_param_counts_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, int64_t *actor_p, int64_t *critic_qc)
{
    adc::Td3Shape sh;
    if (!td3_host_shape(mlp, num_keywords, cfg, false, &sh)) return ADC_EINVAL;
    if (actor_p) *actor_p = adc::td3_params(sh.pol);
    if (critic_qc) *critic_qc = adc::td3_params(sh.q);
    return ADC_OK;
}

ADC_EXPORT int adc_td3_batch_indices_host(uint64_t seed, int64_t update, int64_t size, int32_t count, int32_t *idx_b)
{
    if (update < 0 || update >= 0xFFFFFFFFll || size < 1 || size > (1ll << 30) || count < 1 || !idx_b) return ADC_EINVAL;
    const uint64_t key = adc::td3_key(seed);
    for (int32_t b = 0; b < count; ++b) idx_b[b] = (int32_t)adc::td3_batch_index(key, (uint32_t)b, (uint32_t)update, (uint32_t)size);
    return ADC_OK;
}

namespace {
// adc_td3_target_host; bounded: under adc_td3.h "bounded" (shift_a and scale_a NULL)
int td3_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, uint64_t seed, int64_t update,
                    const float *theta_target_p, const float *psi_target_q, const float *shift_a, const float *scale_a, int32_t count,
                    const float *x2_bd, const float *r_b, const uint8_t *done_b, float *y_b, bool bounded)
{
    adc::Td3Shape sh;
    if (!td3_host_shape(mlp, num_keywords, cfg, shift_a != nullptr, &sh)) return ADC_EINVAL;
    if ((shift_a == nullptr) != (scale_a == nullptr) || update < 0 || update >= 0xFFFFFFFFll || count < 1 || !theta_target_p || !psi_target_q || !x2_bd ||
        !r_b || !done_b || !y_b)
        return ADC_EINVAL;
    const adc::Td3Law law = adc::td3_law_of(*cfg);
    const uint64_t key = adc::td3_key(seed);
    const size_t D = (size_t)sh.D, A = (size_t)sh.A;
    std::vector<float> row(D + A), yp((size_t)adc::td3_outs(sh.pol)), yq((size_t)adc::td3_outs(sh.q));
    for (int32_t b = 0; b < count; ++b) {
        std::copy(x2_bd + (size_t)b * D, x2_bd + (size_t)(b + 1) * D, row.begin());
        adc::td3_forward_host(sh.pol, sh.activation, theta_target_p, row.data(), yp.data());
        const float *mu = yp.data() + adc::td3_hidden(sh.pol);
        for (int a = 0; a < sh.A; ++a) {
            const float n = adc::td3_noise(key, a, (uint32_t)b, (uint32_t)update);
            if (bounded) { row[D + (size_t)a] = adc::td3_target_action(adc::mlp_tanh(mu[a]), n, adc::td3_law_bounded(law)); continue; }
            const float ap = adc::td3_target_action(mu[a], n, law);
            row[D + (size_t)a] = adc::td3_action_norm(ap, shift_a, scale_a, a, sh.norm);
        }
        y_b[b] = adc::td3_y(r_b[b], done_b[b], offpolicy_min_q_host(sh, psi_target_q, row.data(), yq), law);
    }
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_td3_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, uint64_t seed, int64_t update,
                                   const float *theta_target_p, const float *psi_target_q, const float *shift_a, const float *scale_a, int32_t count,
                                   const float *x2_bd, const float *r_b, const uint8_t *done_b, float *y_b)
{
    return td3_target_host(mlp, num_keywords, cfg, seed, update, theta_target_p, psi_target_q, shift_a, scale_a, count, x2_bd, r_b, done_b, y_b, false);
}

ADC_EXPORT int adc_td3_bounded_target_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, uint64_t seed, int64_t update,
                                           const float *theta_target_p, const float *psi_target_q, int32_t count, const float *x2_bd, const float *r_b,
                                           const uint8_t *done_b, float *y_b)
{
    if (cfg && cfg->action_hi > cfg->action_lo) return ADC_EINVAL;          // (the box is [-1, 1])
    return td3_target_host(mlp, num_keywords, cfg, seed, update, theta_target_p, psi_target_q, nullptr, nullptr, count, x2_bd, r_b, done_b, y_b, true);
}

ADC_EXPORT int adc_td3_critic_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *psi_q,
                                        const float *shift_a, const float *scale_a, int32_t count, const float *x_bd, const float *a_ba, const float *y_b,
                                        float *grad_q, double *sums6)
{
    adc::Td3Shape sh;
    if (!td3_host_shape(mlp, num_keywords, cfg, shift_a != nullptr, &sh)) return ADC_EINVAL;
    if ((shift_a == nullptr) != (scale_a == nullptr) || count < 1 || !psi_q || !x_bd || !a_ba || !y_b || !grad_q) return ADC_EINVAL;
    const size_t A = (size_t)sh.A;
    offpolicy_critic_grad_host(sh, psi_q, count, x_bd, y_b, grad_q, sums6,
                               [&](size_t s, size_t a) { return adc::td3_action_norm(a_ba[s * A + a], shift_a, scale_a, (int)a, sh.norm); });
    return ADC_OK;
}

namespace {
// adc_td3_actor_grad_host; bounded: under adc_td3.h "bounded" (shift_a and scale_a NULL)
int td3_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *theta_p, const float *psi_q,
                        const float *shift_a, const float *scale_a, int32_t count, const float *x_bd, float *grad_p, double *sums2, bool bounded)
{
    adc::Td3Shape sh;
    if (!td3_host_shape(mlp, num_keywords, cfg, shift_a != nullptr, &sh)) return ADC_EINVAL;
    if ((shift_a == nullptr) != (scale_a == nullptr) || count < 1 || !theta_p || !psi_q || !x_bd || !grad_p) return ADC_EINVAL;
    const size_t S = (size_t)count, D = (size_t)sh.D, A = (size_t)sh.A, po = (size_t)adc::td3_outs(sh.pol), ph = (size_t)adc::td3_hidden(sh.pol),
                 no = (size_t)adc::td3_outs(sh.q), nh = (size_t)adc::td3_hidden(sh.q);
    std::vector<float> ys(S * po), deltas(S * po), row(D + A), yq(no), dq(no), qpi(S);
    for (size_t s = 0; s < S; ++s) {
        float *y = ys.data() + s * po, *d = deltas.data() + s * po;
        std::copy(x_bd + s * D, x_bd + (s + 1) * D, row.begin());
        adc::td3_forward_host(sh.pol, sh.activation, theta_p, row.data(), y);
        for (int a = 0; a < sh.A; ++a)
            row[D + (size_t)a] = bounded ? adc::mlp_tanh(y[ph + (size_t)a]) : adc::td3_action_norm(y[ph + (size_t)a], shift_a, scale_a, a, sh.norm);
        adc::td3_forward_host(sh.q, sh.activation, psi_q, row.data(), yq.data());
        qpi[s] = yq[nh];
        dq[nh] = 1.0f;
        adc::td3_backward_host(sh.q, sh.activation, psi_q, yq.data(), dq.data());
        adc::td3_input_delta_host(sh.q, psi_q, dq.data(), sh.D, sh.A, d + ph);
        for (int a = 0; a < sh.A; ++a)
            d[ph + (size_t)a] = bounded ? adc::td3_dmu_bounded(d[ph + (size_t)a], row[D + (size_t)a])
                                        : adc::td3_dmu(d[ph + (size_t)a], sh.norm ? scale_a[a] : 0.0f, sh.norm);
        adc::td3_backward_host(sh.pol, sh.activation, theta_p, y, d);
    }
    td3_net_grad_host(sh.pol, count, x_bd, D, ys.data(), po, 0, deltas.data(), po, 0, grad_p);
    if (sums2) {
        sums2[0] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)qpi[(size_t)s]; });
        sums2[1] = adc::pg_csum((int64_t)adc::td3_params(sh.pol), [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_p[p], grad_p[p]); });
    }
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_td3_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *theta_p,
                                       const float *psi_q, const float *shift_a, const float *scale_a, int32_t count, const float *x_bd, float *grad_p,
                                       double *sums2)
{
    return td3_actor_grad_host(mlp, num_keywords, cfg, theta_p, psi_q, shift_a, scale_a, count, x_bd, grad_p, sums2, false);
}

ADC_EXPORT int adc_td3_bounded_actor_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_td3_config *cfg, const float *theta_p,
                                               const float *psi_q, int32_t count, const float *x_bd, float *grad_p, double *sums2)
{
    return td3_actor_grad_host(mlp, num_keywords, cfg, theta_p, psi_q, nullptr, nullptr, count, x_bd, grad_p, sums2, true);
}

ADC_EXPORT int adc_td3_polyak_host(float tau, int64_t n, const float *param_n, float *target_n)
{
    if (!(tau > 0.0f && tau <= 1.0f) || n < 1 || !param_n || !target_n) return ADC_EINVAL;
    for (int64_t p = 0; p < n; ++p) target_n[p] = adc::td3_polyak(target_n[p], param_n[p], tau);
    return ADC_OK;
}
