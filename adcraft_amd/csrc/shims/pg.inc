// pg.inc (part of adc_shims.cpp) - policy-gradient training on the host (adc_pg.h: the code parts/kernel_pg.inc runs): the configuration checks, GAE, the
// gradient (its core also serves shims/imitation.inc and shims/pg_kl.inc), the queued update's decision, the step
ADC_EXPORT int adc_pg_config_check(const adc_pg_config *cfg, const char **message)
{
    const char *msg = nullptr;
    const float inf = __builtin_inff();
    if (!cfg || cfg->struct_size != sizeof(adc_pg_config)) msg = "adc_pg_config: NULL or struct_size mismatch";
    else if (!(cfg->gamma >= 0.0f && cfg->gamma <= 1.0f)) msg = "gamma: 0 to 1";
    else if (!(cfg->lambda >= 0.0f && cfg->lambda <= 1.0f)) msg = "lambda: 0 to 1";
    else if (!(cfg->eps_clip < 1.0f)) msg = "eps_clip < 1 (<= 0: no clip)";
    else if (!(cfg->vf_coef >= 0.0f && cfg->vf_coef < inf)) msg = "vf_coef >= 0";
    else if (!(cfg->ent_coef >= 0.0f && cfg->ent_coef < inf)) msg = "ent_coef >= 0";
    else if (!(cfg->reward_scale != 0.0f && cfg->reward_scale > -inf && cfg->reward_scale < inf)) msg = "reward_scale must be finite and not 0";
    else if (!(cfg->max_grad_norm >= 0.0f && cfg->max_grad_norm < inf)) msg = "max_grad_norm >= 0 (0: off)";
    else if (cfg->optimiser != ADC_PG_ADAM && cfg->optimiser != ADC_PG_SGD) msg = "unknown optimiser";
    else if (!(cfg->lr >= 0.0f && cfg->lr < inf)) msg = "lr >= 0";
    else if (cfg->optimiser == ADC_PG_ADAM && (!(cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f) || !(cfg->beta2 >= 0.0f && cfg->beta2 < 1.0f)))
        msg = "Adam: 0 <= beta1, beta2 < 1";
    else if (cfg->optimiser == ADC_PG_ADAM && !(cfg->eps > 0.0f)) msg = "Adam: eps > 0";
    else if (cfg->minibatch_envs < 0) msg = "minibatch_envs >= 0 (0: all envs)";
    return config_verdict(msg, message);
}

// The frame of the three population checks (adc_pg_pop_config_check here, adc_td3_pop_config_check, adc_sac_pop_config_check): the
// configurations of a population are `count` = 1 (shared by all members) or `members` of them; each passes its own check(cfg, &msg),
// then unequal(cfg, first) names a field that must be equal in all members (or null).  members_ok and the two sentences are the
// family's.  Returns the first failing clause's sentence, or null.
template <class Config, class Check, class Unequal>
static const char *pop_config_clause(const Config *cfgs, int32_t count, int32_t members, bool members_ok, const char *null_sentence,
                                     const char *members_sentence, Check check, Unequal unequal)
{
    if (!cfgs) return null_sentence;
    if (!members_ok) return members_sentence;
    if (count != 1 && count != members) return "count: 1 (one configuration shared by all members) or the number of members";
    for (int i = 0; i < count; ++i) {
        const char *msg = nullptr;
        if (check(cfgs + i, &msg) != ADC_OK) return msg;
        if ((msg = unequal(cfgs[i], cfgs[0]))) return msg;
    }
    return nullptr;
}

ADC_EXPORT int adc_pg_pop_config_check(const adc_pg_config *cfgs, int32_t count, int32_t num_envs, int32_t members, const char **message)
{
    const char *msg = pop_config_clause(
        cfgs, count, members, num_envs >= 1 && members >= 1 && num_envs % members == 0, "adc_pg_config array is NULL", "members must be positive and divide num_envs",
        adc_pg_config_check, [](const adc_pg_config &c, const adc_pg_config &c0) {
            return c.minibatch_envs != c0.minibatch_envs ? "minibatch_envs must be equal in all members' configurations (their minibatches run in the same launches)"
                                                         : (const char *)nullptr;
        });
    if (!msg) {
        const int n = num_envs / members, mb = cfgs[0].minibatch_envs == 0 ? n : cfgs[0].minibatch_envs;
        if (mb > n || n % mb != 0) msg = "minibatch_envs must divide the envs of a member (num_envs / members)";
    }
    return config_verdict(msg, message);
}

// GAE over the record, env by env from the last day back, then the advantages' normalisation; day(i, n, done, v, next, gl, adv): one
// day of env n at row i under the form's own law function
template <class Day>
static void pg_gae_host_run(const adc_pg_config *cfg, int32_t days, int32_t num_envs, const uint8_t *terminated_tn, const uint8_t *truncated_tn,
                            const float *value_tn, const float *bootstrap_n, float *adv_tn, float *ret_tn, Day day)
{
    const size_t N = (size_t)num_envs;
    const float gl = cfg->gamma * cfg->lambda;
    for (size_t n = 0; n < N; ++n) {
        float adv = 0.0f, next = bootstrap_n[n];
        for (int t = days - 1; t >= 0; --t) {
            const size_t i = (size_t)t * N + n;
            const float v = value_tn[i];
            const float a = day(i, n, terminated_tn[i] | truncated_tn[i], v, next, gl, adv);
            adv_tn[i] = a;
            ret_tn[i] = a + v;
            next = v;
        }
    }
    if (cfg->normalize_advantages) {
        const int64_t cnt = (int64_t)days * num_envs;
        const double mean = adc::pg_csum(cnt, [&](double part, int64_t i) { return part + (double)adv_tn[i]; }) / (double)cnt;
        const double var = adc::pg_csum(cnt, [&](double part, int64_t i) { return adc::pg_chain_sqdev(part, adv_tn[i], mean); }) / (double)cnt;
        const double sd = std::sqrt(var);
        for (int64_t i = 0; i < cnt; ++i) adv_tn[i] = adc::pg_normalized(adv_tn[i], mean, sd);
    }
}

ADC_EXPORT int adc_pg_gae_host(const adc_pg_config *cfg, int32_t days, int32_t num_envs, const float *reward_tn, const uint8_t *terminated_tn,
                               const uint8_t *truncated_tn, const float *value_tn, const float *bootstrap_n, float *adv_tn, float *ret_tn)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (days < 1 || num_envs < 1 || !reward_tn || !terminated_tn || !truncated_tn || !value_tn || !bootstrap_n || !adv_tn || !ret_tn) return ADC_EINVAL;
    pg_gae_host_run(cfg, days, num_envs, terminated_tn, truncated_tn, value_tn, bootstrap_n, adv_tn, ret_tn,
                    [&](size_t i, size_t, int done, float v, float next, float gl, float &adv) {
                        return adc::pg_gae_day(reward_tn[i], cfg->reward_scale, done, v, next, cfg->gamma, gl, adv);
                    });
    return ADC_OK;
}

// under a reward normaliser's multipliers scale_n and clip (adc_rew_norm.h)
ADC_EXPORT int adc_pg_gae_norm_host(const adc_pg_config *cfg, int32_t days, int32_t num_envs, const float *reward_tn, const uint8_t *terminated_tn,
                                    const uint8_t *truncated_tn, const float *value_tn, const float *bootstrap_n, const float *scale_n, float clip,
                                    float *adv_tn, float *ret_tn)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (days < 1 || num_envs < 1 || !reward_tn || !terminated_tn || !truncated_tn || !value_tn || !bootstrap_n || !scale_n || !adv_tn || !ret_tn ||
        !(clip >= 0.0f))
        return ADC_EINVAL;
    pg_gae_host_run(cfg, days, num_envs, terminated_tn, truncated_tn, value_tn, bootstrap_n, adv_tn, ret_tn,
                    [&](size_t i, size_t n, int done, float v, float next, float gl, float &adv) {
                        return adc::rew_norm_gae_day(reward_tn[i], cfg->reward_scale, scale_n[n], clip, done, v, next, cfg->gamma, gl, adv);
                    });
    return ADC_OK;
}

ADC_EXPORT int adc_pg_param_count_host(const adc_mlp_config *mlp, int32_t num_keywords, int64_t *count)
{
    if (!count || adc_mlp_config_check(mlp, num_keywords, nullptr) != ADC_OK) return ADC_EINVAL;
    *count = adc::pg_param_count(adc::pg_shape_of(*mlp, num_keywords));
    return ADC_OK;
}

namespace {
// the gradient of `count` samples; addon_of(s): the sample's add-on (adc::PgNoAddon, or adc_pg_kl.h's)
// (`loss`: the configuration's constants - adc_pg_config's, or the imitation loss's vf_coef alone)
template <class AddonOf>
int pg_grad_host_core(const adc_mlp_config *mlp, int32_t num_keywords, const adc::PgLoss &loss, const float *theta_q, int64_t count, const float *obs_sd,
                      const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s, const float *value_old_s, float *grad_q,
                      double *sums10, adc_pg_stats *stats, AddonOf addon_of)
{
    if (adc_mlp_config_check(mlp, num_keywords, nullptr) != ADC_OK) return ADC_EINVAL;
    if (count < 1 || count > 0x7FFFFFFFll || !theta_q || !obs_sd || !action_sa || !logp_old_s || !adv_s || !ret_s || !value_old_s || !grad_q) return ADC_EINVAL;
    const adc::PgShape sh = adc::pg_shape_of(*mlp, num_keywords);
    const size_t S = (size_t)count, na = (size_t)adc::pg_acts_floats(sh), nd = (size_t)adc::pg_deltas_floats(sh), D = (size_t)sh.D, A = (size_t)sh.A;
    std::vector<float> acts(S * std::max<size_t>(na, 1)), deltas(S * nd), pieces(S * adc::kPgPieces);
    for (size_t s = 0; s < S; ++s)
        adc::pg_sample_host_with(sh, loss, theta_q, obs_sd + s * D, action_sa + s * A, logp_old_s[s], adv_s[s], ret_s[s], value_old_s[s],
                                 acts.data() + s * na, deltas.data() + s * nd, pieces.data() + s * adc::kPgPieces, addon_of(s));
    // the gradient's terms in the flat order: every layer (its bias the row j = n_in with x = 1), then log_std's row
    size_t q = 0, ao = 0, dof = 0;
    auto term = [&](const float *X, size_t ldx, int n_in, size_t d_off, int n_out) {
        for (int j = 0; j <= n_in; ++j)
            for (int h = 0; h < n_out; ++h) {
                const double total = adc::pg_csum(count, [&](double part, int64_t s) {
                    return adc::pg_chain_mac(part, j < n_in ? X[(size_t)s * ldx + (size_t)j] : 1.0f, deltas[(size_t)s * nd + d_off + (size_t)h]);
                });
                grad_q[q++] = adc::pg_grad_finish(total, count);
            }
    };
    for (int net = 0; net < 2; ++net) {
        for (int l = 0; l < sh.layers[net]; ++l) {
            const int n_in = adc::pg_n_in(sh, net, l), n_out = sh.n_out[net][l];
            if (l == 0) term(obs_sd, D, n_in, dof, n_out);
            else { term(acts.data() + ao, na, n_in, dof, n_out); ao += (size_t)n_in; }
            dof += (size_t)n_out;
        }
    }
    if (!sh.two_heads) term(nullptr, 0, 0, dof, sh.A);
    double sums[adc::kPgSums];
    for (int c = 0; c < 7; ++c) sums[c] = adc::pg_csum(count, [&](double part, int64_t s) { return part + (double)pieces[(size_t)s * adc::kPgPieces + (size_t)c]; });
    for (int c = 0; c < 2; ++c)
        sums[7 + c] = adc::pg_csum(count, [&](double part, int64_t s) {
            const float x = pieces[(size_t)s * adc::kPgPieces + (size_t)(adc::kPgRet + c)];
            return adc::pg_chain_mac(part, x, x);
        });
    sums[9] = adc::pg_csum((int64_t)q, [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_q[p], grad_q[p]); });
    if (sums10) std::copy(sums, sums + adc::kPgSums, sums10);
    if (stats) {
        const adc::PgStatsOut o = adc::pg_stats_finish(sums, count);
        stats->steps = 0; stats->samples = count;
        stats->policy_loss = o.policy_loss; stats->value_loss = o.value_loss; stats->entropy = o.entropy; stats->approx_kl = o.approx_kl;
        stats->clip_fraction = o.clip_fraction; stats->grad_norm = o.grad_norm; stats->explained_variance = o.explained_variance;
    }
    return ADC_OK;
}
template <class AddonOf>
int pg_grad_host_run(const adc_mlp_config *mlp, int32_t num_keywords, const adc_pg_config *cfg, const float *theta_q, int64_t count, const float *obs_sd,
                     const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s, const float *value_old_s, float *grad_q,
                     double *sums10, adc_pg_stats *stats, AddonOf addon_of)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    return pg_grad_host_core(mlp, num_keywords, adc::PgLoss{cfg->eps_clip, cfg->vf_coef, cfg->ent_coef}, theta_q, count, obs_sd, action_sa, logp_old_s, adv_s,
                             ret_s, value_old_s, grad_q, sums10, stats, addon_of);
}
}  // namespace

ADC_EXPORT int adc_pg_grad_host(const adc_mlp_config *mlp, int32_t num_keywords, const adc_pg_config *cfg, const float *theta_q, int64_t count,
                                const float *obs_sd, const float *action_sa, const float *logp_old_s, const float *adv_s, const float *ret_s,
                                const float *value_old_s, float *grad_q, double *sums10, adc_pg_stats *stats)
{
    return pg_grad_host_run(mlp, num_keywords, cfg, theta_q, count, obs_sd, action_sa, logp_old_s, adv_s, ret_s, value_old_s, grad_q, sums10, stats,
                            [](size_t) { return adc::PgNoAddon{}; });
}

// the host twin of k_pg_decide (parts/kernel_pg_queued.inc): adc_pg_shuffle.h's pg_decide on a live member's minibatch
ADC_EXPORT int adc_pg_decide_host(const adc_pg_config *cfg, float target_kl, const double *sums10, int64_t count, int32_t *evaluated, int32_t *stop,
                                  int32_t *clip, float *scale)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (!sums10 || count < 1 || !(target_kl >= 0.0f && target_kl < __builtin_inff())) return ADC_EINVAL;
    const adc::PgDecision d = adc::pg_decide(cfg->max_grad_norm, target_kl, 1, sums10, count);
    if (evaluated) *evaluated = 1;
    if (stop) *stop = d.stop;
    if (clip) *clip = d.clip;
    if (scale) *scale = d.scale;
    return ADC_OK;
}

ADC_EXPORT int adc_pg_step_host(const adc_pg_config *cfg, int64_t n_params, int64_t steps_taken, const float *grad_q, float *theta_q, float *m_q,
                                float *v_q)
{
    if (adc_pg_config_check(cfg, nullptr) != ADC_OK) return ADC_EINVAL;
    if (n_params < 1 || n_params > 0x7FFFFFFFll || steps_taken < 0 || steps_taken >= 0x7FFFFFFFll || !grad_q || !theta_q || !m_q || !v_q) return ADC_EINVAL;
    const adc::EsStep step = shim_opt_step(cfg->optimiser == ADC_PG_SGD, cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, 0.0f, steps_taken);
    const bool clip = cfg->max_grad_norm > 0.0f;
    float scale = 1.0f;
    if (clip) {
        const double sq = adc::pg_csum(n_params, [&](double part, int64_t p) { return adc::pg_chain_mac(part, grad_q[p], grad_q[p]); });
        scale = adc::pg_clip_scale(cfg->max_grad_norm, std::sqrt(sq));
    }
    for (int64_t p = 0; p < n_params; ++p) {
        const float g = clip ? grad_q[p] * scale : grad_q[p];
        theta_q[p] = adc::pg_apply(step, theta_q[p], g, m_q[p], v_q[p]);
    }
    return ADC_OK;
}
