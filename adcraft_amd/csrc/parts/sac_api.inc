// sac_api.inc - the extern "C" entry points of soft actor-critic training (include/adcraft_engine.h; the kernels are
// parts/kernel_sac.inc, the law csrc/adc_sac.h).  The learner lives in the off-policy trainer's fields (host_api.inc: the ring,
// the critics, their targets, the scratch, the flat vectors and moments) and shares parts/offpolicy_core.inc with TD3; SAC and TD3
// exclude each other.  Here are SAC's own refusals, its view, its update, the temperature cell and its statistics.  Everything
// here runs on the engine's own stream behind ENGINE_GUARD.
// (part of the single translation unit adc_engine.hip)
namespace {
int sac_ready(const adc_engine *e)
{
    if (!e->have_sac) return fail(ADC_ESTATE, "adc_engine_sac_init has not been called (or the policy / the record was re-initialised since)");
    return ADC_OK;
}
// what a soft actor-critic call needs of the engine's state, checked at init and again at every call
int sac_state_check(const adc_engine *e)
{
    if (int rc = mlp_ready(e)) return rc;
    if (int rc = gru_refuses(e, "soft actor-critic training")) return rc;
    if (e->mp.bd_lo) return fail(ADC_ESTATE, "soft actor-critic training under the bounded act is not supported: it needs a log-probability (adc_engine_mlp_set_bounds(NULL, NULL) first)");
    if (!e->mp.two_heads) return fail(ADC_ESTATE, "SAC needs the two-headed policy (2A outputs: means, log-stds): the free log_std head is not supported");
    if (!e->mp.clamp) return fail(ADC_ESTATE, "SAC needs clamp_log_std on: the log-std head is unbounded without it");
    if (!e->mp.sq_lo) return fail(ADC_ESTATE, "SAC needs the squashed action (adc_engine_mlp_set_squash)");
    if (e->pop_M != 0) return fail(ADC_ESTATE, "soft actor-critic training with a population active is not supported (adc_engine_mlp_population(0) first)");
    if (e->lrn_M != 0) return fail(ADC_ESTATE, "soft actor-critic training with learners active is not supported (adc_engine_mlp_learners(0) first)");
    if (e->ro_T == 0) return fail(ADC_ESTATE, "soft actor-critic training needs a rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "soft actor-critic training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    return ADC_OK;
}
// the fields of the configuration that the shared helpers read from td3_cfg
adc_td3_config sac_as_td3(const adc_sac_config &c)
{
    adc_td3_config t{};
    t.struct_size = sizeof(t);
    t.gamma = c.gamma; t.tau = c.tau; t.policy_delay = 1; t.reward_scale = c.reward_scale;
    t.batch_size = c.batch_size; t.capacity = c.capacity; t.n_critic_layers = c.n_critic_layers;
    for (int l = 0; l < 4; ++l) t.critic_widths[l] = c.critic_widths[l];
    t.actor_lr = c.actor_lr; t.critic_lr = c.critic_lr; t.beta1 = c.beta1; t.beta2 = c.beta2; t.eps = c.eps;
    t.optimiser = c.optimiser; t.max_grad_norm = c.max_grad_norm; t.seed = c.seed;
    return t;
}
// the running normalisers' side of a batch kernel's view (all null without adc_engine_sac_norm_init: sac_norm_on is false and the
// NORM = false instantiations of the batch kernels are launched, the kernels as they were)
inline bool sac_norm_on(const SacView &p) { return p.n_shift || p.r_scale; }
void sac_norm_fill(const adc_engine *e, SacView &p)
{
    if (!e->sn.live) return;
    if (e->sn.obs.count) { p.n_shift = e->mp.shift; p.n_scale = e->mp.scale; p.n_stride = e->mp.norm_stride; }
    if (e->sn.rew.count) { p.r_scale = e->sn.rew.scale; p.r_stride = e->sn_cfg.per_member ? 1 : 0; p.r_clip = e->sn_cfg.rew_clip; }
}
SacView sac_view(const adc_engine *e)
{
    SacView p{};
    p.sh = e->td3_shape;
    p.law = e->sac_law;
    p.pol = e->mp.pol;
    for (int i = 0; i < 2; ++i) { p.q[i] = e->td3_q[i]; p.q_t[i] = e->td3_q_t[i]; }
    p.cell = e->sac_cell;
    p.ring = e->td3_ring;
    p.size = (uint32_t)td3_size(e); p.update = (uint32_t)e->td3_updates;
    p.key = e->td3_key;
    p.ybuf = e->td3_ybuf; p.xin = e->td3_xin; p.acts = e->td3_acts; p.deltas = e->td3_deltas; p.pieces = e->td3_pieces;
    p.maxw = adc::td3_max_width(e->td3_shape);
    sac_norm_fill(e, p);
    td3_per_fill(e, p);
    return p;
}
// the device's sums: [0..7] the pieces (the two critic losses, Q1, Q2, y, the actor's loss piece, lp, the picks of critic 2),
// [8] the critics' grad^2, [9] the actor's grad^2
int sac_one_update(adc_engine *e, bool stats_wanted, bool last)
{
    const adc::Td3Shape &sh = e->td3_shape;
    const adc_sac_config &c = e->sac_cfg;
    const int B = c.batch_size, DA = sh.D + sh.A, nh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q), ph = adc::td3_hidden(sh.pol), po = adc::td3_outs(sh.pol);
    const size_t lds = sac_lds_floats(sh) * sizeof(float);
    SacView p = sac_view(e);
    p.na = 2 * nh; p.nd = 2 * no;
    int rc;
    if (e->per_live && (rc = per_sample_run(e, p.update))) return rc;
    const bool norm = sac_norm_on(p);
    hipLaunchKernelGGL(norm ? k_sac_target<true> : k_sac_target<false>, dim3((unsigned)B), dim3(kPgBlock), lds, e->stream, p);
    hipLaunchKernelGGL(norm ? k_sac_critic_sample<true> : k_sac_critic_sample<false>, dim3((unsigned)B), dim3(kPgBlock), lds, e->stream, p);
    for (int i = 0; i < 2; ++i) td3_wgrad_launch(e, sh.q, DA, p.na, i * nh, p.nd, i * no, i * e->td3_Qc, 2 * e->td3_Qc, B);
    HIP_TRY(hipGetLastError());
    if (e->per_live && (rc = per_leaves_run(e))) return rc;
    if ((rc = td3_step_run(e, kTd3Psi, e->td3_mom + 2, 2 * e->td3_Qc, B, stats_wanted && last, 8, c.critic_lr, e->td3_updates))) return rc;
    p.na = ph; p.nd = po;
    hipLaunchKernelGGL(norm ? k_sac_actor_sample<true> : k_sac_actor_sample<false>, dim3((unsigned)B), dim3(kPgBlock), lds, e->stream, p);
    td3_wgrad_launch(e, sh.pol, DA, p.na, 0, p.nd, 0, 0, e->td3_P, B);
    HIP_TRY(hipGetLastError());
    // (the pieces' sums of every update: the temperature's step reads lp's)
    if ((rc = td3_csum_launch(e, e->td3_pieces, B, adc::kTd3Pieces, adc::kTd3Pieces, 0, e->td3_sums))) return rc;
    if ((rc = td3_step_run(e, kTd3Theta, e->td3_mom, e->td3_P, B, stats_wanted && last, 9, c.actor_lr, e->td3_updates))) return rc;
    if (c.alpha_lr > 0.0f)
        hipLaunchKernelGGL(k_sac_alpha, dim3(1), dim3(64), 0, e->stream, e->sac_cell, e->td3_sums + adc::kSacLp, (long long)B, c.target_entropy,
                           td3_step_of(e->td3_cfg, c.alpha_lr, e->td3_updates));
    if ((e->td3_updates + 1) % c.target_update_interval == 0) {
        const PgLayout &lay = e->td3_lay[kTd3PsiT];
        hipLaunchKernelGGL(k_td3_polyak, dim3((unsigned)((lay.Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, lay, e->td3_flat[kTd3PsiT],
                           e->td3_flat[kTd3Psi], c.tau);
    }
    HIP_TRY(hipGetLastError());
    e->td3_updates += 1;
    return ADC_OK;
}
// one learner's statistics from its sums and its temperature cell
void sac_stats_fill(const adc_engine *e, const double *sums, const float *cell, adc_sac_stats *stats)
{
    const double n = (double)e->td3_cfg.batch_size;
    off_stats_fill(e, sums, stats);
    stats->actor_loss = sums[adc::kSacPiLoss] / n;
    stats->logp_mean = sums[adc::kSacLp] / n;
    stats->alpha = cell[kSacCellAlpha]; stats->log_alpha = cell[kSacCellLogAlpha];
    stats->critic_grad_norm = std::sqrt(sums[8]);
    stats->actor_grad_norm = std::sqrt(sums[9]);
}
// (flat[kTd3ThetaT] is null: there is no target actor)
int sac_state_set_check(const float *const flat[4], const float *const mom[4], const float *log_alpha3, int64_t updates)
{
    for (int w = 0; w < 4; ++w)
        if ((!flat[w] && w != kTd3ThetaT) || !mom[w]) return fail(ADC_EINVAL, "a state vector is NULL");
    if (!log_alpha3) return fail(ADC_EINVAL, "a state vector is NULL");
    if (updates < 0 || updates >= 0x7FFFFFFFll) return fail(ADC_EINVAL, "updates: 0 to 2^31 - 2");
    if (!std::isfinite(log_alpha3[0])) return fail(ADC_EINVAL, "log_alpha must be finite");
    return ADC_OK;
}
// a temperature cell {log_alpha, m, v, alpha} from its three state entries; `cell4` is the host's until the stream has been waited for
int sac_cell_upload(adc_engine *e, float *dcell, const float *log_alpha3, float *cell4)
{
    cell4[0] = log_alpha3[0]; cell4[1] = log_alpha3[1]; cell4[2] = log_alpha3[2]; cell4[3] = adc::mlp_exp(log_alpha3[0]);
    HIP_TRY(hipMemcpyAsync(dcell, cell4, 4 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_sac_init(adc_engine *e, const adc_sac_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_sac_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (int rc = sac_state_check(e)) return rc;
    if (e->have_pg || e->have_pg_pop)
        return fail(ADC_ESTATE, "a policy-gradient trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->have_td3 || e->have_td3_pop)
        return fail(ADC_ESTATE, "an off-policy (TD3) trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->on.live)
        return fail(ADC_ESTATE, "a running observation normaliser is alive on this engine: the replay ring would hold inputs normalised by older vectors");
    const adc::Td3Shape sh = adc::sac_shape_of(e->mlp_cfg, e->v.K, *cfg, mlp_frames(e));
    if (sac_lds_floats(sh) * sizeof(float) > 64u * 1024u)
        return fail(ADC_EINVAL, sac_lds_floats(adc::sac_shape_of(e->mlp_cfg, e->v.K, *cfg)) * sizeof(float) > 64u * 1024u
                                    ? "num_keywords too large for soft actor-critic training (LDS)"
                                    : "frames: the stacked input row is too large for soft actor-critic training (LDS); fewer frames fit");
    ENGINE_GUARD(e);
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    MlpNet nets[4] = {};                    // critic 1, critic 2, target critic 1, target critic 2
    OffBufs o;
    float *cell = nullptr;
    int rc;
    if ((rc = off_solo_nets(e, fresh, sh, nets, 4)) || (rc = mlp_alloc(e, fresh, &cell, (size_t)4)) ||
        (rc = off_alloc(e, fresh, sh, cfg->batch_size, (size_t)cfg->capacity, 1, false, o))) {
        mlp_free(e, fresh);
        return rc;
    }
    td3_drop(e);
    e->td3_allocs.swap(fresh);
    off_install(e, o, sh);
    e->sac_cfg = *cfg; e->td3_cfg = sac_as_td3(*cfg); e->sac_law = adc::sac_law_of(e->mlp_cfg, *cfg);
    e->td3_key = adc::td3_key(cfg->seed ? cfg->seed : e->cfg.seed);
    e->td3_q[0] = nets[0]; e->td3_q[1] = nets[1]; e->td3_q_t[0] = nets[2]; e->td3_q_t[1] = nets[3]; e->td3_pol_t = MlpNet{};
    e->td3_lay[kTd3Theta] = flat_layout(&e->mp.pol, 1);
    off_layouts(e, e->td3_q, e->td3_q_t, e->td3_pol_t);
    e->td3_a_shift = e->td3_a_scale = nullptr; e->td3_ring = o.ring;
    e->sac_cell = cell;
    // theta starts as the device's policy; the target critics as copies (zeros until the critics are uploaded and synchronised)
    const float la = adc::sac_log_alpha_init(cfg->init_alpha);
    const float cell0[4] = {la, 0.0f, 0.0f, adc::mlp_exp(la)};
    HIP_TRY(hipMemcpyAsync(cell, cell0, sizeof(cell0), hipMemcpyHostToDevice, e->stream));
    td3_params_copy(e, kTd3Theta, 1);
    if ((rc = off_sync_run(e, kOffSolo, 1, 1))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_sac = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_set_critic_layer(adc_engine *e, int32_t critic, int32_t layer, const float *weights_in_out, const float *bias_out)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sac_ready(e)) return rc;
    return off_set_critic_layer(e, kOffSolo, critic, layer, weights_in_out, bias_out);
}

ADC_EXPORT int adc_engine_sac_sync_targets(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sac_ready(e)) return rc;
    ENGINE_GUARD(e);
    if (int rc = off_sync_run(e, kOffSolo, 1, 1)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_store(adc_engine *e, int64_t *stored)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sac_ready(e)) || (rc = sac_state_check(e)) || (rc = off_store_check(e))) return rc;
    if (e->ro_teacher > 0) return fail(ADC_ESTATE, "the record holds teacher days: a soft actor-critic ring would need the pre-squash action of the teacher");
    ENGINE_GUARD(e);
    const long long count = (long long)(e->ro_t - e->td3_stored_t) * e->v.N;        // (every env is the one learner's)
    // (raw rows under a running observation normaliser - SAC's set, e->sn: the last day's x' is the raw row an act would read now)
    // (with an observation history the last day's x' is the stacked row, peeked)
    if (e->nstep_n) off_store_nstep_launch(e, false, e->sn.obs.count != 0, count);       // (n-step returns: the window's R, done and gn)
    else if (e->mp.frames > 1)
        hipLaunchKernelGGL(k_td3_store_hist, dim3((unsigned)count), dim3(kPgBlock), 0, e->stream, e->v, e->sn.obs.count ? nullptr : e->mp.shift,
                           e->sn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A, e->ro_obs, e->ro_action,
                           e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->td3_ring, (unsigned long long)e->td3_written,
                           (unsigned long long)e->td3_cfg.capacity,
                           e->mp.hist, e->mp.last, e->mp.from, e->mp.frames);
    else
        hipLaunchKernelGGL(k_td3_store, dim3((unsigned)count), dim3(kPgBlock), 0, e->stream, e->v, e->sn.obs.count ? nullptr : e->mp.shift,
                           e->sn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A, e->ro_obs, e->ro_action,
                           e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->td3_ring, (unsigned long long)e->td3_written,
                           (unsigned long long)e->td3_cfg.capacity);
    return off_store_done(e, count, stored);
}

ADC_EXPORT int adc_engine_sac_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sac_ready(e)) return rc;
    return off_buffer_info(e, size, written, capacity, nullptr);
}

ADC_EXPORT int adc_engine_sac_buffer_fetch(adc_engine *e, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done, float *x2)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sac_ready(e)) return rc;
    return off_ring_fetch(e, kOffSolo, slot, count, x, a, r, done, x2);
}

ADC_EXPORT int adc_engine_sac_buffer_load(adc_engine *e, int64_t slot, int64_t count, const float *x, const float *a, const float *r, const uint8_t *done,
                                          const float *x2, int64_t written)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sac_ready(e)) return rc;
    return off_ring_load(e, kOffSolo, slot, count, x, a, r, done, x2, written);
}

ADC_EXPORT int adc_engine_sac_batch_size(adc_engine *e, int32_t *batch_size)
{
    if (!e || !batch_size) return fail(ADC_EINVAL, "engine handle or batch_size is NULL");
    if (int rc = sac_ready(e)) return rc;
    *batch_size = e->td3_cfg.batch_size;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_batch_indices(adc_engine *e, int64_t update, int32_t *idx_b)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sac_ready(e)) return rc;
    return off_batch_indices(e, e->td3_key, update, idx_b, "the replay buffer is empty (adc_engine_sac_store)");
}

ADC_EXPORT int adc_engine_sac_update(adc_engine *e, int32_t updates, adc_sac_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = sac_ready(e)) || (rc = sac_state_check(e)) ||
        (rc = off_update_check(e, updates, false, "a critic layer has not been uploaded (adc_engine_sac_set_critic_layer)",
                               "the replay buffer is empty (adc_engine_sac_store)", 0x7FFFFFFFll)))
        return rc;
    ENGINE_GUARD(e);
    HIP_TRY(hipMemsetAsync(e->td3_sums, 0, 16 * sizeof(double), e->stream));
    // (without a norm clip nothing below waits: every step's Adam constants travel with its launch)
    for (int i = 0; i < updates; ++i)
        if ((rc = sac_one_update(e, stats != nullptr, i + 1 == updates))) return rc;
    double sums[10] = {};
    float cell[4] = {};
    if (stats) {
        HIP_TRY(hipMemcpyAsync(sums, e->td3_sums, sizeof(sums), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(cell, e->sac_cell, sizeof(cell), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats) sac_stats_fill(e, sums, cell, stats);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sac_ready(e)) return rc;
    return off_param_counts(e, actor_p, critics_2qc);
}

ADC_EXPORT int adc_engine_sac_state_get(adc_engine *e, float *theta_p, float *psi_q, float *psi_target_q, float *m_theta_p, float *v_theta_p, float *m_psi_q,
                                        float *v_psi_q, float *log_alpha3, int64_t *updates)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = sac_ready(e)) return rc;
    ENGINE_GUARD(e);
    float *flat[4] = {theta_p, psi_q, nullptr, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    if (int rc = off_state_get(e, kOffSolo, flat, mom)) return rc;
    if (log_alpha3) HIP_TRY(hipMemcpyAsync(log_alpha3, e->sac_cell, 3 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (updates) *updates = e->td3_updates;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_sac_state_set(adc_engine *e, const float *theta_p, const float *psi_q, const float *psi_target_q, const float *m_theta_p,
                                        const float *v_theta_p, const float *m_psi_q, const float *v_psi_q, const float *log_alpha3, int64_t updates)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const float *flat[4] = {theta_p, psi_q, nullptr, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    int rc;
    if ((rc = sac_ready(e)) || (rc = sac_state_set_check(flat, mom, log_alpha3, updates))) return rc;
    ENGINE_GUARD(e);
    float cell[4];
    if ((rc = sac_cell_upload(e, e->sac_cell, log_alpha3, cell))) return rc;
    return off_state_set(e, kOffSolo, flat, mom, updates);     // (waits: `cell` is the host's until then)
}
