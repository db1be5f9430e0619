// td3_api.inc - the extern "C" entry points of off-policy (TD3) training (include/adcraft_engine.h; the kernels are
// parts/kernel_td3.inc, the law csrc/adc_td3.h).  What TD3 shares with the other off-policy front ends - the ring, the critic
// upload, the state vectors, the allocation, an update's launch helpers - is parts/offpolicy_core.inc; here are TD3's own
// refusals, its view, its update and its statistics.  Everything here runs on the engine's own stream behind ENGINE_GUARD, that is
// after the env groups have joined: results do not depend on how the days were grouped.
// (part of the single translation unit adc_engine.hip)
namespace {
int td3_ready(const adc_engine *e)
{
    if (!e->have_td3) return fail(ADC_ESTATE, "adc_engine_td3_init has not been called (or the policy / the record was re-initialised since)");
    return ADC_OK;
}
// what an off-policy call needs of the engine's state, checked at init and again at every call
int td3_state_check(const adc_engine *e)
{
    if (int rc = mlp_ready(e)) return rc;
    if (int rc = gru_refuses(e, "off-policy training")) return rc;
    if (e->mp.two_heads) return fail(ADC_ESTATE, "TD3 needs the policy with the free log_std head: a two-headed policy (2A outputs) is not supported");
    if (e->pop_M != 0) return fail(ADC_ESTATE, "off-policy training with a population active is not supported (adc_engine_mlp_population(0) first)");
    if (e->lrn_M != 0) return fail(ADC_ESTATE, "off-policy training with learners active is not supported (adc_engine_mlp_learners(0) first)");
    if (e->ro_T == 0) return fail(ADC_ESTATE, "off-policy training needs a rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "off-policy training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    return ADC_OK;
}
// the running normalisers' side of a batch kernel's view (all null without adc_engine_td3_norm_init: the kernels are what they were)
void td3_norm_fill(const adc_engine *e, Td3View &p)
{
    if (!e->tn.live) return;
    if (e->tn.obs.count) { p.n_shift = e->mp.shift; p.n_scale = e->mp.scale; p.n_stride = e->mp.norm_stride; }
    if (e->tn.rew.count) { p.r_scale = e->tn.rew.scale; p.r_stride = e->tn_cfg.per_member ? 1 : 0; p.r_clip = e->tn_cfg.rew_clip; }
}
Td3View td3_view(const adc_engine *e)
{
    Td3View p{};
    p.sh = e->td3_shape;
    p.sh.norm = e->td3_norm_set ? 1 : 0;
    p.law = adc::td3_law_of(e->td3_cfg);
    p.pol = e->mp.pol; p.pol_t = e->td3_pol_t;
    for (int i = 0; i < 2; ++i) { p.q[i] = e->td3_q[i]; p.q_t[i] = e->td3_q_t[i]; }
    p.a_shift = e->td3_a_shift; p.a_scale = e->td3_a_scale;
    p.ring = e->td3_ring;
    p.size = (uint32_t)td3_size(e); p.update = (uint32_t)e->td3_updates;
    p.key = e->td3_key;
    p.ybuf = e->td3_ybuf; p.xin = e->td3_xin; p.acts = e->td3_acts; p.deltas = e->td3_deltas; p.pieces = e->td3_pieces;
    p.maxw = adc::td3_max_width(e->td3_shape);
    td3_norm_fill(e, p);
    td3_per_fill(e, p);
    return p;
}
// the device's sums: [0..4] the critic pieces, [5] the critics' grad^2, [8] Q1(x, mu(x)), [9] the actor's grad^2
int td3_one_update(adc_engine *e, bool stats_wanted, bool last, bool last_actor)
{
    const adc::Td3Shape &sh = e->td3_shape;
    const adc_td3_config &c = e->td3_cfg;
    const int B = c.batch_size, DA = sh.D + sh.A, nh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q), ph = adc::td3_hidden(sh.pol), po = adc::td3_outs(sh.pol);
    const size_t lds = td3_lds_floats(sh) * sizeof(float);
    Td3View p = td3_view(e);
    p.na = 2 * nh; p.nd = 2 * no;
    int rc;
    if (e->per_live && (rc = per_sample_run(e, p.update))) return rc;
    hipLaunchKernelGGL(e->td3_bounded ? k_td3_target_bounded : k_td3_target, dim3((unsigned)B), dim3(kPgBlock), lds, e->stream, p);
    hipLaunchKernelGGL(k_td3_critic_sample, dim3((unsigned)B), dim3(kPgBlock), lds, e->stream, p);
    for (int i = 0; i < 2; ++i) td3_wgrad_launch(e, sh.q, DA, p.na, i * nh, p.nd, i * no, i * e->td3_Qc, 2 * e->td3_Qc, B);
    HIP_TRY(hipGetLastError());
    if (e->per_live && (rc = per_leaves_run(e))) return rc;
    if (stats_wanted && last && (rc = td3_csum_launch(e, e->td3_pieces, B, adc::kTd3Pieces, 5, 0, e->td3_sums))) return rc;
    if ((rc = td3_step_run(e, kTd3Psi, e->td3_mom + 2, 2 * e->td3_Qc, B, stats_wanted && last, 5, c.critic_lr, e->td3_updates))) return rc;
    if ((e->td3_updates + 1) % c.policy_delay == 0) {
        p.na = ph; p.nd = po;
        hipLaunchKernelGGL(e->td3_bounded ? k_td3_actor_sample_bounded : k_td3_actor_sample, dim3((unsigned)B), dim3(kPgBlock), lds, e->stream, p);
        td3_wgrad_launch(e, sh.pol, DA, p.na, 0, p.nd, 0, 0, e->td3_P, B);
        HIP_TRY(hipGetLastError());
        if (stats_wanted && last_actor && (rc = td3_csum_launch(e, e->td3_pieces + adc::kTd3QPi, B, adc::kTd3Pieces, 1, 0, e->td3_sums + 8))) return rc;
        if ((rc = td3_step_run(e, kTd3Theta, e->td3_mom, e->td3_P, B, stats_wanted && last_actor, 9, c.actor_lr, e->td3_actor_steps))) return rc;
        for (int w = 0; w < 2; ++w) {
            const PgLayout &lay = e->td3_lay[kTd3ThetaT + w];
            hipLaunchKernelGGL(k_td3_polyak, dim3((unsigned)((lay.Q + kPgBlock - 1) / kPgBlock)), dim3(kPgBlock), 0, e->stream, lay, e->td3_flat[kTd3ThetaT + w],
                               e->td3_flat[kTd3Theta + w], c.tau);
        }
        HIP_TRY(hipGetLastError());
        e->td3_actor_steps += 1;
    }
    e->td3_updates += 1;
    return ADC_OK;
}
// the action inputs' shift and scale of the critics (the populations share one pair)
int td3_action_norm_run(adc_engine *e, const float *shift_a, const float *scale_a)
{
    if (!shift_a || !scale_a) return fail(ADC_EINVAL, "shift or scale is NULL");
    if (e->td3_bounded) return fail(ADC_ESTATE, "bounded TD3 with an action normalisation is not supported: the critics read the act's action in [-1, 1] as stored");
    ENGINE_GUARD(e);
    HIP_TRY(hipMemcpyAsync(e->td3_a_shift, shift_a, (size_t)e->td3_shape.A * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->td3_a_scale, scale_a, (size_t)e->td3_shape.A * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->td3_norm_set = true;
    return ADC_OK;
}
// one learner's statistics from its sums
void td3_stats_fill(const adc_engine *e, const double *sums, adc_td3_stats *stats)
{
    const double qpi = sums[8] / (double)e->td3_cfg.batch_size;
    off_stats_fill(e, sums, stats);
    stats->actor_steps = e->td3_actor_steps;
    stats->actor_loss = -qpi;
    stats->critic_grad_norm = std::sqrt(sums[5]);
    stats->actor_grad_norm = std::sqrt(sums[9]);
}
int td3_state_set_check(const float *const flat[4], const float *const mom[4], int64_t updates, int64_t actor_steps)
{
    for (int w = 0; w < 4; ++w)
        if (!flat[w] || !mom[w]) return fail(ADC_EINVAL, "a state vector is NULL");
    if (updates < 0 || updates >= 0x7FFFFFFFll || actor_steps < 0 || actor_steps > updates) return fail(ADC_EINVAL, "updates: 0 to 2^31 - 2; actor_steps: 0 to updates");
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_td3_init(adc_engine *e, const adc_td3_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const char *why = nullptr;
    if (adc_td3_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (int rc = td3_state_check(e)) return rc;
    if (e->have_sac || e->have_sac_pop) return fail(ADC_ESTATE, "a soft actor-critic trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->rn.live) return fail(ADC_ESTATE, "a running reward normaliser is alive on this engine: it belongs to the policy-gradient trainer");
    if (e->have_pg) return fail(ADC_ESTATE, "a policy-gradient trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->on.live)
        return fail(ADC_ESTATE, "a running observation normaliser is alive on this engine: the replay ring would hold inputs normalised by older vectors");
    const adc::Td3Shape sh = adc::td3_shape_of(e->mlp_cfg, e->v.K, *cfg, 0, mlp_frames(e));
    if (td3_lds_floats(sh) * sizeof(float) > 64u * 1024u)
        return fail(ADC_EINVAL, td3_lds_floats(adc::td3_shape_of(e->mlp_cfg, e->v.K, *cfg, 0)) * sizeof(float) > 64u * 1024u
                                    ? "num_keywords too large for off-policy training (LDS)"
                                    : "frames: the stacked input row is too large for off-policy training (LDS); fewer frames fit");
    ENGINE_GUARD(e);
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    MlpNet nets[5] = {};                    // critic 1, critic 2, target critic 1, target critic 2, target actor
    OffBufs o;
    float *shift = nullptr, *scale = nullptr;
    int rc;
    if ((rc = off_solo_nets(e, fresh, sh, nets, 5)) || (rc = mlp_alloc(e, fresh, &shift, (size_t)sh.A)) || (rc = mlp_alloc(e, fresh, &scale, (size_t)sh.A)) ||
        (rc = off_alloc(e, fresh, sh, cfg->batch_size, (size_t)cfg->capacity, 1, true, o))) {
        mlp_free(e, fresh);
        return rc;
    }
    td3_drop(e);
    e->td3_allocs.swap(fresh);
    off_install(e, o, sh);
    e->td3_cfg = *cfg;
    e->td3_key = adc::td3_key(cfg->seed ? cfg->seed : e->cfg.seed);
    e->td3_q[0] = nets[0]; e->td3_q[1] = nets[1]; e->td3_q_t[0] = nets[2]; e->td3_q_t[1] = nets[3]; e->td3_pol_t = nets[4];
    e->td3_lay[kTd3Theta] = flat_layout(&e->mp.pol, 1);
    off_layouts(e, e->td3_q, e->td3_q_t, e->td3_pol_t);
    e->td3_a_shift = shift; e->td3_a_scale = scale; e->td3_ring = o.ring;
    // theta starts as the device's policy; the targets as copies (of the critics too: zeros until they are uploaded and synchronised)
    td3_params_copy(e, kTd3Theta, 1);
    if ((rc = off_sync_run(e, kOffSolo, 1, 0))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_td3 = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_set_critic_layer(adc_engine *e, int32_t critic, int32_t layer, const float *weights_in_out, const float *bias_out)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    return off_set_critic_layer(e, kOffSolo, critic, layer, weights_in_out, bias_out);
}

ADC_EXPORT int adc_engine_td3_set_action_norm(adc_engine *e, const float *shift_a, const float *scale_a)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    return td3_action_norm_run(e, shift_a, scale_a);
}

ADC_EXPORT int adc_engine_td3_sync_targets(adc_engine *e)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    ENGINE_GUARD(e);
    if (int rc = off_sync_run(e, kOffSolo, 1, 0)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_store(adc_engine *e, int64_t *stored)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = td3_ready(e)) || (rc = td3_state_check(e)) || (rc = td3_bounded_check(e, &e->td3_cfg, 1)) || (rc = off_store_check(e))) return rc;
    if (e->ro_dagger > 0)
        return fail(ADC_ESTATE, "the record holds DAgger days: their recorded action is the teacher's label, not the action the step consumed, so they are "
                                "not demonstrations (adc_engine_rollout_reset, adc_engine_teach_days)");
    ENGINE_GUARD(e);
    const long long count = (long long)(e->ro_t - e->td3_stored_t) * e->v.N;        // (every env is the one learner's)
    // (raw rows under a running observation normaliser - TD3's set, e->tn: the last day's x' is the raw row an act would read now)
    // (with an observation history the last day's x' is the stacked row, peeked)
    if (e->nstep_n) off_store_nstep_launch(e, false, e->tn.obs.count != 0, count);       // (n-step returns: the window's R, done and gn)
    else if (e->mp.frames > 1)
        hipLaunchKernelGGL(k_td3_store_hist, dim3((unsigned)count), dim3(kPgBlock), 0, e->stream, e->v, e->tn.obs.count ? nullptr : e->mp.shift,
                           e->tn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A, e->ro_obs,
                           e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->td3_ring, (unsigned long long)e->td3_written,
                           (unsigned long long)e->td3_cfg.capacity,
                           e->mp.hist, e->mp.last, e->mp.from, e->mp.frames);
    else
        hipLaunchKernelGGL(k_td3_store, dim3((unsigned)count), dim3(kPgBlock), 0, e->stream, e->v, e->tn.obs.count ? nullptr : e->mp.shift,
                           e->tn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A, e->ro_obs,
                           e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->td3_ring, (unsigned long long)e->td3_written,
                           (unsigned long long)e->td3_cfg.capacity);
    return off_store_done(e, count, stored);
}

ADC_EXPORT int adc_engine_td3_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    return off_buffer_info(e, size, written, capacity, nullptr);
}

ADC_EXPORT int adc_engine_td3_batch_size(adc_engine *e, int32_t *batch_size)
{
    if (!e || !batch_size) return fail(ADC_EINVAL, "engine handle or batch_size is NULL");
    if (int rc = td3_ready(e)) return rc;
    *batch_size = e->td3_cfg.batch_size;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_buffer_fetch(adc_engine *e, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done, float *x2)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    return off_ring_fetch(e, kOffSolo, slot, count, x, a, r, done, x2);
}

ADC_EXPORT int adc_engine_td3_buffer_load(adc_engine *e, int64_t slot, int64_t count, const float *x, const float *a, const float *r, const uint8_t *done,
                                          const float *x2, int64_t written)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    return off_ring_load(e, kOffSolo, slot, count, x, a, r, done, x2, written);
}

ADC_EXPORT int adc_engine_td3_batch_indices(adc_engine *e, int64_t update, int32_t *idx_b)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    return off_batch_indices(e, e->td3_key, update, idx_b, "the replay buffer is empty (adc_engine_td3_store)");
}

ADC_EXPORT int adc_engine_td3_update(adc_engine *e, int32_t updates, adc_td3_stats *stats)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = td3_ready(e)) || (rc = td3_state_check(e)) || (rc = td3_bounded_check(e, &e->td3_cfg, 1)) ||
        (rc = off_update_check(e, updates, false, "a critic layer has not been uploaded (adc_engine_td3_set_critic_layer)",
                               "the replay buffer is empty (adc_engine_td3_store)", 0xFFFFFFFFll)))
        return rc;
    ENGINE_GUARD(e);
    HIP_TRY(hipMemsetAsync(e->td3_sums, 0, 16 * sizeof(double), e->stream));
    for (int i = 0; i < updates; ++i)
        // (the statistics' sums are taken for the call's last update and for its last actor step alone)
        if ((rc = td3_one_update(e, stats != nullptr, i + 1 == updates, updates - 1 - i < e->td3_cfg.policy_delay))) return rc;
    double sums[10] = {};
    if (stats) HIP_TRY(hipMemcpyAsync(sums, e->td3_sums, sizeof(sums), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats) td3_stats_fill(e, sums, stats);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    return off_param_counts(e, actor_p, critics_2qc);
}

ADC_EXPORT int adc_engine_td3_state_get(adc_engine *e, float *theta_p, float *psi_q, float *theta_target_p, float *psi_target_q, float *m_theta_p,
                                        float *v_theta_p, float *m_psi_q, float *v_psi_q, int64_t *updates, int64_t *actor_steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = td3_ready(e)) return rc;
    ENGINE_GUARD(e);
    float *flat[4] = {theta_p, psi_q, theta_target_p, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    if (int rc = off_state_get(e, kOffSolo, flat, mom)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (updates) *updates = e->td3_updates;
    if (actor_steps) *actor_steps = e->td3_actor_steps;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_state_set(adc_engine *e, const float *theta_p, const float *psi_q, const float *theta_target_p, const float *psi_target_q,
                                        const float *m_theta_p, const float *v_theta_p, const float *m_psi_q, const float *v_psi_q, int64_t updates,
                                        int64_t actor_steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const float *flat[4] = {theta_p, psi_q, theta_target_p, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    int rc;
    if ((rc = td3_ready(e)) || (rc = td3_state_set_check(flat, mom, updates, actor_steps))) return rc;
    ENGINE_GUARD(e);
    if ((rc = off_state_set(e, kOffSolo, flat, mom, updates))) return rc;
    e->td3_actor_steps = actor_steps;
    return ADC_OK;
}
