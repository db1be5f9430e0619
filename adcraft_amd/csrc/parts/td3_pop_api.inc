// td3_pop_api.inc - the extern "C" entry points of TD3 learner populations: M off-policy learners in lock-step on one engine, every
// launch over all members (include/adcraft_engine.h; the kernels are parts/kernel_td3_pop.inc and the k_pg_pop_* of
// parts/kernel_pg.inc, the law csrc/adc_td3.h).  The population shares the solo trainer's engine fields, sized for all members:
// td3_flat / td3_mom are [M][P] and [M][2 Qc], the scratch [M][B][...], td3_sums [M][16]; td3_cfg holds the shared fields
// (batch_size, capacity, the critics' shape, policy_delay), td3_lay member 0's stores (a member's tp_stride[w] floats further).
// The ring, the critic upload, the state vectors, the allocation, the tp_* launch helpers and the update driver are
// parts/offpolicy_core.inc's; here are the population's refusals, its members' fill, its step table and its update.
// (part of the single translation unit adc_engine.hip)
namespace {
int tp_ready(const adc_engine *e)
{
    if (!e->have_td3_pop)
        return fail(ADC_ESTATE, "adc_engine_td3_pop_init has not been called (or the policy, the learners or the record were re-initialised since)");
    return ADC_OK;
}
int tp_state_check(const adc_engine *e)
{
    if (int rc = mlp_ready(e)) return rc;
    if (e->lrn_M == 0) return fail(ADC_ESTATE, "population training needs learners (adc_engine_mlp_learners)");
    if (e->mp.two_heads) return fail(ADC_ESTATE, "TD3 needs the policy with the free log_std head: a two-headed policy (2A outputs) is not supported");
    if (e->ro_T == 0) return fail(ADC_ESTATE, "off-policy training needs a rollout record (adc_engine_rollout_enable)");
    if (!e->ro_obs) return fail(ADC_ESTATE, "off-policy training needs the recorded network input (adc_engine_rollout_enable with ADC_ROLLOUT_OBS)");
    return ADC_OK;
}
// a member's law constants and key from its configuration
void tp_member_fill(const adc_engine *e, Td3Member &m, const adc_td3_config &c)
{
    m.law = adc::td3_law_of(c);
    m.key = adc::td3_key(c.seed ? c.seed : e->cfg.seed);
}
int tp_members_upload(adc_engine *e)
{
    HIP_TRY(hipMemcpyAsync(e->tp_dmem, e->tp_mem.data(), e->tp_mem.size() * sizeof(Td3Member), hipMemcpyHostToDevice, e->stream));
    return ADC_OK;
}
// row `row` of the step table: every member's constants of its next critic (actor = false) or actor step; no clip until a scale is known
void tp_steps_fill(adc_engine *e, int row, bool actor, int64_t steps_taken)
{
    const size_t M = (size_t)e->lrn_M;
    for (size_t m = 0; m < M; ++m) {
        const adc_td3_config &c = e->tp_cfg[m];
        Td3PopStep &s = e->tp_steps[(size_t)row * M + m];
        s.clip = 0; s.scale = 1.0f;
        s.step = td3_step_of(c, actor ? c.actor_lr : c.critic_lr, steps_taken);
    }
}
// one update of every member; `index`: the update's place in the call's block of kTd3PopBlock (its rows of the step table).
// The members' sums as in the solo path: [0..4] the critic pieces, [5] the critics' grad^2, [8] Q1(x, mu(x)), [9] the actor's grad^2
int tp_one_update(adc_engine *e, int index, bool stats_wanted, bool last, bool last_actor, bool any_clip)
{
    const adc::Td3Shape &sh = e->td3_shape;
    const int M = e->lrn_M, B = e->td3_cfg.batch_size, DA = sh.D + sh.A;
    const int nh = adc::td3_hidden(sh.q), no = adc::td3_outs(sh.q), ph = adc::td3_hidden(sh.pol), po = adc::td3_outs(sh.pol);
    const size_t lds = td3_lds_floats(sh) * sizeof(float);
    const dim3 grid((unsigned)B, (unsigned)M);
    Td3View p{};
    p.sh = sh;
    p.sh.norm = e->td3_norm_set ? 1 : 0;
    p.a_shift = e->td3_a_shift; p.a_scale = e->td3_a_scale;
    p.size = (uint32_t)td3_size(e); p.update = (uint32_t)e->td3_updates;
    p.ybuf = e->td3_ybuf; p.xin = e->td3_xin; p.acts = e->td3_acts; p.deltas = e->td3_deltas; p.pieces = e->td3_pieces;
    p.maxw = adc::td3_max_width(sh);
    td3_norm_fill(e, p);
    td3_per_fill(e, p);
    p.na = 2 * nh; p.nd = 2 * no;
    int rc;
    if (e->per_live && (rc = per_sample_run(e, p.update))) return rc;
    hipLaunchKernelGGL(e->td3_bounded ? k_td3_pop_target_bounded : k_td3_pop_target, grid, dim3(kPgBlock), lds, e->stream, p, e->tp_dmem);
    hipLaunchKernelGGL(k_td3_pop_critic_sample, grid, dim3(kPgBlock), lds, e->stream, p, e->tp_dmem);
    for (int i = 0; i < 2; ++i) tp_wgrad_launch(e, sh.q, DA, p.na, i * nh, p.nd, i * no, i * e->td3_Qc, 2 * e->td3_Qc, B);
    HIP_TRY(hipGetLastError());
    if (e->per_live && (rc = per_leaves_run(e))) return rc;
    if (stats_wanted && last && (rc = tp_csum_launch(e, e->td3_pieces, B, (size_t)B, adc::kTd3Pieces, 5, 0, 0))) return rc;
    if ((rc = tp_step_run(e, kTd3Psi, e->td3_mom + 2, 2 * e->td3_Qc, B, stats_wanted && last, 5, 2 * index, any_clip))) return rc;
    if ((e->td3_updates + 1) % e->td3_cfg.policy_delay == 0) {
        p.na = ph; p.nd = po;
        hipLaunchKernelGGL(e->td3_bounded ? k_td3_pop_actor_sample_bounded : k_td3_pop_actor_sample, grid, dim3(kPgBlock), lds, e->stream, p, e->lrn_tab, e->tp_dmem);
        tp_wgrad_launch(e, sh.pol, DA, p.na, 0, p.nd, 0, 0, e->td3_P, B);
        HIP_TRY(hipGetLastError());
        if (stats_wanted && last_actor && (rc = tp_csum_launch(e, e->td3_pieces + adc::kTd3QPi, B, (size_t)B, adc::kTd3Pieces, 1, 0, 8))) return rc;
        if ((rc = tp_step_run(e, kTd3Theta, e->td3_mom, e->td3_P, B, stats_wanted && last_actor, 9, 2 * index + 1, any_clip))) return rc;
        for (int w = 0; w < 2; ++w) {
            const PgLayout &lay = e->td3_lay[kTd3ThetaT + w];
            hipLaunchKernelGGL(k_td3_pop_polyak, dim3(pg_blocks(lay.Q), (unsigned)M), dim3(kPgBlock), 0, e->stream, lay, e->tp_stride[kTd3ThetaT + w],
                               e->td3_flat[kTd3ThetaT + w], e->td3_flat[kTd3Theta + w], e->tp_dmem);
        }
        HIP_TRY(hipGetLastError());
        e->td3_actor_steps += 1;
    }
    e->td3_updates += 1;
    return ADC_OK;
}
}  // namespace

ADC_EXPORT int adc_engine_td3_pop_init(adc_engine *e, const adc_td3_config *cfgs, int32_t count)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = tp_state_check(e)) return rc;
    const int N = e->v.N, M = e->lrn_M;
    const char *why = nullptr;
    if (adc_td3_pop_config_check(cfgs, count, N, M, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    if (e->have_td3) return fail(ADC_ESTATE, "a single-learner off-policy (TD3) trainer is alive on this engine (adc_engine_td3_init)");
    if (e->have_sac || e->have_sac_pop) return fail(ADC_ESTATE, "a soft actor-critic trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->rn.live) return fail(ADC_ESTATE, "a running reward normaliser is alive on this engine: it belongs to the policy-gradient trainer");
    if (e->have_pg || e->have_pg_pop)
        return fail(ADC_ESTATE, "a policy-gradient trainer is alive on this engine: one trainer at a time owns the policy's weights");
    if (e->on.live)
        return fail(ADC_ESTATE, "a running observation normaliser is alive on this engine: the replay ring would hold inputs normalised by older vectors");
    const adc::Td3Shape sh = adc::td3_shape_of(e->mlp_cfg, e->v.K, cfgs[0], 0, mlp_frames(e));
    if (td3_lds_floats(sh) * sizeof(float) > 64u * 1024u)
        return fail(ADC_EINVAL, td3_lds_floats(adc::td3_shape_of(e->mlp_cfg, e->v.K, cfgs[0], 0)) * sizeof(float) > 64u * 1024u
                                    ? "num_keywords too large for off-policy training (LDS)"
                                    : "frames: the stacked input row is too large for off-policy training (LDS); fewer frames fit");
    ENGINE_GUARD(e);
    const size_t Ms = (size_t)M, C = (size_t)cfgs[0].capacity;
    const OffBlock k = off_block_layout(sh, 5);
    // (the new state is allocated before the old one goes: a failure leaves the engine as it was)
    std::vector<void *> fresh;
    OffBufs o;
    float *block = nullptr, *shift = nullptr, *scale = nullptr;
    Td3Member *dmem = nullptr;
    Td3PopStep *dsteps = nullptr;
    int rc;
    if ((rc = off_alloc(e, fresh, sh, cfgs[0].batch_size, C, Ms, true, o)) || (rc = mlp_alloc(e, fresh, &block, Ms * k.stride)) ||
        (rc = mlp_alloc(e, fresh, &shift, (size_t)sh.A)) || (rc = mlp_alloc(e, fresh, &scale, (size_t)sh.A)) || (rc = mlp_alloc(e, fresh, &dmem, Ms)) ||
        (rc = mlp_alloc(e, fresh, &dsteps, Ms * 2u * (size_t)kTd3PopBlock))) {
        mlp_free(e, fresh);
        return rc;
    }
    td3_drop(e);
    e->td3_allocs.swap(fresh);
    off_install(e, o, sh);
    e->td3_cfg = cfgs[0];
    e->tp_cfg.assign(Ms, cfgs[0]);
    if (count > 1) e->tp_cfg.assign(cfgs, cfgs + M);
    e->tp_mem.assign(Ms, Td3Member{});
    for (size_t m = 0; m < Ms; ++m) {
        tp_member_fill(e, e->tp_mem[m], e->tp_cfg[m]);
        off_member_place(e->tp_mem[m], m, k, 5, block, o, sh, C);
    }
    // member 0's stores against the flat orders; theta's are the learners' policy layers
    tp_theta_layout(e, k.stride);
    off_layouts(e, e->tp_mem[0].q, e->tp_mem[0].q_t, e->tp_mem[0].pol_t);
    e->td3_a_shift = shift; e->td3_a_scale = scale; e->td3_ring = Td3Ring{};
    e->tp_dmem = dmem; e->tp_dsteps = dsteps; e->tp_part_stride = o.part_stride;
    e->tp_steps.assign(Ms * 2u * (size_t)kTd3PopBlock, Td3PopStep{});
    e->tp_host_sums.assign(Ms * 16u, 0.0);
    e->tp_critic_set.assign(Ms * kOffCriticFlags, 0);
    if ((rc = tp_members_upload(e))) return rc;
    // every member's theta starts as its device policy; the targets as copies (of the critics too: zeros until they are uploaded and synchronised)
    tp_params_copy(e, kTd3Theta, 0, M, 1);
    if ((rc = off_sync_run(e, 0, M, 0))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->have_td3_pop = true;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_pop_set_critic_layer(adc_engine *e, int32_t member, int32_t critic, int32_t layer, const float *weights_in_out,
                                                   const float *bias_out)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    return off_set_critic_layer(e, member, critic, layer, weights_in_out, bias_out);
}

ADC_EXPORT int adc_engine_td3_pop_set_action_norm(adc_engine *e, const float *shift_a, const float *scale_a)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = tp_ready(e)) return rc;
    return td3_action_norm_run(e, shift_a, scale_a);
}

ADC_EXPORT int adc_engine_td3_pop_sync_targets(adc_engine *e, int32_t member)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (member != -1 && (rc = tp_member_check(e, member)))) return rc;
    ENGINE_GUARD(e);
    if ((rc = member == -1 ? off_sync_run(e, 0, e->lrn_M, 0) : off_sync_run(e, member, 1, 0))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_pop_store(adc_engine *e, int64_t *stored_per_member)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_state_check(e)) || (rc = td3_bounded_check(e, e->tp_cfg.data(), e->tp_cfg.size())) || (rc = off_store_check(e))) return rc;
    ENGINE_GUARD(e);
    const long long count = (long long)(e->ro_t - e->td3_stored_t) * e->lrn_n;      // (a member's envs, not the engine's)
    // (raw rows under a running observation normaliser - TD3's set, e->tn)
    // (with an observation history the last day's x' is the stacked row, peeked)
    if (e->nstep_n) off_store_nstep_launch(e, true, e->tn.obs.count != 0, count);       // (n-step returns: the window's R, done and gn)
    else if (e->mp.frames > 1)
        hipLaunchKernelGGL(k_td3_pop_store_hist, dim3((unsigned)count, (unsigned)e->lrn_M), dim3(kPgBlock), 0, e->stream, e->v, e->tn.obs.count ? nullptr : e->mp.shift,
                           e->tn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A,
                           e->ro_obs, e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->lrn_n, e->tp_dmem,
                           (unsigned long long)e->td3_written, (unsigned long long)e->td3_cfg.capacity,
                           e->mp.hist, e->mp.last, e->mp.from, e->mp.frames);
    else
        hipLaunchKernelGGL(k_td3_pop_store, dim3((unsigned)count, (unsigned)e->lrn_M), dim3(kPgBlock), 0, e->stream, e->v, e->tn.obs.count ? nullptr : e->mp.shift,
                           e->tn.obs.count ? nullptr : e->mp.scale, e->mp.D, e->mp.A,
                           e->ro_obs, e->ro_action, e->ro_reward, e->ro_term, e->ro_trunc, e->td3_stored_t, e->ro_t, e->lrn_n, e->tp_dmem,
                           (unsigned long long)e->td3_written, (unsigned long long)e->td3_cfg.capacity);
    return off_store_done(e, count, stored_per_member);
}

ADC_EXPORT int adc_engine_td3_pop_buffer_info(adc_engine *e, int64_t *size, int64_t *written, int64_t *capacity, int32_t *batch_size)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = tp_ready(e)) return rc;
    return off_buffer_info(e, size, written, capacity, batch_size);
}

ADC_EXPORT int adc_engine_td3_pop_buffer_fetch(adc_engine *e, int32_t member, int64_t slot, int64_t count, float *x, float *a, float *r, uint8_t *done,
                                               float *x2)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    return off_ring_fetch(e, member, slot, count, x, a, r, done, x2);
}

ADC_EXPORT int adc_engine_td3_pop_buffer_load(adc_engine *e, int32_t member, int64_t slot, int64_t count, const float *x, const float *a, const float *r,
                                              const uint8_t *done, const float *x2, int64_t written)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    return off_ring_load(e, member, slot, count, x, a, r, done, x2, written);
}

ADC_EXPORT int adc_engine_td3_pop_batch_indices(adc_engine *e, int32_t member, int64_t update, int32_t *idx_b)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    return off_batch_indices(e, e->tp_mem[(size_t)member].key, update, idx_b, "the replay buffer is empty (adc_engine_td3_pop_store)");
}

ADC_EXPORT int adc_engine_td3_pop_update(adc_engine *e, int32_t updates, adc_td3_stats *stats_m)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_state_check(e)) || (rc = td3_bounded_check(e, e->tp_cfg.data(), e->tp_cfg.size())) ||
        (rc = off_update_check(e, updates, true, "a critic layer of a member has not been uploaded (adc_engine_td3_pop_set_critic_layer)",
                               "the replay buffer is empty (adc_engine_td3_pop_store)", 0xFFFFFFFFll)))
        return rc;
    ENGINE_GUARD(e);
    const int M = e->lrn_M, delay = e->td3_cfg.policy_delay;
    bool any_clip = false;
    for (const adc_td3_config &c : e->tp_cfg) any_clip = any_clip || c.max_grad_norm > 0.0f;
    rc = off_pop_updates(
        e, updates, 2,
        [&](int nb) {
            int64_t actor_steps = e->td3_actor_steps;
            for (int i = 0; i < nb; ++i) {
                tp_steps_fill(e, 2 * i, false, e->td3_updates + i);
                if ((e->td3_updates + i + 1) % delay == 0) tp_steps_fill(e, 2 * i + 1, true, actor_steps++);
            }
        },
        [&](int u, int i) {
            const int left = updates - 1 - u;
            // (the statistics' sums are taken for the call's last update and for its last actor step alone)
            return tp_one_update(e, i, stats_m != nullptr, left == 0, left < delay, any_clip);
        });
    if (rc) return rc;
    if (stats_m) HIP_TRY(hipMemcpyAsync(e->tp_host_sums.data(), e->td3_sums, (size_t)M * 16 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (stats_m)
        for (int m = 0; m < M; ++m) td3_stats_fill(e, e->tp_host_sums.data() + (size_t)m * 16, stats_m + m);
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_pop_param_counts(adc_engine *e, int64_t *actor_p, int64_t *critics_2qc)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    if (int rc = tp_ready(e)) return rc;
    return off_param_counts(e, actor_p, critics_2qc);
}

ADC_EXPORT int adc_engine_td3_pop_state_get(adc_engine *e, int32_t member, float *theta_p, float *psi_q, float *theta_target_p, float *psi_target_q,
                                            float *m_theta_p, float *v_theta_p, float *m_psi_q, float *v_psi_q, int64_t *updates, int64_t *actor_steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    ENGINE_GUARD(e);
    float *flat[4] = {theta_p, psi_q, theta_target_p, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    if ((rc = off_state_get(e, member, flat, mom))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (updates) *updates = e->td3_updates;
    if (actor_steps) *actor_steps = e->td3_actor_steps;
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_pop_state_set(adc_engine *e, int32_t member, const float *theta_p, const float *psi_q, const float *theta_target_p,
                                            const float *psi_target_q, const float *m_theta_p, const float *v_theta_p, const float *m_psi_q,
                                            const float *v_psi_q, int64_t updates, int64_t actor_steps)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    const float *flat[4] = {theta_p, psi_q, theta_target_p, psi_target_q}, *mom[4] = {m_theta_p, v_theta_p, m_psi_q, v_psi_q};
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_member_check(e, member)) || (rc = td3_state_set_check(flat, mom, updates, actor_steps))) return rc;
    ENGINE_GUARD(e);
    if ((rc = off_state_set(e, member, flat, mom, updates))) return rc;
    e->td3_actor_steps = actor_steps;       // (the members move together: one pair of counters for all)
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_pop_set_config(adc_engine *e, int32_t member, const adc_td3_config *cfg)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_member_check(e, member))) return rc;
    const char *why = nullptr;
    if (adc_td3_config_check(cfg, &why) != ADC_OK) return fail(ADC_EINVAL, why);
    const adc_td3_config shared[2] = {e->td3_cfg, *cfg};
    if (adc_td3_pop_config_check(shared, 2, 2, 2, &why) != ADC_OK)
        return fail(ADC_EINVAL, "batch_size, capacity, the critics' shape and policy_delay may not change: the members' updates run in the same launches");
    ENGINE_GUARD(e);
    HIP_TRY(hipStreamSynchronize(e->stream));       // (an upload of the host's table may still be in flight)
    e->tp_cfg[(size_t)member] = *cfg;
    tp_member_fill(e, e->tp_mem[(size_t)member], *cfg);
    if ((rc = tp_members_upload(e))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ADC_OK;
}

ADC_EXPORT int adc_engine_td3_pop_copy(adc_engine *e, int32_t src, int32_t dst, int32_t with_ring)
{
    if (!e) return fail(ADC_EINVAL, "engine handle is NULL");
    int rc;
    if ((rc = tp_ready(e)) || (rc = tp_member_check(e, src)) || (rc = tp_member_check(e, dst))) return rc;
    if (src == dst) return ADC_OK;
    ENGINE_GUARD(e);
    return off_pop_copy(e, src, dst, with_ring);
}
